"""DeviceModel: one annotator network living on one MI355X, driven through the C ABI (include/dnnca.h).

This is the object that replaces the compiled tf.keras.Model of the reference (engine.py:254-288): it owns the
weights, the Adam slots and the activations in HBM and exposes forward / train_step / eval_step."""

import ctypes as C
from collections import OrderedDict, namedtuple

import numpy as np

from . import _lib
from ._lib import check, fptr, as_f32

# what DeviceModel.integrated_gradients returns
Attribution = namedtuple('Attribution', 'signed absolute endpoints map')


def init_device(ordinal=0):
    check(_lib.load().dnnca_init(int(ordinal)))


def device_count():
    n = C.c_int(0)
    lib = _lib.load()
    if lib.dnnca_device_count(C.byref(n)) != 0:
        return 0
    return n.value


class DeviceBuffer:
    """A raw HBM allocation holding a float32 array (device-resident batches for the benchmark loop)."""

    def __init__(self, array):
        array = as_f32(array)
        self.shape = array.shape
        self.nbytes = array.nbytes
        self.ptr = C.c_void_p()
        check(_lib.load().dnnca_dev_alloc(C.byref(self.ptr), self.nbytes))
        check(_lib.load().dnnca_memcpy_h2d(self.ptr, array.ctypes.data_as(C.c_void_p), self.nbytes))

    def to_host(self):
        out = np.empty(self.shape, np.float32)
        check(_lib.load().dnnca_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.ptr, self.nbytes))
        return out

    def free(self):
        if self.ptr:
            _lib.load().dnnca_dev_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class RawDeviceBuffer:
    """An HBM allocation of `nbytes` bytes (uint8 source batches of the device-side augmentation; grown on demand)."""

    def __init__(self):
        self.ptr, self.nbytes = C.c_void_p(), 0

    def reserve(self, nbytes):
        if nbytes > self.nbytes:
            self.free()
            check(_lib.load().dnnca_dev_alloc(C.byref(self.ptr), nbytes))
            self.nbytes = nbytes

    def upload(self, array):
        array = np.ascontiguousarray(array)
        self.reserve(array.nbytes)
        check(_lib.load().dnnca_memcpy_h2d(self.ptr, array.ctypes.data_as(C.c_void_p), array.nbytes))

    def free(self):
        if self.ptr:
            _lib.load().dnnca_dev_free(self.ptr)
            self.ptr, self.nbytes = C.c_void_p(), 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceView:
    """A float32 tensor inside a RawDeviceBuffer (what train_step_dev takes: .ptr and .shape)."""

    def __init__(self, buf, shape):
        self.buf, self.ptr, self.shape = buf, buf.ptr, tuple(shape)
        self.nbytes = int(np.prod(shape)) * 4

    def to_host(self):
        out = np.empty(self.shape, np.float32)
        check(_lib.load().dnnca_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.ptr, self.nbytes))
        return out


def threshold_vector(thresholds):
    """a scalar, a sequence or None -> the contiguous float32 vector the library takes"""
    return as_f32(() if thresholds is None else thresholds).ravel()


def confusion_rows(n, fill):
    """[(tp, fp, fn, tn)] per threshold: `fill` has the library write an array of n dnnca_confusion records"""
    out = (_lib.Confusion * max(n, 1))()
    fill(out)
    return [(c.tp, c.fp, c.fn, c.tn) for c in out[:n]]


def region_specs(specs):
    """[(thresholds, iou_threshold, resize_factor, morph_filter_size)] -> (dnnca_region_spec array, threshold arrays to keep alive)"""
    keep = [threshold_vector(s[0]) for s in specs]
    arr = (_lib.RegionSpec * max(len(specs), 1))()
    for a, s, thr in zip(arr, specs, keep):
        a.thresholds, a.n_thresholds = fptr(thr), thr.size
        a.iou_threshold, a.resize_factor, a.morph_filter_size = float(s[1]), float(s[2]), int(s[3])
    return arr, keep


def split_region_counts(out, sizes):
    rows = np.array([(c.tp_label, c.fn, c.tp_pred, c.fp) for c in out[:sum(sizes)]], np.int64).reshape(-1, 4)
    res, lo = [], 0
    for n in sizes:
        res.append(rows[lo:lo + n])
        lo += n
    return res


# ---- the plane inputs of the analysis calls (lesion tables, boundary distances, spread, calibration) ----------------------------
def _slices(a, what):
    """`a` [B, h, w] or [B, h, w, 1] -> contiguous float32 [B, h, w]"""
    a = as_f32(a)
    if a.ndim == 4 and a.shape[-1] == 1:
        a = np.ascontiguousarray(a[..., 0])
    if a.ndim != 3:
        raise ValueError('%s must be [B, h, w], got %s' % (what, a.shape))
    return a


def _labels(y, batch=None):
    """the labels of an analysis call -> float32 [B, h, w], of `batch` slices where that is given"""
    y = _slices(y, 'y')
    if batch is not None and int(batch) != y.shape[0]:
        raise ValueError('batch %d but y holds %d slices' % (batch, y.shape[0]))
    return y


def _host_prob(prob, y, same_shape):
    """host probabilities beside the labels y [B, h, w]: [B, h, w(, 1)] like y (same_shape), else anything of y's size"""
    if same_shape:
        prob = _slices(prob, 'prob')
        if prob.shape != y.shape:
            raise ValueError('prob %s and y %s differ in shape' % (prob.shape, y.shape))
        return prob
    prob = as_f32(prob).reshape(-1)
    if prob.size != y.size:
        raise ValueError('prob and y differ in size')
    return prob


def _continues(continues, batch):
    """one flag per slice -> uint8 [batch]"""
    flags = np.ascontiguousarray(np.asarray(continues).astype(bool), np.uint8)
    if flags.shape != (batch,):
        raise ValueError('continues must hold one flag per slice (%d), got shape %s' % (batch, flags.shape))
    return flags


def _analysed_plane(query):
    """the size query of a lesion or boundary call (`query(hw)`: the call without output buffers) -> (hw, oh, ow)"""
    hw = (C.c_int32 * 2)()
    check(query(hw))
    return hw, hw[0], hw[1]


def _lesion_table_buffers(batch, oh, ow, max_lesions, mask, links):
    """the buffers of one lesion table on planes of oh x ow: (rows, totals, links or None, masks or None)"""
    per_slice = min(int(max_lesions), (oh * ow + 1) // 2)
    rows = np.zeros(batch * per_slice, _lib.LESION_ROW_DTYPE)
    links = np.zeros(batch * min(per_slice * per_slice, (oh * ow + 1) // 2), _lib.LESION_LINK_DTYPE) if links else None
    return rows, np.zeros(batch, np.int32), links, np.empty((batch, oh, ow), np.uint8) if mask else None


class StagingRing:
    """The model's staging slots in HBM + its copy stream (include/dnnca.h, dnnca_stage_*): what ds.prefetch + Keras' asynchronous
    input feeding are for the reference (annotator/data.py:110,143; engine.py:126-135).  `upload` may run on a second thread."""

    MAX_SLOTS = 8          # engine: slots 0-3 feed the train steps, 4-7 the evaluation / validation steps

    def __init__(self, dm, slots=8, slot_bytes=0):
        self.dm, self.slots = dm, int(slots)
        check(dm.lib.dnnca_stage_init(dm.handle, self.slots, int(slot_bytes)))
        x_bytes = dm.max_batch * int(np.prod(dm.in_shape)) * 4
        y_bytes = dm.max_batch * dm.in_shape[0] * dm.in_shape[1] * 4
        self.slot_bytes = max(int(slot_bytes), ((x_bytes + 255) & ~255) + y_bytes)

    def fits(self, a, b=None):
        return ((a.nbytes + 255) & ~255) + (0 if b is None else b.nbytes) <= self.slot_bytes

    def upload(self, slot, a, b=None, wait=True):
        """host arrays -> the slot, on the copy stream (behind the step that read the slot's previous content); returns the device
        addresses (c_void_p) of a and b.  wait=True blocks the CALLING thread until the copy has completed, so the arrays may be
        reused or freed afterwards; with wait=False the caller keeps them alive and unchanged until the slot's step has run."""
        a = np.ascontiguousarray(a)
        b = None if b is None else np.ascontiguousarray(b)
        pa, pb = C.c_void_p(), C.c_void_p()
        check(self.dm.lib.dnnca_stage_upload(self.dm.handle, int(slot), a.ctypes.data_as(C.c_void_p), a.nbytes,
                                             None if b is None else b.ctypes.data_as(C.c_void_p), 0 if b is None else b.nbytes,
                                             C.byref(pa), C.byref(pb)))
        if wait:
            check(self.dm.lib.dnnca_stage_uploaded(self.dm.handle, int(slot)))
        return pa, (None if b is None else pb)

    def wait(self, slot):
        """the model's stream waits for the slot's upload (before kernels other than the train step read it)"""
        check(self.dm.lib.dnnca_stage_wait(self.dm.handle, int(slot)))

    def train_step(self, slot, x_ptr, y_ptr, batch, lr, cfg):
        """asynchronous train step on device-resident (x, y) that depend on the slot's upload; outputs: out(slot)"""
        check(self.dm.lib.dnnca_train_step_staged(self.dm.handle, int(slot), x_ptr, y_ptr, int(batch), float(lr), C.byref(cfg)))

    # keras Model.evaluate (engine.py:198-203) over the ring: the confusion histogram of ALL thresholds stays on the device
    def eval_begin(self, thresholds=()):
        thr = threshold_vector(thresholds)
        self._n_thr = int(thr.size)
        check(self.dm.lib.dnnca_eval_begin(self.dm.handle, thr.ctypes.data_as(C.c_void_p) if thr.size else None, self._n_thr))

    def eval_step(self, slot, x_ptr, y_ptr, batch, cfg):
        check(self.dm.lib.dnnca_eval_step_staged(self.dm.handle, int(slot), x_ptr, y_ptr, int(batch), C.byref(cfg)))

    def eval_end(self):
        """[(tp, fp, fn, tn)] per threshold of eval_begin, summed over every eval_step since (exact integers)"""
        return confusion_rows(self._n_thr, lambda out: check(self.dm.lib.dnnca_eval_end(self.dm.handle, out)))

    # region-based metrics of the same evaluation (kernels_region.hip): between eval_begin and the first eval_step
    def eval_region_begin(self, specs):
        """specs: [RegionSpec-like (thresholds, iou_threshold, resize_factor, morph_filter_size)]; every later eval_step adds its
        batch's region counts on the device"""
        arr, self._region_keep = region_specs(specs)
        self._region_n = [len(k) for k in self._region_keep]
        check(self.dm.lib.dnnca_eval_region_begin(self.dm.handle, arr, len(self._region_n)))

    def eval_region_end(self):
        """[array [T, 4] int64 (tp_label, fn, tp_pred, fp) per spec of eval_region_begin], summed over every eval_step since"""
        out = (_lib.RegionCounts * sum(self._region_n))()
        check(self.dm.lib.dnnca_eval_region_end(self.dm.handle, out))
        return split_region_counts(out, self._region_n)

    def confusion(self, slot):
        """[(tp, fp, fn, tn)] per threshold of DeviceModel.train_metrics for the train step that last ran on the slot (exact
        integers); waits for that step like out(slot) does -- read it before the slot takes its next batch"""
        return confusion_rows(self.dm._tm_n, lambda out: check(self.dm.lib.dnnca_staged_confusion(self.dm.handle, int(slot), out)))

    def out(self, slot):
        """waits for the step that last ran on the slot; raises what train_step would have raised (label / weight assertions)"""
        out = _lib.StepOut()
        check(self.dm.lib.dnnca_staged_out(self.dm.handle, int(slot), C.byref(out)))
        return out


class _AveragedWeights:
    """`with dm.averaged_weights():` -- the averaged weights stand in for the raw ones inside the block (DeviceModel.exchange_ema)"""

    def __init__(self, dm):
        self.dm = dm

    def __enter__(self):
        self.dm.exchange_ema()
        return self.dm

    def __exit__(self, *exc):
        self.dm.exchange_ema()
        return False


class DeviceModel:
    def __init__(self, arch, in_channels, height, width, max_batch, n_filters_first, n_downsample, rate=2, kernel_size=3,
                 conv_stride=1, bn=False, padding='valid', leaky_alpha=0.0, l2=0.0, reference_index=0, n_conv=2,
                 dtype='f32', force_generic=False):
        self.lib = _lib.load()
        d = _lib.ModelDesc()
        d.arch = {'unet': _lib.ARCH_UNET, 'mulmo': _lib.ARCH_MULMO, 'multires': _lib.ARCH_MULTIRES}[arch]
        d.in_channels, d.height, d.width, d.max_batch = int(in_channels), int(height), int(width), int(max_batch)
        d.n_filters_first, d.n_downsample, d.rate = int(n_filters_first), int(n_downsample), int(rate)
        d.kernel_size, d.conv_stride, d.bn = int(kernel_size), int(conv_stride), int(bool(bn))
        d.padding = {'same': _lib.PAD_SAME, 'valid': _lib.PAD_VALID}[padding]
        d.reference_index, d.n_conv = int(reference_index), int(n_conv)
        d.leaky_alpha, d.l2 = float(leaky_alpha), float(l2)
        d.dtype = {'f32': _lib.F32, 'bf16': _lib.BF16}[dtype]
        d.flags = _lib.FLAG_GENERIC if force_generic else 0
        self.desc = d
        self.handle = C.c_void_p()
        check(self.lib.dnnca_model_create(C.byref(d), C.byref(self.handle)))
        self.in_shape = (int(height), int(width), int(in_channels))
        self.max_batch = int(max_batch)
        n = C.c_int64()
        check(self.lib.dnnca_num_trainable(self.handle, C.byref(n)))
        self.n_trainable = n.value
        check(self.lib.dnnca_num_state(self.handle, C.byref(n)))
        self.n_state = n.value
        self._tm_n = 0
        self.n_members = 0

    # ---- life-cycle -------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, 'handle', None):
            self.lib.dnnca_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- variables --------------------------------------------------------------------------------------------
    def param_infos(self):
        """[(name, shape, trainable, offset)] in Keras creation order."""
        cnt = C.c_int()
        check(self.lib.dnnca_param_count(self.handle, C.byref(cnt)))
        out = []
        name = C.create_string_buffer(256)
        shape = (C.c_int64 * 4)()
        ndim, tr, off = C.c_int(), C.c_int(), C.c_int64()
        for i in range(cnt.value):
            check(self.lib.dnnca_param_info(self.handle, i, name, 256, shape, C.byref(ndim), C.byref(tr), C.byref(off)))
            out.append((name.value.decode(), tuple(shape[k] for k in range(ndim.value)), bool(tr.value), off.value))
        return out

    def _get(self, fn, n):
        out = np.empty(n, np.float32)
        check(fn(self.handle, fptr(out), n))
        return out

    def get_params(self):
        return self._get(self.lib.dnnca_get_params, self.n_trainable)

    def get_state(self):
        return self._get(self.lib.dnnca_get_state, self.n_state)

    def get_grads(self):
        return self._get(self.lib.dnnca_get_grads, self.n_trainable)

    def set_params(self, flat):
        flat = as_f32(flat).ravel()
        check(self.lib.dnnca_set_params(self.handle, fptr(flat), flat.size))

    def set_state(self, flat):
        flat = as_f32(flat).ravel()
        check(self.lib.dnnca_set_state(self.handle, fptr(flat), flat.size))

    def get_opt_state(self):
        m = np.empty(self.n_trainable, np.float32)
        v = np.empty(self.n_trainable, np.float32)
        it = C.c_int64()
        check(self.lib.dnnca_get_opt_state(self.handle, fptr(m), fptr(v), self.n_trainable, C.byref(it)))
        return m, v, it.value

    def set_opt_state(self, m, v, iterations):
        m, v = as_f32(m).ravel(), as_f32(v).ravel()
        check(self.lib.dnnca_set_opt_state(self.handle, fptr(m), fptr(v), m.size, int(iterations)))

    def set_adam(self, beta1=0.9, beta2=0.999, epsilon=1e-7):
        check(self.lib.dnnca_set_adam(self.handle, beta1, beta2, epsilon))

    # ---- configurable optimizers (dnnca_model_set_optimizer) -------------------------------------------------------
    OPTIMIZER_KINDS = {'adam': _lib.OPT_ADAM, 'adamw': _lib.OPT_ADAMW, 'sgd': _lib.OPT_SGD}

    def trainable_names(self):
        """the names of the trainable variables, in the order the per-variable arrays of the optimizer use"""
        return [name for name, _, trainable, _ in self.param_infos() if trainable]

    def decay_mask(self, exclude=('bias', 'beta', 'gamma')):
        """one flag per trainable variable: it takes AdamW's weight decay unless its name contains one of `exclude`"""
        return np.array([not any(e in name for e in exclude) for name in self.trainable_names()], np.uint8)

    def set_optimizer(self, kind='adam', beta1=0.9, beta2=0.999, epsilon=1e-7, momentum=0.0, nesterov=False, weight_decay=0.0,
                      clipvalue=0.0, clipnorm=0.0, global_clipnorm=0.0, decay_mask=None):
        """kind 'adam' | 'adamw' | 'sgd' with Keras' gradient transforms (0: off).  'adam' with nothing else stores the betas and
        epsilon and leaves the model launching what it launched before; anything else makes the train step run pg_fold
        [grad_sqnorm grad_clip_scale] opt_<kind>[_ema].  decay_mask: one flag per trainable variable ('adamw'; default decay_mask())"""
        cfg = _lib.OptimizerCfg()
        cfg.kind = self.OPTIMIZER_KINDS[kind]
        cfg.beta1, cfg.beta2, cfg.epsilon = float(beta1), float(beta2), float(epsilon)
        cfg.momentum, cfg.nesterov, cfg.weight_decay = float(momentum), int(bool(nesterov)), float(weight_decay)
        cfg.clipvalue, cfg.clipnorm, cfg.global_clipnorm = float(clipvalue), float(clipnorm), float(global_clipnorm)
        if decay_mask is None:
            decay_mask = self.decay_mask()
        mask = np.ascontiguousarray(decay_mask, np.uint8).ravel()
        check(self.lib.dnnca_model_set_optimizer(self.handle, C.byref(cfg), mask.ctypes.data_as(C.POINTER(C.c_uint8)), mask.size))

    def last_grad_norm(self):
        """(global norm, per-variable norms) of the gradient the last optimizer step received, after clipvalue: float64, accumulated
        in double on the device; needs clipnorm or global_clipnorm.  Waits for the stream"""
        n = len(self.trainable_names())
        total, per = C.c_double(), np.empty(n, np.float64)
        check(self.lib.dnnca_last_grad_norm(self.handle, C.byref(total), per.ctypes.data_as(C.POINTER(C.c_double)), n))
        return total.value, per

    def apply_gradients(self, g, lr):
        """Keras' optimizer.apply_gradients: the flat gradient vector g goes to the device and the optimizer's launches run on it
        (no all-reduce, scale 1); counts one iteration"""
        g = as_f32(g).ravel()
        check(self.lib.dnnca_apply_gradients(self.handle, fptr(g), g.size, float(lr)))

    # ---- gradient accumulation (dnnca_model_set_accumulation) -------------------------------------------------------
    def set_accumulation(self, steps):
        """steps 2..4096: every later train_step / apply_gradients is a micro-step that adds its gradient to a device-side float32
        accumulator, and every steps-th one applies the optimizer to their mean (one iteration, one weight-average update per
        cycle).  steps 1 drops it: the model runs the launches it ran before.  Discards a partial cycle; waits for the stream"""
        check(self.lib.dnnca_model_set_accumulation(self.handle, int(steps)))

    def get_accumulation(self):
        """(the accumulator as a flat float32 vector, steps, position): position micro-steps are in it; right after an update
        position is 0 and the vector is the sum that was applied.  Waits for the stream"""
        out = np.empty(self.n_trainable, np.float32)
        steps, pos = C.c_int(), C.c_int()
        check(self.lib.dnnca_get_accumulation(self.handle, fptr(out), self.n_trainable, C.byref(steps), C.byref(pos)))
        return out, steps.value, pos.value

    def grad_accumulate_of(self, acc, g, first):
        """the accumulation kernel alone on host vectors of any length: g when first, else acc + g (acc may be None when first)"""
        g = as_f32(g).ravel()
        out = np.empty(g.size, np.float32)
        if acc is not None:
            acc = as_f32(acc).ravel()
            if acc.size != g.size:
                raise ValueError('grad_accumulate_of: %d accumulator elements for %d gradient elements' % (acc.size, g.size))
        check(self.lib.dnnca_grad_accumulate_of(self.handle, fptr(acc) if acc is not None else None, fptr(g), g.size,
                                                int(bool(first)), fptr(out)))
        return out

    # ---- exponential moving average of the weights (dnnca_model_set_ema) ------------------------------------------
    def set_ema(self, decay, warmup=True):
        """decay in (0, 1): every later train step also moves a device-side average of the trainable variables towards the weights
        it has just written (tf.train.ExponentialMovingAverage, with num_updates warm-up unless warmup=False); the average starts
        as a copy of the weights.  decay 0 drops it: the model runs the launches it ran before"""
        check(self.lib.dnnca_model_set_ema(self.handle, float(decay), int(bool(warmup))))

    def get_ema(self):
        """(the average as a flat float32 vector, num_updates); while averaged_weights() is active: the raw weights"""
        out = np.empty(self.n_trainable, np.float32)
        n = C.c_int64()
        check(self.lib.dnnca_get_ema(self.handle, fptr(out), self.n_trainable, C.byref(n)))
        return out, n.value

    def set_ema_state(self, flat, num_updates):
        flat = as_f32(flat).ravel()
        check(self.lib.dnnca_set_ema_state(self.handle, fptr(flat), flat.size, int(num_updates)))

    def exchange_ema(self):
        """one launch on the model's stream that exchanges the contents of the weights and their average (exact; twice restores
        both).  Until the second call every forward / eval_step / analysis call runs on the average, get_params returns it, and
        train steps and set_params / set_opt_state are refused"""
        check(self.lib.dnnca_ema_exchange(self.handle))

    def averaged_weights(self):
        """context manager: exchange_ema() on entry, and always again on exit"""
        return _AveragedWeights(self)

    def named_params(self):
        """OrderedDict name -> ndarray (trainable and state variables)."""
        p, s = self.get_params(), self.get_state()
        out = OrderedDict()
        for name, shape, tr, off in self.param_infos():
            src = p if tr else s
            out[name] = src[off:off + int(np.prod(shape))].reshape(shape).copy()
        return out

    def init_glorot(self, seed=None):
        """Keras default initialisers: glorot_uniform kernels, zero biases (BN defaults are set by the library)."""
        rng = np.random.default_rng(seed)
        flat = self.get_params()
        for name, shape, tr, off in self.param_infos():
            if tr and name.endswith('.kernel'):
                kh, kw, a, b = shape
                limit = np.sqrt(6.0 / (kh * kw * (a + b)))
                flat[off:off + kh * kw * a * b] = rng.uniform(-limit, limit, kh * kw * a * b).astype(np.float32)
        self.set_params(flat)

    # ---- hot path ---------------------------------------------------------------------------------------------
    @staticmethod
    def loss_cfg(weight=None, weight_add=0.0, weight_mul=1.0, label_smoothing=False, label_smoothing_filter_size=6,
                 label_smoothing_sigma=3, **ignored):
        c = _lib.LossCfg()
        c.has_weight = 0 if weight is None else 1
        c.weight = 0.0 if weight is None else float(weight)
        c.weight_add, c.weight_mul = float(weight_add), float(weight_mul)
        c.label_smoothing = int(bool(label_smoothing))
        c.label_smoothing_filter_size, c.label_smoothing_sigma = int(label_smoothing_filter_size), float(label_smoothing_sigma)
        return c

    def _check_x(self, x):
        x = as_f32(x)
        if x.ndim != 4 or x.shape[1:] != self.in_shape:
            raise ValueError('x shape %s does not match the built input %s' % (x.shape, ('B',) + self.in_shape))
        if not 1 <= x.shape[0] <= self.max_batch:
            raise ValueError('batch %d outside [1, %d]' % (x.shape[0], self.max_batch))
        return x

    def forward(self, x, training=False, return_logits=False, return_prob=True):
        """return_prob=False: the probabilities stay on the device (for region_confusion* / render_composite); returns None"""
        x = self._check_x(x)
        B = x.shape[0]
        if not return_prob:
            check(self.lib.dnnca_forward(self.handle, fptr(x), B, int(training), None, None))
            return None
        prob = np.empty((B, self.in_shape[0], self.in_shape[1], 1), np.float32)
        logits = np.empty_like(prob) if return_logits else None
        check(self.lib.dnnca_forward(self.handle, fptr(x), B, int(training), fptr(prob),
                                     fptr(logits) if return_logits else None))
        return (prob, logits) if return_logits else prob

    def forward_tta(self, x, views, return_prob=True):
        """Test-time augmentation (dnnca_forward_tta): one inference forward per view of the bit mask `views` (tta.mask_of), the mean
        of the mapped-back probabilities in the model's probability buffer, where every consumer of the last forward reads it.
        return_prob=False: it stays on the device; returns None"""
        x = self._check_x(x)
        B = x.shape[0]
        prob = np.empty((B, self.in_shape[0], self.in_shape[1], 1), np.float32) if return_prob else None
        check(self.lib.dnnca_forward_tta(self.handle, fptr(x), B, int(views), fptr(prob) if return_prob else None))
        return prob

    def forward_tta_spread(self, x, views, return_prob=True, return_spread=True):
        """forward_tta that also keeps how much the views disagree (dnnca_forward_tta_spread): the probability buffer receives bit for
        bit forward_tta's mean, the model's spread plane the population standard deviation of the views per pixel (float32, in
        [0, 0.5]; 0 where all views agree).  The plane stays valid -- for lesion_table_spread / spread_by_outcome / last_spread --
        until the next call that rewrites the probabilities.  Returns (prob [B, H, W, 1] or None, spread [B, H, W] or None)"""
        x = self._check_x(x)
        B = x.shape[0]
        prob = np.empty((B, self.in_shape[0], self.in_shape[1], 1), np.float32) if return_prob else None
        spread = np.empty((B, self.in_shape[0], self.in_shape[1]), np.float32) if return_spread else None
        check(self.lib.dnnca_forward_tta_spread(self.handle, fptr(x), B, int(views), fptr(prob) if return_prob else None,
                                                fptr(spread) if return_spread else None))
        return prob, spread

    def last_spread(self, batch):
        """the spread plane [batch, H, W] of the last forward_tta_spread, or the total spread of the last forward_ensemble(spread=True)
        (an error once it is no longer valid)"""
        out = np.empty((int(batch), self.in_shape[0], self.in_shape[1]), np.float32)
        check(self.lib.dnnca_get_tta_spread(self.handle, int(batch), fptr(out)))
        return out

    # ---- ensembles (dnnca_model_set_members, dnnca_forward_ensemble) -------------------------------------------------
    MAX_MEMBERS = 16

    def set_members(self, members):
        """members: a list of up to 16 (params, state) pairs, the flat vectors of get_params / get_state (what a checkpoint holds);
        they live on the device inside this model until the next set_members.  An empty list frees them"""
        members = [(as_f32(p).ravel(), as_f32(s).ravel()) for p, s in members]
        check(self.lib.dnnca_model_set_members(self.handle, len(members)))
        for m, (p, s) in enumerate(members):
            check(self.lib.dnnca_member_store(self.handle, m, fptr(p), p.size, fptr(s) if s.size else None, s.size))
        self.n_members = len(members)

    def member(self, m):
        """(params, state) of member m as they are on the device"""
        p, s = np.empty(self.n_trainable, np.float32), np.empty(self.n_state, np.float32)
        check(self.lib.dnnca_member_get(self.handle, int(m), fptr(p), fptr(s) if s.size else None))
        return p, s

    def forward_ensemble(self, x, views=1, spread=False, return_prob=True):
        """One call per batch for all members (dnnca_forward_ensemble): for each member in turn its weights are copied in, the body of
        forward_tta (spread and more than one view: forward_tta_spread) runs on the staged batch -- views 1 is the plain forward --
        and ens_join takes the member in.  Afterwards the probability buffer holds the mean of the members' means and, with spread,
        the spread plane the total spread (last_spread; its two components: last_ensemble_spread); the model's own weights are back
        bit for bit.  return_prob=False: the mean stays on the device; returns None"""
        x = self._check_x(x)
        B = x.shape[0]
        prob = np.empty((B, self.in_shape[0], self.in_shape[1], 1), np.float32) if return_prob else None
        check(self.lib.dnnca_forward_ensemble(self.handle, fptr(x), B, int(views), int(bool(spread)), fptr(prob) if return_prob else None))
        return prob

    def last_ensemble_spread(self, batch):
        """(between, within) [batch, H, W] of the last forward_ensemble(spread=True): how much the members' means disagree and the
        root mean square of their own view spreads; last_spread's total is sqrt(between^2 + within^2)"""
        between = np.empty((int(batch), self.in_shape[0], self.in_shape[1]), np.float32)
        within = np.empty_like(between)
        check(self.lib.dnnca_get_ensemble_spread(self.handle, int(batch), fptr(between), fptr(within)))
        return between, within

    def ensemble_of(self, means, withins=None, spread=True):
        """ens_join alone on host planes means [n, B, h, w] (and the members' own spreads withins, same shape; None: zeros); none of
        the model's planes is touched.  Returns (mean, between, within, total) [B, h, w], or the mean alone with spread=False"""
        means = as_f32(means)
        if means.ndim != 4:
            raise ValueError('ensemble_of: means %s is not [n, B, h, w]' % (means.shape,))
        if withins is not None:
            withins = as_f32(withins)
            if withins.shape != means.shape:
                raise ValueError('ensemble_of: withins %s against means %s' % (withins.shape, means.shape))
        n, B, h, w = means.shape
        outs = [np.empty((B, h, w), np.float32) for _ in range(4 if spread else 1)]
        ptrs = [fptr(o) for o in outs] + [None] * (4 - len(outs))
        check(self.lib.dnnca_ensemble_of(self.handle, fptr(means), fptr(withins) if withins is not None else None, n, B, h, w, *ptrs))
        return tuple(outs) if spread else outs[0]

    def train_step(self, x, y, lr, cfg):
        x = self._check_x(x)
        y = as_f32(y)
        if y.shape != x.shape[:3]:
            raise ValueError('y shape %s does not match x %s' % (y.shape, x.shape))
        out = _lib.StepOut()
        check(self.lib.dnnca_train_step(self.handle, fptr(x), fptr(y), x.shape[0], float(lr), C.byref(cfg), C.byref(out)))
        return out

    def eval_step(self, x, y, cfg, return_prob=False):
        x = self._check_x(x)
        y = as_f32(y)
        if y.shape != x.shape[:3]:
            raise ValueError('y shape %s does not match x %s' % (y.shape, x.shape))
        out = _lib.StepOut()
        prob = np.empty(x.shape[:3] + (1,), np.float32) if return_prob else None
        check(self.lib.dnnca_eval_step(self.handle, fptr(x), fptr(y), x.shape[0], C.byref(cfg), C.byref(out),
                                       fptr(prob) if return_prob else None))
        return (out, prob) if return_prob else out

    def check_dev(self, xbuf, ybuf, batch):
        """Device-resident (x, y) that carry their shapes (DeviceBuffer, DeviceView) must match the built model: the staged and the
        *_dev entry points take bare pointers, a mismatched batch would be read as misaligned memory (the host entry points check in
        _check_x).  Raises ValueError like them."""
        xs, ys = getattr(xbuf, 'shape', None), getattr(ybuf, 'shape', None)
        if xs is None:
            return
        if len(xs) != 4 or tuple(xs[1:]) != self.in_shape:
            raise ValueError('x shape %s does not match the built input %s' % (tuple(xs), ('B',) + self.in_shape))
        if ys is not None and tuple(ys) != tuple(xs[:3]):
            raise ValueError('y shape %s does not match x %s' % (tuple(ys), tuple(xs)))
        if not 1 <= int(batch) <= min(int(xs[0]), self.max_batch):
            raise ValueError('batch %d outside [1, %d]' % (batch, min(int(xs[0]), self.max_batch)))

    def train_step_dev(self, xbuf, ybuf, batch, lr, cfg, want_out=False):
        self.check_dev(xbuf, ybuf, batch)
        out = _lib.StepOut() if want_out else None
        check(self.lib.dnnca_train_step_dev(self.handle, xbuf.ptr, ybuf.ptr, int(batch), float(lr), C.byref(cfg),
                                            C.byref(out) if want_out else None))
        return out

    # ---- per-step training metrics (Keras fit's compiled metrics, engine.py:273,286) ------------------------------
    def train_metrics(self, thresholds):
        """every later train step also counts its own probabilities (training=True forward pass, before the update) against its
        raw labels at these thresholds (any order, at most 1024); None or empty switches it off"""
        thr = threshold_vector(thresholds)
        check(self.lib.dnnca_train_metrics(self.handle, fptr(thr) if thr.size else None, int(thr.size)))
        self._tm_n = int(thr.size)

    def last_step_confusion(self):
        """[(tp, fp, fn, tn)] per threshold of train_metrics for the last train_step / train_step_dev (exact integers)"""
        return confusion_rows(self._tm_n, lambda out: check(self.lib.dnnca_last_step_confusion(self.handle, out)))

    def last_prob(self, batch):
        """the probability buffer [batch, H, W] (last forward / eval step, or a train step with train_metrics on)"""
        out = np.empty((int(batch), self.in_shape[0], self.in_shape[1]), np.float32)
        check(self.lib.dnnca_get_prob(self.handle, fptr(out), out.size))
        return out

    # ---- region (Tversky / Dice) term of the loss (losses.TverskyCrossentropy) ----------------------------------------
    def set_region_loss(self, cfg=None, **kw):
        """every later train / eval step adds region_weight * mean_b (1 - Tversky index of image b) to crossentropy_weight * the
        weighted cross-entropy (dnnca_model_set_region_loss).  cfg: a dict of region_weight, crossentropy_weight, alpha, beta,
        smooth (or the same as keywords; defaults 1, 1, 0.5, 0.5, 1); None with no keyword switches it off"""
        if cfg is None and not kw:
            check(self.lib.dnnca_model_set_region_loss(self.handle, None))
            return
        v = dict(region_weight=1.0, crossentropy_weight=1.0, alpha=0.5, beta=0.5, smooth=1.0)
        given = dict(cfg or {}, **kw)
        unknown = sorted(set(given) - set(v))
        if unknown:
            raise ValueError('set_region_loss: unknown keys %s' % unknown)
        v.update(given)
        c = _lib.RegionLoss(*(float(v[k]) for k in ('region_weight', 'crossentropy_weight', 'alpha', 'beta', 'smooth')))
        check(self.lib.dnnca_model_set_region_loss(self.handle, C.byref(c)))

    def region_loss_sums(self, batch=None):
        """[batch, 3] float64: I = sum p y, P = sum p, Y = sum y per image of the last step that ran with the region loss"""
        batch = self.max_batch if batch is None else int(batch)
        out = np.empty((batch, 3), np.float64)
        check(self.lib.dnnca_region_loss_sums(self.handle, batch, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    # ---- boundary (signed-distance) term of the loss (losses.BoundaryCrossentropy) --------------------------------------
    def set_boundary_loss(self, boundary_weight):
        """every later train / eval step adds boundary_weight * mean_b sum_i p_i phi_i / (H W), phi the signed Euclidean distance map
        of the step's raw labels (dnnca_model_set_boundary_loss).  Needs set_region_loss first (the term rides its launches); 0
        switches it off, and so does set_region_loss(None)"""
        check(self.lib.dnnca_model_set_boundary_loss(self.handle, float(boundary_weight)))

    def boundary_loss_sums(self, batch=None):
        """[batch] float64: S_b = sum_i p_i phi_i per image of the last step that ran with the boundary term"""
        batch = self.max_batch if batch is None else int(batch)
        out = np.empty(batch, np.float64)
        check(self.lib.dnnca_boundary_loss_sums(self.handle, batch, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def boundary_distance(self, batch=None):
        """[batch, H, W] float32: the signed distance map phi of the last step that ran with the boundary term"""
        batch = self.max_batch if batch is None else int(batch)
        out = np.empty((batch, self.in_shape[0], self.in_shape[1]), np.float32)
        check(self.lib.dnnca_boundary_distance(self.handle, batch, fptr(out)))
        return out

    def signed_distance_of(self, y, want_d2=False):
        """the signed distance map of label planes y [batch, h, w] of any size up to 16384 a side (batch within max_batch), by the
        kernels of the boundary term: phi float32 [batch, h, w], and with want_d2 (phi, d2): the exact squared distances, int32 (0
        where the other set is empty).  Touches nothing of the model"""
        y = np.ascontiguousarray(y, np.float32)
        if y.ndim != 3:
            raise ValueError('signed_distance_of: y must be [batch, h, w], got shape %s' % (y.shape,))
        phi = np.empty(y.shape, np.float32)
        d2 = np.empty(y.shape, np.int32) if want_d2 else None
        check(self.lib.dnnca_signed_distance_of(self.handle, fptr(y), y.shape[0], y.shape[1], y.shape[2], fptr(phi),
                                                d2.ctypes.data_as(C.POINTER(C.c_int32)) if want_d2 else None))
        return (phi, d2) if want_d2 else phi

    # ---- top-k (hard-pixel) cross-entropy (the key crossentropy_topk of losses.TverskyCrossentropy) ----------------------
    def set_topk_loss(self, fraction):
        """every later train / eval step takes the cross-entropy of an image over its k = max(1, ceil(fraction H W)) pixels of
        largest loss (and every tie of the k-th) in the place of all H W (dnnca_model_set_topk_loss).  Needs set_region_loss first
        (with crossentropy_weight > 0: the term rides its launches); 0 switches it off, and so does set_region_loss(None)"""
        check(self.lib.dnnca_model_set_topk_loss(self.handle, float(fraction)))

    def topk_loss_state(self, batch=None):
        """(k int32, n_kept int32, tau float32, sum float64), [batch] each: per image of the last step that ran with the top-k loss
        the k asked for, the pixels kept (those with a loss >= tau), the threshold and the sum of the kept losses"""
        batch = self.max_batch if batch is None else int(batch)
        k, n = np.empty(batch, np.int32), np.empty(batch, np.int32)
        tau, s = np.empty(batch, np.float32), np.empty(batch, np.float64)
        i32 = C.POINTER(C.c_int32)
        check(self.lib.dnnca_topk_loss_state(self.handle, batch, k.ctypes.data_as(i32), n.ctypes.data_as(i32), fptr(tau),
                                             s.ctypes.data_as(C.POINTER(C.c_double))))
        return k, n, tau, s

    def topk_pixel_loss(self, batch=None):
        """[batch, H, W] float32: the per-pixel weighted cross-entropy of the last step that ran with the top-k loss"""
        batch = self.max_batch if batch is None else int(batch)
        out = np.empty((batch, self.in_shape[0], self.in_shape[1]), np.float32)
        check(self.lib.dnnca_topk_pixel_loss(self.handle, batch, fptr(out)))
        return out

    def topk_select_of(self, v, k):
        """(tau float32 [batch], n_kept int32 [batch]): the k-th largest value of every plane of v [batch, hw] (non-negative floats,
        batch within max_batch) and the count of the values >= it, by the selection kernels of the top-k loss.  Touches nothing of
        the model"""
        v = np.ascontiguousarray(v, np.float32)
        if v.ndim != 2:
            raise ValueError('topk_select_of: v must be [batch, hw], got shape %s' % (v.shape,))
        tau, n = np.empty(v.shape[0], np.float32), np.empty(v.shape[0], np.int32)
        check(self.lib.dnnca_topk_select_of(self.handle, fptr(v), v.shape[0], v.shape[1], int(k), fptr(tau),
                                            n.ctypes.data_as(C.POINTER(C.c_int32))))
        return tau, n

    def last_step_out(self):
        out = _lib.StepOut()
        check(self.lib.dnnca_last_step_out(self.handle, C.byref(out)))
        return out

    def sync(self):
        check(self.lib.dnnca_sync(self.handle))

    def staging(self, slots=StagingRing.MAX_SLOTS, slot_bytes=0):
        """the model's StagingRing (created on first use; one per model)"""
        if getattr(self, '_ring', None) is None:
            self._ring = StagingRing(self, slots, slot_bytes)
        return self._ring

    def pixel_confusion(self, y, thresholds):
        y, thr = as_f32(y), threshold_vector(thresholds)
        return confusion_rows(thr.size, lambda out: check(
            self.lib.dnnca_pixel_confusion(self.handle, fptr(y), y.shape[0], fptr(thr), thr.size, out)))

    def pixel_confusion_of(self, prob, y, thresholds):
        """Metric.update_state(y_true, y_pred) on caller-supplied probabilities: [(tp, fp, fn, tn)] per threshold (exact)."""
        prob, y = as_f32(prob).ravel(), as_f32(y).ravel()
        if prob.size != y.size:
            raise ValueError('prob and y differ in size: %d vs %d' % (prob.size, y.size))
        thr = threshold_vector(thresholds)
        return confusion_rows(thr.size, lambda out: check(
            self.lib.dnnca_pixel_confusion_of(self.handle, fptr(prob), fptr(y), prob.size, fptr(thr), thr.size, out)))

    def region_confusion(self, y, spec):
        """region counts of the last forward / eval probabilities against y [B, H, W]: int64 [T, 4] (tp_label, fn, tp_pred, fp).
        spec: (thresholds, iou_threshold, resize_factor, morph_filter_size)"""
        y = as_f32(y)
        arr, keep = region_specs([spec])
        out = (_lib.RegionCounts * keep[0].size)()
        check(self.lib.dnnca_region_confusion(self.handle, fptr(y), y.shape[0], arr, out))
        return split_region_counts(out, [keep[0].size])[0]

    def region_confusion_of(self, prob, y, spec):
        """region counts of caller-supplied probabilities and labels [B, h, w] (any size): int64 [T, 4]"""
        prob, y = as_f32(prob), as_f32(y)
        if prob.ndim == 4:
            prob = prob[..., 0]
        if prob.shape != y.shape or prob.ndim != 3:
            raise ValueError('prob %s and y %s must both be [B, h, w]' % (prob.shape, y.shape))
        arr, keep = region_specs([spec])
        out = (_lib.RegionCounts * keep[0].size)()
        B, h, w = y.shape
        check(self.lib.dnnca_region_confusion_of(self.handle, fptr(np.ascontiguousarray(prob)), fptr(y), B, h, w, arr, out))
        return split_region_counts(out, [keep[0].size])[0]

    # ---- the Visualizer of `annotator evaluate` (casewise.py) ---------------------------------------------------
    def region_confusion_slices(self, y, specs, prob=None):
        """per-slice region counts of the last forward's probabilities (or of `prob` [B, H, W(, 1)], host) against y [B, H, W]:
        int64 [B, T, 4] (tp_label, fn, tp_pred, fp), T = all thresholds of `specs` in order.  A spec of more than 64 thresholds runs as several device specs (one label
        labelling for all of them).  The labels stay on the device for render_composite(None, ...)."""
        y = as_f32(y)
        if y.ndim != 3:
            raise ValueError('y must be [B, H, W], got %s' % (y.shape,))
        if prob is not None:
            prob = as_f32(prob)
            if prob.size != y.size:
                raise ValueError('prob %s and y %s differ in size' % (prob.shape, y.shape))
        pieces = []
        for thr, iou, rf, k in specs:
            thr = threshold_vector(thr)
            n = -(-thr.size // 64)
            pieces += [(part, iou, rf, k) for part in np.array_split(thr, n)] if n > 1 else [(thr, iou, rf, k)]
        arr, keep = region_specs(pieces)
        T = sum(k.size for k in keep)
        out = (_lib.RegionCounts * (y.shape[0] * T))()
        check(self.lib.dnnca_region_confusion_slices(self.handle, None if prob is None else fptr(prob), fptr(y), y.shape[0], arr,
                                                     len(pieces), out))
        return split_region_counts(out, [y.shape[0] * T])[0].reshape(y.shape[0], T, 4)

    def render_composite(self, y, batch, ratio=0.5, overlay=False):
        """the Visualizer's composite of the last forward's `batch` slices: uint8 [batch, oh, ow, 1 or 3] (input features | label |
        probability, resized by `ratio`).  y [batch, H, W], or None: the labels of the region_confusion_slices call just before."""
        hwc = (C.c_int32 * 3)()
        ya = None if y is None else as_f32(y)
        yp = None if ya is None else fptr(ya)
        check(self.lib.dnnca_render_composite(self.handle, yp, int(batch), float(ratio), int(bool(overlay)), None, 0, hwc))
        out = np.empty((int(batch), hwc[0], hwc[1], hwc[2]), np.uint8)
        check(self.lib.dnnca_render_composite(self.handle, yp, int(batch), float(ratio), int(bool(overlay)),
                                              out.ctypes.data_as(C.c_void_p), out.nbytes, hwc))
        return out

    # ---- mask refinement of the lesion tables and the boundary distances (kernels_refine.hip) --------------------
    def set_lesion_refine(self, hysteresis=None, closing=0, fill_holes=False):
        """every later lesion_table*, lesion_table_matched (its prediction side) and surface_distances call refines the prediction
        mask on the analysed plane (dnnca_model_set_lesion_refine): hysteresis (a low threshold in (0, 1) below the call's own: the
        4-connected regions at `hysteresis` that hold a pixel at the threshold), then the opening, a closing x closing closing (odd, 3
        .. 15; 0 or 1: none), then hole filling.  No argument switches it off.  Changing the configuration ends the chains of
        lesion_table_linked and lesion_table_matched"""
        c = _lib.LesionRefine(0.0 if hysteresis is None else float(hysteresis), int(closing), int(fill_holes))
        check(self.lib.dnnca_model_set_lesion_refine(self.handle, C.byref(c)))

    def lesion_refine(self):
        """(hysteresis or None, closing, fill_holes) as set_lesion_refine last set them"""
        c = _lib.LesionRefine()
        check(self.lib.dnnca_model_get_lesion_refine(self.handle, C.byref(c)))
        return (float(c.hysteresis_low) if c.hysteresis_low != 0.0 else None, int(c.closing_size), bool(c.fill_holes))

    # ---- `annotator predict` (kernels_region.hip: lesion_scan / lesion_stats / lesion_mask) ---------------------
    def lesion_table(self, batch=None, prob=None, threshold=0.5, resize_factor=1.0, filter_size=5, min_area=0, max_lesions=256,
                     mask=True):
        """the lesions of the last forward's `batch` slices, or of `prob` [B, h, w(, 1)] (host, any size): (rows, totals, masks).
        Per slice: resize by resize_factor, >= threshold, filter_size x filter_size opening (1: none), 4-connected components of at
        least min_area pixels, numbered in raster order of their first pixel.  rows: structured array (_lib.LESION_ROW_DTYPE: slice,
        row, area, x0, y0, x1, y1 inclusive, max_prob, sum_x, sum_y, sum_prob_q24), slice after slice, at most max_lesions per
        slice; totals int32 [B]: the kept components of every slice (> max_lesions: its rows are truncated); masks uint8
        [B, oh, ow], 255 on every kept component (None with mask=False).  Exact integers: bit-identical from run to run."""
        return self._lesion_call(batch, prob, None, threshold, resize_factor, filter_size, min_area, max_lesions, mask)

    def lesion_table_spread(self, batch=None, prob=None, spread=None, threshold=0.5, resize_factor=1.0, filter_size=5, min_area=0,
                            max_lesions=256, mask=True):
        """lesion_table plus the spread of the test-time-augmentation views under it: (rows, totals, masks, srows, stotals); the first
        three are what lesion_table returns.  The spread is that of the last forward_tta_spread (batch=...), or `spread` [B, h, w]
        beside `prob` (both host planes, or neither).  srows: structured array (_lib.LESION_SPREAD_DTYPE: slice, row, area,
        max_spread, sum_spread_q24), srows[i] belongs to rows[i] (mean = sum / area / 2^24); stotals (_lib.SLICE_SPREAD_DTYPE:
        pixels, max_spread, sum_spread_q24) [B]: every pixel of the analysed plane of a slice.  Exact integers and extrema."""
        if (prob is None) != (spread is None):
            raise ValueError('lesion_table_spread: prob and spread go together (both host planes, or neither)')
        if spread is not None:
            spread, prob = _slices(spread, 'spread'), _slices(prob, 'prob')
            if spread.shape != prob.shape:
                raise ValueError('spread %s and prob %s differ in shape' % (spread.shape, prob.shape))
        return self._lesion_call(batch, prob, None, threshold, resize_factor, filter_size, min_area, max_lesions, mask, spread=spread,
                                 with_spread=True)

    def lesion_table_features(self, batch=None, prob=None, x=None, threshold=0.5, resize_factor=1.0, filter_size=5, min_area=0,
                              max_lesions=256, mask=True, bins=32, ring=3):
        """lesion_table plus what every lesion looks like in the input channels: (rows, totals, masks, shape, body, ring, hist); the
        first three are what lesion_table returns.  The channels are the staged batch of the last forward (batch=...; under
        forward_tta the untransformed batch), or `x` [B, h, w, C] beside `prob` (both host planes, or neither).  A value is x read
        through the resize of the probabilities, clamped to [0, 1] (NaN: 0), and enters the sums as q = rint(v * 2^16).
        shape (_lib.LESION_SHAPE_DTYPE: slice, row, area, boundary, edges, sum_xx, sum_yy, sum_xy) [n]; body and ring
        (_lib.LESION_INTENSITY_DTYPE: slice, row, channel, n, min, max, sum_q16, sum_sq_q16) [n, C]: the lesion's own pixels, and
        the background pixels within `ring` pixels (a square window) that are nearer to no lesion of a lower row -- ring=0: None;
        hist uint32 [n, C, bins]: the body's values by bin min(bins - 1, floor(v * bins)) -- bins=0: None.  casewise.feature_* turn
        the integers into means, deviations, percentiles and axes.  Exact integers and extrema: bit-identical from run to run."""
        if (prob is None) != (x is None):
            raise ValueError('lesion_table_features: prob and x go together (both host planes, or neither)')
        if x is not None:
            x, prob = as_f32(x), _slices(prob, 'prob')
            if x.ndim != 4 or x.shape[:3] != prob.shape:
                raise ValueError('x %s must be [B, h, w, C] beside prob %s' % (x.shape, prob.shape))
        return self._lesion_call(batch, prob, None, threshold, resize_factor, filter_size, min_area, max_lesions, mask,
                                 features=(x, int(bins), int(ring)))

    def spread_by_outcome(self, y, thresholds=(0.5,), batch=None, prob=None, spread=None):
        """pixels and spread per pixel outcome (dnnca_spread_by_outcome): structured array (_lib.SPREAD_OUTCOME_DTYPE: n [4],
        sum_q24 [4]) [T, B] over the classes TN, FP, FN, TP = 2 (y > 0.5) + (prob >= threshold).  y [B, h, w]; the probabilities
        and the spread are those of the last forward_tta_spread, or the host planes `prob` and `spread` [B, h, w] (both or neither).
        At most 64 thresholds.  Exact integers."""
        y = _labels(y, batch)
        if (prob is None) != (spread is None):
            raise ValueError('spread_by_outcome: prob and spread go together (both host planes, or neither)')
        B, h, w = y.shape
        pp = sp = None
        if prob is not None:
            prob, spread = _host_prob(prob, y, False), _host_prob(spread, y, False)
            pp, sp = fptr(prob), fptr(spread)
        thr = threshold_vector(thresholds)
        out = np.zeros((thr.size, B), _lib.SPREAD_OUTCOME_DTYPE)
        check(self.lib.dnnca_spread_by_outcome(self.handle, pp, sp, fptr(y), B, h if pp is not None else 0, w if pp is not None else 0,
                                               fptr(thr), thr.size, out.ctypes.data_as(C.POINTER(_lib.SpreadOutcome))))
        return out

    # ---- `evaluate --calibration`, `--temperature` (kernels_calib.hip) ---------------------------------------------
    def calibration(self, y, n_bins=15, temperatures=(), batch=None, prob=None):
        """the reliability table of the probabilities against the labels y [B, h, w] (dnnca_calibration): (bins, totals, nll).  bins:
        structured array (_lib.CALIB_BIN_DTYPE: n [2], sum_q24 [2] per class 0 / 1 = y > 0.5) [B, n_bins], bin k = min(n_bins - 1,
        floor(p * n_bins)) of the probability clamped to [0, 1]; totals (_lib.CALIB_TOTAL_DTYPE: n, sum_q24, sq_lo, sq_hi) [B] with
        sum q^2 = sq_hi * 2^32 + sq_lo; nll float64 [B, T]: the negative log-likelihood summed over the slice at every one of
        `temperatures` (at most 64, each in [0.05, 20]; none: an empty array and no NLL launch).  The probabilities are those of the
        last forward / forward_tta, or the host plane `prob` [B, h, w].  casewise.calibration_* turn the integers into ECE, MCE and
        Brier score.  The tables are exact integers; everything is bit-identical from run to run."""
        y = _labels(y, batch)
        B, h, w = y.shape
        pp = None
        if prob is not None:
            prob = _host_prob(prob, y, False)
            pp = fptr(prob)
        temps = np.ascontiguousarray(np.asarray(temperatures, np.float32).reshape(-1))
        bins = np.zeros((B, int(n_bins)), _lib.CALIB_BIN_DTYPE)
        totals = np.zeros(B, _lib.CALIB_TOTAL_DTYPE)
        nll = np.zeros((B, temps.size), np.float64)
        check(self.lib.dnnca_calibration(self.handle, pp, fptr(y), B, h if pp is not None else 0, w if pp is not None else 0, int(n_bins),
                                         fptr(temps) if temps.size else None, int(temps.size),
                                         bins.ctypes.data_as(C.POINTER(_lib.CalibBin)), totals.ctypes.data_as(C.POINTER(_lib.CalibTotal)),
                                         nll.ctypes.data_as(C.POINTER(C.c_double)) if temps.size else None))
        return bins, totals, nll

    def scale_temperature(self, temperature, batch, prob=None):
        """temperature scaling (dnnca_prob_temperature): p -> sigmoid(logit(p) / temperature), in double, rounded once.  Without
        `prob` the model's probability buffer is scaled in place for the last forward's `batch` slices -- every consumer that reads
        it afterwards sees the calibrated values; call it ONCE per forward, a second call scales again -- and None is returned.
        With a host plane `prob` [B, h, w] the scaled plane is returned and the model's buffer stays untouched."""
        if prob is None:
            check(self.lib.dnnca_prob_temperature(self.handle, None, int(batch), 0, 0, float(temperature), None))
            return None
        prob = _slices(prob, 'prob')
        if batch is not None and int(batch) != prob.shape[0]:
            raise ValueError('prob must be [B, h, w] of batch slices, got %s' % (prob.shape,))
        out = np.empty_like(prob)
        check(self.lib.dnnca_prob_temperature(self.handle, fptr(prob), prob.shape[0], prob.shape[1], prob.shape[2], float(temperature),
                                              fptr(out)))
        return out

    def _detection(self, prob, batch, min_confidence=0.1, factor=0.4, max_candidates=5, min_area=10, rounds=16):
        cfg = _lib.DetectionCfg(float(min_confidence), float(factor), int(max_candidates), int(min_area), int(rounds))
        B = int(batch) if prob is None else prob.shape[0]
        rows = np.zeros(max(B, 0) * min(max(int(max_candidates), 0), 64), _lib.DETECTION_ROW_DTYPE)
        slices = np.zeros(max(B, 0), _lib.DETECTION_SLICE_DTYPE)
        n_rows = C.c_int64(0)
        out = None if prob is None else np.empty_like(prob)
        h, w = (0, 0) if prob is None else prob.shape[1:]
        check(self.lib.dnnca_detection_map(self.handle, None if prob is None else fptr(prob), B, h, w, C.byref(cfg),
                                           None if out is None else fptr(out), rows.ctypes.data_as(C.POINTER(_lib.DetectionRow)),
                                           C.byref(n_rows), slices.ctypes.data_as(C.POINTER(_lib.DetectionSlice))))
        return out, rows[:n_rows.value].copy(), slices

    def detection_map(self, batch, **cfg):
        """the detection map of the last forward's `batch` slices (dnnca_detection_map), IN PLACE: the model's probability buffer is
        replaced by the map D (a candidate's confidence on every one of its pixels, 0 elsewhere), so every later consumer of "the last
        forward" reads D.  Returns (rows, slices): rows a structured array (_lib.DETECTION_ROW_DTYPE: slice, number, seed, area,
        confidence) sorted by (slice, number), slices (_lib.DETECTION_SLICE_DTYPE: candidates, rounds, dropped, exhausted) [batch].
        cfg: min_confidence 0.1, factor 0.4, max_candidates 5, min_area 10, rounds 16.  Everything is bit-identical from run to run."""
        _, rows, slices = self._detection(None, batch, **cfg)
        return rows, slices

    def detection_map_of(self, prob, **cfg):
        """the same of a host plane `prob` [B, h, w] of any size: (D, rows, slices); the model's buffer stays untouched."""
        return self._detection(_slices(prob, 'prob'), None, **cfg)

    # ---- `evaluate --bootstrap` (kernels_bootstrap.hip) ---------------------------------------------------------
    @staticmethod
    def _bootstrap_resampling(E, strata):
        """(pool, sizes) int32 from `strata`: None (plain: the identity, one stratum) or what casewise.bootstrap_pool returned"""
        if strata is None:
            return np.arange(E, dtype=np.int32), np.array([E], np.int32)
        pool, sizes = strata
        return np.ascontiguousarray(pool, np.int32).reshape(-1), np.ascontiguousarray(sizes, np.int32).reshape(-1)

    def bootstrap_sums(self, cols, replicates, seed=0, strata=None, multiplicities=False):
        """R = `replicates` bootstrap resamples of the E rows of cols [E, K] (integers that fit int32, K <= 64), drawn with
        replacement by the definition of include/dnnca.h (Philox4x32-10 keyed by `seed`; within the strata of `strata` = (pool,
        sizes), casewise.bootstrap_pool, when given): a structured array [R] with 'sums' int64 [K], sums[r][k] = sum_e m_r[e]
        cols[e][k], exact, and with `multiplicities` also 'multiplicities' uint16 [E], the m_r themselves.  The draws depend on
        (seed, E, strata) alone.  Bit-identical from run to run; touches nothing of the model"""
        cols = np.ascontiguousarray(cols, np.int32)
        if cols.ndim != 2:
            raise ValueError('bootstrap_sums: cols must be [E, K], got shape %s' % (cols.shape,))
        E, K = cols.shape
        R = int(replicates)
        pool, sizes = self._bootstrap_resampling(E, strata)
        out = np.zeros(max(R, 0), [('sums', '<i8', (K,))] + ([('multiplicities', '<u2', (E,))] if multiplicities else []))
        sums = np.zeros((max(R, 0), K), np.int64)
        mult = np.zeros((max(R, 0), E), np.uint16) if multiplicities else None
        i32 = C.POINTER(C.c_int32)
        check(self.lib.dnnca_bootstrap_sums(self.handle, cols.ctypes.data_as(i32), E, K, pool.ctypes.data_as(i32), sizes.ctypes.data_as(i32),
                                            sizes.size, R, int(seed), sums.ctypes.data_as(C.POINTER(C.c_int64)),
                                            mult.ctypes.data_as(C.POINTER(C.c_uint16)) if multiplicities else None))
        out['sums'] = sums
        if multiplicities:
            out['multiplicities'] = mult
        return out

    def bootstrap_detection(self, exams, candidates, replicates, seed=0, strata=None, multiplicities=False):
        """R = `replicates` bootstrap resamples of the exams of a detection pass: exams (_lib.BOOTSTRAP_EXAM_DTYPE) [E] and
        candidates (_lib.BOOTSTRAP_CANDIDATE_DTYPE) [N] as casewise.detection_bootstrap_inputs makes them; seed, strata and
        multiplicities as in bootstrap_sums.  Returns a structured array [R] (_lib.BOOTSTRAP_DETECTION_ROW_DTYPE: positive_exams,
        tumours, candidates, tp, fp, auroc_pairs, auroc_twice, tp_at [7], ap), with `multiplicities` plus 'multiplicities' uint16 [E].
        casewise.detection_replicate_values turns a row into AP, AUROC, the sensitivities and CPM.  Bit-identical from run to run"""
        exams = np.ascontiguousarray(exams, _lib.BOOTSTRAP_EXAM_DTYPE).reshape(-1)
        cands = np.ascontiguousarray(candidates, _lib.BOOTSTRAP_CANDIDATE_DTYPE).reshape(-1)
        E, R = exams.size, int(replicates)
        pool, sizes = self._bootstrap_resampling(E, strata)
        rows = np.zeros(max(R, 0), _lib.BOOTSTRAP_DETECTION_ROW_DTYPE)
        mult = np.zeros((max(R, 0), E), np.uint16) if multiplicities else None
        i32 = C.POINTER(C.c_int32)
        check(self.lib.dnnca_bootstrap_detection(self.handle, exams.ctypes.data_as(C.POINTER(_lib.BootstrapExam)), E,
                                                 cands.ctypes.data_as(C.POINTER(_lib.BootstrapCandidate)), cands.size,
                                                 pool.ctypes.data_as(i32), sizes.ctypes.data_as(i32), sizes.size, R, int(seed),
                                                 rows.ctypes.data_as(C.POINTER(_lib.BootstrapDetectionRow)),
                                                 mult.ctypes.data_as(C.POINTER(C.c_uint16)) if multiplicities else None))
        if not multiplicities:
            return rows
        out = np.zeros(rows.size, _lib.BOOTSTRAP_DETECTION_ROW_DTYPE.descr + [('multiplicities', '<u2', (E,))])
        for name in rows.dtype.names:
            out[name] = rows[name]
        out['multiplicities'] = mult
        return out

    def lesion_table_linked(self, batch=None, prob=None, continues=None, threshold=0.5, resize_factor=1.0, filter_size=5, min_area=0,
                            max_lesions=256, mask=True):
        """lesion_table plus the links between neighbouring slices: (rows, totals, masks, links); the first three are what
        lesion_table returns.  continues [B] (bool): slice b is the next slice of the exam of slice b - 1; continues[0] refers to the
        last slice of the previous lesion_table_linked call on this model (an error when there was none, or one on planes of
        another size).  links: structured array (_lib.LESION_LINK_DTYPE: slice, row_prev, row, overlap), one entry per pair of a
        lesion of slice - 1 (row_prev) and a lesion of slice (row) that share `overlap` pixels, sorted by (slice, row_prev, row);
        lesions beyond max_lesions link to nothing."""
        if continues is None:
            raise ValueError('lesion_table_linked needs `continues`, one flag per slice')
        return self._lesion_call(batch, prob, continues, threshold, resize_factor, filter_size, min_area, max_lesions, mask)

    def _lesion_call(self, batch, prob, continues, threshold, resize_factor, filter_size, min_area, max_lesions, mask, spread=None,
                     with_spread=False, features=None):
        """dnnca_lesion_table, with `continues` dnnca_lesion_table_linked, with_spread dnnca_lesion_table_spread, with features (x or
        None, bins, ring) dnnca_lesion_table_features: the size query, then the call on buffers of that size"""
        pp, h, w = None, 0, 0
        if prob is not None:
            prob = _slices(prob, 'prob')
            if batch is not None and int(batch) != prob.shape[0]:
                raise ValueError('batch %d but prob holds %d slices' % (batch, prob.shape[0]))
            (batch, h, w), pp = prob.shape, fptr(prob)
        elif batch is None:
            raise ValueError('lesion_table needs `batch` (the slices of the last forward) or `prob`')
        B = int(batch)
        args = (self.handle, pp, B, int(h), int(w), float(threshold), float(resize_factor), int(filter_size), int(min_area),
                int(max_lesions))
        hw, oh, ow = _analysed_plane(lambda hw: self.lib.dnnca_lesion_table(*args, None, 0, None, None, None, 0, hw))
        rows, totals, links, masks = _lesion_table_buffers(B, oh, ow, max_lesions, mask, links=continues is not None)
        n = C.c_int64()
        out = (rows.ctypes.data_as(C.POINTER(_lib.LesionRow)), len(rows), C.byref(n), totals.ctypes.data_as(C.POINTER(C.c_int32)),
               masks.ctypes.data_as(C.c_void_p) if mask else None, masks.nbytes if mask else 0, hw)
        if features is not None:
            x, bins, ring = features
            ch = self.in_shape[2] if x is None else x.shape[3]
            shape = np.zeros(len(rows), _lib.LESION_SHAPE_DTYPE)
            body = np.zeros((len(rows), ch), _lib.LESION_INTENSITY_DTYPE)
            rng = np.zeros((len(rows), ch), _lib.LESION_INTENSITY_DTYPE) if ring > 0 else None
            hist = np.zeros((len(rows), ch, bins), np.uint32) if bins > 0 else None
            rec = C.POINTER(_lib.LesionIntensity)
            check(self.lib.dnnca_lesion_table_features(*args, *out, None if x is None else fptr(x), int(ch), bins, ring,
                                                       shape.ctypes.data_as(C.POINTER(_lib.LesionShape)), body.ctypes.data_as(rec),
                                                       None if rng is None else rng.ctypes.data_as(rec),
                                                       None if hist is None else hist.ctypes.data_as(C.POINTER(C.c_uint32))))
            cut = lambda a: None if a is None else a[:n.value].copy()
            return rows[:n.value].copy(), totals, masks, cut(shape), cut(body), cut(rng), cut(hist)
        if with_spread:
            srows = np.zeros(len(rows), _lib.LESION_SPREAD_DTYPE)
            stotals = np.zeros(B, _lib.SLICE_SPREAD_DTYPE)
            check(self.lib.dnnca_lesion_table_spread(*args, *out, None if spread is None else fptr(spread),
                                                     srows.ctypes.data_as(C.POINTER(_lib.LesionSpread)),
                                                     stotals.ctypes.data_as(C.POINTER(_lib.SliceSpread))))
            return rows[:n.value].copy(), totals, masks, srows[:n.value].copy(), stotals
        if continues is None:
            check(self.lib.dnnca_lesion_table(*args, *out))
            return rows[:n.value].copy(), totals, masks
        flags = _continues(continues, B)
        nl = C.c_int64()
        check(self.lib.dnnca_lesion_table_linked(*args, *out, flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                 links.ctypes.data_as(C.POINTER(_lib.LesionLink)), len(links), C.byref(nl)))
        return rows[:n.value].copy(), totals, masks, links[:nl.value].copy()

    def lesion_table_matched(self, y, batch=None, prob=None, continues=None, threshold=0.5, resize_factor=1.0, filter_size=5,
                             min_area=0, max_lesions=256, mask=False):
        """lesion_table_linked on the probabilities, the same on the labels `y` [B, h, w(, 1)] (y' > 0.5, no opening, no area
        filter, the same max_lesions) and the common pixels of labelled and predicted lesions, in one call:
        (rows, totals, masks, links, true_rows, true_totals, true_links, pairs).  The first four are what lesion_table_linked
        returns, the next three what it returns for `y` in the place of the probabilities.  pairs: structured array
        (_lib.LESION_PAIR_DTYPE: slice, row_true, row, overlap), one entry per labelled lesion (row_true) and predicted lesion (row)
        of one slice that share `overlap` pixels, sorted by (slice, row_true, row).  continues[0] refers to the last slice of the
        previous lesion_table_matched call on this model; the chain of lesion_table_linked is a separate one."""
        if continues is None:
            raise ValueError('lesion_table_matched needs `continues`, one flag per slice')
        y = _labels(y, batch)
        if prob is not None:
            prob = _host_prob(prob, y, True)
        B, h, w = y.shape                # without `prob` the library holds h and w against the size of the last forward
        flags = _continues(continues, B)
        args = (self.handle, None if prob is None else fptr(prob), fptr(y), B, h, w, float(threshold), float(resize_factor),
                int(filter_size), int(min_area), int(max_lesions), flags.ctypes.data_as(C.POINTER(C.c_uint8)))
        hw, oh, ow = _analysed_plane(lambda hw: self.lib.dnnca_lesion_table_matched(*args, None, None, 0, None, None, hw))

        def plane(mask):
            rows, totals, links, masks = _lesion_table_buffers(B, oh, ow, max_lesions, mask, links=True)
            out = _lib.LesionPlaneOut(rows.ctypes.data_as(C.POINTER(_lib.LesionRow)), len(rows), 0,
                                      totals.ctypes.data_as(C.POINTER(C.c_int32)), links.ctypes.data_as(C.POINTER(_lib.LesionLink)),
                                      len(links), 0)
            return rows, totals, links, masks, out
        rows, totals, links, masks, pred = plane(mask)
        true_rows, true_totals, true_links, _, truth = plane(False)
        pairs = np.zeros(len(links), _lib.LESION_PAIR_DTYPE)
        po = _lib.LesionPairsOut(pairs.ctypes.data_as(C.POINTER(_lib.LesionPair)), len(pairs), 0)
        check(self.lib.dnnca_lesion_table_matched(*args, C.byref(pred), masks.ctypes.data_as(C.c_void_p) if mask else None,
                                                  masks.nbytes if mask else 0, C.byref(truth), C.byref(po), hw))
        return (rows[:pred.n_rows].copy(), totals, masks, links[:pred.n_links].copy(), true_rows[:truth.n_rows].copy(), true_totals,
                true_links[:truth.n_links].copy(), pairs[:po.n_pairs].copy())

    def surface_distances(self, y, batch=None, prob=None, threshold=0.5, resize_factor=1.0, filter_size=5, min_area=0,
                          max_samples=65536, edges=False):
        """the squared distances between the outline of the prediction mask (side 0: lesion_table's mask for the same arguments) and
        the outline of the label foreground (side 1: y' > 0.5 of `y` [B, h, w(, 1)]), of the last forward's `batch` slices or of
        `prob`: (counts, samples, edges).  counts int32 [B, 5]: area_pred, area_true, common, edge_pred, edge_true.  samples:
        structured array (_lib.SURFACE_SAMPLE_DTYPE: slice, side, pixel = y * ow + x, d2), one entry per boundary pixel of either
        side with the exact squared distance to the nearest boundary pixel of the other side, sorted by (slice, side, pixel); a
        slice with an empty outline or more than max_samples boundary pixels on a side gives none.  edges: uint8 [B, oh, ow], bit 0
        on the prediction's boundary, bit 1 on the label's (None with edges=False)."""
        y = _labels(y, batch)
        if prob is not None:
            prob = _host_prob(prob, y, True)
        B, h, w = y.shape                # without `prob` the library holds h and w against the size of the last forward
        args = (self.handle, None if prob is None else fptr(prob), fptr(y), B, h, w, float(threshold), float(resize_factor),
                int(filter_size), int(min_area), int(max_samples))
        hw, oh, ow = _analysed_plane(lambda hw: self.lib.dnnca_surface_distances(*args, None, None, 0, None, None, 0, hw))
        cap = B * 2 * min(int(max_samples), oh * ow)
        counts = np.zeros((B, 5), np.int32)
        samples = np.zeros(max(cap, 0), _lib.SURFACE_SAMPLE_DTYPE)
        planes = np.empty((B, oh, ow), np.uint8) if edges else None
        n = C.c_int64()
        check(self.lib.dnnca_surface_distances(*args, counts.ctypes.data_as(C.POINTER(C.c_int32)),
                                               samples.ctypes.data_as(C.POINTER(_lib.SurfaceSample)), cap, C.byref(n),
                                               planes.ctypes.data_as(C.c_void_p) if edges else None, planes.nbytes if edges else 0, hw))
        return counts, samples[:n.value].copy(), planes

    def input_sensitivity(self, x=None, batch=None):
        """float64 [B, C]: sum over the image of |d sum(prob of slice b) / d x[b, :, :, c]| in inference mode (the raw sums of the
        reference's sensitivity map; casewise.normalise_sensitivity divides each row by its sum).  x [B, H, W, C], or None with
        `batch`: the slices the last forward(x) left on the device.  dtype f32 models only."""
        if x is None:
            B, xp = int(batch), None
        else:
            x = self._check_x(x)
            B, xp = x.shape[0], fptr(x)
        out = np.empty((B, self.in_shape[2]), np.float64)
        check(self.lib.dnnca_input_sensitivity(self.handle, xp, B, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    ATTRIBUTION_BASELINES = {'black': 0, 'mean': 1}

    def integrated_gradients(self, x=None, batch=None, steps=32, baseline='black', return_map=False):
        """Integrated gradients of F_b = sum(prob of slice b) in inference mode along the straight path from a constant baseline
        plane per (slice, channel) -- 'black': 0, 'mean': the plane's mean -- to the slice, midpoint rule with `steps` points
        (include/dnnca.h: dnnca_integrated_gradients).  Returns Attribution(signed, absolute, endpoints, map): float64 [B, C] sums of
        attr and of |attr| over the image, float64 [B, 2] (F(x), F(baseline)), and attr itself as float32 [B, H, W, C] with
        return_map (else None).  x [B, H, W, C], or None with `batch`: the slices the last forward(x) left on the device.
        dtype f32 U-Net / mulmo models only."""
        if baseline not in self.ATTRIBUTION_BASELINES:
            raise ValueError('baseline %r is none of %s' % (baseline, sorted(self.ATTRIBUTION_BASELINES)))
        if x is None:
            B, xp = int(batch), None
        else:
            x = self._check_x(x)
            B, xp = x.shape[0], fptr(x)
        n = max(B, 0)
        H, W, Cn = self.in_shape
        dp = C.POINTER(C.c_double)
        signed, absolute, ends = np.empty((n, Cn), np.float64), np.empty((n, Cn), np.float64), np.empty((n, 2), np.float64)
        amap = np.empty((n, H, W, Cn), np.float32) if return_map else None
        check(self.lib.dnnca_integrated_gradients(self.handle, xp, B, int(steps), self.ATTRIBUTION_BASELINES[baseline],
                                                  signed.ctypes.data_as(dp), absolute.ctypes.data_as(dp), ends.ctypes.data_as(dp),
                                                  fptr(amap) if return_map else None))
        return Attribution(signed, absolute, ends, amap)

    # ---- device-side augmentation (annotator/data.py:62-111 train_ds) ------------------------------------------
    def _aug_buffers(self, name, *nbytes):
        """the buffers of the augmentation call `name` (kept as self._<name>, made by its first call), each reserved to its size"""
        bufs = self.__dict__.setdefault('_' + name, tuple(RawDeviceBuffer() for _ in nbytes))
        for buf, n in zip(bufs, nbytes):
            buf.reserve(n)
        return bufs

    def augment_u8(self, raw, params, out_size, label_index, contrast_channels=None, src_ptr=None):
        """raw uint8 [B, Hs, Ws, Cs] (host) + per-image draws [(dy, dx, flip, contrast)] -> device-resident (x [B, Ho, Wo, Cs-1],
        y [B, Ho, Wo]) views, valid until the next call.  contrast_channels: source channels to adjust (default: all features).
        src_ptr: the batch is in HBM already (a StagingRing slot; `raw` is then only read for its shape)."""
        if src_ptr is None:
            raw = np.ascontiguousarray(raw, np.uint8)
        if raw.ndim != 4:
            raise ValueError('raw batch must be [B, H, W, C] uint8, got %s' % (raw.shape,))
        B, hs, ws, cs = raw.shape
        ho, wo = int(out_size[0]), int(out_size[1])
        if len(params) != B:
            raise ValueError('%d parameter rows for %d images' % (len(params), B))
        if contrast_channels is None:
            contrast_channels = [c for c in range(cs) if c != label_index]
        mask = 0
        for c in contrast_channels:
            mask |= 1 << int(c)
        src, xb, yb = self._aug_buffers('aug', 0, B * ho * wo * (cs - 1) * 4, B * ho * wo * 4)      # (src: sized by its upload)
        own_upload = src_ptr is None
        if own_upload:
            src.upload(raw)
            src_ptr = src.ptr
        prm = (_lib.AugParam * B)(*[_lib.AugParam(int(p[0]), int(p[1]), int(p[2]), float(p[3])) for p in params])
        check(self.lib.dnnca_augment_u8(self.handle, src_ptr, B, hs, ws, cs, int(label_index), mask, prm, ho, wo, xb.ptr, yb.ptr))
        if own_upload:
            # dnnca_augment_u8 is asynchronous on the model's stream (a staged batch keeps the loop one step ahead); the batch this
            # call uploaded itself lives in a buffer the next call overwrites with a blocking copy, so here the stream is drained
            self.sync()
        return DeviceView(xb, (B, ho, wo, cs - 1)), DeviceView(yb, (B, ho, wo))

    def affine(self, xv, yv, mats):
        """random_affine on device-resident (x, y) views: mats float64 [B, 2, 3] from augment.draw_affine (output pixel -> source
        position, bilinear, zero outside).  Asynchronous on the model's stream; the views are valid until the next call."""
        B, h, w, c = xv.shape
        mats = np.ascontiguousarray(mats, np.float64)
        if mats.shape != (B, 2, 3):
            raise ValueError('affine matrices %s are not [B, 2, 3] for a batch of %d' % (mats.shape, B))
        xo, yo = self._aug_buffers('affine', xv.nbytes, yv.nbytes)
        check(self.lib.dnnca_affine_f32(self.handle, xv.ptr, yv.ptr, B, h, w, c, mats.ctypes.data_as(C.POINTER(C.c_double)), xo.ptr, yo.ptr))
        return DeviceView(xo, xv.shape), DeviceView(yo, yv.shape)

    def warp(self, xv, yv, ctrl, wv):
        """random_warp's dense part on device-resident (x, y) views: ctrl [B, n, 2], wv [B, n + 3, 2] from augment.solve_warp."""
        B, h, w, c = xv.shape
        ctrl, wv = np.ascontiguousarray(ctrl, np.float64), np.ascontiguousarray(wv, np.float64)
        dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))        # noqa: E731
        xo, yo = self._aug_buffers('warp', xv.nbytes, yv.nbytes)
        check(self.lib.dnnca_warp_f32(self.handle, xv.ptr, yv.ptr, B, h, w, c, ctrl.shape[1], dptr(ctrl), dptr(wv), xo.ptr, yo.ptr))
        return DeviceView(xo, xv.shape), DeviceView(yo, yv.shape)

    def warp_groups(self, xv, yv, group_of, ctrl, wv, label_index=None):
        """random_intrachannelwarp's dense part on device-resident (x, y) views, one launch for every group of every image:
        ctrl [B, G, n, 2], wv [B, G, n + 3, 2] from augment.solve_intrawarp.  group_of: the group of every feature channel, then
        the label's ([c + 1]); with `label_index` it is the table of the raw slice's channels (augment.group_table, label at
        label_index) and is reordered here.  Asynchronous on the model's stream; the views are valid until the next call."""
        B, h, w, c = xv.shape
        ctrl, wv = np.ascontiguousarray(ctrl, np.float64), np.ascontiguousarray(wv, np.float64)
        group_of = np.asarray(group_of, np.int32).ravel()
        if label_index is not None:
            group_of = np.concatenate([np.delete(group_of, label_index), group_of[label_index:label_index + 1]])
        group_of = np.ascontiguousarray(group_of, np.int32)
        if group_of.size != c + 1:
            raise ValueError('%d group entries for %d feature channels + label' % (group_of.size, c))
        if ctrl.ndim != 4 or ctrl.shape[0] != B or wv.shape != ctrl.shape[:2] + (ctrl.shape[2] + 3, 2):
            raise ValueError('ctrl %s / wv %s are not [B, G, n, 2] / [B, G, n + 3, 2] for a batch of %d' % (ctrl.shape, wv.shape, B))
        dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))        # noqa: E731
        xo, yo = self._aug_buffers('warp_groups', xv.nbytes, yv.nbytes)
        check(self.lib.dnnca_warp_groups_f32(self.handle, xv.ptr, yv.ptr, B, h, w, c, ctrl.shape[1], group_of.ctypes.data_as(C.POINTER(C.c_int)),
                                             ctrl.shape[2], dptr(ctrl), dptr(wv), xo.ptr, yo.ptr))
        return DeviceView(xo, xv.shape), DeviceView(yo, yv.shape)

    def intensity(self, xv, records):
        """random_intensity on a device-resident x view: records uint32 [B, C, 32] from augment.draw_intensity (one per image and
        feature channel: gamma, bias field, blur taps, noise sigma and key; include/dnnca.h).  The label is not touched.
        Asynchronous on the model's stream; the view is valid until the next call."""
        B, h, w, c = xv.shape
        records = np.ascontiguousarray(records, np.uint32)
        if records.shape != (B, c, _lib.INTENSITY_WORDS):
            raise ValueError('intensity records %s are not [B, C, %d] for a batch of %d with %d channels'
                             % (records.shape, _lib.INTENSITY_WORDS, B, c))
        xo, = self._aug_buffers('intensity', xv.nbytes)
        check(self.lib.dnnca_intensity_f32(self.handle, xv.ptr, B, h, w, c, records.ctypes.data_as(C.POINTER(C.c_uint32)), xo.ptr))
        return DeviceView(xo, xv.shape)

    # ---- data parallel ----------------------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = C.create_string_buffer(_lib.UNIQUE_ID_BYTES)
        check(_lib.load().dnnca_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, rank, world, unique_id):
        check(self.lib.dnnca_comm_init(self.handle, int(rank), int(world), unique_id, len(unique_id) if unique_id else 0))

    def comm_collectives(self):
        """gradient all-reduce calls of the last train step (> 1: bucketed)"""
        n = C.c_int()
        check(self.lib.dnnca_comm_collectives(self.handle, C.byref(n)))
        return n.value

    def comm_collective_floats(self):
        """floats the last of those calls covered (n_trainable + 1: gradients and the loss slot; 1: the loss slot alone)"""
        n = C.c_int64()
        check(self.lib.dnnca_comm_collective_floats(self.handle, C.byref(n)))
        return n.value

    def comm_broadcast_weights(self, root=0):
        check(self.lib.dnnca_comm_broadcast_weights(self.handle, int(root)))

    def comm_average_state(self):
        check(self.lib.dnnca_comm_average_state(self.handle))

    def comm_allreduce(self, values, op='sum'):
        v = np.array(values, dtype=np.float64).ravel()
        check(self.lib.dnnca_comm_allreduce_host(self.handle, v.ctypes.data_as(C.POINTER(C.c_double)), v.size, 1 if op == 'max' else 0))
        return v

    # ---- measurement ------------------------------------------------------------------------------------------
    def timer_start(self):
        check(self.lib.dnnca_timer_start(self.handle))

    def timer_stop(self):
        ms = C.c_float()
        check(self.lib.dnnca_timer_stop(self.handle, C.byref(ms)))
        return ms.value

    def profile_enable(self, mode=1, focus=None, period=1):
        check(self.lib.dnnca_profile_sample(self.handle, int(period)))
        if focus is not None:
            check(self.lib.dnnca_profile_focus(self.handle, focus.encode()))
        check(self.lib.dnnca_profile_enable(self.handle, int(mode)))

    def profile_reset(self):
        check(self.lib.dnnca_profile_reset(self.handle))

    def profile(self):
        """[(kernel, launches, total_ms, algorithmic bytes per launch, flops per launch)]"""
        cnt = C.c_int()
        check(self.lib.dnnca_profile_count(self.handle, C.byref(cnt)))
        name = C.create_string_buffer(128)
        n, ms, by, fl = C.c_int64(), C.c_double(), C.c_double(), C.c_double()
        out = []
        for i in range(cnt.value):
            check(self.lib.dnnca_profile_get(self.handle, i, name, 128, C.byref(n), C.byref(ms), C.byref(by), C.byref(fl)))
            out.append((name.value.decode(), n.value, ms.value, by.value, fl.value))
        return out

    PLAN_PASSES = {'train': 0, 'eval': 1, 'forward': 2, 'sensitivity': 3, 'lesion': 4, 'lesion_linked': 5, 'lesion_matched': 6,
                   'surface': 7, 'attribution': 8, 'lesion_features': 9, 'detection': 10}

    def plan(self, variants=False, mode='train', batch=None):
        """The launch schedule of one pass: [(kernel, algorithmic bytes, flops)].  mode 'train': one train step; 'eval': one
        eval_step (inference forward + loss; a staged evaluation step launches the same); 'forward': forward(training=False);
        'sensitivity': input_sensitivity; 'lesion': lesion_table on the last forward's probabilities, with the resize factor,
        filter size and mask choice of the last lesion_table / lesion_table_linked call; 'lesion_linked': lesion_table_linked likewise;
        'lesion_matched': lesion_table_matched with the three values of the last lesion_table_matched call; 'surface':
        surface_distances with the resize factor and filter size of the last surface_distances call; 'attribution':
        integrated_gradients with the steps and baseline of the last integrated_gradients call (before any: 32, 'black') and the map;
        'lesion_features': lesion_table_features on the staged batch with the resize factor, filter size, mask choice, bins and ring
        of the last lesion_table_features call (before any: 1.0, 5, with mask, 32, 3); 'detection': detection_map in place with the
        parameters of the last detection_map / detection_map_of call (before any: the defaults).
        batch: None = max_batch.  variants: keep the template variant the library appends to a launch name
        (`ig_conv_fwd#3n2w8`): the kernel-coverage test tells them apart.  A dry run: the model is unchanged."""
        if mode not in self.PLAN_PASSES:
            raise ValueError('plan mode %r is none of %s' % (mode, sorted(self.PLAN_PASSES)))
        buf = C.create_string_buffer(1 << (24 if mode == 'attribution' else 20))      # up to 256 passes in one plan
        if mode == 'train' and batch is None:
            check(self.lib.dnnca_plan_dump(self.handle, buf, len(buf)))
        else:
            check(self.lib.dnnca_plan_dump_pass(self.handle, self.PLAN_PASSES[mode], int(self.max_batch if batch is None else batch),
                                                buf, len(buf)))
        out = []
        for line in buf.value.decode().splitlines():
            k, b, f = line.split('\t')
            out.append((k if variants else k.split('#')[0], float(b), float(f)))
        return out
