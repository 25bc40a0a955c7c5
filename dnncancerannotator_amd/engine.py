"""Engine facade: the MI355X stand-in for annotator/engine.py:36-288 (class TFKerasModel).

Same constructor, same methods (train / eval / predict / save / load / get_ckpts / get_config), same save-directory
layout (checkpoints/ckpt-{step}.index, options.yaml, results.csv); underneath, a DeviceModel (libdnnca, hand-written HIP)
instead of a compiled tf.keras.Model.  One Keras "epoch" of the reference is one optimizer step (engine.py:126-135), so
the loop here is a plain step loop.

Data parallel (deploy_options.enable_multigpu, engine.py:260-263): one process per GPU.  Each rank takes its contiguous
shard of every global batch, libdnnca sums the gradients with one RCCL all-reduce per step, rank 0 writes files.
Ranks come from RANK / LOCAL_RANK / WORLD_SIZE (set by `python -m dnncancerannotator_amd.launch` or torchrun)."""

import contextlib
import copy
import json
import logging
import os
import re
import time
from collections import OrderedDict, namedtuple

import numpy as np

from . import augment, casewise, device, distributed, losses as custom_losses, metrics as custom_metrics, models, region_metrics
from . import tta as tta_modes
from .feeder import BatchFeeder


class History:
    """The part of keras.callbacks.History that utils/dump.py:68-73 reads."""

    def __init__(self, model):
        self.epoch = []
        self.history = {}
        self.params = {}
        self.model = model

    def log(self, step, logs):
        self.epoch.append(step)
        for k, v in logs.items():
            self.history.setdefault(k, []).append(v)


def _element_shape(dataset):
    """Input shape [B, H, W, C] of a dataset: `element_spec[0].shape` (engine.py:93) or, failing that, its first batch."""
    spec = getattr(dataset, 'element_spec', None)
    if spec is not None:
        return tuple(spec[0].shape)
    for element in dataset:          # (x, y) for train / eval, (x,) for predict
        return tuple(np.shape(element[0]))
    raise ValueError('empty dataset')


def _forward_on_device(dm, xb, tta_mask, spread=False, temperature=None, ensemble=None):
    """the inference forward whose probabilities stay on the device: the plain one or, with a view mask (tta.mask_of), the test-time
    augmented one; with `spread` the augmented one that also keeps the views' spread on the device (--uncertainty).  With
    `ensemble` (--ensemble: the members are set in dm) one DeviceModel.forward_ensemble in place of the three: the mean over the
    members of what each of them gives, and with `spread` the total spread.  With a temperature (--temperature,
    check_temperature) the probabilities are then scaled once, in place: every consumer reads the calibrated values; the spread
    stays that of the unscaled views"""
    if ensemble:
        dm.forward_ensemble(xb, tta_mask or 1, spread=spread, return_prob=False)
    elif tta_mask is None:
        dm.forward(xb, training=False, return_prob=False)
    elif spread:
        dm.forward_tta_spread(xb, tta_mask, return_prob=False, return_spread=False)
    else:
        dm.forward_tta(xb, tta_mask, return_prob=False)
    if temperature is not None:
        dm.scale_temperature(temperature, len(xb))


class _SliceChain:
    """Which slices of a split continue the slice before them, for the linked and matched lesion tables: the same exam path and the
    next slice number, across splits and batches.  A model that was re-sized since the last split broke the chain -- the row numbers
    of the slice before stayed behind on the model the batch outgrew -- with a warning led by `who`."""

    def __init__(self, who):
        self.who, self.model, self.last = who, None, None       # last: (exam, slice) of the slice before

    def continues(self, dm, pk):
        """one flag per slice of pk = [(path, sliceID)], the split that `dm` has just forwarded"""
        if self.last is not None and dm is not self.model:
            logging.warning('%s: the model was re-sized before slice %s of %s: it is not linked to the slice before', self.who, pk[0][1], pk[0][0])
            self.last = None
        self.model = dm
        flags = []
        for p, k in pk:
            flags.append(self.last is not None and p == self.last[0] and int(k) == self.last[1] + 1)
            self.last = (p, int(k))
        return flags


_SplitTables = namedtuple('_SplitTables', 'rows totals masks links srows stotals feats')     # annotate's tables of one split


class _Pass:
    """One extra pass of eval: whether it is on, run(step) -> the new lines of each of its files after a checkpoint, its files
    [(file name, lead columns, columns)] and their lines so far, one list per file"""

    def __init__(self, on, run, files, tables=None):
        self.on, self.run, self.files = on, run, files
        self.tables = [[] for _ in files] if tables is None else tables

    def append(self, new):
        for table, lines in zip(self.tables, new):
            table += lines

    def write(self, root):
        os.makedirs(root, exist_ok=True)
        for (name, lead, cols), table in zip(self.files, self.tables):
            with open(os.path.join(root, name), 'w', newline='') as f:
                f.write(casewise.plain_csv(lead + cols, table))


def check_uncertainty(uncertainty, tta, ensemble=None):
    """--uncertainty measures the disagreement of the test-time-augmentation views and of the members of an ensemble: without views
    and without members there is nothing to measure.  With --ensemble alone the spread is purely between the members"""
    if uncertainty and tta == tta_modes.NONE and not ensemble:
        raise ValueError('--uncertainty needs the views of test-time augmentation: add --tta flips (or --tta d4 on square slices)')


def check_temperature(temperature):
    """--temperature T: None for no scaling (no flag, or T = 1: no new call runs), else the float; outside the range the library
    accepts (casewise.TEMPERATURE_RANGE) or NaN: a ValueError, before anything is read"""
    if temperature is None:
        return None
    t = float(temperature)
    if not casewise.TEMPERATURE_RANGE[0] <= t <= casewise.TEMPERATURE_RANGE[1]:
        raise ValueError('--temperature must lie in [%g, %g], got %r' % (casewise.TEMPERATURE_RANGE + (temperature,)))
    return None if t == 1.0 else t


def check_attribution(attribution, steps, baseline, export_csv, export_images):
    """--visualize_attribution writes per-slice files: it needs --export_csv and / or --export_images; --attribution_steps must lie
    in casewise.ATTRIBUTION_STEP_RANGE and --attribution_baseline be one of casewise.ATTRIBUTION_BASELINES.  A ValueError, before
    anything is read; the two options without the flag are an error too.  Returns (steps, baseline)"""
    if not attribution:
        if steps is not None or baseline is not None:
            raise ValueError('--attribution_steps / --attribution_baseline need --visualize_attribution')
        return None
    if not (export_csv or export_images):
        raise ValueError('--visualize_attribution writes per-slice files: add --export_csv and / or --export_images')
    steps = casewise.ATTRIBUTION_STEPS if steps is None else int(steps)
    lo, hi = casewise.ATTRIBUTION_STEP_RANGE
    if not lo <= steps <= hi:
        raise ValueError('--attribution_steps must lie in %d..%d, got %r' % (lo, hi, steps))
    baseline = casewise.ATTRIBUTION_BASELINES[0] if baseline is None else baseline
    if baseline not in casewise.ATTRIBUTION_BASELINES:
        raise ValueError('--attribution_baseline must be one of %s, got %r' % (', '.join(casewise.ATTRIBUTION_BASELINES), baseline))
    return steps, baseline


def check_calibration(n_bins, temperatures):
    """--calibration_bins and --calibration_temperatures: (bins, the temperature grid of casewise.calibration_grid) or a ValueError"""
    if not 1 <= int(n_bins) <= 256:
        raise ValueError('--calibration_bins must lie in 1..256, got %r' % (n_bins,))
    return int(n_bins), casewise.calibration_grid(temperatures)


def check_detection(detection, min_confidence=None, factor=None, max_candidates=None, min_area=None, rounds=None, iou=None,
                    link_min_overlap=None, max_lesions=None, flag='--detection'):
    """the values of the --detection_* flags (None: not given) -> None without `detection` (any value given is then a ValueError:
    they mean nothing without the flag), else dict(cfg=the keywords of DeviceModel.detection_map with the defaults filled in, iou,
    link_min_overlap, max_lesions).  Every value outside what the library accepts (casewise.DETECTION_RANGES; rounds at least
    max_candidates), NaN included, is a ValueError -- before anything is read"""
    given = dict(min_confidence=min_confidence, factor=factor, max_candidates=max_candidates, min_area=min_area, rounds=rounds)
    if not detection:
        if any(v is not None for v in list(given.values()) + [iou, link_min_overlap, max_lesions]):
            raise ValueError('the --detection_* options set the candidate extraction of %s: add %s' % (flag, flag))
        return None
    cfg = {}
    for key, default in casewise.DETECTION_DEFAULTS.items():
        v = default if given[key] is None else given[key]
        lo, hi = casewise.DETECTION_RANGES[key]
        if isinstance(default, int):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError('--detection_%s must be an integer, got %r' % (key, v))
            v = int(v)
        else:
            v = float(v)
        if not lo <= v <= hi:                                       # (False for a NaN)
            raise ValueError('--detection_%s must lie in [%g, %g], got %r' % (key, lo, hi, given[key]))
        cfg[key] = v
    if cfg['rounds'] < cfg['max_candidates']:
        raise ValueError('--detection_rounds %d is below --detection_max_candidates %d: every candidate costs a round'
                         % (cfg['rounds'], cfg['max_candidates']))
    iou = casewise.DETECTION_IOU if iou is None else float(iou)
    if not 0.0 < iou <= 1.0:
        raise ValueError('--detection_iou must lie in (0, 1], got %r' % (iou,))
    link_min_overlap = 1 if link_min_overlap is None else int(link_min_overlap)
    max_lesions = 256 if max_lesions is None else int(max_lesions)
    if link_min_overlap < 1 or max_lesions < 1:
        raise ValueError('--detection_link_min_overlap and --detection_max_lesions must be at least 1, got %d and %d'
                         % (link_min_overlap, max_lesions))
    return dict(cfg=cfg, iou=iou, link_min_overlap=link_min_overlap, max_lesions=max_lesions)


REFINE_MAX_CLOSING = 15


def check_refine(hysteresis=None, closing=None, fill_holes=False, thresholds=(), consumers=True):
    """the values of --refine_hysteresis LOW, --refine_closing K and --refine_fill_holes (None / False: not given) -> None when
    nothing is asked for (no flag, or a closing of 0 or 1 alone), else the keywords of DeviceModel.set_lesion_refine.
    thresholds: every threshold the run's refined tables will use.  A ValueError that names the flag -- before anything is read --
    for: LOW outside (0, 1) or NaN, or not below every threshold (as float32, the comparison the library makes); K negative, even
    (its window is asymmetric: the closed mask would not contain its input) or above 15; any of the flags without a pass that
    reads the refined mask (consumers=False: `evaluate` without --exam_lesions / --surface_distances)"""
    if hysteresis is None and closing is None and not fill_holes:
        return None
    if not consumers:
        raise ValueError('the --refine_* options refine the masks of --exam_lesions / --surface_distances: add one of them')
    low = None
    if hysteresis is not None:
        low = float(hysteresis)
        if not 0.0 < low < 1.0:                                         # (False for a NaN)
            raise ValueError('--refine_hysteresis must lie strictly between 0 and 1, got %r' % (hysteresis,))
        above = [float(t) for t in thresholds]
        if above and not np.float32(low) < np.float32(min(above)):
            raise ValueError('--refine_hysteresis %r must lie below every threshold of the run (the smallest is %r): it is the low '
                             'threshold around the pixels at the high one' % (hysteresis, min(above)))
    k = 0 if closing is None else closing
    if isinstance(k, bool) or int(k) != k:
        raise ValueError('--refine_closing must be an integer, got %r' % (closing,))
    k = int(k)
    if k < 0 or k > REFINE_MAX_CLOSING or (k > 1 and k % 2 == 0):
        raise ValueError('--refine_closing must be an odd size in 3..%d (0 or 1: no closing), got %r' % (REFINE_MAX_CLOSING, closing))
    if low is None and k <= 1 and not fill_holes:
        return None
    return dict(hysteresis=low, closing=k, fill_holes=bool(fill_holes))


EMA_KEYS = ('decay', 'warmup', 'validate')
WEIGHT_CHOICES = ('raw', 'ema')


def check_bootstrap(bootstrap=None, seed=None, level=None, stratified=False, detection=False, exam_lesions=False):
    """the values of --bootstrap R and the --bootstrap_* flags (None / False: not given) -> None without `bootstrap` (a
    --bootstrap_* flag is then a ValueError: it means nothing without it), else dict(replicates, seed, level, stratified) with the
    defaults filled in.  ValueError: R no integer in casewise.BOOTSTRAP_RANGE, neither --detection nor --exam_lesions (there is
    nothing to resample), a seed outside 0 .. 2^64 - 1, a level not strictly between 0.5 and 1, --bootstrap_stratified without
    --detection (the exam-lesion pass has no positive-exam flag to split on)."""
    if bootstrap is None:
        if seed is not None or level is not None or stratified:
            raise ValueError('the --bootstrap_* options set the resampling of --bootstrap: add --bootstrap R')
        return None
    lo, hi = casewise.BOOTSTRAP_RANGE
    if isinstance(bootstrap, bool) or not isinstance(bootstrap, (int, np.integer)) or not lo <= bootstrap <= hi:
        raise ValueError('--bootstrap must be an integer in [%d, %d], got %r' % (lo, hi, bootstrap))
    if not (detection or exam_lesions):
        raise ValueError('--bootstrap resamples the exams of --detection / --exam_lesions: add one of them')
    seed = 0 if seed is None else seed
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 1 << 64:
        raise ValueError('--bootstrap_seed must be an integer in [0, 2^64 - 1], got %r' % (seed,))
    level = casewise.BOOTSTRAP_LEVEL if level is None else level
    if isinstance(level, bool) or not isinstance(level, (int, float, np.floating)) or not 0.5 < level < 1.0:
        raise ValueError('--bootstrap_level must lie strictly between 0.5 and 1, got %r' % (level,))
    if stratified and not detection:
        raise ValueError('--bootstrap_stratified splits the exams of --detection by their labelled tumours; --exam_lesions has no '
                         'such flag to split on: add --detection or drop it')
    return dict(replicates=int(bootstrap), seed=int(seed), level=float(level), stratified=bool(stratified))


def check_ema(options):
    """deploy_options.ema -> dict(decay, warmup, validate), or None without the key.  decay: finite, in (0, 1); warmup: the
    num_updates warm-up of tf.train.ExponentialMovingAverage (default on); validate: 'ema' (default: validation inside train() and
    early stopping read the averaged weights) or 'raw'.  Unknown keys and bad values are a ValueError"""
    if options is None:
        return None
    if not isinstance(options, dict):
        raise ValueError('deploy_options.ema must be a mapping of %s, got %r' % (', '.join(EMA_KEYS), options))
    unknown = sorted(set(options) - set(EMA_KEYS))
    if unknown:
        raise ValueError('deploy_options.ema: unknown keys %s (known: %s)' % (unknown, ', '.join(EMA_KEYS)))
    decay = options.get('decay', 0.999)
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not np.isfinite(decay) or not 0.0 < float(decay) < 1.0:
        raise ValueError('deploy_options.ema.decay must be a finite number in (0, 1), got %r' % (decay,))
    warmup = options.get('warmup', True)
    if not isinstance(warmup, bool):
        raise ValueError('deploy_options.ema.warmup must be true or false, got %r' % (warmup,))
    validate = options.get('validate', 'ema')
    if validate not in WEIGHT_CHOICES:
        raise ValueError("deploy_options.ema.validate must be 'ema' or 'raw', got %r" % (validate,))
    return dict(decay=float(decay), warmup=warmup, validate=validate)


ACCUMULATION_MAX = 4096


def check_accumulation(value):
    """deploy_options.gradient_accumulation_steps -> k, an int in 1..4096 (None, the key absent: 1, nothing changes).  One optimizer
    update takes the mean gradient of k consecutive train steps (micro-steps).  Bools, floats, strings and values outside the range
    are a ValueError"""
    if value is None:
        return 1
    if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= ACCUMULATION_MAX:
        raise ValueError('deploy_options.gradient_accumulation_steps must be an integer in 1..%d, got %r' % (ACCUMULATION_MAX, value))
    return int(value)


def check_accumulation_schedule(k, save_freq, max_steps, resumed_step):
    """train() with k > 1: checkpoints, validation passes and the end of the run must fall between cycles, and a resumed run must
    start on one; a ValueError that names the numbers otherwise"""
    if k <= 1:
        return
    key = 'deploy_options.gradient_accumulation_steps'
    if save_freq % k:
        raise ValueError('%s %d does not divide save_freq %d: a checkpoint would fall inside a cycle' % (key, k, save_freq))
    if max_steps is not None and max_steps % k:
        raise ValueError('%s %d does not divide max_steps %d: the run would end inside a cycle' % (key, k, max_steps))
    if resumed_step % k:
        raise ValueError('%s %d does not divide the resumed step %d: the checkpoint was written inside a cycle' % (key, k, resumed_step))


# deploy_options.optimizer as a mapping: what Keras' optimizers.get takes in model.compile (engine.py:276-284) [TF-2.6]
OPTIMIZER_KINDS = {'Adam': 'adam', 'AdamW': 'adamw', 'SGD': 'sgd'}
_CLIP_KEYS = ('clipvalue', 'clipnorm', 'global_clipnorm')
OPTIMIZER_KEYS = {
    'Adam': ('learning_rate', 'beta_1', 'beta_2', 'epsilon', 'amsgrad') + _CLIP_KEYS,
    'AdamW': ('learning_rate', 'weight_decay', 'exclude_from_weight_decay', 'beta_1', 'beta_2', 'epsilon', 'amsgrad') + _CLIP_KEYS,
    'SGD': ('learning_rate', 'momentum', 'nesterov') + _CLIP_KEYS,
}
# Keras' defaults: Adam / AdamW start at 0.001, SGD at 0.01; AdamW decays by 0.004 [TF-2.6 / Keras 2.11 for AdamW]
OPTIMIZER_DEFAULTS = dict(beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, momentum=0.0, nesterov=False, weight_decay=0.004,
                          exclude_from_weight_decay=('bias', 'beta', 'gamma'), clipvalue=None, clipnorm=None, global_clipnorm=None)


def _number(where, key, value, lo, hi=None, lo_open=False):
    """a finite int / float (no bool, no string) in [lo, hi) -- or (lo, ...) with lo_open -- as a float, or a ValueError"""
    ok = not isinstance(value, bool) and isinstance(value, (int, float)) and np.isfinite(value)
    if ok:
        ok = (value > lo if lo_open else value >= lo) and (hi is None or value < hi)
    if not ok:
        rng = '%s%g, %s' % ('(' if lo_open else '[', lo, 'inf)' if hi is None else '%g)' % hi)
        raise ValueError('%s.%s must be a finite number in %s, got %r' % (where, key, rng, value))
    return float(value)


def check_optimizer(spec):
    """deploy_options.optimizer -> None for the string 'adam' (the reference's compile call: nothing changes), else a dict
    class_name, config (every key of the class with its value, as it goes into a checkpoint's index), learning_rate (the starting
    value the LearningRateScheduler lambda receives), exclude (AdamW), and device (the keywords of DeviceModel.set_optimizer).
    Accepted: the strings 'adamw' / 'sgd' (the class with its defaults) or {class_name: Adam | AdamW | SGD, config: {...}}.
    Unknown classes, unknown keys, amsgrad, clipnorm together with global_clipnorm and bad values are a ValueError"""
    if spec == 'adam':
        return None
    if isinstance(spec, str):
        by_lower = {k.lower(): k for k in OPTIMIZER_KINDS}
        if spec.lower() not in by_lower:
            raise ValueError("deploy_options.optimizer: unknown optimizer %r (known: adam, adamw, sgd, or a mapping)" % (spec,))
        spec = {'class_name': by_lower[spec.lower()], 'config': {}}
    if not isinstance(spec, dict) or set(spec) - {'class_name', 'config'} or 'class_name' not in spec:
        raise ValueError("deploy_options.optimizer must be 'adam' or a mapping {class_name, config}, got %r" % (spec,))
    cls = spec['class_name']
    if cls not in OPTIMIZER_KINDS:
        raise ValueError('deploy_options.optimizer: unknown class_name %r (known: %s)' % (cls, ', '.join(OPTIMIZER_KINDS)))
    given = spec.get('config') or {}
    if not isinstance(given, dict):
        raise ValueError('deploy_options.optimizer.config must be a mapping, got %r' % (given,))
    unknown = sorted(set(given) - set(OPTIMIZER_KEYS[cls]))
    if unknown:
        raise ValueError('deploy_options.optimizer.config: unknown keys %s for %s (known: %s)' % (unknown, cls, ', '.join(OPTIMIZER_KEYS[cls])))
    where = 'deploy_options.optimizer.config'
    defaults = dict(OPTIMIZER_DEFAULTS, learning_rate=0.01 if cls == 'SGD' else 0.001)
    cfg = {k: given.get(k, defaults[k]) for k in OPTIMIZER_KEYS[cls]}
    cfg['learning_rate'] = _number(where, 'learning_rate', cfg['learning_rate'], 0.0)
    dev = dict(kind=OPTIMIZER_KINDS[cls])
    for k in _CLIP_KEYS:          # None: off, as in Keras
        if cfg[k] is not None:
            cfg[k] = _number(where, k, cfg[k], 0.0, lo_open=True)
        dev[k] = cfg[k] or 0.0
    if cfg['clipnorm'] is not None and cfg['global_clipnorm'] is not None:
        raise ValueError('%s: clipnorm and global_clipnorm exclude each other (as in Keras)' % where)
    if cls == 'SGD':
        dev['momentum'] = cfg['momentum'] = _number(where, 'momentum', cfg['momentum'], 0.0, 1.0)
        if not isinstance(cfg['nesterov'], bool):
            raise ValueError('%s.nesterov must be true or false, got %r' % (where, cfg['nesterov']))
        dev['nesterov'] = cfg['nesterov']
    else:
        dev['beta1'] = cfg['beta_1'] = _number(where, 'beta_1', cfg['beta_1'], 0.0, 1.0)
        dev['beta2'] = cfg['beta_2'] = _number(where, 'beta_2', cfg['beta_2'], 0.0, 1.0)
        dev['epsilon'] = cfg['epsilon'] = _number(where, 'epsilon', cfg['epsilon'], 0.0)
        if not isinstance(cfg['amsgrad'], bool):
            raise ValueError('%s.amsgrad must be true or false, got %r' % (where, cfg['amsgrad']))
        if cfg['amsgrad']:
            raise ValueError('%s.amsgrad: true is not supported (AMSGrad needs a third slot per weight)' % where)
    exclude = ()
    if cls == 'AdamW':
        dev['weight_decay'] = cfg['weight_decay'] = _number(where, 'weight_decay', cfg['weight_decay'], 0.0)
        exclude = cfg['exclude_from_weight_decay']
        if isinstance(exclude, str) or not isinstance(exclude, (list, tuple)) or not all(isinstance(e, str) and e for e in exclude):
            raise ValueError('%s.exclude_from_weight_decay must be a list of name fragments, got %r' % (where, exclude))
        exclude = cfg['exclude_from_weight_decay'] = list(exclude)
    return dict(class_name=cls, config=cfg, learning_rate=cfg['learning_rate'], exclude=tuple(exclude), device=dev)


def slot_family(class_name):
    """what a checkpoint's adam_m / adam_v arrays hold: Adam's two moments (Adam, AdamW), or SGD's accumulator and zeros"""
    return 'sgd' if class_name == 'SGD' else 'adam'


def check_weights(weights):
    if weights not in WEIGHT_CHOICES:
        raise ValueError("--weights must be 'raw' or 'ema', got %r" % (weights,))
    return weights


def select_ckpts(ckpts, min_interval=1, step_range=None):
    """the checkpoints {step: path} (ascending) that `evaluate` visits: inside step_range and min_interval apart"""
    lo, hi = (0, float('inf')) if step_range is None else step_range
    out, previous = OrderedDict(), None
    for step, path in ckpts.items():
        if not lo <= step <= hi or (previous is not None and step - previous < min_interval):
            continue
        out[step] = path
        previous = step
    return out


def list_ckpts(base_path, pattern='ckpt-{epoch}'):
    """{step: path without extension}, ascending, of the complete checkpoints under base_path (TFKerasModel.get_ckpts without a model)"""
    regex_pattern = fr'^{pattern}\.index$'.format(epoch=r'(\d+)')
    files = [f for f in os.listdir(base_path) if re.match(regex_pattern, f)]
    steps = [int(re.sub(regex_pattern, r'\1', f)) for f in files]
    paths = [os.path.join(base_path, f[:-len('.index')]) for f in files]
    return OrderedDict(sorted(zip(steps, paths), key=lambda x: x[0]))


def check_ema_checkpoints(paths):
    """--weights ema: every checkpoint that will be read must hold a weight average (`"ema"` in its index).  A ValueError that names
    the first one that does not -- raised from the index files alone, before any data set is opened"""
    for path in paths:
        with open(path + '.index') as f:
            if 'ema' not in json.load(f):
                raise ValueError('--weights ema: checkpoint %s holds no weight average (it was trained without deploy_options.ema)' % path)


MAX_ENSEMBLE_MEMBERS = 15       # --ensemble: members beside the checkpoint of save_path (DeviceModel.MAX_MEMBERS - 1)


def parse_member(text):
    """one MEMBER of --ensemble, RUN_DIR[:STEP] -> (run directory, pinned step or None: the step being evaluated)"""
    if isinstance(text, (tuple, list)):
        run, step = text
        return str(run), None if step is None else int(step)
    run, sep, step = str(text).rpartition(':')
    if sep and run and step.isdigit():
        return run, int(step)
    return str(text), None


def _index_variables(path):
    with open(path + '.index') as f:
        return [(v['name'], tuple(v['shape']), v['trainable'], v['offset']) for v in json.load(f)['variables']]


def check_ensemble(save_path, members, steps, weights='raw', param_infos=None):
    """--ensemble: every member (parse_member) resolved to a checkpoint for every step of save_path that will be read -> {step:
    [path of each member, in the order given]}.  The checkpoint of save_path itself is member 0 and not in the lists.  A member
    without a pinned step follows the step; a step of None (predict without --step) stands for the latest checkpoint, of save_path
    and of every such member alike.  One ValueError that names the first checkpoint that is missing, and one for more than
    MAX_ENSEMBLE_MEMBERS members, for a member whose variables are not the model's (param_infos: DeviceModel.param_infos(); None:
    those of save_path's own checkpoint, before a model exists) and, with weights='ema', for one without a weight average
    (check_ema_checkpoints) -- raised from the index files alone, before any data is read"""
    members = [parse_member(m) for m in members]
    if not members:
        raise ValueError('--ensemble needs at least one member (RUN_DIR[:STEP])')
    if len(members) > MAX_ENSEMBLE_MEMBERS:
        raise ValueError('--ensemble takes at most %d members beside the checkpoint of --save_path, got %d' % (MAX_ENSEMBLE_MEMBERS, len(members)))
    listed = {}

    def ckpts_of(run):
        if run not in listed:
            base = os.path.join(run, 'checkpoints')
            listed[run] = list_ckpts(base) if os.path.isdir(base) else OrderedDict()
        return listed[run]
    out = OrderedDict()
    own = ckpts_of(save_path)
    for step in steps:
        paths = []
        for run, pinned in members:
            have = ckpts_of(run)
            want = pinned if pinned is not None else step
            if want is None and have:
                want = max(have)
            if want is None:
                raise ValueError('--ensemble: no checkpoint under %s/checkpoints' % run)
            if want not in have:
                raise ValueError('--ensemble: no checkpoint of step %s under %s/checkpoints (have %s)' % (want, run, sorted(have)))
            paths.append(have[want])
        out[step] = paths
    for step, paths in out.items():          # every member is there: now what the index files say
        want_vars = param_infos
        if want_vars is None:
            mine = max(own) if step is None and own else step
            want_vars = _index_variables(own[mine]) if mine in own else None
        if want_vars is not None:
            want_vars = [(n, tuple(s), t, o) for n, s, t, o in want_vars]
            for path in paths:
                if _index_variables(path) != want_vars:
                    raise ValueError(f'--ensemble: checkpoint {path} does not match the model (every member must have its architecture)')
        if weights == 'ema':
            check_ema_checkpoints(paths)
    return out


def read_member(path, weights='raw'):
    """(params, state) of a checkpoint as flat float32 vectors: what load() would make the parameters and the BatchNorm state"""
    with np.load(path + '.data-00000-of-00001') as z:
        return (np.ascontiguousarray(z['ema' if weights == 'ema' else 'params'], np.float32).ravel(),
                np.ascontiguousarray(z['state'], np.float32).ravel())


def _csv_value(v):
    """one value of a train_log.csv line: %.8g, a list of them in brackets (a metric of several thresholds)"""
    if isinstance(v, (list, tuple)):
        return '[%s]' % ' '.join('%.8g' % x for x in v)
    return '%.8g' % v


def _spread_counts(metric_objs, counts):
    """a [T, 4] count array over the concatenated thresholds of `metric_objs` -> added onto each metric's own rows"""
    lo = 0
    for m in metric_objs:
        m.counts += counts[lo:lo + len(m.thresholds)]
        lo += len(m.thresholds)


def _log_value(metric):
    """a pixel metric's result() for a log line: a float, or a list of floats (several thresholds)"""
    r = metric.result()
    return float(r) if np.ndim(r) == 0 else [float(v) for v in r]


def augment_on_device(dm, batch, shard, src_ptr=None):
    """The train-time augmentation chain of an augment.RawBatch (uint8 slices + their random draws) on the device `dm`: crop /
    flip / contrast / 255 / feature-label split, then every option the batch carries draws for, in its fixed place: affine, warp,
    intra-channel warp, intensity.  shard: this rank's part of an array; src_ptr: the slices are in a staging slot already.
    Returns the device-resident (x, y) views."""
    part = lambda a: shard(a)[0]        # noqa: E731
    xb, yb = dm.augment_u8(part(batch.raw), part(batch.params), batch.output_size, batch.label_index,
                           contrast_channels=batch.contrast_channels, src_ptr=src_ptr)
    if batch.affine is not None:
        xb, yb = dm.affine(xb, yb, part(batch.affine))
    if batch.warp is not None:
        xb, yb = dm.warp(xb, yb, part(batch.warp[0]), part(batch.warp[1]))
    if batch.intrawarp is not None:      # after random_warp: the overlay's key comes behind data_options.yaml's
        xb, yb = dm.warp_groups(xb, yb, batch.intrawarp[2], part(batch.intrawarp[0]), part(batch.intrawarp[1]), label_index=batch.label_index)
    if batch.intensity is not None:      # last: noise added before a resampling would be smoothed away by it
        xb = dm.intensity(xb, part(batch.intensity))
    return xb, yb


class TFKerasModel:
    """Encapsulates the DNN model and the library behind it (name kept from the reference for drop-in use)."""

    def __init__(self, model_config):
        self.model_config = copy.deepcopy(model_config)
        self.ctx = distributed.context()
        self.model = self.from_config(model_config)
        self.current_step = 0
        self.ckpt_pattern = 'ckpt-{epoch}'
        self.device_model = None

    # ---- construction (engine.py:254-288) --------------------------------------------------------------------
    def from_config(self, model_config):
        assert 'model' in model_config
        assert 'model_options' in model_config
        assert 'deploy_options' in model_config
        deploy = copy.deepcopy(model_config['deploy_options'])
        self.enable_multigpu = deploy.pop('enable_multigpu', True)
        if not self.enable_multigpu and self.ctx.world > 1:
            raise ValueError('enable_multigpu is false but WORLD_SIZE is %d' % self.ctx.world)
        self.learning_rate_scheduler = deploy.pop('LearningRateScheduler', None)
        model = getattr(models, model_config['model'])(**model_config['model_options'])
        self.loss = custom_losses.get(deploy['loss']) if 'loss' in deploy else custom_losses.WeightedCrossentropy()
        metric_specs = deploy.get('metrics', [])
        # region_metrics: device -- the region-based metrics of deploy_options.metrics are counted on the GPU
        # (region_metrics.py); without the key they are skipped with a warning (metrics.solve_metric)
        region_mode = deploy.pop('region_metrics', None)
        if region_mode not in (None, 'device'):
            raise ValueError("deploy_options.region_metrics: only 'device' is supported, got %r" % (region_mode,))
        self.region_metrics = []
        if region_mode == 'device':
            self.region_metrics = [m for m in map(region_metrics.solve_region_metric, metric_specs) if m is not None]
            metric_specs = [s for s in metric_specs if not region_metrics.is_region_spec(s)]
        self.metrics = [m for m in map(custom_metrics.solve_metric, metric_specs) if m is not None]
        # train_metrics: device -- every train step also reports the pixel metrics of its own batch, counted on the GPU from the
        # probabilities of the step's training=True forward pass (Keras fit updates the compiled metrics per step, engine.py:273,286);
        # without the key a train step logs loss and lr only
        train_mode = deploy.pop('train_metrics', None)
        if train_mode not in (None, 'device'):
            raise ValueError("deploy_options.train_metrics: only 'device' is supported, got %r" % (train_mode,))
        self.train_metrics = train_mode == 'device'
        if self.train_metrics and any(region_metrics.is_region_spec(s) for s in deploy.get('metrics', [])):
            logging.warning('train_metrics: region-based metrics are not counted per train step (validation still runs them)')
        # ema: {decay, warmup, validate} -- an exponential moving average of the weights, kept on the device by the Adam launches
        self.ema = check_ema(deploy.pop('ema', None))
        # gradient_accumulation_steps: k -- one optimizer update from the mean gradient of k consecutive train steps (micro-steps)
        self.accumulation = check_accumulation(deploy.pop('gradient_accumulation_steps', None))
        # optimizer: adam -- the reference's compile call (engine.py:276-284), unchanged; a mapping {class_name, config} or the
        # strings adamw / sgd: the configurable optimizers with Keras' gradient clipping (check_optimizer)
        self.optimizer = check_optimizer(deploy.get('optimizer'))
        self.learning_rate = 0.001          # engine.py:278
        self.adam = dict(beta1=0.9, beta2=0.999, epsilon=1e-7)
        if self.optimizer is not None:
            self.learning_rate = self.optimizer['learning_rate']
            self.adam = {k: self.optimizer['device'].get(k, v) for k, v in self.adam.items()}
        return model

    def _build(self, dataset, max_batch=None, also=()):
        """model.build(element_spec.shape) (engine.py:93).  `also`: further datasets that will be fed to this model (the
        validation set of train(): configs/additionals/data_options.yaml has train batch 8, eval batch 64) -- the device
        model is sized for the largest per-rank batch so that a validation batch is ONE eval step and its positive-rate
        weight is computed over the whole per-replica batch, as utils/losses.py:24-27,87-95 does."""
        shape = _element_shape(dataset)
        global_batch = max_batch or shape[0]
        if global_batch is None:
            raise ValueError('dataset batch size unknown')
        if global_batch % self.ctx.world:
            raise ValueError('global batch %d is not divisible by %d ranks' % (global_batch, self.ctx.world))
        per_rank = global_batch // self.ctx.world
        for other in also:
            if other is not None:
                b = _element_shape(other)[0]
                if b:
                    per_rank = max(per_rank, -(-b // self.ctx.world))
        if self.device_model is not None:
            self._ensure_capacity(per_rank)
            return
        device.init_device(self.ctx.local_rank)
        if self.enable_multigpu and self.ctx.world == 1 and device.device_count() > 1:
            logging.warning('enable_multigpu: %d GPUs visible but one process; launch with '
                            '`python -m dnncancerannotator_amd.launch --nproc N ...` for data parallel', device.device_count())
        self._input_shape = list(shape[1:])
        self.device_model = self.model.build([per_rank] + self._input_shape, seed=0)
        self.device_model.set_adam(**self.adam)
        self._set_optimizer(self.device_model)
        self._set_region_loss(self.device_model)
        self._set_ema(self.device_model)
        self._set_accumulation(self.device_model)
        self._join_ranks()

    def _set_region_loss(self, dm):
        """loss: TverskyCrossentropy / DiceCrossentropy -- the region term is stored in the device model once, and every later
        train / eval step reads it there; any other loss leaves the model as it was built (no call).  BoundaryCrossentropy: the
        boundary term behind it, which rides the region term's launches"""
        if isinstance(self.loss, custom_losses.TverskyCrossentropy):
            dm.set_region_loss(self.loss.region_cfg())
            if self.loss.topk_cfg() is not None:          # crossentropy_topk: the cross-entropy over the hardest pixels of an image
                dm.set_topk_loss(self.loss.topk_cfg())
        if isinstance(self.loss, custom_losses.BoundaryCrossentropy):
            dm.set_boundary_loss(self.loss.boundary_cfg())

    def _set_optimizer(self, dm):
        """a mapping in deploy_options.optimizer: stored in the device model once (kind, betas, momentum, decay, clips and the decay
        mask: every trainable variable whose name contains none of exclude_from_weight_decay); the string adam makes no call"""
        if self.optimizer is not None:
            names = [name for name, _, trainable, _ in dm.param_infos() if trainable]
            mask = np.array([not any(e in name for e in self.optimizer['exclude']) for name in names], np.uint8)
            dm.set_optimizer(decay_mask=mask, **self.optimizer['device'])

    def _set_accumulation(self, dm):
        """deploy_options.gradient_accumulation_steps: k > 1 is stored in the device model; without the key (or with 1) no call"""
        if self.accumulation > 1:
            dm.set_accumulation(self.accumulation)

    def _set_ema(self, dm):
        """deploy_options.ema: the average starts as a copy of the weights; without the key no call is made"""
        if self.ema is not None:
            dm.set_ema(self.ema['decay'], self.ema['warmup'])

    def _join_ranks(self):
        if self.ctx.world > 1:
            self.device_model.comm_init(self.ctx.rank, self.ctx.world, distributed.exchange_unique_id(self.ctx, device.DeviceModel))
            distributed.cleanup(self.ctx)     # ncclCommInitRank returned: every rank has read the id file
            # identical initial weights on every replica (MirroredStrategy mirrors rank 0's variables); the weight average, which
            # _set_ema has switched on by now, and its update count travel with them
            self.device_model.comm_broadcast_weights(0)

    def _ensure_capacity(self, per_rank_batch):
        """Grow the device model to `per_rank_batch` slices per step (weights, BN statistics and Adam slots carried over).
        Returns False when HBM cannot hold it (the caller then evaluates in chunks)."""
        dm = self.device_model
        if per_rank_batch <= dm.max_batch:
            return True
        if self.ctx.world > 1:
            return False      # the communicator belongs to the existing handle; _build sizes DP models up front
        if getattr(self, '_averaged_in_use', False):
            return False      # validation on the averaged weights: they live in this handle until the exchange back
        params, state, (m, v, it) = dm.get_params(), dm.get_state(), dm.get_opt_state()
        average = dm.get_ema() if self.ema is not None else None
        try:
            bigger = self.model.build([per_rank_batch] + self._input_shape, seed=0)
        except Exception as e:           # out of HBM: keep the model we have
            logging.warning('cannot size the model for a batch of %d (%s): evaluating in chunks', per_rank_batch, e)
            self.model.device_model = dm
            return False
        dm.close()
        bigger.set_params(params)
        if bigger.n_state:
            bigger.set_state(state)
        bigger.set_opt_state(m, v, it)
        bigger.set_adam(**self.adam)
        self._set_optimizer(bigger)
        self._set_region_loss(bigger)
        if average is not None:
            self._set_ema(bigger)
            bigger.set_ema_state(*average)
        self._set_accumulation(bigger)
        if getattr(self, '_members', None):       # --ensemble: the members lived in the model the batch outgrew
            bigger.set_members(self._members)
        if getattr(self, '_refine', None):        # --refine_*: so did the mask refinement
            bigger.set_lesion_refine(**self._refine)
        self.device_model = bigger
        return True

    def _set_ensemble(self, own_path, paths, weights='raw'):
        """--ensemble: the checkpoint own_path (member 0: what load() has just put into the model) and those of `paths` are read
        from their data files and stored in the device model; kept for _ensure_capacity"""
        self._members = [read_member(p, weights) for p in [own_path] + list(paths)]
        self.device_model.set_members(self._members)

    def _set_refine(self, refine):
        """--refine_*: what check_refine returned is stored in the device model once, before the first table call, and every later
        lesion_table* / surface_distances call reads it there; kept for _ensure_capacity.  None: no call is made"""
        self._refine = refine
        if refine:
            self.device_model.set_lesion_refine(**refine)

    @contextlib.contextmanager
    def _unrefined(self, dm):
        """around the table calls on a detection map, whose regions are already final: the refinement off, and back on afterwards.
        The kept planes of the lesions' chain count again once it is back (they remember the configuration that made them).  Without
        --refine_* no call is made"""
        refine = getattr(self, '_refine', None)
        if refine:
            dm.set_lesion_refine()
        try:
            yield
        finally:
            if refine:
                dm.set_lesion_refine(**refine)

    def _shard(self, x, y=None):
        """Contiguous shard of a global batch for this rank (Keras splits the batch across replicas [TF-2.6]); a batch
        that does not divide evenly (the last batch of an evaluation set) gives its remainder to the first ranks."""
        if self.ctx.world == 1:
            return x, y
        lo, hi = distributed.shard_bounds(len(x), self.ctx.rank, self.ctx.world, even=False)
        return x[lo:hi], (None if y is None else y[lo:hi])

    def _rank_sum(self, a):
        """the sum of an array over the ranks (counts travel as doubles: exact integers far beyond 2^24 pixels)"""
        return np.asarray(self.device_model.comm_allreduce(a.ravel()), np.float64).reshape(a.shape)

    def _shard_fn(self, dataset):
        """the split for the elements of `dataset`: none for one rank and for datasets that hand every rank its part already
        (tfrecord.TFRecordDataset(shard=...): `pre_sharded`)"""
        if self.ctx.world == 1 or getattr(dataset, 'pre_sharded', False):
            return lambda x, y=None: (x, y)
        return self._shard

    # ---- checkpoints (engine.py:55-78, 103-106, 224-231) -----------------------------------------------------
    def get_ckpts(self, base_path):
        return list_ckpts(base_path, self.ckpt_pattern)

    def _auto_resume(self, base_path):
        if not os.path.exists(base_path):
            return
        ckpts = self.get_ckpts(base_path)
        if not ckpts:
            return
        latest_step = max(ckpts.keys())
        self.load(ckpts[latest_step])
        self.current_step = latest_step
        logging.warning(f'Resumed from {latest_step}')

    def save(self, path, fileformat=None):
        """Weights + Adam slots + BN moving statistics + step counters: `<path>.index` (JSON) and `<path>.data-00000-of-00001`."""
        dm = self.device_model
        if self.ctx.world > 1:
            dm.comm_average_state()      # BN moving statistics: mean over replicas (ON_READ / MEAN aggregation [TF-2.6])
        if self.ctx.rank != 0:
            return self
        m, v, iterations = dm.get_opt_state()
        # deploy_options.ema: the array `ema` and the index entry "ema" beside the raw weights (always written with the raw weights
        # in place); without the option both files are what they were
        more, more_index = {}, {}
        if self.ema is not None:
            average, num_updates = dm.get_ema()
            more = dict(ema=average)
            more_index = dict(ema=dict(decay=self.ema['decay'], warmup=self.ema['warmup'], num_updates=int(num_updates)))
        # a mapping in deploy_options.optimizer: the index entry "optimizer" (class name and config).  The data file keeps its
        # arrays: SGD's accumulator is adam_m, its adam_v zeros.  With the string adam both files are what they were
        if self.optimizer is not None:
            more_index['optimizer'] = dict(class_name=self.optimizer['class_name'], config=self.optimizer['config'])
        os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
        with open(path + '.data-00000-of-00001', 'wb') as f:
            np.savez(f, params=dm.get_params(), state=dm.get_state(), adam_m=m, adam_v=v, **more)
        index = dict(format='dnnca-ckpt-1', step=int(self.current_step), iterations=int(iterations),
                     learning_rate=float(self.learning_rate),
                     variables=[dict(name=n, shape=list(s), trainable=t, offset=o) for n, s, t, o in dm.param_infos()], **more_index)
        with open(path + '.index', 'w') as f:      # written last: its presence marks a complete checkpoint
            json.dump(index, f)
        return self

    def load(self, path, weights='raw'):
        """weights='raw': the checkpoint as it was written; with deploy_options.ema the average and its update count come back too
        (a checkpoint without one: the average restarts from the loaded weights, with a warning; an average in the file is ignored
        without the option).  weights='ema': the file's averaged weights become the parameters (inference; needs no device average)"""
        check_weights(weights)
        dm = self.device_model
        with open(path + '.index') as f:
            index = json.load(f)
        have = [(v['name'], tuple(v['shape']), v['trainable'], v['offset']) for v in index['variables']]
        if have != [(n, tuple(s), t, o) for n, s, t, o in dm.param_infos()]:
            raise ValueError(f'checkpoint {path} does not match the model (assert_existing_objects_matched)')
        # the slots of another family (Adam / AdamW <-> SGD) mean something else; a checkpoint without the entry was written by Adam
        wrote = index.get('optimizer', {}).get('class_name', 'Adam')
        mine = 'Adam' if self.optimizer is None else self.optimizer['class_name']
        if slot_family(wrote) != slot_family(mine):
            raise ValueError(f'checkpoint {path} holds the optimizer slots of {wrote}: they cannot resume {mine}')
        if weights == 'ema' and 'ema' not in index:
            raise ValueError(f'checkpoint {path} holds no weight average (weights=\'ema\')')
        with np.load(path + '.data-00000-of-00001') as z:
            dm.set_params(z['ema' if weights == 'ema' else 'params'])
            if dm.n_state:
                dm.set_state(z['state'])
            dm.set_opt_state(z['adam_m'], z['adam_v'], index['iterations'])
            if self.ema is not None and weights == 'raw':
                if 'ema' in index:
                    dm.set_ema_state(z['ema'], index['ema']['num_updates'])
                else:
                    logging.warning('checkpoint %s holds no weight average: it restarts from the loaded weights', path)
                    self._set_ema(dm)          # e <- p, num_updates = 0
        return self

    # ---- training (engine.py:80-137) -------------------------------------------------------------------------
    def train(self, dataset, val_data=None, save_path=None, save_freq=100, max_steps=None, early_stop_steps=None,
              visualization=None, auto_resume=True, profile=False):
        # gradient accumulation: a train step is a micro-step, and everything below keeps counting micro-steps; checkpoints,
        # validation passes and the end of the run only ever fall between cycles (refused here, before any data is read)
        check_accumulation_schedule(self.accumulation, save_freq, max_steps, 0)
        self._build(dataset, also=(val_data,))
        dm = self.device_model
        if auto_resume and save_path is not None:
            self._auto_resume(os.path.join(save_path, 'checkpoints'))
        check_accumulation_schedule(self.accumulation, save_freq, max_steps, self.current_step)
        schedule = eval(self.learning_rate_scheduler) if self.learning_rate_scheduler is not None else None  # engine.py:98-100
        log_file = None
        if save_path is not None and self.ctx.rank == 0:
            os.makedirs(os.path.join(save_path, 'checkpoints'), exist_ok=True)
            os.makedirs(os.path.join(save_path, 'tfevents'), exist_ok=True)
            log_file = open(os.path.join(save_path, 'tfevents', 'train_log.csv'), 'a')
        if visualization:
            logging.warning('visualization callbacks are outside the accelerated path: ignored')
        cfg = dm.loss_cfg(**self.loss.device_cfg())
        results = History(self.model)
        results.params = dict(epochs=max_steps, steps=1, verbose=0)
        best_val, wait = np.inf, 0
        shard = self._shard_fn(dataset)
        source = iter(dataset)
        step = self.current_step
        if profile:
            dm.profile_enable(1)
        # Input side (annotator/data.py:110,143 `.prefetch(AUTOTUNE)` + Keras' asynchronous feeding): a BatchFeeder thread draws
        # the elements, shards them and uploads them into the model's staging slots on a copy stream while the GPU is still on
        # the previous step; the loop enqueues the step and reads the scalars of the step BEFORE it, so one step is always queued
        # behind the running one.  Checkpoint / validation steps, the last step and DNNCA_NO_FEEDER=1 read them at once.
        feeder = None
        if hasattr(dm, 'staging') and not os.environ.get('DNNCA_NO_FEEDER') and (max_steps is None or step < max_steps):
            try:
                first = next(source)
            except StopIteration:
                first = None
            if first is not None:
                feeder = source = BatchFeeder(dm, source, shard, first=first)
            else:
                source = iter(())
        pending = None          # (slot, step, lr) of an enqueued step whose scalars have not been read
        t0 = time.time()
        train_objs = self._train_metrics_begin(dm)      # None: the option is off

        def log_step(at, out, lr, extra=None, counts=None):
            logs = dict(loss=float(out.loss))
            if train_objs is not None:
                logs.update(self._train_metric_logs(train_objs, counts))
            logs['lr'] = lr
            if extra:
                logs.update(extra)
            results.log(at - 1, logs)
            if log_file is not None:
                log_file.write('%d,%s\n' % (at, ','.join('%s=%s' % (k, _csv_value(v)) for k, v in logs.items())))
            if self.ctx.rank == 0 and (at % 100 == 0 or at == max_steps):
                logging.info('step %d loss %.6f lr %.3g (%.1f steps/s)', at, out.loss, lr,
                             (at - results.epoch[0]) / max(time.time() - t0, 1e-9))

        def read_pending():
            nonlocal pending
            if pending is not None:
                slot_, at, lr = pending
                pending = None
                out_ = feeder.ring.out(slot_)       # waits for that step only; raises its label / weight assertions
                counts_ = feeder.ring.confusion(slot_) if train_objs is not None else None
                feeder.release(slot_)
                log_step(at, out_, lr, counts=counts_)

        try:
            while max_steps is None or step < max_steps:
                try:
                    item = next(source)
                except StopIteration:
                    logging.warning('dataset exhausted at step %d', step)
                    break
                if schedule is not None:
                    self.learning_rate = float(schedule(step, self.learning_rate))
                if feeder is None:
                    item = ('host', item)
                slot, out, counts = None, None, None
                if item[0] == 'staged':              # float (x, y), already on its way into a staging slot
                    _, slot, px, py, n = item
                    feeder.ring.train_step(slot, px, py, n, self.learning_rate, cfg)
                elif item[0] == 'raw':               # uint8 source batch in a staging slot: augmentation kernels, then the step
                    _, slot, src, batch, n = item
                    feeder.ring.wait(slot)
                    xb, yb = augment_on_device(dm, batch, shard, src_ptr=src)
                    dm.check_dev(xb, yb, n)
                    feeder.ring.train_step(slot, xb.ptr, yb.ptr, n, self.learning_rate, cfg)
                else:
                    batch = item[1]
                    if isinstance(batch, augment.RawBatch):
                        xb, yb = augment_on_device(dm, batch, shard)
                        out = dm.train_step_dev(xb, yb, xb.shape[0], self.learning_rate, cfg, want_out=True)
                    else:
                        x, y = shard(np.asarray(batch[0]), np.asarray(batch[1]))
                        out = dm.train_step(x, y, self.learning_rate, cfg)
                    counts = dm.last_step_confusion() if train_objs is not None else None
                step += 1
                self.current_step = step
                read_pending()                       # the step before this one (its slot goes back to the feeder)
                boundary = step % save_freq == 0 and (save_path is not None or val_data is not None)
                if slot is not None:
                    if not boundary and (max_steps is None or step < max_steps):
                        pending = (slot, step, self.learning_rate)
                        continue
                    out = feeder.ring.out(slot)
                    if train_objs is not None:
                        counts = feeder.ring.confusion(slot)
                    feeder.release(slot)
                extra = {}
                if save_path is not None and step % save_freq == 0:
                    self.save(os.path.join(save_path, 'checkpoints', self.ckpt_pattern.format(epoch=step)))
                stop = False
                if val_data is not None and step % save_freq == 0:
                    if self.ema is not None and self.ema['validate'] == 'ema':
                        # the exchange launches go on the model's stream, behind the step just read; val_* and early stopping
                        # refer to the averaged weights, and the raw ones are back before the next step
                        self._averaged_in_use = True          # (_ensure_capacity: this model cannot be replaced now)
                        try:
                            with dm.averaged_weights():
                                val = self._evaluate(val_data, staged=feeder is not None)
                        finally:
                            self._averaged_in_use = False
                    else:
                        val = self._evaluate(val_data, staged=feeder is not None)      # on the ring's evaluation slots
                    extra.update({'val_' + k: v for k, v in val.items()})
                    if early_stop_steps is not None:
                        if val['loss'] < best_val:
                            best_val, wait = val['loss'], 0
                        else:
                            wait += 1
                            stop = wait >= early_stop_steps
                log_step(step, out, self.learning_rate, extra, counts)
                if stop:
                    logging.warning('early stopping at step %d', step)
                    break
            read_pending()
            if self.accumulation > 1 and step % self.accumulation:
                # the data set ended (or the run stopped) inside a cycle: its gradients are dropped, never applied as a short mean
                logging.warning('gradient accumulation: step %d ends %d micro-steps into a cycle of %d; the partial cycle is dropped',
                                step, step % self.accumulation, self.accumulation)
                dm.set_accumulation(self.accumulation)
        finally:
            if feeder is not None:
                feeder.close()
            if train_objs is not None and self.device_model is dm:
                dm.train_metrics(None)
        if log_file is not None:
            log_file.close()
        if profile and save_path is not None and self.ctx.rank == 0:
            with open(os.path.join(save_path, 'tfevents', 'kernel_profile.txt'), 'w') as f:
                for row in sorted(dm.profile(), key=lambda r: -r[2]):
                    f.write('%-28s launches %8d  total %10.3f ms\n' % row[:3])
        return results

    def _train_metrics_begin(self, dm):
        """train_metrics: device -- a set of pixel metric objects of the train steps' own (never the validation objects), their
        thresholds (all metrics' at once, as _evaluate_staged takes them) switched on in the device model.  None when off."""
        if not self.train_metrics:
            return None
        objs = [copy.deepcopy(m) for m in self.metrics]
        thr = np.concatenate([m.thresholds for m in objs]) if objs else np.zeros(0, np.float32)
        if thr.size > 1024:
            raise ValueError('train_metrics: %d thresholds over all pixel metrics, at most 1024' % thr.size)
        dm.train_metrics(thr)
        return objs

    def _train_metric_logs(self, objs, counts):
        """the step's (tp, fp, fn, tn) rows of every threshold -> {metric name: result()}.  Data parallel: the counts are summed
        over ranks first (as doubles: exact integers), as MirroredStrategy's sync-on-read metric variables are"""
        counts = np.asarray(counts if counts is not None else [], np.float64).reshape(-1, 4)
        if self.ctx.world > 1:
            counts = self._rank_sum(counts)
        for m in objs:
            m.reset_state()
        _spread_counts(objs, counts)
        return OrderedDict((m.name, _log_value(m)) for m in objs)

    # ---- evaluation (engine.py:139-210) ----------------------------------------------------------------------
    def _evaluate(self, dataset, staged=False, tta_mask=None, temperature=None, ensemble=None):
        """keras Model.evaluate(return_dict=True): mean loss over batches + pixel metrics, training=False.  One batch of
        the dataset is one test step per replica: the positive-rate class weight (utils/losses.py:24-27) is taken over the
        whole per-replica batch, never over a chunk of it.
        tta_mask (evaluate --tta): after a batch's test step DeviceModel.forward_tta runs on the same slices, so the pixel and
        region metrics read the mean over the views; `loss` stays the loss of the untransformed view (the test step's own).
        temperature (evaluate --temperature): the probabilities the metrics read are scaled once behind the test step (and behind
        forward_tta when that runs); `loss` stays the unscaled test step's.
        ensemble (evaluate --ensemble: the members are set in the device model): after a batch's test step
        DeviceModel.forward_ensemble runs on the same slices in the place of forward_tta, so the metrics read the mean over the
        members (and their views); `loss` stays the loss of member 0's untransformed view.  Under data parallel every rank holds
        the same members."""
        cfg_kw = self.loss.device_cfg()
        for m in self.metrics + self.region_metrics:
            m.reset_state()
        region_groups = region_metrics.group_by_spec(self.region_metrics)

        total, count = 0.0, 0

        def step(dm_, xb, yb, cfg):         # one test step: loss, pixel metrics, region counts (one device run per distinct spec)
            nonlocal total, count
            out = dm_.eval_step(xb, yb, cfg)
            total += float(out.loss) * len(xb)
            count += len(xb)
            if ensemble:
                dm_.forward_ensemble(xb, tta_mask or 1, return_prob=False)
            elif tta_mask is not None:
                dm_.forward_tta(xb, tta_mask, return_prob=False)
            if temperature is not None:
                dm_.scale_temperature(temperature, len(xb))
            for m in self.metrics:
                m.update_state(dm_, yb)
            for spec, ms in region_groups:
                c = dm_.region_confusion(yb, spec)
                for m in ms:
                    m.add_counts(c)
        shard = self._shard_fn(dataset)
        if staged and self._staged_eval_possible():
            total, count, dataset = self._evaluate_staged(dataset, cfg_kw, shard, region_groups)  # what is left: batches the ring could not take
        for el in dataset:
            x, y = augment.raw_to_float(el) if isinstance(el, augment.RawBatch) else el
            x, y = shard(np.asarray(x), np.asarray(y))
            if len(x):
                self._ensure_capacity(len(x))
            dm = self.device_model
            if 0 < len(x) <= dm.max_batch:
                step(dm, x, y, dm.loss_cfg(**cfg_kw))
            elif len(x):
                # HBM cannot hold the batch in one step: chunks, each with the weight of the WHOLE batch passed explicitly
                kw = dict(cfg_kw)
                if kw.get('weight') is None:
                    if kw.get('label_smoothing'):
                        logging.warning('label smoothing + chunked validation: the class weight is taken per chunk')
                    else:
                        rate = float(np.asarray(y, np.float64).mean())
                        kw['weight'] = 1.0 / rate if rate > 0 else 1.0          # utils/losses.py:25-27
                cfg = dm.loss_cfg(**kw)
                for i in range(0, len(x), dm.max_batch):        # (region metrics are per slice: chunks give the whole batch's counts)
                    step(dm, x[i:i + dm.max_batch], y[i:i + dm.max_batch], cfg)
        if self.ctx.world > 1:
            total, count = (float(v) for v in self.device_model.comm_allreduce([total, count]))
            for m in self.metrics + self.region_metrics:
                m.merge(self._rank_sum)
        results = OrderedDict(loss=total / max(count, 1))
        for m in self.metrics:
            results[m.name] = _log_value(m)
        for m in self.region_metrics:
            results[m.name] = m.result()
        return results

    def _staged_eval_possible(self):
        n_thr = sum(len(m.thresholds) for m in self.metrics)
        return (hasattr(self.device_model, 'staging') and not os.environ.get('DNNCA_NO_FEEDER') and n_thr <= 1024 and
                all(hasattr(m, 'thresholds') and hasattr(m, 'counts') for m in self.metrics))

    def _evaluate_staged(self, dataset, cfg_kw, shard, region_groups=()):
        """The test steps of _evaluate over the staging ring (feeder.py): batches travel to HBM on the copy stream while the
        previous one is evaluated, every metric's thresholds share ONE confusion histogram that stays on the device and is read
        once at the end (exact integer counts), and a batch's loss is read one step late.  Region metrics (region_groups: one
        device spec each) count on the device beside the histogram and are read once too.  Returns (loss sum, sample count,
        the batches the ring could not take -- larger than max_batch -- for the chunked path)."""
        dm = self.device_model
        source = iter(dataset)
        try:
            first = next(source)
        except StopIteration:
            return 0.0, 0, []
        self._ensure_capacity(len(shard(np.asarray(first.raw if isinstance(first, augment.RawBatch) else first[0]))[0]))
        dm = self.device_model
        feeder = BatchFeeder(dm, source, shard, slots=BatchFeeder.EVAL_SLOTS, first=first)
        ring = feeder.ring
        thr = np.concatenate([m.thresholds for m in self.metrics]) if self.metrics else np.zeros(0, np.float32)
        cfg = dm.loss_cfg(**cfg_kw)
        total, count, left, pending = 0.0, 0, [], None
        ring.eval_begin(thr)
        region_on = False
        try:
            if region_groups:
                ring.eval_region_begin([spec for spec, _ in region_groups])
                region_on = True
            for item in feeder:
                if item[0] == 'host':
                    left.append(item[1])
                    continue
                if item[0] == 'raw':         # uint8 slices in the slot: centre crop, / 255 and the feature-label split on the device
                    _, slot, src, batch, n = item
                    ring.wait(slot)
                    xv, yv = dm.augment_u8(shard(batch.raw)[0], augment.plain_params(n), batch.output_size, batch.label_index,
                                           contrast_channels=(), src_ptr=src)
                    dm.check_dev(xv, yv, n)
                    px, py = xv.ptr, yv.ptr
                else:
                    _, slot, px, py, n = item
                ring.eval_step(slot, px, py, n, cfg)
                if pending is not None:
                    total += float(ring.out(pending[0]).loss) * pending[1]
                    count += pending[1]
                    feeder.release(pending[0])
                pending = (slot, n)
            if pending is not None:
                total += float(ring.out(pending[0]).loss) * pending[1]
                count += pending[1]
        finally:
            feeder.close()
            region_counts = ring.eval_region_end() if region_on else []
            counts = np.asarray(ring.eval_end(), np.float64).reshape(-1, 4)
        _spread_counts(self.metrics, counts)
        for (_, ms), c in zip(region_groups, region_counts):
            for m in ms:
                m.add_counts(c)
        return total, count, left

    def eval(self, dataset, save_path, viz_ds=None, tag='val', avoid_overwrite=False, export_path=None, export_images=False,
             visualize_sensitivity=False, export_csv=False, min_interval=1, step_range=None, overlay=False,
             export_casewise_metrics=False, exam_ds=None, exam_lesions=False, exam_threshold=(0.5,), exam_iou=casewise.EXAM_IOU,
             exam_min_area=0, exam_filter_size=5, exam_resize_factor=1.0, exam_max_lesions=256, exam_link_min_overlap=1,
             surface_ds=None, surface_distances=False, surface_threshold=(0.5,), surface_percentile=casewise.SURFACE_PERCENTILE,
             surface_min_area=0, surface_filter_size=5, surface_resize_factor=1.0, surface_max_samples=65536, tta='none',
             uncertainty_ds=None, uncertainty=False, uncertainty_thresholds=(0.5,), calibration_ds=None, calibration=False,
             calibration_bins=casewise.CALIBRATION_BINS, calibration_temperatures=None, temperature=None,
             visualize_attribution=False, attribution_steps=None, attribution_baseline=None, weights='raw', detection_ds=None,
             detection=False, detection_min_confidence=None, detection_factor=None, detection_max_candidates=None,
             detection_min_area=None, detection_rounds=None, detection_iou=None, detection_link_min_overlap=None,
             detection_max_lesions=None, bootstrap=None, bootstrap_seed=None, bootstrap_level=None, bootstrap_stratified=False,
             ensemble=None, refine_hysteresis=None, refine_closing=None, refine_fill_holes=False):
        """weights (`evaluate --weights ema`): every checkpoint is loaded with its averaged weights as the parameters (load(...,
        weights='ema')); everything downstream reads that model unchanged.  Checkpoints without an average are an error that names
        the first, raised before anything is evaluated.
        exam_lesions (`evaluate --exam_lesions`): after every checkpoint's evaluation rank 0 also runs _exam_lesion_pass over
        exam_ds (batches (x, y, paths, sliceIDs), a data set of its own: viz_ds is not needed) and writes exam_lesion_results.csv,
        exam_lesion_cases.csv and exam_lesion_matches.csv under <export_path>/<tag>/; every other file is what it is without it.
        surface_distances (`evaluate --surface_distances`): likewise rank 0 runs _surface_pass over surface_ds (the same kind of data
        set; the two flags may share one) and writes surface_results.csv, surface_cases.csv and surface_slices.csv there.
        tta (`evaluate --tta`, tta.MODES): with a mode other than 'none' the probabilities every pass reads -- the pixel and region
        metrics of the per-batch test step, the Visualizer, the exam-lesion and the surface pass -- are the mean over the mode's
        flip / transpose views (DeviceModel.forward_tta).  The evaluation then runs batch by batch, not over the staged ring;
        `loss` stays the loss of the untransformed view, and --visualize_sensitivity the gradient of the plain forward.
        uncertainty (`evaluate --tta MODE --uncertainty`): after every checkpoint's evaluation rank 0 also runs _uncertainty_pass
        over uncertainty_ds (the same kind of data set as exam_ds; the flags may share one) and writes uncertainty_results.csv and
        uncertainty_slices.csv under <export_path>/<tag>/: pixels and mean spread of the views per pixel outcome at every one of
        uncertainty_thresholds.  Every other file is what it is without the flag.  Needs a tta mode other than 'none'.
        calibration (`evaluate --calibration`): after every checkpoint's evaluation rank 0 also runs _calibration_pass over
        calibration_ds (the same kind of data set; the flags may share one) and writes calibration_results.csv, calibration_bins.csv
        and calibration_slices.csv under <export_path>/<tag>/: reliability table, ECE, MCE, Brier score, NLL and the temperature
        that minimises the NLL over calibration_temperatures (None: casewise.CALIBRATION_GRID; T = 1 is always in).  With and
        without a tta mode.
        temperature (`evaluate --temperature T`): every probability read -- by the pixel and region metrics, the Visualizer and every
        extra pass, --calibration included -- is scaled by DeviceModel.scale_temperature, once per forward.  The evaluation then
        runs batch by batch, `loss` stays the unscaled test step's and the spread of --uncertainty that of the unscaled views.
        None or 1: nothing new runs.
        visualize_attribution (`evaluate --visualize_attribution`): the Visualizer pass also runs DeviceModel.integrated_gradients
        (attribution_steps path points, default casewise.ATTRIBUTION_STEPS; attribution_baseline 'black' or 'mean') on the slices
        each plain forward left on the device and writes per slice step_<step>_attribution.csv (export_csv) and
        step_<step>_attribution.png (export_images: only then does a map leave the device), and per checkpoint a line of
        attribution_results.csv under <export_path>/<tag>/.  Like the sensitivity it is the attribution of the plain forward, also
        under tta / temperature.  Needs export_csv or export_images; every other file is what it is without the flag.
        detection (`evaluate --detection`): after every checkpoint's evaluation rank 0 also runs _detection_pass over detection_ds
        (the same kind of data set as exam_ds; the flags may share one) and writes detection_results.csv, detection_froc.csv,
        detection_cases.csv and detection_candidates.csv under <export_path>/<tag>/: ranked lesion candidates of the detection map
        (DeviceModel.detection_map with the detection_* values, check_detection), lesion-level AP and FROC, exam-level AUROC.  Under
        tta / temperature / weights the map is that of the probabilities they give.  Every other file is what it is without it.
        bootstrap (`evaluate --bootstrap R`, check_bootstrap): the detection and the exam-lesion pass also resample their exams R
        times on the device (DeviceModel.bootstrap_detection / bootstrap_sums, once per checkpoint and threshold) and write
        detection_bootstrap.csv, detection_bootstrap_replicates.csv and exam_lesion_bootstrap.csv under <export_path>/<tag>/: per
        metric the estimate, and mean, deviation and the bootstrap_level interval of its replicates.  bootstrap_stratified draws
        within the exams with and without a labelled tumour (detection only).  Every other file is what it is without it.
        ensemble (`evaluate --ensemble MEMBER [MEMBER ...]`, MEMBER = RUN_DIR[:STEP], at most 15): every probability read -- by
        the pixel and region metrics, the Visualizer and every extra pass -- is the mean over the checkpoint of save_path (member
        0) and the members' checkpoints of the same step (or of their pinned step), each under the tta mode when one is given
        (DeviceModel.forward_ensemble, one call per batch; check_ensemble resolves and checks every member before anything is
        evaluated).  The evaluation then runs batch by batch; `loss`, --visualize_sensitivity and --visualize_attribution stay
        those of member 0's plain forward.  With uncertainty (which --ensemble allows without a tta mode) the spread every file
        reads is the total over members and views, and ensemble_uncertainty_results.csv is written too: the mean between-member,
        within-member and total spread per pixel outcome.  None: nothing new runs.
        refine_hysteresis, refine_closing, refine_fill_holes (`evaluate --refine_hysteresis LOW --refine_closing K
        --refine_fill_holes`, check_refine): stored in the device model once (DeviceModel.set_lesion_refine), before the first
        table call; the prediction masks of the exam-lesion and the surface pass are then the refined ones -- one setting for both;
        LOW lies below every exam_threshold and surface_threshold.  Labels, the region metrics, the casewise counts and the
        detection pass (the refinement is switched off around its table calls and back on) are what they are without the flags.
        Needs exam_lesions or surface_distances; without the flags no call is made."""
        check_uncertainty(uncertainty, tta, ensemble)
        refine = check_refine(refine_hysteresis, refine_closing, refine_fill_holes,
                              [float(t) for t in (exam_threshold if exam_lesions else ())] +
                              [float(t) for t in (surface_threshold if surface_distances else ())],
                              consumers=bool(exam_lesions or surface_distances))
        bootstrap = check_bootstrap(bootstrap, bootstrap_seed, bootstrap_level, bootstrap_stratified, detection, exam_lesions)
        detection = check_detection(detection, detection_min_confidence, detection_factor, detection_max_candidates, detection_min_area,
                                    detection_rounds, detection_iou, detection_link_min_overlap, detection_max_lesions)
        attribution = check_attribution(visualize_attribution, attribution_steps, attribution_baseline, export_csv, export_images)
        temperature = check_temperature(temperature)
        if calibration:
            calibration_bins, calibration_grid = check_calibration(calibration_bins, calibration_temperatures)
        for flag, given in (('--visualize_sensitivity', visualize_sensitivity), ('--visualize_attribution', attribution)):
            if given and not getattr(self.model, 'supports_sensitivity', True):
                raise NotImplementedError('%s is not implemented for model: %s (the input-gradient pass covers the U-Net models only)'
                                          % (flag, self.model_config['model']))
        load_kw = {}
        if check_weights(weights) == 'ema':
            check_ema_checkpoints(select_ckpts(self.get_ckpts(os.path.join(save_path, 'checkpoints')), min_interval, step_range).values())
            load_kw = dict(weights='ema')
        visited = select_ckpts(self.get_ckpts(os.path.join(save_path, 'checkpoints')), min_interval, step_range) if ensemble else {}
        if ensemble:
            check_ensemble(save_path, ensemble, list(visited), weights)
        tta_mask = None if tta == tta_modes.NONE else tta_modes.mask_of(tta, *_element_shape(dataset)[1:3])
        self._build(dataset)
        self._set_refine(refine)
        member_paths = check_ensemble(save_path, ensemble, list(visited), weights, self.device_model.param_infos()) if ensemble else {}
        if ensemble:
            logging.info('evaluate --ensemble: %d members beside %s; the evaluation runs batch by batch (the staged ring has no '
                         'ensemble) and `loss` stays the loss of member 0\'s untransformed view', len(ensemble), save_path)
        if tta_mask is not None:
            logging.info('evaluate --tta %s: the evaluation runs batch by batch (the staged ring has no test-time augmentation)', tta)
        if temperature is not None:
            logging.info('evaluate --temperature %g: the evaluation runs batch by batch (the staged ring does not scale)', temperature)
        more = {} if temperature is None else dict(temperature=temperature)     # the passes get the keyword only with a temperature
        if ensemble:                         # and that of --ensemble only with members
            more['ensemble'] = True
        ckpt_path = os.path.join(save_path, 'checkpoints')
        if not export_path:
            export_path = os.path.join(save_path, 'tfevents')
        if os.path.exists(os.path.join(export_path, tag)):
            if avoid_overwrite:
                while os.path.exists(os.path.join(export_path, tag)):
                    tag += '_'
            else:
                raise ValueError(f'tag: {tag} already exists.')
        if step_range is None:
            step_range = 0, float('inf')
        else:
            assert len(step_range) == 2
            assert 0 <= step_range[0] <= step_range[1]
        # the Visualizer (engine.py:171-183, callbacks.py): casewise counts and images of viz_ds after each checkpoint's evaluation,
        # on rank 0 alone over the whole of viz_ds (data parallel: the other ranks skip it)
        visualize = viz_ds is not None and (export_csv or export_images) and self.ctx.rank == 0
        viz_root = os.path.join(export_path, tag)
        casewise_rows = []
        writer = casewise.Writer() if visualize else None
        attribution_table, attribution_names = [], []      # the lines of attribution_results.csv; the modalities of its share columns
        # the keywords travel only with their flags: the temperature to every pass, the bootstrap to the two that resample exams
        # (the exam-lesion pass has no strata)
        exam_more = dict(bootstrap=dict(bootstrap, stratified=False)) if bootstrap else {}
        detection_more = dict(bootstrap=bootstrap) if bootstrap else {}
        on = lambda flag, ds: bool(flag) and ds is not None and self.ctx.rank == 0       # noqa: E731
        lead, C = ['step', 'threshold'], casewise
        passes = [          # in the order they run, after a checkpoint's evaluation and its Visualizer pass
            _Pass(on(exam_lesions, exam_ds),
                  lambda step: self._exam_lesion_pass(
                      exam_ds, step, [float(t) for t in exam_threshold], exam_iou, exam_link_min_overlap,
                      dict(resize_factor=exam_resize_factor, filter_size=exam_filter_size, min_area=exam_min_area,
                           max_lesions=exam_max_lesions), tta_mask=tta_mask, **more, **exam_more),
                  [('exam_lesion_results.csv', lead, C.EXAM_RESULT_COLUMNS), ('exam_lesion_cases.csv', lead, C.EXAM_CASE_COLUMNS),
                   ('exam_lesion_matches.csv', lead, C.EXAM_MATCH_COLUMNS)] +
                  ([('exam_lesion_bootstrap.csv', lead, C.BOOTSTRAP_COLUMNS)] if bootstrap else [])),
            _Pass(on(surface_distances, surface_ds),
                  lambda step: self._surface_pass(
                      surface_ds, step, [float(t) for t in surface_threshold], float(surface_percentile),
                      dict(resize_factor=surface_resize_factor, filter_size=surface_filter_size, min_area=surface_min_area,
                           max_samples=surface_max_samples), tta_mask=tta_mask, **more),
                  [('surface_results.csv', lead, C.SURFACE_RESULT_COLUMNS), ('surface_cases.csv', lead, C.SURFACE_CASE_COLUMNS),
                   ('surface_slices.csv', lead, C.SURFACE_SLICE_COLUMNS)]),
            _Pass(on(uncertainty, uncertainty_ds),
                  lambda step: self._uncertainty_pass(uncertainty_ds, step, [float(t) for t in uncertainty_thresholds], tta_mask, **more),
                  [('uncertainty_results.csv', lead, C.UNCERTAINTY_RESULT_COLUMNS), ('uncertainty_slices.csv', lead, C.UNCERTAINTY_SLICE_COLUMNS)] +
                  ([('ensemble_uncertainty_results.csv', lead, C.ENSEMBLE_UNCERTAINTY_RESULT_COLUMNS)] if ensemble else [])),
            _Pass(on(calibration, calibration_ds),
                  lambda step: self._calibration_pass(calibration_ds, step, calibration_bins, calibration_grid, tta_mask, **more),
                  [('calibration_results.csv', ['step'], C.CALIBRATION_RESULT_COLUMNS),
                   ('calibration_bins.csv', ['step'], C.CALIBRATION_BIN_COLUMNS),
                   ('calibration_slices.csv', ['step'], C.CALIBRATION_SLICE_COLUMNS)]),
            _Pass(on(detection, detection_ds),
                  lambda step: self._detection_pass(detection_ds, step, detection, tta_mask=tta_mask, **more, **detection_more),
                  [('detection_results.csv', ['step'], C.DETECTION_RESULT_COLUMNS), ('detection_froc.csv', ['step'], C.DETECTION_FROC_COLUMNS),
                   ('detection_cases.csv', ['step'], C.DETECTION_CASE_COLUMNS),
                   ('detection_candidates.csv', ['step'], C.DETECTION_CANDIDATE_COLUMNS)] +
                  ([('detection_bootstrap.csv', ['step'], C.BOOTSTRAP_COLUMNS),
                    ('detection_bootstrap_replicates.csv', ['step'], C.DETECTION_REPLICATE_COLUMNS)] if bootstrap else []))]
        rows = OrderedDict()
        previous_step = None
        for ckpt_step, ckpt_path_ in self.get_ckpts(ckpt_path).items():
            if not step_range[0] <= ckpt_step <= step_range[1]:
                continue
            if previous_step is not None and (ckpt_step - previous_step) < min_interval:
                logging.warning(f'Ignored {ckpt_path_} due to min_interval:{min_interval}.')
                continue
            previous_step = ckpt_step
            self.load(ckpt_path_, **load_kw)
            if ensemble:
                self._set_ensemble(ckpt_path_, member_paths[ckpt_step], weights)
            rows[ckpt_step] = self._evaluate(dataset, staged=True) if tta_mask is None and not more else \
                self._evaluate(dataset, staged=False, tta_mask=tta_mask, **more)
            if visualize:
                self._visualize(viz_ds, ckpt_step, viz_root, export_csv, export_images, overlay, casewise_rows, writer,
                                sensitivity=bool(visualize_sensitivity), tta_mask=tta_mask, **more,
                                **(dict(attribution=attribution + (attribution_table, attribution_names)) if attribution else {}))
            for ps in passes:
                if ps.on:
                    ps.append(ps.run(ckpt_step))
        if attribution and visualize:
            cols = casewise.ATTRIBUTION_RESULT_COLUMNS + ['share_%s' % n for n in attribution_names] + ['mean_relative_gap', 'max_relative_gap']
            passes.append(_Pass(True, None, [('attribution_results.csv', ['step'], cols)], [attribution_table]))
        for ps in passes:
            if ps.on:
                ps.write(os.path.join(export_path, tag))
        if writer is not None:
            writer.close()
        if export_csv and self.ctx.rank == 0:
            os.makedirs(os.path.join(export_path, tag), exist_ok=True)
            with open(os.path.join(export_path, tag, 'results.csv'), 'w') as f:
                cols = list(next(iter(rows.values())).keys()) if rows else ['loss']
                f.write('step,' + ','.join(cols) + '\n')
                for step, r in rows.items():
                    f.write(str(step) + ',' + ','.join(str(r[c]) for c in cols) + '\n')
            if visualize:
                with open(os.path.join(export_path, tag, 'casewise_results.csv'), 'w', newline='') as f:
                    f.write(casewise.table_csv(casewise.column_names(), casewise_rows))
        return rows

    def _visualize(self, viz_ds, step, root, export_csv, export_images, overlay, casewise_rows, writer, sensitivity=False,
                   tta_mask=None, temperature=None, attribution=None, ensemble=None):
        """One Visualizer pass (callbacks.py process_batch / _emit) over viz_ds batches (x, y, paths, sliceIDs): forward
        (training=False), the per-slice region counts (export_csv), the composite images (export_images), then the files.  The
        probabilities stay on the device; only the counts and the uint8 images come back.  casewise_rows gains one row per slice,
        in dataset order.  sensitivity (--visualize_sensitivity, callbacks.py:290-313): the input-gradient pass on the slices the
        forward left on the device; per slice a CSV (export_csv) and a bar chart (export_images) of the normalised channel sums.
        attribution (--visualize_attribution): (steps, baseline, table, names) -- DeviceModel.integrated_gradients on the same
        slices; per slice a CSV (export_csv) and the per-modality maps (export_images: the map is fetched only then); `table` gains
        this checkpoint's line of attribution_results.csv and `names` is set to the modalities."""
        spec = casewise.device_spec()
        attr_shares, attr_gaps = [], []
        names = casewise.column_names()
        for dm, xb, yb, pk in self._forwarded_splits(viz_ds, tta_mask, temperature=temperature, **self._with(ensemble)):
            tags = [casewise.tag_of(p, k) for p, k in pk]
            if export_csv:
                counts = dm.region_confusion_slices(yb, [spec])
                for t, c in zip(tags, counts):
                    values = casewise.row_values(c, t)
                    casewise_rows.append(values)
                    writer.submit(casewise.csv_path(root, t, step), casewise.series_csv, names, values)
            if export_images:
                # the labels went up with the counts already: the renderer reuses them
                images = dm.render_composite(None if export_csv else yb, len(xb), casewise.RATIO, overlay)
                for t, im in zip(tags, images):
                    writer.submit(casewise.image_path(root, t, step), casewise.encode_png, im)
            if sensitivity:
                sens = casewise.normalise_sensitivity(dm.input_sensitivity(batch=len(xb)))
                mods = casewise.modality_names(getattr(viz_ds, 'slice_types', None), sens.shape[1])
                for t, row in zip(tags, sens):
                    if export_csv:
                        writer.submit(casewise.sensitivity_path(root, t, step, 'csv'), casewise.sensitivity_csv, mods, row)
                    if export_images:
                        writer.submit(casewise.sensitivity_path(root, t, step, 'images'),
                                      lambda r: casewise.encode_png(casewise.sensitivity_chart(r)), row)
            if attribution:
                ig = dm.integrated_gradients(batch=len(xb), steps=attribution[0], baseline=attribution[1],
                                             return_map=bool(export_images))
                shares = casewise.attribution_shares(ig.absolute)
                mods = casewise.modality_names(getattr(viz_ds, 'slice_types', None), shares.shape[1])
                attribution[3][:] = mods
                attr_shares += list(shares)
                attr_gaps += list(casewise.attribution_gap(ig.signed, ig.endpoints)[1])
                for b, t in enumerate(tags):
                    if export_csv:
                        writer.submit(casewise.attribution_path(root, t, step, 'csv'), casewise.attribution_csv, mods, shares[b],
                                      ig.signed[b], ig.absolute[b], ig.endpoints[b])
                    if export_images:
                        writer.submit(casewise.attribution_path(root, t, step, 'images'),
                                      lambda m, n: casewise.encode_png(casewise.attribution_image(m, n)), ig.map[b], mods)
        if attribution:
            attribution[2].append([int(step)] + casewise.attribution_summary(attribution[0], attribution[1], attr_shares, attr_gaps))

    @staticmethod
    def _with(ensemble):
        """the keyword of --ensemble for _forwarded_splits: it travels only with the flag"""
        return dict(ensemble=True) if ensemble else {}

    def _forwarded_splits(self, ds, tta_mask, spread=False, temperature=None, labels=True, ensemble=None):
        """The one walk over an analysis data set, ds batches (x, y, paths, sliceIDs) or, with labels=False, annotate's (x, ...,
        paths, sliceIDs), where a label in between is never looked at: empty batches skipped, the model grown to the batch, the
        batch split by max_batch and every split forwarded with its probabilities left on the device (_forward_on_device).
        Yields (the device model, x and y of the split, [(path, sliceID)] of its slices); y is None with labels=False."""
        for el in ds:
            x, paths, ids = np.asarray(el[0], np.float32), el[-2], el[-1]
            y = np.asarray(el[1], np.float32) if labels else None
            if not len(x):
                continue
            self._ensure_capacity(len(x))
            dm = self.device_model
            for i in range(0, len(x), dm.max_batch):
                xb, yb = x[i:i + dm.max_batch], None if y is None else y[i:i + dm.max_batch]
                _forward_on_device(dm, xb, tta_mask, spread=spread, temperature=temperature, **self._with(ensemble))
                yield dm, xb, yb, list(zip(paths[i:i + dm.max_batch], ids[i:i + dm.max_batch]))

    def _exam_lesion_pass(self, ds, step, thresholds, iou, min_overlap, kw, tta_mask=None, temperature=None, bootstrap=None,
                          ensemble=None):
        """One pass over ds batches (x, y, paths, sliceIDs) for `evaluate --exam_lesions`: per max_batch split one forward whose
        probabilities stay on the device and one DeviceModel.lesion_table_matched per threshold; then per threshold and exam
        casewise.link_lesions on either plane and casewise.match_exam_lesions.  Returns the new lines of (exam_lesion_results.csv,
        exam_lesion_cases.csv, exam_lesion_matches.csv), each led by step and threshold.
        A slice continues the one before it by _SliceChain's rule: the same exam path and the next slice number, across splits and
        batches.  continues[0] of a matched call refers to the model's last matched call, which with several thresholds was
        another threshold's: the call is then led by a one-slice call that puts this threshold's rows of the slice before back
        (its probabilities and labels are kept on the host for that; a single threshold needs neither).
        bootstrap (what check_bootstrap returned): per threshold one DeviceModel.bootstrap_sums over the exams' counts after the
        summary, and a fourth table, the new lines of exam_lesion_bootstrap.csv."""
        several = len(thresholds) > 1
        found = [[] for _ in thresholds]     # per threshold: the casewise.SliceRecord of every slice
        chain, tail, carry_of = _SliceChain('evaluate'), None, None
        for dm, xb, yb, pk in self._forwarded_splits(ds, tta_mask, temperature=temperature, **self._with(ensemble)):
            continues = chain.continues(dm, pk)
            for ti, thr in enumerate(thresholds):
                if continues[0] and carry_of != ti:
                    dm.lesion_table_matched(tail[1], prob=tail[0], continues=[False], threshold=thr, **kw)
                found[ti] += casewise.slice_records(dm.lesion_table_matched(yb, batch=len(xb), continues=continues, threshold=thr, **kw), pk)
                carry_of = ti
            if several:
                tail = dm.last_prob(len(xb))[-1:], yb[-1:].reshape(1, *yb.shape[1:3])
        results, cases, matches, intervals = [], [], [], []
        for thr, mine in zip(thresholds, found):
            lead = [int(step), repr(thr)]
            mine_cases = []
            for exam, recs in casewise.by_exam(mine).items():
                case, lines = casewise.match_records(casewise.match_exam_lesions, exam, recs, min_overlap, iou=iou)
                mine_cases.append(case)
                matches += [lead + l for l in lines]
            cases += [lead + c for c in mine_cases]
            results.append(lead + casewise.exam_match_summary(mine_cases))
            if bootstrap and mine_cases:
                sums = self.device_model.bootstrap_sums(np.array([c[1:7] for c in mine_cases], np.int32), bootstrap['replicates'],
                                                        seed=bootstrap['seed'])['sums']
                values = [casewise.exam_match_replicate_values(s, len(mine_cases)) for s in sums]
                intervals += [lead + l for l in casewise.bootstrap_lines(casewise.EXAM_BOOTSTRAP_METRICS, results[-1][-4:], values,
                                                                         bootstrap)]
        return (results, cases, matches, intervals) if bootstrap else (results, cases, matches)

    def _detection_pass(self, ds, step, det, tta_mask=None, temperature=None, bootstrap=None, ensemble=None):
        """One pass over ds batches (x, y, paths, sliceIDs) for `evaluate --detection`: per max_batch split one forward whose
        probabilities stay on the device, DeviceModel.detection_map in place (the buffer then holds the map) and one
        DeviceModel.lesion_table_matched on it (casewise.detection_table_args: the rows are the candidates, max_prob their
        confidence); then per exam casewise.link_lesions on either plane and casewise.detection_match, and casewise.detection_summary
        over all exams.  det: what check_detection returned.  Returns the new lines of (detection_results.csv, detection_froc.csv,
        detection_cases.csv, detection_candidates.csv), each led by step.  Slices continue each other by _SliceChain's rule.
        bootstrap (what check_bootstrap returned): one DeviceModel.bootstrap_detection over the same cases after the summary, and
        two more tables, the new lines of detection_bootstrap.csv and detection_bootstrap_replicates.csv."""
        kw = casewise.detection_table_args(det['cfg'], det['max_lesions'])
        found, exhausted = [], 0             # the casewise.SliceRecord of every slice
        chain = _SliceChain('evaluate')
        for dm, xb, yb, pk in self._forwarded_splits(ds, tta_mask, temperature=temperature, **self._with(ensemble)):
            continues = chain.continues(dm, pk)
            _, map_records = dm.detection_map(len(xb), **det['cfg'])
            exhausted += int(map_records['exhausted'].sum())
            with self._unrefined(dm):        # the map's regions are final
                found += casewise.slice_records(dm.lesion_table_matched(yb, batch=len(xb), continues=continues, **kw), pk)
        lead, cases, candidates = [int(step)], [], []
        for exam, recs in casewise.by_exam(found).items():
            case, lines = casewise.match_records(casewise.detection_match, exam, recs, det['link_min_overlap'], iou=det['iou'])
            cases.append(case)
            candidates += [lead + l for l in lines]
        result, froc = casewise.detection_summary(cases, exhausted)
        tables = [lead + result], [lead + l for l in froc], [lead + casewise.detection_case_values(c) for c in cases], candidates
        if not bootstrap:
            return tables
        intervals, replicates = [], []
        if cases:
            exams, ranked = casewise.detection_bootstrap_inputs(cases)
            rows = self.device_model.bootstrap_detection(exams, ranked, bootstrap['replicates'], seed=bootstrap['seed'],
                                                         strata=casewise.bootstrap_pool(exams['tumours'] > 0, bootstrap['stratified']))
            values = [casewise.detection_replicate_values(r, len(cases)) for r in rows]
            intervals = [lead + l for l in casewise.bootstrap_lines(casewise.DETECTION_BOOTSTRAP_METRICS, result[7:18], values, bootstrap)]
            replicates = [lead + casewise.detection_replicate_line(i, r, v) for i, (r, v) in enumerate(zip(rows, values))]
        return tables + (intervals, replicates)

    def _surface_pass(self, ds, step, thresholds, percentile, kw, tta_mask=None, temperature=None, ensemble=None):
        """One pass over ds batches (x, y, paths, sliceIDs) for `evaluate --surface_distances`: per max_batch split one forward whose
        probabilities stay on the device and one DeviceModel.surface_distances per threshold; only the counts and the boundary
        pixels' squared distances come back.  Then per threshold casewise.surface_slice_values per slice, surface_exam_values per
        exam (the slices of one exam path, in the order of the data set) and surface_summary.  Returns the new lines of
        (surface_results.csv, surface_cases.csv, surface_slices.csv), each led by step and threshold.  No slice depends on another:
        nothing is carried between calls."""
        found = [[] for _ in thresholds]     # per threshold and slice: (exam, slice, counts, d2 of the prediction, d2 of the label)
        for dm, xb, yb, pk in self._forwarded_splits(ds, tta_mask, temperature=temperature, **self._with(ensemble)):
            for ti, thr in enumerate(thresholds):
                counts, samples, _ = dm.surface_distances(yb, batch=len(xb), threshold=thr, **kw)
                for b, (p, k) in enumerate(pk):
                    mine = samples[samples['slice'] == b]
                    found[ti].append((p, int(k), counts[b], mine['d2'][mine['side'] == 0], mine['d2'][mine['side'] == 1]))
        results, cases, slices = [], [], []
        for thr, mine in zip(thresholds, found):
            lead = [int(step), repr(thr)]
            slice_values = [casewise.surface_slice_values(*rec, percentile=percentile) for rec in mine]
            exam_values = [casewise.surface_exam_values(exam, [(c, d2_pred, d2_true) for _, _, c, d2_pred, d2_true in recs], percentile=percentile)
                           for exam, recs in casewise.by_exam(mine).items()]
            slices += [lead + v for v in slice_values]
            cases += [lead + v for v in exam_values]
            results.append(lead + casewise.surface_summary(slice_values, exam_values))
        return results, cases, slices

    def _uncertainty_pass(self, ds, step, thresholds, tta_mask, temperature=None, ensemble=None):
        """One pass over ds batches (x, y, paths, sliceIDs) for `evaluate --tta MODE --uncertainty`: per max_batch split one
        DeviceModel.forward_tta_spread whose mean and spread stay on the device and one DeviceModel.spread_by_outcome for all
        thresholds (in runs of 64); only the counts and sums per outcome come back.  Returns the new lines of
        (uncertainty_results.csv, uncertainty_slices.csv), each led by step and threshold.
        ensemble (--ensemble): the forward is DeviceModel.forward_ensemble and the spread those two files read the total; the
        between- and within-member planes are then read back with the mean and go through spread_by_outcome's plane inputs too,
        and a third table comes back, the new lines of ensemble_uncertainty_results.csv."""
        found = [[] for _ in thresholds]     # per threshold and slice: (exam, slice, outcome entry)
        parts = [[[] for _ in thresholds] for _ in range(2)] if ensemble else []      # between, within: per threshold the outcome entries
        for dm, xb, yb, pk in self._forwarded_splits(ds, tta_mask, spread=True, temperature=temperature, **self._with(ensemble)):
            y = yb.reshape(len(xb), *yb.shape[1:3])
            planes = (dm.last_prob(len(xb)),) + dm.last_ensemble_spread(len(xb)) if ensemble else None
            for t0 in range(0, len(thresholds), 64):
                out = dm.spread_by_outcome(y, thresholds[t0:t0 + 64], batch=len(xb))
                for ti, per_slice in enumerate(out, t0):
                    found[ti] += [(p, int(k), o) for (p, k), o in zip(pk, per_slice)]
                for part, plane in zip(parts, planes[1:] if ensemble else ()):
                    for ti, per_slice in enumerate(dm.spread_by_outcome(y, thresholds[t0:t0 + 64], prob=planes[0], spread=plane), t0):
                        part[ti] += list(per_slice)
        results, slices, components = [], [], []
        for ti, (thr, mine) in enumerate(zip(thresholds, found)):
            lead = [int(step), repr(thr)]
            slices += [lead + casewise.outcome_slice_values(*rec) for rec in mine]
            results.append(lead + casewise.outcome_summary([rec[2] for rec in mine]))
            if ensemble:
                components.append(lead + casewise.ensemble_outcome_summary(parts[0][ti], parts[1][ti], [rec[2] for rec in mine]))
        return (results, slices, components) if ensemble else (results, slices)

    def _calibration_pass(self, ds, step, n_bins, temperatures, tta_mask=None, temperature=None, ensemble=None):
        """One pass over ds batches (x, y, paths, sliceIDs) for `evaluate --calibration`: per max_batch split one forward whose
        probabilities stay on the device and one DeviceModel.calibration for all temperatures; only the integer tables and the NLL
        sums come back.  Returns the new lines of (calibration_results.csv, calibration_bins.csv, calibration_slices.csv), each led
        by step; the pooled values come from the tables and NLL rows of all slices summed (casewise.calibration_summary)."""
        at_1 = [float(t) for t in temperatures].index(1.0)
        bins, totals, nll, slices = [], [], [], []
        for dm, xb, yb, pk in self._forwarded_splits(ds, tta_mask, temperature=temperature, **self._with(ensemble)):
            b, t, n = dm.calibration(yb.reshape(len(xb), *yb.shape[1:3]), n_bins, temperatures, batch=len(xb))
            bins.append(b), totals.append(t), nll.append(n)
            slices += [[int(step)] + casewise.calibration_slice_values(p, k, b[j], t[j], n[j, at_1]) for j, (p, k) in enumerate(pk)]
        if not bins:
            return [], [], []
        result, lines = casewise.calibration_summary(np.concatenate(bins), np.concatenate(totals), temperatures, np.concatenate(nll))
        return [[int(step)] + result], [[int(step)] + l for l in lines], slices

    def predict(self, dataset):
        """Probabilities [N, H, W, 1] for every element of `dataset` (elements are x or (x, ...))."""
        self._build(dataset)
        dm = self.device_model
        outs = []
        for el in dataset:
            x = np.asarray(el[0] if isinstance(el, (tuple, list)) else el)
            for i in range(0, len(x), dm.max_batch):
                outs.append(dm.forward(x[i:i + dm.max_batch], training=False))
        return np.concatenate(outs) if outs else np.zeros((0,))

    def annotate(self, dataset, save_path, output, step=None, threshold=0.5, min_area=0, filter_size=5, resize_factor=1.0,
                 max_lesions=256, export_images=False, link_slices=False, link_min_overlap=1, tta='none', uncertainty=False,
                 temperature=None, lesion_features=False, feature_bins=None, feature_ring=None, weights='raw', detection_map=False,
                 detection_min_confidence=None, detection_factor=None, detection_max_candidates=None, detection_min_area=None,
                 detection_rounds=None, detection_link_min_overlap=None, detection_max_lesions=None, ensemble=None,
                 refine_hysteresis=None, refine_closing=None, refine_fill_holes=False):
        """`annotator predict`: the lesions of slices that have no label.  Loads checkpoint `step` of save_path (None: the latest);
        per batch (x, paths, sliceIDs) of `dataset` (make_dataset(..., include_meta=True, labels=False)) one forward whose
        probabilities stay on the device, then DeviceModel.lesion_table: threshold, filter_size x filter_size opening, components
        of at least min_area pixels -- only the table and the uint8 masks come back.  Files under `output`: lesions.csv (one line
        per lesion, dataset order then row order), slices.csv (one line per slice; truncated = 1: more than max_lesions
        components, lesions.csv holds the first max_lesions) and, with export_images, <exam>/<slice>/mask.png (the opened,
        area-filtered mask).  Returns {'step', 'slices', 'lesions'}.
        link_slices: DeviceModel.lesion_table_linked instead, which also counts the common pixels of the lesions of neighbouring
        slices.  A slice continues the one before it when it has the same exam path and the next slice number -- across max_batch
        splits and across batches of `dataset`; the first slice of the run continues nothing.  casewise.link_lesions joins lesions
        that share at least link_min_overlap pixels into exam lesions: exam_lesions.csv (one line per exam lesion) and
        exam_lesion_parts.csv (one line per line of lesions.csv, in its order) are written beside the other files, which are
        what they are without the flag; the returned dict gains 'exam_lesions'.
        tta (`predict --tta`, tta.MODES): with a mode other than 'none' the one forward per chunk is DeviceModel.forward_tta with the
        mode's view mask: the tables and masks are those of the mean probability over the views.
        uncertainty (`predict --tta MODE --uncertainty`): the forward is DeviceModel.forward_tta_spread and the table comes from
        DeviceModel.lesion_table_spread (with link_slices lesion_table_linked runs as it does without the flag and the spread records
        come from a second call); lesion_uncertainty.csv (one line per line of lesions.csv, in its order) and slice_uncertainty.csv
        are written beside the other files, which are what they are without the flag, and with export_images
        <exam>/<slice>/uncertainty.png (only then does a spread plane leave the device).  Needs a tta mode other than 'none'.
        temperature (`predict --temperature T`): the probabilities are scaled by DeviceModel.scale_temperature, once behind every
        forward, before the table reads them; the spread stays that of the unscaled views.  None or 1: nothing new runs.
        lesion_features (`predict --lesion_features [--feature_bins 32] [--feature_ring 3]`): the table comes from
        DeviceModel.lesion_table_features, which also reads the staged input batch -- the untransformed one under tta -- below and
        around every lesion (with link_slices or uncertainty the table runs as it does without the flag and the feature records
        come from a second call); lesion_features.csv (one line per line of lesions.csv, in its order: outline, axes and per
        modality mean, deviation, extrema, percentiles and the contrast against the ring of feature_ring pixels around the
        lesion) and with link_slices exam_lesion_features.csv (one line per line of exam_lesions.csv, pooled from the parts'
        integers) are written beside the other files, which are what they are without the flag.
        weights (`predict --weights ema`): the checkpoint's averaged weights become the parameters (load(..., weights='ema')); a
        checkpoint without an average is an error that names it.  Every table and mask is then that of the averaged model.
        detection_map (`predict --detection_map [--detection_* ...]`, check_detection): per chunk, LAST -- it replaces the
        probability buffer -- DeviceModel.detection_map in place, then a table read from the map (casewise.detection_table_args):
        DeviceModel.lesion_table, or with link_slices DeviceModel.lesion_table_matched against empty labels, whose carry is a chain
        of its own, so the candidates' links do not disturb those of the lesions.  candidates.csv (the columns of lesions.csv plus
        confidence), slice_candidates.csv (candidates, rounds, dropped, exhausted per slice), with link_slices exam_candidates.csv
        and with export_images <exam>/<slice>/detection.png (8-bit grey, rint(D * 255): only then does a map leave the device) are
        written beside the other files, which are what they are without the flag; the returned dict gains 'candidates'.
        ensemble (`predict --ensemble MEMBER [MEMBER ...]`, MEMBER = RUN_DIR[:STEP], at most 15): the one forward per chunk is
        DeviceModel.forward_ensemble over the checkpoint of save_path (member 0) and the members' checkpoints -- of their pinned
        step, else of `step`, else their run's latest -- each under the tta mode when one is given; every table and mask is that
        of the mean over the members.  With uncertainty (which --ensemble allows without a tta mode) the spread every file reads
        is the total over members and views, and slice_ensemble_uncertainty.csv is written too: per slice the mean and largest
        between-member and within-member spread (the two planes leave the device only then).  None: nothing new runs.
        refine_hysteresis, refine_closing, refine_fill_holes (`predict --refine_hysteresis LOW --refine_closing K
        --refine_fill_holes`, check_refine): stored in the device model once (DeviceModel.set_lesion_refine), before the first
        table call; every table and mask.png then reads the refined mask -- the region at LOW around the pixels at `threshold`,
        opened, closed by K x K, its holes filled.  The table read from a detection map is not refined: the refinement is switched
        off around it and back on.  No file gains or loses a column; without the flags no call is made."""
        check_uncertainty(uncertainty, tta, ensemble)
        refine = check_refine(refine_hysteresis, refine_closing, refine_fill_holes, [threshold])
        det = check_detection(detection_map, detection_min_confidence, detection_factor, detection_max_candidates, detection_min_area,
                              detection_rounds, None, detection_link_min_overlap, detection_max_lesions, flag='--detection_map')
        check_weights(weights)
        temperature = check_temperature(temperature)
        feature_bins, feature_ring = casewise.check_features(lesion_features, feature_bins, feature_ring)
        if self.ctx.world > 1:
            raise RuntimeError('annotate runs in a single process (WORLD_SIZE is %d): start it without the launcher' % self.ctx.world)
        tta_mask = None if tta == tta_modes.NONE else tta_modes.mask_of(tta, *_element_shape(dataset)[1:3])
        if ensemble:
            check_ensemble(save_path, ensemble, [step], weights)
        self._build(dataset)
        self._set_refine(refine)
        member_paths = check_ensemble(save_path, ensemble, [step], weights, self.device_model.param_infos())[step] if ensemble else None
        step = self._load_step(save_path, step, weights)
        if ensemble:
            self._set_ensemble(self.get_ckpts(os.path.join(save_path, 'checkpoints'))[step], member_paths, weights)
        features = dict(bins=feature_bins, ring=feature_ring) if lesion_features else None
        modalities = casewise.modality_names(getattr(dataset, 'slice_types', None), _element_shape(dataset)[3]) if lesion_features else None
        scale = {} if temperature is None else dict(temperature=temperature)      # the forward gets the keyword only with a temperature
        scale.update(self._with(ensemble))   # and that of --ensemble only with members
        component_rows = []                  # ensemble + uncertainty: the lines of slice_ensemble_uncertainty.csv
        lesion_rows, slice_rows, lesion_spread_rows, slice_spread_rows = [], [], [], []
        feature_rows, linked_features = [], []       # linked_features: beside `linked`, every slice's feature records per lesion
        candidate_rows, slice_candidate_rows, candidates_linked = [], [], []         # detection_map: as lesion_rows / slice_rows / linked
        linked, chain = [], _SliceChain('predict')   # link_slices: the casewise.SliceRecord of every slice
        writer = casewise.Writer() if export_images else None
        try:
            for dm, xb, _, pk in self._forwarded_splits(dataset, tta_mask, spread=bool(uncertainty), labels=False, **scale):
                continues = chain.continues(dm, pk) if link_slices else None
                t = self._lesion_tables(dm, dict(batch=len(xb), threshold=threshold, resize_factor=resize_factor, filter_size=filter_size,
                                                 min_area=min_area, max_lesions=max_lesions, mask=bool(export_images)),
                                        continues, uncertainty, features)
                spread = dm.last_spread(len(xb)) if uncertainty and export_images else None
                if ensemble and uncertainty:
                    component_rows += [casewise.slice_ensemble_uncertainty_values(p, k, b_, w_)
                                       for (p, k), b_, w_ in zip(pk, *dm.last_ensemble_spread(len(xb)))]
                if det:                              # last: from here on the buffer holds the map, whose regions are final
                    with self._unrefined(dm):
                        new_tables = self._candidate_tables(dm, xb, pk, det, continues, writer, output)
                    for table, new in zip((candidate_rows, slice_candidate_rows, candidates_linked), new_tables):
                        table += new
                if link_slices:
                    linked += casewise.slice_records((t.rows, t.totals, t.masks, t.links), pk)
                for b, (p, k) in enumerate(pk):
                    mine = t.rows[t.rows['slice'] == b]
                    lesion_rows += [casewise.lesion_values(p, k, r) for r in mine]
                    slice_rows.append(casewise.slice_values(p, k, mine, t.totals[b]))
                    if export_images:
                        writer.submit(casewise.mask_path(output, casewise.tag_of(p, k)), casewise.encode_png, t.masks[b])
                    if lesion_features:
                        fmine = [None if f is None else f[t.rows['slice'] == b] for f in t.feats]
                        per_lesion = [tuple(None if f is None else f[j] for f in fmine) for j in range(len(mine))]
                        feature_rows += [casewise.lesion_feature_values(p, k, r, *f) for r, f in zip(mine, per_lesion)]
                        if link_slices:
                            linked_features.append(per_lesion)
                    if uncertainty:
                        smine = t.srows[t.rows['slice'] == b]
                        lesion_spread_rows += [casewise.lesion_uncertainty_values(p, k, r, q) for r, q in zip(mine, smine)]
                        slice_spread_rows.append(casewise.slice_uncertainty_values(p, k, mine, smine, t.totals[b], t.stotals[b]))
                        if export_images:
                            writer.submit(casewise.uncertainty_path(output, casewise.tag_of(p, k)),
                                          lambda s_: casewise.encode_png(casewise.uncertainty_image(s_)), spread[b])
        finally:
            if writer is not None:
                writer.close()
        os.makedirs(output, exist_ok=True)
        tables = [('lesions.csv', casewise.LESION_COLUMNS, lesion_rows), ('slices.csv', casewise.SLICE_COLUMNS, slice_rows)]
        res = dict(step=int(step), slices=len(slice_rows), lesions=len(lesion_rows))
        if uncertainty:
            tables += [('lesion_uncertainty.csv', casewise.LESION_UNCERTAINTY_COLUMNS, lesion_spread_rows),
                       ('slice_uncertainty.csv', casewise.SLICE_UNCERTAINTY_COLUMNS, slice_spread_rows)]
            if ensemble:
                tables.append(('slice_ensemble_uncertainty.csv', casewise.SLICE_ENSEMBLE_UNCERTAINTY_COLUMNS, component_rows))
        if lesion_features:
            tables.append(('lesion_features.csv', casewise.lesion_feature_columns(modalities), feature_rows))
        if link_slices:
            exam_rows, part_rows, exam_feature_rows = self._exam_tables(linked, linked_features if lesion_features else None, link_min_overlap)
            tables += [('exam_lesions.csv', casewise.EXAM_LESION_COLUMNS, exam_rows),
                       ('exam_lesion_parts.csv', casewise.EXAM_PART_COLUMNS, part_rows)]
            res['exam_lesions'] = len(exam_rows)
            if lesion_features:
                tables.append(('exam_lesion_features.csv', casewise.exam_lesion_feature_columns(modalities), exam_feature_rows))
        if det:
            tables += [('candidates.csv', casewise.CANDIDATE_COLUMNS, candidate_rows),
                       ('slice_candidates.csv', casewise.SLICE_CANDIDATE_COLUMNS, slice_candidate_rows)]
            res['candidates'] = len(candidate_rows)
            if link_slices:
                exam_candidates = []
                for exam, recs in casewise.by_exam(candidates_linked).items():
                    table, _ = casewise.link_records(exam, recs, det['link_min_overlap'])
                    exam_candidates += [r + [r[15]] for r in table]
                tables.append(('exam_candidates.csv', casewise.EXAM_CANDIDATE_COLUMNS, exam_candidates))
        for name, cols, table in tables:
            with open(os.path.join(output, name), 'w', newline='') as f:
                f.write(casewise.plain_csv(cols, table))
        return res

    def _load_step(self, save_path, step, weights):
        """annotate's checkpoint: `step` of save_path (None: the latest) loaded, raw or with its averaged weights -> its step"""
        ckpts = self.get_ckpts(os.path.join(save_path, 'checkpoints'))
        if not ckpts:
            raise ValueError(f'no checkpoint under {save_path}/checkpoints')
        if step is None:
            step = max(ckpts)
        if step not in ckpts:
            raise ValueError(f'no checkpoint of step {step} under {save_path}/checkpoints (have {sorted(ckpts)})')
        if weights == 'ema':
            check_ema_checkpoints([ckpts[step]])
        self.load(ckpts[step], **(dict(weights='ema') if weights == 'ema' else {}))
        return step

    @staticmethod
    def _lesion_tables(dm, kw, continues, uncertainty, features):
        """annotate's table calls on the split `dm` has just forwarded -> _SplitTables.  kw: the keywords every lesion_table* call
        takes; continues (link_slices, else None): lesion_table_linked; uncertainty: lesion_table_spread; features (lesion_features:
        dict(bins, ring), else None): lesion_table_features.  There is no linked table with spread or features and none with both:
        the spread and feature records of the same rows then come from a call of their own, without masks"""
        links = srows = stotals = feats = None
        if continues is not None:
            rows, totals, masks, links = dm.lesion_table_linked(continues=continues, **kw)
            if uncertainty:
                _, _, _, srows, stotals = dm.lesion_table_spread(**dict(kw, mask=False))
        elif uncertainty:
            rows, totals, masks, srows, stotals = dm.lesion_table_spread(**kw)
        elif features:
            rows, totals, masks, *feats = dm.lesion_table_features(**features, **kw)
        else:
            rows, totals, masks = dm.lesion_table(**kw)
        if features:
            if continues is not None or uncertainty:
                feats = dm.lesion_table_features(**features, **dict(kw, mask=False))[3:]
            if len(feats[0]) != len(rows):
                raise RuntimeError('predict: %d feature records beside %d lesions' % (len(feats[0]), len(rows)))
        if uncertainty and len(srows) != len(rows):
            raise RuntimeError('predict: %d spread records beside %d lesions' % (len(srows), len(rows)))
        return _SplitTables(rows, totals, masks, links, srows, stotals, feats)

    @staticmethod
    def _candidate_tables(dm, xb, pk, det, continues, writer, output):
        """annotate's detection-map part on a split, after every other read of the probabilities: DeviceModel.detection_map in
        place, then the table read from the map -- lesion_table, or with `continues` (link_slices) lesion_table_matched against
        empty labels -- and with a writer (export_images) the map itself.  Returns the split's (candidates.csv lines,
        slice_candidates.csv lines, SliceRecords for exam_candidates.csv: none without link_slices)"""
        _, map_records = dm.detection_map(len(xb), **det['cfg'])
        kw = casewise.detection_table_args(det['cfg'], det['max_lesions'])
        if continues is not None:
            rows, totals, masks, links, *_ = dm.lesion_table_matched(np.zeros((len(xb),) + xb.shape[1:3], np.float32), batch=len(xb),
                                                                     continues=continues, **kw)
        else:
            rows, _, _ = dm.lesion_table(batch=len(xb), mask=False, **kw)
        maps = dm.last_prob(len(xb)) if writer is not None else None
        candidates, slices = [], []
        for b, (p, k) in enumerate(pk):
            candidates += [casewise.candidate_values(p, k, r) for r in rows[rows['slice'] == b]]
            slices.append([p, int(k)] + [int(map_records[b][f]) for f in ('candidates', 'rounds', 'dropped', 'exhausted')])
            if writer is not None:
                writer.submit(casewise.detection_path(output, casewise.tag_of(p, k)),
                              lambda d_: casewise.encode_png(casewise.detection_image(d_)), maps[b])
        return candidates, slices, casewise.slice_records((rows, totals, masks, links), pk) if continues is not None else []

    @staticmethod
    def _exam_tables(linked, linked_features, min_overlap):
        """annotate --link_slices after the walk: the SliceRecords of every slice (and with lesion_features, beside them, every
        slice's feature records per lesion; else None) -> the lines of (exam_lesions.csv, exam_lesion_parts.csv,
        exam_lesion_features.csv)"""
        exam_rows, exam_feature_rows, parts_of = [], [], [None] * len(linked)
        # exam path -> the positions of its slices in `linked`, in the order of the data set
        for exam, where in casewise.by_exam([(rec.exam, pos) for pos, rec in enumerate(linked)]).items():
            where = [pos for _, pos in where]
            table, parts = casewise.link_records(exam, [linked[pos] for pos in where], min_overlap)
            exam_rows += table
            if linked_features is not None:      # the parts are in the order of the exam's lesions: gather every exam lesion's
                of = [f for pos in where for f in linked_features[pos]]
                exam_feature_rows += [casewise.exam_lesion_feature_values(exam, e, [f for f, part in zip(of, parts) if part[3] == e])
                                      for e in range(len(table))]
            for pos in where:        # the parts come slice after slice; lesions.csv is in the order of the data set
                n = len(linked[pos].rows)
                parts_of[pos], parts = parts[:n], parts[n:]
        return exam_rows, sum(parts_of, []), exam_feature_rows

    def get_config(self):
        return self.model_config
