/*
 * dnnca.h -- C ABI of libdnnca.so: the MI355X-native (gfx950, hand-written HIP) U-Net train/evaluate engine that
 * stands in for the TensorFlow/Keras numeric back-end of yoshihikoueno/DNNCancerAnnotator's hot path.
 *
 * The reference has no FFI boundary of its own on this path (it is Python on top of TensorFlow); each entry point below
 * cites the reference interface (file:line under annotator/) whose work it takes over.  The Python host
 * (dnncancerannotator_amd/engine.py, a mirror of annotator/engine.py:36-288) binds these with ctypes; INTEGRATION.md
 * shows the stub.
 *
 * Conventions: every function returns 0 on success or a negative DNNCA_E* code (message via dnnca_last_error());
 * nothing throws across the ABI; the caller owns host buffers; the library owns device memory; tensors are NHWC float32;
 * a model handle is bound to one HIP device + one stream and is not thread-safe; data parallel = one process per GPU,
 * each with its own handle, joined by dnnca_comm_init (RCCL over xGMI).
 */
#ifndef DNNCA_H
#define DNNCA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DNNCA_OK 0
#define DNNCA_EINVAL (-1)      /* bad argument / unsupported configuration */
#define DNNCA_EHIP (-2)        /* HIP runtime error (no device, launch failure, out of memory) */
#define DNNCA_ECOMM (-3)       /* RCCL error */
#define DNNCA_ESTATE (-4)      /* call sequence error (e.g. step before init) */
#define DNNCA_EASSERT (-5)     /* a reference-side tf.debugging.assert_* would have fired (utils/losses.py:30,91-99) */

enum { DNNCA_ARCH_UNET = 0, DNNCA_ARCH_MULMO = 1 };     /* models/tf_models/unet.py:194 UNetAnnotator, :285 MulmoUNetAnnotator */
/* models/tf_models/multiresunet.py MultiResUnet (configs/multiresunet.yaml).  Of dnnca_model_desc it reads arch, in_channels, height,
   width (multiples of 16), max_batch, n_filters_first (the U of the first MultiRes block, doubled per level; the reference uses 32)
   and dtype (DNNCA_F32 only); every other field is ignored: the graph is fixed (five levels, 2x2 pooling, 1x1 and 3x3 convs without
   bias, BatchNorm everywhere, ReLU, no regulariser).  It always runs on the shape-generic kernels plus the residual-join kernels. */
enum { DNNCA_ARCH_MULTIRES = 2 };
enum { DNNCA_PAD_VALID = 0, DNNCA_PAD_SAME = 1 };       /* model_options.padding (configs/unet.yaml:9) */
/* arithmetic type of the conv contractions.  DNNCA_BF16: the operands of the 3x3 convolutions with >= 32 channels and of the
   transposed convolutions with channel counts that are multiples of 64 are rounded to bfloat16 (round to nearest even) on
   their way into the matrix cores; weights, optimizer state, BatchNorm statistics and every accumulation stay float32.
   Activations ("bf16 acts", BASELINE.md configs[2]): tensors whose every reader rounds them anyway are kept as bfloat16 in
   HBM (bit-identical results), and so are -- this does round -- the input of a BatchNorm written by a 64-channel-multiple
   conv / transposed conv (batch statistics are those of the stored values) and the gradient arriving at a BatchNorm whose
   users are all such layers or a 2x2 max-pool.  DNNCA_NO_HALF_Z / DNNCA_NO_HALF_DY in the environment keep those in float32 */
enum { DNNCA_F32 = 0, DNNCA_BF16 = 1 };
enum { DNNCA_UNIQUE_ID_BYTES = 128 };

/* model_options of configs/{unet,unet_big,mulmo_unet}.yaml (unet.py:195-207) + the input element spec
 * (engine.py:93 model.build(dataset.element_spec[0].shape)). */
typedef struct dnnca_model_desc {
    int32_t arch;             /* DNNCA_ARCH_* */
    int32_t in_channels;      /* C of x[B,H,W,C]; mulmo builds one encoder per channel (unet.py:151-165) */
    int32_t height, width;    /* must be divisible by rate^n_downsample */
    int32_t max_batch;        /* activations are allocated once for this batch size */
    int32_t n_filters_first;  /* unet.yaml:3 */
    int32_t n_downsample;     /* unet.yaml:4 */
    int32_t rate;             /* unet.yaml:5 (pool window/stride, transposed-conv kernel/stride) */
    int32_t kernel_size;      /* unet.yaml:6 */
    int32_t conv_stride;      /* unet.yaml:7 (only 1 is supported; the reference configs use 1) */
    int32_t bn;               /* unet.yaml:8 */
    int32_t padding;          /* DNNCA_PAD_* (only SAME is supported; every reference config uses same) */
    int32_t reference_index;  /* unet.py:114 (mulmo: which encoder's skips feed the decoder) */
    int32_t n_conv;           /* components.py:25 (2) */
    float leaky_alpha;        /* 0 = relu; 0.3 = configs/additionals/leakyReLU.yaml */
    float l2;                 /* 0 = none; 0.01 = configs/additionals/kernel_regularizer.yaml */
    int32_t dtype;            /* DNNCA_F32 | DNNCA_BF16 */
    int32_t flags;            /* bit 0: force the generic (untuned) kernels everywhere -- used by the parity tests */
} dnnca_model_desc;

/* deploy_options.loss.config of configs/additionals/deploy_options.yaml:4-7 (utils/losses.py:41-56) */
typedef struct dnnca_loss_cfg {
    int32_t has_weight;       /* 0: weight = 1/positive_rate (or 1 when there are no positives), losses.py:24-27 */
    float weight;
    float weight_add;         /* losses.py:29 */
    float weight_mul;
    /* utils/losses.py:62-67: y_true = tfa.image.gaussian_filter2d(y_true, filter_shape, sigma) before everything else (positive
       rate, assertions, loss): REFLECT padding of (k-1)/2 rows/columns before and k-1-(k-1)/2 after, separable kernel
       softmax(-u^2 / (2 sigma^2)) over u = -k/2+1 .. k/2 (tensorflow-addons, absent third-party dependency: restated from its
       published algorithm) */
    int32_t label_smoothing;  /* 0 = off (the default, losses.py:46) */
    int32_t label_smoothing_filter_size;
    float label_smoothing_sigma;
} dnnca_loss_cfg;

typedef struct dnnca_step_out {
    float loss;               /* scalar Keras loss of the step (mean over batch [+ L2]); mean over ranks under DP */
    float positive_rate;      /* utils/losses.py:87-102 (rank-local) */
    float weight;             /* the positive-class weight actually applied (rank-local) */
    float label_min, label_max;
} dnnca_step_out;

/* pixel confusion counts at one threshold (prob > threshold: Keras Precision/Recall convention, metrics.yaml:2-6) */
typedef struct dnnca_confusion {
    double tp, fp, fn, tn;
} dnnca_confusion;

/* ---- process / device ---------------------------------------------------------------------------------------- */
const char* dnnca_version(void);
const char* dnnca_last_error(void);
int dnnca_device_count(int* count);
int dnnca_init(int device_ordinal);                 /* hipSetDevice; engine.py:260-263 (strategy creation) */

/* ---- model life-cycle: engine.py:254-288 from_config + engine.py:93 model.build ------------------------------- */
int dnnca_model_create(const dnnca_model_desc* desc, void** model_out);
int dnnca_model_destroy(void* model);

/* variables in Keras creation order (components.py:69-75,226-233,292-312; unet.py:166-176,273-277).
 * Conv2D kernels are HWIO, Conv2DTranspose kernels [kh,kw,Cout,Cin]. offset = position in the trainable (or state) flat vector. */
int dnnca_param_count(void* model, int* count);
int dnnca_param_info(void* model, int index, char* name, size_t name_cap, int64_t shape[4], int* ndim,
                     int* trainable, int64_t* offset);
int dnnca_num_trainable(void* model, int64_t* n);   /* floats in the trainable flat vector */
int dnnca_num_state(void* model, int64_t* n);       /* floats in the non-trainable flat vector (BN moving statistics) */

/* model.load_weights / save_weights (engine.py:197,224-231, ModelCheckpoint engine.py:103-106) */
int dnnca_set_params(void* model, const float* flat, int64_t n);
int dnnca_get_params(void* model, float* flat, int64_t n);
int dnnca_set_state(void* model, const float* flat, int64_t n);
int dnnca_get_state(void* model, float* flat, int64_t n);
int dnnca_get_grads(void* model, float* flat, int64_t n);          /* gradients of the last train step (parity tests) */
/* Adam slots + iteration counter (engine.py:276-284); checkpoint / auto-resume (engine.py:67-78) */
int dnnca_set_opt_state(void* model, const float* m, const float* v, int64_t n, int64_t iterations);
int dnnca_get_opt_state(void* model, float* m, float* v, int64_t n, int64_t* iterations);
int dnnca_set_adam(void* model, float beta1, float beta2, float epsilon);

/* Exponential moving average of the trainable variables (tf.train.ExponentialMovingAverage with num_updates): a float32 vector e of
 * dnnca_num_trainable elements on the device; the BatchNorm moving statistics are averages already and stay what they are.
 *   dnnca_model_set_ema    decay in (0, 1): allocates e, copies the weights into it and zeroes num_updates; decay == 0: frees it, and
 *                          every launch is again the one a model without an average runs; anything else: DNNCA_EINVAL
 * While it is on, the launch that applies Adam (pg_fold_adam_ema, g_adam_ema: 36 instead of 28 bytes per parameter) also moves e:
 * the thread that stores weight i computes e_i <- e_i - om * (e_i - p_i) with the p_i it has just written and
 * om = (float)(1 - d_n), d_n = min(decay, (1 + n) / (10 + n)) with warmup, d_n = decay without, formed in double for the n-th
 * update since set_ema / set_ema_state (plan dumps never count).  One thread per element, no atomics, nothing crosses to the host;
 * under data parallel every rank applies the same update to the same weights.
 *   dnnca_get_ema          e to host `flat` (NULL: only the count) and num_updates; synchronises
 *   dnnca_set_ema_state    `flat` into e and the count (checkpoint resume); synchronises
 *   dnnca_ema_exchange     one launch (ema_exchange) that exchanges the CONTENTS of the weight vector and e, exactly; a second call
 *                          restores both.  Every forward pass rebuilds its weight-derived operands from the weight vector, so all
 *                          inference entry points then run on the average.  While the average is in the weight vector,
 *                          dnnca_get_params returns it, dnnca_get_ema the raw weights, and dnnca_train_step*, dnnca_set_params,
 *                          dnnca_set_opt_state, dnnca_set_ema_state, dnnca_comm_broadcast_weights and dnnca_model_set_ema return
 *                          DNNCA_ESTATE.  Asynchronous: the launch goes on the model's stream.
 * The last three return DNNCA_ESTATE while no average is set. */
int dnnca_model_set_ema(void* model, float decay, int warmup);
int dnnca_get_ema(void* model, float* flat, int64_t n, int64_t* num_updates);
int dnnca_set_ema_state(void* model, const float* flat, int64_t n, int64_t num_updates);
int dnnca_ema_exchange(void* model);

/* ---- configurable optimizers: Adam, AdamW, SGD and gradient clipping (Keras 2.6 OptimizerV2 semantics [TF-2.6]) ---------------
 * g is the vector the optimizer receives: the folded gradient with the kernel_regularizer term, under data parallel after the
 * all-reduce and times 1 / world.  A "variable" is one trainable entry of dnnca_param_info, in that order.  Keras' order of the
 * gradient transforms: clipvalue c (g_i <- min(max(g_i, -c), c)), then clipnorm c (per variable V: g_V <- g_V * c / max(|g_V|, c))
 * or global_clipnorm c (the same with the norm over all of g).  The squares are summed in double in a fixed order (launches
 * grad_sqnorm, grad_clip_scale: no atomics), the scale c / max(norm, c) is formed in double and rounded to float once -- exactly 1
 * while norm <= c, so that such a gradient passes bit for bit -- and stays on the device: nothing synchronises with the host.
 *   DNNCA_OPT_ADAM   today's update, lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) formed on the host in double (launch opt_adam;
 *                    with every scale 1 bit-identical to g_adam)
 *   DNNCA_OPT_ADAMW  the same behind the decoupled decay p <- p - lr * weight_decay * p of the variables whose decay flag is set,
 *                    lr being this step's learning rate (Keras >= 2.11 / PyTorch; tfa.optimizers.AdamW leaves the lr factor out)
 *   DNNCA_OPT_SGD    momentum 0: p <- p - lr g; else a <- momentum a - lr g, p <- p + a, with nesterov p <- p + momentum a - lr g.
 *                    a lives in Adam's m slot (dnnca_get_opt_state), the v slot stays untouched, iterations counts as before
 * With a weight average (dnnca_model_set_ema) the launches are opt_adam_ema / opt_adamw_ema / opt_sgd_ema and carry it.
 *   dnnca_model_set_optimizer  a value of 0 switches its feature off.  kind ADAM with momentum, nesterov, weight_decay and the three
 *                    clips 0 stores beta1 / beta2 / epsilon (as dnnca_set_adam does), frees the tables, and the model launches what
 *                    it launched before (pg_fold_adam, g_adam).  Anything else builds a chunk table (fixed-size chunks, none across
 *                    two variables) once; train steps then run pg_fold [grad_sqnorm grad_clip_scale] opt_*: the fold does not wait
 *                    for the optimizer launch.  decay_per_variable: n_variables flags (kind ADAMW; may be NULL otherwise).
 *                    DNNCA_EINVAL, with nothing changed: an unknown kind; beta1 / beta2 outside [0, 1), epsilon < 0, momentum
 *                    outside [0, 1), weight_decay < 0, a clip < 0, or any of them not finite; clipnorm together with
 *                    global_clipnorm; momentum / nesterov with a kind other than SGD, weight_decay with one other than ADAMW;
 *                    n_variables other than the number of trainable variables.  DNNCA_ESTATE while the averaged weights are in
 *                    use.  Waits for the stream.
 *   dnnca_last_grad_norm  waits for the stream; *global = the norm over all of g (after clipvalue) of the last optimizer step,
 *                    per_variable[0 .. n) = the variables' norms (either may be NULL; n = 0 or the number of trainable variables);
 *                    zeros before the first step.  DNNCA_ESTATE when no clipping by norm is set
 *   dnnca_apply_gradients  Keras' optimizer.apply_gradients: uploads g_host [n = dnnca_num_trainable] into the gradient vector and
 *                    runs exactly the optimizer launches of a train step on it with learning rate lr (g_adam when no optimizer is
 *                    set), without a communicator: no all-reduce, scale 1.  Counts one iteration.  g_host has been copied when the call
 *                    returns; the launches go on the model's stream */
enum { DNNCA_OPT_ADAM = 0, DNNCA_OPT_ADAMW = 1, DNNCA_OPT_SGD = 2 };
typedef struct dnnca_optimizer_cfg {
    int32_t kind;               /* DNNCA_OPT_* */
    float beta1, beta2, epsilon;
    float momentum;             /* SGD, in [0, 1) */
    int32_t nesterov;           /* SGD with momentum > 0 */
    float weight_decay;         /* ADAMW, >= 0 */
    float clipvalue, clipnorm, global_clipnorm;      /* 0: off */
} dnnca_optimizer_cfg;
int dnnca_model_set_optimizer(void* model, const dnnca_optimizer_cfg* cfg, const uint8_t* decay_per_variable, int n_variables);
int dnnca_last_grad_norm(void* model, double* global, double* per_variable, int n);
int dnnca_apply_gradients(void* model, const float* g_host, int64_t n, float lr);

/* ---- gradient accumulation: one optimizer update from k micro-batches (deploy_options.gradient_accumulation_steps) -------------
 * A micro-step is one dnnca_train_step* (or dnnca_apply_gradients) call; a cycle is `steps` consecutive ones.  Every micro-step runs
 * forward, loss and backward as before (BatchNorm statistics per micro-batch, the step outputs of that micro-batch alone) and
 * leaves its gradient in g; a float32 accumulator a of dnnca_num_trainable elements takes a <- g on the first micro-step of a cycle
 * and a <- a + g on the later ones: one add per element per micro-step, in micro-step order, no atomics, bit-identical from run to
 * run (launch grad_accumulate: 8 bytes per parameter when it starts a cycle, 12 when it adds; on the pixel-group plan the fold of
 * such a micro-step takes the add and the step outputs along: pg_fold_acc, unless DNNCA_NO_FOLD_ACC is set when the model is
 * created).  Micro-steps 1 .. steps - 1 change nothing else: weights, optimizer slots, iterations, the weight average and its
 * num_updates stay bit for bit.  On micro-step `steps` the optimizer's launches (grad_sqnorm, grad_clip_scale, opt_*, g_adam[_ema])
 * read a in the place of g with gscale = (float)(1 / (steps * world)), formed in double: the mean of the cycle's gradients, a mean
 * of per-batch means.  The clips and dnnca_last_grad_norm refer to that mean; iterations and the weight average count one update
 * per cycle; lr is the value passed to that micro-step.  dnnca_get_grads keeps returning the last micro-batch's gradient.
 * Data parallel: micro-steps 1 .. steps - 1 all-reduce the loss slot alone (1 float), micro-step `steps` the accumulator with the
 * loss slot behind it (dnnca_num_trainable + 1 floats), one call each on the model's stream; the backward pass sends no buckets.
 * Plan dumps never move the position; DNNCA_PLAN_TRAIN lists the micro-step that would run next.
 *   dnnca_model_set_accumulation  steps 1: off, frees a, and every launch is again the one a model without it runs; 2 .. 4096:
 *                    allocates a (zeroed).  Sets the position to 0 -- a partial cycle is discarded -- and waits for the stream.
 *                    DNNCA_EINVAL outside [1, 4096], with nothing changed; DNNCA_ESTATE while the averaged weights are in use
 *   dnnca_get_accumulation  waits for the stream; a to host `flat` (NULL: none), *steps and *position = the micro-steps in a
 *                    (either may be NULL).  Right after an update: position 0 and the sum that was applied.  DNNCA_ESTATE while
 *                    accumulation is off
 *   dnnca_grad_accumulate_of  the kernel alone on host vectors of any length n >= 1: out_host = first ? g_host : acc_host + g_host
 *                    (with `first`, acc_host may be NULL); none of the model's vectors is touched.  Synchronises
 * dnnca_set_params and dnnca_set_opt_state set the position to 0; dnnca_model_set_optimizer and dnnca_model_set_ema keep it. */
int dnnca_model_set_accumulation(void* model, int steps);
int dnnca_get_accumulation(void* model, float* flat /* nullable */, int64_t n, int* steps, int* position);
int dnnca_grad_accumulate_of(void* model, const float* acc_host, const float* g_host, int64_t n, int first, float* out_host);

/* ---- the hot path, host buffers ------------------------------------------------------------------------------ */
/* UNetAnnotator.call (unet.py:279-282): probabilities [B,H,W,1]; logits = the tensor Keras caches as _keras_logits */
int dnnca_forward(void* model, const float* x_nhwc, int batch, int training, float* prob_out, float* logit_out);
/* ---- test-time augmentation (`annotator predict --tta`, `annotator evaluate --tta`; the reference has none) --------------------------
 * A view is a number k = 4 t + 2 v + h in 0..7 (the dihedral group of the square).  Applied to x [B,H,W,C]: first the flips,
 * xf[b,i,j,c] = x[b, v ? H-1-i : i, h ? W-1-j : j, c], then, with t, the transpose xk[b,i,j,c] = xf[b,j,i,c] (H == W).  `views` is a
 * bit mask in 1..255: bit k selects view k (0x0F: identity and the three flips; 0xFF: all eight).
 * dnnca_forward_tta stages x as dnnca_forward does and runs, for every selected view in ascending order, one inference forward
 * (training = 0) on that view of the batch; with p_k the sigmoid of its logits (the expression of dnnca_forward), i' = v ? H-1-i : i
 * and j' = h ? W-1-j : j the model's probability buffer receives
 *     prob[b,i,j] = (sum over the selected k, ascending, in float32, of p_k[b, t ? (j',i') : (i',j')]) / n      (float32 division)
 * n = the number of views.  No atomics: bit-identical from run to run.  Every consumer of "the last forward's probabilities"
 * (dnnca_get_prob, dnnca_pixel_confusion, dnnca_region_confusion*, dnnca_lesion_table*, dnnca_surface_distances,
 * dnnca_render_composite) then works on the mean; the staged batch that dnnca_render_composite and dnnca_input_sensitivity read is
 * the untransformed x (the views live in a buffer of their own, allocated for max_batch by the first call that needs it).  The
 * logits buffer holds the LAST selected view's logits, in that view's geometry, not the mean's.  Variables, BatchNorm state and
 * optimizer slots are untouched.  prob_out: NULL, or host [batch, H, W]; synchronises when it is given.
 * DNNCA_EINVAL, with nothing launched and nothing allocated: views of 0 or above 255; a transposed view (bits 4..7) when H != W; a
 * model whose output size is not its input size; batch outside [1, max_batch]. */
int dnnca_forward_tta(void* model, const float* x_nhwc, int batch, unsigned views, float* prob_out /* nullable */);
/* the two kernels of dnnca_forward_tta alone, on host buffers [batch, h, w(, c)] of any plane size (the library grows its own device
 * buffers); 1 <= batch <= max_batch, at most 65535 rows; both synchronise.
 *   dnnca_tta_view_of   dst = view `view` (0..7) of src [batch, h, w, c], c >= 1
 *   dnnca_tta_mean_of   prob_out [batch, h, w] = the mean above of the planes vals [n, batch, h, w], which hold the selected views'
 *                       outputs in ascending view order: probabilities (is_logits = 0), or logits that first go through the sigmoid
 * Both refuse what dnnca_forward_tta refuses, with h != w standing in for H != W. */
int dnnca_tta_view_of(void* model, const float* src, int batch, int h, int w, int c, int view, float* dst);
int dnnca_tta_mean_of(void* model, const float* vals, int batch, int h, int w, unsigned views, int is_logits, float* prob_out);
/* ---- how much the views disagree (`predict --tta MODE --uncertainty`, `evaluate --tta MODE --uncertainty`) ------------------------------
 * With p_k and n as above and the mean taken in exact arithmetic,
 *     spread[b,i,j] = sqrt((1/n) * sum over the selected k of (p_k - mean)^2)        (population standard deviation, float32)
 * computed in the shifted form d_k = p_k - p_first, var = (sum d^2 - (sum d)^2 / n) / n: |spread - want| <= 2^-18 want + 2^-23 against
 * the float64 standard deviation `want` of the same float32 p_k; exactly 0 where all selected p_k are the same float32 (so for a
 * single view everywhere); at most 0.5 up to that error.
 * dnnca_forward_tta_spread does and refuses everything dnnca_forward_tta does -- the probability buffer receives bit for bit that
 * call's mean -- with tta_moments in the place of tta_accumulate: the spread lands in a plane [max_batch, H, W] of the model's own,
 * allocated with three planes of running moments by the first call of this function (a model that never calls it allocates
 * neither).  The call marks the plane VALID for its batch; every other call that rewrites the probability buffer (dnnca_forward*,
 * dnnca_forward_tta, the train and eval steps, dnnca_pixel_confusion_of) marks it invalid.  prob_out, spread_out: NULL, or host
 * [batch, H, W]; synchronises when one is given.
 *   dnnca_tta_spread_of    the kernel alone on host planes vals [n, batch, h, w], as dnnca_tta_mean_of (its refusals included):
 *                          prob_out receives bit for bit that call's mean, spread_out the spread; both required; synchronises
 *   dnnca_get_tta_spread   the valid plane's first `batch` slices to host [batch, H, W]; DNNCA_ESTATE while it is not valid or holds
 *                          fewer slices; waits for the stream */
int dnnca_forward_tta_spread(void* model, const float* x_nhwc, int batch, unsigned views, float* prob_out /* nullable */,
                             float* spread_out /* nullable */);
int dnnca_tta_spread_of(void* model, const float* vals, int batch, int h, int w, unsigned views, int is_logits, float* prob_out,
                        float* spread_out);
int dnnca_get_tta_spread(void* model, int batch, float* out);
/* ---- ensembles (`evaluate --ensemble`, `predict --ensemble`; the reference has none) ---------------------------------------------------
 * The members of an ensemble (cross-validation folds, snapshots of one run) are weight sets of ONE architecture that live on the
 * device inside the one model: no second model, no second stream, one set of activations.
 *   dnnca_model_set_members  n in 0..DNNCA_MAX_MEMBERS; allocates n + 1 slots of num_trainable + num_state floats (the members and
 *                            the spare that keeps the model's own weights during a call) and forgets every member stored before;
 *                            0 frees the slots and the ensemble's planes.  Waits for the stream
 *   dnnca_member_store       member m <- the host vectors params [nT] and state [nS] (the flat vectors of dnnca_get_params /
 *                            dnnca_get_state, what a checkpoint holds); state may be NULL when nS == 0.  Synchronises
 *   dnnca_member_get         reads member m back (either output may be NULL); DNNCA_ESTATE for a slot never stored
 * dnnca_forward_ensemble stages x as dnnca_forward does, saves the model's own (p, state) to the spare slot and then, for every
 * member in ascending order: copies the member's vectors over (p, state) on the model's stream (device to device; nothing is cached
 * from the weights, as dnnca_set_params shows), runs the body of dnnca_forward_tta (with_spread and more than one view: of
 * dnnca_forward_tta_spread) on the staged batch -- views == 1 is the plain forward --, so that the probability buffer and the spread
 * plane hold bit for bit what those calls give with the member's weights loaded, and launches ens_join.  After the last member
 * (p, state) are put back, bit for bit, and
 *     prob    = (sum over the members, ascending, in float32, of mean_m) / n                       (float32 division)
 * and, with_spread, the model's spread plane (valid for `batch`, exactly as after dnnca_forward_tta_spread) holds
 *     total   = sqrt(between^2 + within^2)                  (the law of total variance over the n x V forwards)
 *     between = sqrt(max(0, (sum d^2 - (sum d)^2 / n) / n)),  d = mean_m - mean_0        (exactly 0 for n == 1 and for equal members)
 *     within  = sqrt((sum s_m^2) / n),  s_m the member's spread over its views           (exactly 0 for one view)
 * each within 2^-18 want + 2^-23 of the float64 value `want` of the same float32 inputs.  Every consumer of the probabilities and of
 * the spread plane reads them unchanged.  No atomics: bit-identical from run to run.  The planes of running state are allocated by
 * the first call (a model without members allocates none).  prob_out: NULL, or host [batch, H, W]; synchronises when it is given.
 * DNNCA_EINVAL: what dnnca_forward_tta refuses.  DNNCA_ESTATE, with nothing launched: no members; a member slot that was never
 * stored; the averaged weights exchanged in (dnnca_ema_exchange).
 *   dnnca_get_ensemble_spread  between and within of the last dnnca_forward_ensemble with_spread, host [batch, H, W] each (either
 *                              may be NULL); DNNCA_ESTATE once the spread plane is no longer valid or is not an ensemble's
 *   dnnca_ensemble_of          ens_join alone on host planes means [n, batch, h, w] and withins (same shape, or NULL for zeros),
 *                              1 <= n <= DNNCA_MAX_MEMBERS, any plane size; none of the model's planes is touched.  mean_out is
 *                              required; between_out, within_out and total_out go together (all three, or all NULL for the mean
 *                              alone); synchronises */
#define DNNCA_MAX_MEMBERS 16
int dnnca_model_set_members(void* model, int n);
int dnnca_member_store(void* model, int m, const float* params, int64_t nT, const float* state, int64_t nS);
int dnnca_member_get(void* model, int m, float* params /* nullable */, float* state /* nullable */);
int dnnca_forward_ensemble(void* model, const float* x_nhwc, int batch, unsigned views, int with_spread, float* prob_out /* nullable */);
int dnnca_get_ensemble_spread(void* model, int batch, float* between_out /* nullable */, float* within_out /* nullable */);
int dnnca_ensemble_of(void* model, const float* means, const float* withins /* nullable */, int n, int batch, int h, int w,
                      float* mean_out, float* between_out, float* within_out, float* total_out);
/* keras Model.train_step under engine.py:126-135: forward(training=True) + TFWeightedCrossentropy (losses.py:60-72)
 * + backward + [RCCL all-reduce] + Adam apply with learning rate lr (LearningRateScheduler, engine.py:97-100) */
int dnnca_train_step(void* model, const float* x_nhwc, const float* y_hw, int batch, float lr,
                     const dnnca_loss_cfg* cfg, dnnca_step_out* out);
/* keras Model.test_step under engine.py:198-203: forward(training=False) + loss; optional probabilities */
int dnnca_eval_step(void* model, const float* x_nhwc, const float* y_hw, int batch,
                    const dnnca_loss_cfg* cfg, dnnca_step_out* out, float* prob_out);

/* ---- the hot path, device-resident batches (what bench.py times) ---------------------------------------------- */
int dnnca_dev_alloc(void** dev_ptr, size_t bytes);
int dnnca_dev_free(void* dev_ptr);
int dnnca_memcpy_h2d(void* dev_dst, const void* host_src, size_t bytes);
int dnnca_memcpy_d2h(void* host_dst, const void* dev_src, size_t bytes);
/* ---- train-time augmentation on the device (annotator/data.py:62-111 train_ds): crop + flip + contrast + feature/label split
   of a uint8 batch [batch, hs, ws, cs] resident in HBM (upload it with dnnca_memcpy_h2d as stored in the TFRecords), written as
   x [batch, ho, wo, cs-1] and y [batch, ho, wo] float32.  Per image the host passes its random draws:
     dy, dx    crop jitter added to the centre offsets (data.py:677-689 random_crop: clip(int(N(0, 4)), -6, 6))
     flip      1 = tf.image.random_flip_left_right took the flip branch (data.py:620-625)
     contrast  factor of tf.image.random_contrast, U[0.8, 1.2) (data.py:586-609); applied to the source channels whose bit is
               set in contrast_mask (never to the label channel); 1.0 = identity
   Fails with DNNCA_EINVAL when a crop window leaves the source image (tf.image.crop_to_bounding_box asserts the same).
   Asynchronous on the model's stream: params_host has been copied when the call returns (it may be reused at once); x_dev / y_dev
   are complete for later work on that stream (a train step), a host read needs dnnca_sync first. */
typedef struct { int32_t dy, dx, flip; float contrast; } dnnca_aug_param;
int dnnca_augment_u8(void* model, const void* src_dev, int batch, int hs, int ws, int cs, int label_index, unsigned contrast_mask,
                     const dnnca_aug_param* params_host, int ho, int wo, float* x_dev, float* y_dev);
/* random_warp (annotator/data.py:725-763 -> tfa.image.sparse_image_warp, interpolation order 2, no boundary points): dense part.
   ctrl_host [batch, n_points, 2] = the destination control points (row, column); wv_host [batch, n_points + 3, 2] = the solution
   (w; v) of the polyharmonic-spline system for the control-point flows (dest - source), solved by the caller
   (dnncancerannotator_amd/augment.py solve_warp).  Every output pixel q evaluates flow(q) and samples x [batch, h, w, c] and
   y [batch, h, w] bilinearly at q - flow(q) (tfa dense_image_warp); outputs must not alias the inputs.
   1 <= n_points <= 2046: the n_points * 4 + 6 doubles of one spline live in LDS and must fit the 64 KB a launch gets without
   opting in; more is DNNCA_EINVAL (the message names the limit) and nothing is launched.  The same bound holds for
   dnnca_warp_groups_f32. */
int dnnca_warp_f32(void* model, const float* x_dev, const float* y_dev, int batch, int h, int w, int c, int n_points,
                   const double* ctrl_host, const double* wv_host, float* x_out_dev, float* y_out_dev);
/* random_intrachannelwarp (annotator/data.py:656-715): the channels of a slice, label included, are split into n_groups groups
   and every group is warped by a random_warp of its own (data.py:706), in ONE launch for all groups of all images.
   group_of [c + 1]: the group (0 .. n_groups - 1) of feature channel i; entry c is the label's.  ctrl_host [batch, n_groups,
   n_points, 2] and wv_host [batch, n_groups, n_points + 3, 2] as for dnnca_warp_f32, one spline per image and group.  Arithmetic
   and bilinear clamping are those of dnnca_warp_f32; 1 <= n_groups <= c + 1; outputs must not alias the inputs.
   Asynchronous on the model's stream like dnnca_augment_u8: the host arrays have been copied when the call returns; a host read
   of the outputs needs dnnca_sync first. */
int dnnca_warp_groups_f32(void* model, const float* x_dev, const float* y_dev, int batch, int h, int w, int c, int n_groups,
                          const int* group_of, int n_points, const double* ctrl_host, const double* wv_host, float* x_out_dev,
                          float* y_out_dev);
/* random_affine (this project's own augmentation option; augment.py draw_affine): rotation, zoom, shift and a flip / transpose of
   the plane in one bilinear resampling.  mat_host [batch, 2, 3] double: output pixel q = (row, column) of image b is sampled at
   s_r = mat[b][r][0] * q_row + mat[b][r][1] * q_col + mat[b][r][2], formed in double; the cell is floor(s), the fractions are
   float32, x [batch, h, w, c] and y [batch, h, w] are blended with the same four taps and weights (the label comes out soft).
   Outside the image is zero: a tap outside [0, h-1] x [0, w-1] contributes 0 and is never addressed, however far away s lies.
   h, w, c >= 1.  DNNCA_EINVAL (the message names the function, nothing is launched, the outputs are untouched) for: a null
   pointer; batch (1..65535), h, w or c < 1; an output overlapping an input or the other output; a NaN or infinite matrix entry.
   Asynchronous on the model's stream like dnnca_augment_u8: mat_host has been copied when the call returns; a host read of the
   outputs needs dnnca_sync first. */
int dnnca_affine_f32(void* model, const float* x_dev, const float* y_dev, int batch, int h, int w, int c, const double* mat_host,
                     float* x_out_dev, float* y_out_dev);
/* random_intensity (this project's own augmentation option; augment.py draw_intensity): per image and feature channel a gamma, a
   smooth multiplicative bias field, a separable Gaussian blur and Gaussian or Rician noise, in that order, then a clamp to [0, 1].
   rec_host [batch, c, 32] uint32, one 128-byte record per plane, floats as their float32 bit patterns:
       word 0        flags: bit 0 gamma, bit 1 bias, bit 2 blur, bit 3 noise, bit 4 Rician (with bit 3; Gaussian without it)
       word 1        gamma g                                  v <- v <= 0 ? 0 : powf(v, g)
       words 2..10   bias coefficients a[9]                   v <- v * expf(f),  f = sum a[n] P_i(u) P_j(t) over (i, j) = (1,0) (0,1)
                     (2,0) (1,1) (0,2) (3,0) (2,1) (1,2) (0,3), P Legendre, u = 2 row / (h - 1) - 1, t = 2 col / (w - 1) - 1 (0 where
                     the size is 1)
       word 11       blur radius R (integer, 0..8)
       words 12..20  taps w[0..8], w[0] the centre, 0 beyond R: rows, then columns; a tap outside the image reads the nearest edge
                     pixel (after gamma and bias on that pixel)
       word 21       noise sigma s
       words 22, 23  Philox4x32-10 key; counter (row * w + col, 0, 0, 0); output words r0, r1: u1 = ((r0 >> 9) + 1) * 2^-23,
                     u2 = (r1 >> 8) * 2^-24, rad = sqrtf(-2 logf(u1)), z0 = rad cospif(2 u2), z1 = rad sinpif(2 u2);
                     v <- v + s z0 (Gaussian) or sqrtf((v + s z0)^2 + (s z1)^2) (Rician)
       words 24..31  0
   A plane whose flags are 0 is copied bit for bit (no clamp).  Out of place; h, w, c >= 1 and h * w < 2^32.  DNNCA_EINVAL (the
   message names the function, nothing is launched, the output is untouched) for: a null pointer; batch (1..65535), h, w or c < 1; an
   output overlapping the input; unknown flag bits; a NaN or infinite float word; gamma <= 0 with bit 0; R > 8; a negative tap;
   |w[0] + 2 sum w[k] - 1| > 1e-5 with bit 2; s < 0; a non-zero reserved word.
   Asynchronous on the model's stream like dnnca_augment_u8: rec_host has been copied when the call returns; a host read of the
   output needs dnnca_sync first. */
int dnnca_intensity_f32(void* model, const float* x_dev, int batch, int h, int w, int c, const unsigned* rec_host, float* x_out_dev);
/* same as dnnca_train_step with x/y already in HBM; asynchronous on the model's stream; out may be NULL (no sync) */
int dnnca_train_step_dev(void* model, const float* x_dev, const float* y_dev, int batch, float lr,
                         const dnnca_loss_cfg* cfg, dnnca_step_out* out);
int dnnca_forward_dev(void* model, const float* x_dev, int batch, int training);   /* results stay on the device */
int dnnca_last_step_out(void* model, dnnca_step_out* out);        /* synchronises, then reads the last step's scalars */
int dnnca_sync(void* model);

/* ---- host-side helper of the exam-file reader (dnncancerannotator_amd/tfrecord.py; no device involved) ------------------------
 * CRC-32C (Castagnoli) of `n` bytes: tf.data.TFRecordDataset (annotator/data.py:448-470) checks the masked CRC-32C of every record
 * length and payload; the SSE4.2 crc32 instruction where the host has it */
int dnnca_crc32c(const void* data, size_t n, uint32_t* crc_out);

/* ---- input pipeline: what `ds.prefetch(AUTOTUNE)` (annotator/data.py:110,143) + Keras fit's asynchronous input feeding
 * (engine.py:126-135) do for the reference.  A ring of `slots` (<= 8) staging slots in HBM and a copy stream: the next
 * batch travels host -> HBM while the main stream still works on the previous step, and the step outputs come back through a
 * pinned host ring, so the host never has to wait for the step it has just enqueued.
 *   dnnca_stage_init           once per model; bytes_per_slot 0 = one float batch (x, y) at max_batch
 *   dnnca_stage_upload         copies host_a (and host_b right behind it, 256-byte aligned) into the slot on the copy stream, first
 *                              waiting for the step that consumed the slot's previous content; returns the device addresses.
 *                              May run on other host threads beside the thread that enqueues steps (each on slots of its own).
 *   dnnca_stage_uploaded       blocks the calling host thread until the slot's upload has completed: the host buffers may then be
 *                              reused or freed (hipMemcpyAsync from pageable memory gives no such promise on return)
 *   dnnca_stage_wait           the model's stream waits for the slot's upload (for work other than the step, e.g. dnnca_augment_u8)
 *   dnnca_train_step_staged    = dnnca_stage_wait + dnnca_train_step_dev(x_dev, y_dev) + outputs to the pinned ring; asynchronous
 *   dnnca_staged_out           waits for the step that last ran on the slot and reads its scalars (label / weight assertions of
 *                              utils/losses.py:30,91-92 surface here, i.e. one fetch later than with dnnca_train_step) */
int dnnca_stage_init(void* model, int slots, size_t bytes_per_slot);
int dnnca_stage_upload(void* model, int slot, const void* host_a, size_t bytes_a, const void* host_b, size_t bytes_b,
                       void** a_dev, void** b_dev);
int dnnca_stage_uploaded(void* model, int slot);
int dnnca_stage_wait(void* model, int slot);
int dnnca_train_step_staged(void* model, int slot, const float* x_dev, const float* y_dev, int batch, float lr,
                            const dnnca_loss_cfg* cfg);
int dnnca_staged_out(void* model, int slot, dnnca_step_out* out);
/* keras Model.evaluate (engine.py:198-203) over the staging ring: test steps (forward with training=False + loss) on staged
 * batches; the pixel TP/FP/FN/TN histogram of the n thresholds (all metrics' thresholds at once, any order, n may be 0) stays
 * on the device and keeps adding up over the batches -- exact integer counts, read once by dnnca_eval_end.  Per-batch losses come
 * back through dnnca_staged_out (rank-local, like dnnca_eval_step).  dnnca_pixel_confusion* must not be called in between. */
int dnnca_eval_begin(void* model, const float* thresholds, int n);
int dnnca_eval_step_staged(void* model, int slot, const float* x_dev, const float* y_dev, int batch, const dnnca_loss_cfg* cfg);
int dnnca_eval_end(void* model, dnnca_confusion* out /* n entries, the caller's threshold order */);

/* per-step training metrics (Keras fit updates the compiled metrics on every train step, from that step's training=True forward
 * pass, engine.py:273,286): with n > 0 thresholds (at most 1024, any order) every later train step stores its own
 * sigmoid into the model's probability buffer (the fused head kernels' PROB variants) and counts it against the step's RAW labels
 * (never the label-smoothed copy of the loss) into a histogram of its own: one extra launch, exact integer counts.  n = 0 switches
 * it off.  The call waits for the model's stream.
 *   dnnca_last_step_confusion  TP/FP/FN/TN per threshold (the caller's order) of the last dnnca_train_step / _dev; waits for it
 *   dnnca_staged_confusion     ... of the train step that last ran on the staging slot; waits for it like dnnca_staged_out, so
 *                              reading both adds no second synchronisation.  Call it before the slot takes its next batch.
 * Counts are rank-local (data parallel: the caller sums them).  While the option is on, a train step leaves its probabilities in
 * the buffer that dnnca_pixel_confusion reads; with it off, train steps do not write that buffer (as before). */
int dnnca_train_metrics(void* model, const float* thresholds, int n);
int dnnca_last_step_confusion(void* model, dnnca_confusion* out);
int dnnca_staged_confusion(void* model, int slot, dnnca_confusion* out);
/* the model's probability buffer (the last forward / eval step, or a train step with the training metrics on): the first n_pixels
 * floats [B, H, W] to host; waits for the stream */
int dnnca_get_prob(void* model, float* prob_out, int64_t n_pixels);

/* ---- region (Tversky / Dice) term of the training loss ----------------------------------------------------------------------
 * Per image b, with p = sigmoid(logit), y the step's label (the blurred one under label_smoothing) and sums over that image's
 * H x W pixels only: I = sum p y, P = sum p, Y = sum y,
 *   N = I + smooth,  D = (1 - alpha - beta) I + alpha P + beta Y + smooth,  T = N / D    (alpha = beta = 0.5: soft Dice)
 *   loss = mean_b [ crossentropy_weight * wBCE_b + region_weight * (1 - T_b) ] (+ L2)
 * where wBCE_b is the weighted cross-entropy of dnnca_loss_cfg as without this call.  The configuration is stored in the model and
 * read by every later train / eval step of every entry point (host, _dev, _staged); cfg == NULL switches it off and the steps run
 * the launches they ran before.  With it on, a train step declines the head-in-conv / tail3 fusions (as label_smoothing does) and
 * runs head_region_fwd_<C>, region_loss_finish, head_region_train_<C> (heads of 3, 16, 64 channels) or, from the logits,
 * region_sums, region_loss_finish, region_loss_grad (eval steps, DNNCA generic flag, any other head).  No float atomics: sums, loss
 * and gradients are bit-identical from run to run.  Every statistic is per image: nothing changes under data parallel.
 * DNNCA_EINVAL unless region_weight > 0, crossentropy_weight >= 0, alpha >= 0, beta >= 0, alpha + beta > 0, smooth > 0 (all
 * finite), and for dtype bf16 models.  The call waits for the model's stream. */
typedef struct dnnca_region_loss {
    float region_weight;        /* lambda_r */
    float crossentropy_weight;  /* lambda_ce; 0 skips the cross-entropy arithmetic (label statistics and assertions stay) */
    float alpha;                /* weight of the false positives P - I */
    float beta;                 /* weight of the false negatives Y - I */
    float smooth;               /* s */
} dnnca_region_loss;
int dnnca_model_set_region_loss(void* model, const dnnca_region_loss* cfg);
/* I, P, Y per image of the last train / eval step that ran with the region loss on (out: batch x 3 doubles); waits for the stream */
int dnnca_region_loss_sums(void* model, int batch, double* out);

/* ---- boundary (signed-distance) term of the training loss (Kervadec et al., MIDL 2019) --------------------------------------
 * Per image b, G = { y > 0.5 } of the step's RAW label (under label_smoothing: the label before the blur; the blurred one still
 * feeds the cross-entropy and the region term).  For a pixel q of the H x W plane, d2(q) is the exact squared Euclidean distance
 * to the nearest pixel of G (q outside G) or to the nearest pixel of the plane outside G (q inside), and
 *   phi(q) = float(sqrt((double)d2))        outside G
 *          = 1.0f - float(sqrt((double)d2)) inside G (0 on the inner rim, negative deeper in)
 *          = 0                              on an image where G is empty or the whole plane
 *   S_b = sum_i p_i phi_i (double),  loss += boundary_weight * mean_b S_b / (H W)
 *   dloss/dlogit_i += boundary_weight * phi_i p_i (1 - p_i) / (H W B);  phi is a constant of the step.
 * The term rides the launches of the region loss: a step runs boundary_cols, boundary_rows (the map, rebuilt from the step's labels)
 * in front of them and their phi-reading variants; train and eval steps of every entry point carry it.  No atomics: map, sums,
 * loss and gradients are bit-identical from run to run.  boundary_weight > 0 switches the term on, 0 off (every launch is then the
 * region loss's own).  DNNCA_EINVAL, with nothing changed, for a negative or non-finite value and while no region loss is set;
 * dnnca_model_set_region_loss(model, NULL) clears the term too, setting a region loss again keeps it.  Waits for the stream. */
int dnnca_model_set_boundary_loss(void* model, float boundary_weight);
/* S_b of the last train / eval step that ran with the term (out: batch doubles); DNNCA_ESTATE when there was none; waits */
int dnnca_boundary_loss_sums(void* model, int batch, double* out);
/* phi of the last such step, [batch, H, W] floats to host; DNNCA_ESTATE when there was none; waits */
int dnnca_boundary_distance(void* model, int batch, float* phi_out);
/* The same two kernels on host label planes y_hw [batch, h, w] of any size from 1 x 1 to 16384 pixels a side (batch within the
 * model's): phi_out [batch, h, w] and, d2_out != NULL, the squared distances (0 where the other set is empty).  Touches no tensor
 * of the model and no map of a step. */
int dnnca_signed_distance_of(void* model, const float* y_hw, int batch, int h, int w, float* phi_out, int32_t* d2_out);

/* ---- top-k (hard-pixel) cross-entropy of the training loss (as the TopK-CE of nnU-Net's DC_and_topk_loss) --------------------
 * z the label the loss sees (blurred under label_smoothing), w the step's positive weight, x the logit:
 *   mk_i = 1 + z_i (w - 1),   l_i = mk_i (max(x_i, 0) - x_i z_i + log1p(exp(-|x_i|))) >= 0      (the summand of the weighted BCE)
 * Per image b of H W pixels, k = max(1, ceil(fraction H W)) (in double), tau_b the k-th largest l_i, K_b = { i : l_i >= tau_b },
 * n_b = |K_b| >= k: every tie at the threshold is kept, so the result does not depend on the order of the pixels.
 *   the image's cross-entropy becomes (1 / n_b) sum_{K_b} l_i in the place of (1 / (H W)) sum_i l_i
 *   dloss/dlogit_i = crossentropy_weight [i in K_b] mk_i (sigmoid(x_i) - z_i) / (n_b B);  tau is a constant of the step.
 * Everything else of the loss (crossentropy_weight, the region and boundary terms, label_smoothing, the batch mean) is as it was.
 * l_i is stored once per step as a float32 with a clear sign bit (-0 becomes +0) and compared as an unsigned integer; tau is found
 * exactly by a three-digit radix selection (11 + 10 + 10 bits) with integer histograms.  A step runs topk_pixel_loss,
 * topk_count_mid, topk_count_low, topk_finish once its logits exist and in front of region_loss_finish, and the `tk` variants of
 * the region loss's launches that form the cross-entropy's gradient and sum.  No float atomics: plane, tau, n and the sum are
 * bit-identical from run to run.  fraction in (0, 1] switches the term on, 0 off (every launch is then the region loss's own).
 * DNNCA_EINVAL, with nothing changed: a fraction outside [0, 1] or not finite; no region loss set; a region loss whose
 * crossentropy_weight is 0 (and dnnca_model_set_region_loss refuses such a one while the term is on).
 * dnnca_model_set_region_loss(model, NULL) clears the term too, setting a region loss again keeps it.  Waits for the stream. */
int dnnca_model_set_topk_loss(void* model, double fraction);
/* per image of the last train / eval step that ran with the term: k, n_b, tau_b and sum_{K_b} l_i (batch entries each);
 * DNNCA_ESTATE when there was none; waits */
int dnnca_topk_loss_state(void* model, int batch, int32_t* k_out, int32_t* n_kept_out, float* tau_out, double* sum_out);
/* l of the last such step, [batch, H, W] floats to host; DNNCA_ESTATE when there was none; waits */
int dnnca_topk_pixel_loss(void* model, int batch, float* out);
/* The selection kernels alone (topk_count_high, topk_count_mid, topk_count_low, topk_finish) on host planes v [batch, hw] of
 * non-negative floats (the sign bit of a value is ignored; batch within the model's): tau_out[b] the k-th largest value of plane
 * b, n_kept_out[b] the values >= it.  DNNCA_EINVAL for k outside [1, hw], hw above 2^30 or a null pointer.  Touches no plane and no threshold of
 * a step. */
int dnnca_topk_select_of(void* model, const float* v, int batch, int hw, int k, float* tau_out, int32_t* n_kept_out);

/* pixel TP/FP/FN/TN of the last forward/eval probabilities against y at n thresholds (metrics.yaml:2-23 pixel metrics;
 * utils/metrics.py:37-77 FBetaScore builds on them). y_hw is a host buffer [B,H,W]. */
int dnnca_pixel_confusion(void* model, const float* y_hw, int batch, const float* thresholds, int n, dnnca_confusion* out);
/* the same counts for probabilities the caller supplies: tf.keras.metrics.{Precision,Recall,AUC}.update_state(y_true, y_pred)
 * as utils/metrics.py:53-56 calls it.  Both host buffers hold n_pixels floats (at most max_batch * H * W); any number of
 * thresholds up to 1024 in any order (AUC(num_thresholds=150), metrics.yaml:8-15); counts are exact integers. */
int dnnca_pixel_confusion_of(void* model, const float* prob_hw, const float* y_hw, int64_t n_pixels, const float* thresholds,
                             int n, dnnca_confusion* out);

/* ---- region-based (lesion-level) metrics (utils/metrics.py:80-510; the region entries of configs/additionals/metrics.yaml) ------
 * Per slice: label and probability resized to (int(fp16(H) * fp16(rf)), int(fp16(W) * fp16(rf))) by tf.image.resize bilinear
 * (rf = 1: identity), label' > 0.5, prediction prob' >= thresholds[t] opened by a k x k erosion + dilation (utils/image.py:12-26,
 * out-of-bounds pixels ignored), 4-connected components of both, IoU(L_i, P_j) = float(|L_i n P_j|) / float(|L_i u P_j|) > iou.
 *   tp_label  label components with some IoU > iou_threshold        fn  label components with none
 *   tp_pred   prediction components with some IoU > iou_threshold   fp  prediction components with none
 * Counts are exact integers summed over the slices, one entry per threshold in the caller's order.  Limits: 1..64 thresholds, each
 * >= 0 (metrics.py:96); iou_threshold in [0, 1); resize_factor > 0 with a non-empty result; morph_filter_size 1..15; otherwise
 * DNNCA_EINVAL. */
typedef struct dnnca_region_spec {
    const float* thresholds;     /* host array of n_thresholds */
    int32_t n_thresholds;
    float iou_threshold;         /* IoU_threshold, metrics.py:93 (0.30) */
    float resize_factor;         /* resize_factor (1.0; metrics.yaml: 0.5) */
    int32_t morph_filter_size;   /* morph_filter_size (5) */
} dnnca_region_spec;
typedef struct dnnca_region_counts { int64_t tp_label, fn, tp_pred, fp; } dnnca_region_counts;
/* region counts of caller-supplied slices: prob_hw / y_hw are host buffers [batch, h, w] of any size (the library grows its own
 * device buffers); out has spec->n_thresholds entries */
int dnnca_region_confusion_of(void* model, const float* prob_hw, const float* y_hw, int batch, int h, int w,
                              const dnnca_region_spec* spec, dnnca_region_counts* out);
/* the same on the probabilities of the last forward / eval step (like dnnca_pixel_confusion); y_hw is a host buffer [batch, H, W] */
int dnnca_region_confusion(void* model, const float* y_hw, int batch, const dnnca_region_spec* spec, dnnca_region_counts* out);
/* staged evaluation with region metrics: call dnnca_eval_region_begin after dnnca_eval_begin and before the first
 * dnnca_eval_step_staged; every staged eval step then also adds the region counts of its batch for each of the n specs (on the
 * device, no host round trip); dnnca_eval_region_end, after the last step and before or after dnnca_eval_end, synchronises and
 * writes sum(n_thresholds) entries, spec after spec.  Without dnnca_eval_region_begin a staged evaluation launches nothing of it.
 * dnnca_region_confusion* must not be called in between. */
int dnnca_eval_region_begin(void* model, const dnnca_region_spec* specs, int n);
int dnnca_eval_region_end(void* model, dnnca_region_counts* out);

/* ---- the Visualizer of `annotator evaluate` (utils/callbacks.py:55-446): casewise region counts and composite images ----------
 * dnnca_region_confusion_slices: the region counts of the last forward's probabilities (or of prob_hw, host [batch, H, W], when
 * it is not NULL) against y_hw (host [batch, H, W]), PER SLICE, for n specs (each as above, up to 64 thresholds; specs of one resized size share the label labelling).  out holds
 * batch * sum(n_thresholds) entries: slice after slice, spec after spec within a slice.  The labels stay on the device for
 * dnnca_render_composite.
 * dnnca_render_composite: generate_image + make_summary_constructor + `* 255` cast of the reference for the last forward's
 * input and probabilities: the C feature channels, the label and the probability side by side ([H, W (C + 2)]; overlay: the
 * feature panels grey, the label and probability panels stack([v, f0, f0])), resized by tf.image.resize bilinear (half-pixel
 * centres, float32) to (int(f32(H) * ratio), int(f32(W (C + 2)) * ratio)), then uint8(trunc(v * 255)) (clamped to 0..255).
 * out: host uint8 [batch, oh, ow, overlay ? 3 : 1] of `capacity` bytes; out_hwc receives (oh, ow, channels); out == NULL only
 * queries the size.  y_hw == NULL reuses the labels of the dnnca_region_confusion_slices call just before (same batch): each
 * label crosses the bus once.  The model's output must have the input's size (padding 'same'). */
int dnnca_region_confusion_slices(void* model, const float* prob_hw, const float* y_hw, int batch, const dnnca_region_spec* specs,
                                  int n, dnnca_region_counts* out);
int dnnca_render_composite(void* model, const float* y_hw, int batch, float ratio, int overlay, uint8_t* out, int64_t capacity,
                           int32_t* out_hwc);

/* ---- `annotator predict`: the lesions of slices that have no label (the reference left runs/predict.py empty) -------------------
 * dnnca_lesion_table works on the probabilities of the last forward (prob_hw == NULL; h and w are then 0 or the model's output
 * size) or on prob_hw, host [batch, h, w] of any size.  Per slice: resize by resize_factor as above (1: identity), prob' >=
 * threshold, k x k opening (filter_size 1: none), 4-connected components; a component is KEPT when it has at least min_area
 * pixels.  Kept components are numbered per slice in raster order of their first (smallest-index) pixel; the first max_lesions of
 * a slice give one row each:
 *   slice, row             the slice in the batch, the component's number in the slice
 *   area                   pixels
 *   x0, y0, x1, y1         bounding box, inclusive, in pixels of the analysed (resized) plane
 *   max_prob               the largest prob' of its pixels
 *   sum_x, sum_y           sums of the pixel coordinates (centroid = sum / area)
 *   sum_prob_q24           sum of rint(prob' * 2^24) over its pixels (mean = sum / area / 2^24); prob' is expected in [0, 1]
 * Every field is an integer sum or an extremum: the table is bit-identical from run to run.  rows receives the rows slice after
 * slice (*n_rows of them); rows_capacity must be at least batch * min(max_lesions, (oh * ow + 1) / 2).  totals [batch]: the kept
 * components of each slice, which may exceed max_lesions (the slice's table is then truncated).  mask: NULL, or host uint8
 * [batch, oh, ow] of mask_capacity bytes: 255 on every kept component (truncated or not), 0 elsewhere -- the opened and
 * area-filtered mask.  out_hw receives (oh, ow); rows == NULL only queries it.
 * DNNCA_EINVAL, with nothing launched: batch outside [1, max_batch], filter_size outside 1..15, a threshold that is NaN or negative,
 * a resize factor that is not positive or gives an empty plane, min_area < 0, max_lesions < 1, a buffer that is too small.
 * Variables, state and the probabilities of the last forward are untouched.  Synchronises. */
typedef struct dnnca_lesion_row {
    int32_t slice, row, area, x0, y0, x1, y1;
    float max_prob;
    uint64_t sum_x, sum_y, sum_prob_q24;
} dnnca_lesion_row;                                 /* 56 bytes, no padding */
int dnnca_lesion_table(void* model, const float* prob_hw, int batch, int h, int w, float threshold, float resize_factor,
                       int filter_size, int min_area, int max_lesions, dnnca_lesion_row* rows, int64_t rows_capacity,
                       int64_t* n_rows, int32_t* totals, uint8_t* mask, int64_t mask_capacity, int32_t* out_hw);

/* ---- mask refinement: hysteresis, closing and hole filling (`--refine_hysteresis`, `--refine_closing`, `--refine_fill_holes`) -----
 * Model state, like the region loss: dnnca_lesion_table, _spread, _features, _linked, _matched and dnnca_surface_distances apply it
 * to the PREDICTION plane (the last forward's or prob_hw), on the analysed (resized) plane, in this order:
 *   hysteresis_low   0: off.  Else in (0, 1) and below the call's threshold: M_low = prob' >= hysteresis_low, M_high = prob' >=
 *                    threshold (float32, the same prob'); kept are the 4-connected components of M_low that hold a pixel of M_high
 *   (the opening)    filter_size, as without the refinement
 *   closing_size     0 or 1: off.  Else odd, 3 .. 15: dilation (OR over the in-plane part of [y - c, y + c] x [x - c, x + c],
 *                    c = (closing_size - 1) / 2), then erosion (AND over the in-plane part of the same window).  The closed mask
 *                    contains the opened one; closing twice is closing once
 *   fill_holes       0 or 1.  A 4-connected component of the background with no pixel in the plane's first or last row or column
 *                    becomes foreground (scipy.ndimage.binary_fill_holes's default)
 * then components, area filter, numbering, statistics and mask as before, over all pixels of the refined components.  Nothing
 * crosses from one slice into the next.  The label plane of the matched and surface calls, dnnca_region_confusion* and
 * dnnca_detection_map are not refined.  Off (the default; cfg == NULL or all zero): every launch, plan string and output byte is
 * what it is without these functions, and nothing is allocated.  On: the stage borrows planes of the call's own workspace.
 * dnnca_model_set_lesion_refine: DNNCA_EINVAL, with nothing changed: hysteresis_low NaN, or not 0 and outside (0, 1); closing_size
 * negative, even and above 1, or above 15; fill_holes other than 0 or 1.  The kept predecessor planes of dnnca_lesion_table_linked
 * and dnnca_lesion_table_matched count only under the configuration that made them: after a call that CHANGES it, continues[0] != 0
 * is refused as before the first such call, so no chain mixes masks made under two rules (a caller that switches the refinement
 * off for one kind of call and back on keeps the chain of the other kind).  A table call whose threshold is not above a set hysteresis_low
 * returns DNNCA_EINVAL with nothing launched.  Every mark of the stage is an integer flag: results are bit-identical from run to
 * run.  dnnca_plan_dump_pass lists the stage's launches (region_hyst_seed, region_hyst_keep, region_close, region_complement,
 * region_hole_border, region_hole_fill, and one region_ccl_* set per labelling) while it is on. */
typedef struct dnnca_lesion_refine {
    float hysteresis_low;
    int32_t closing_size;
    int32_t fill_holes;
} dnnca_lesion_refine;
int dnnca_model_set_lesion_refine(void* model, const dnnca_lesion_refine* cfg);
int dnnca_model_get_lesion_refine(void* model, dnnca_lesion_refine* out);

/* ---- the same table plus the spread of the views under it (`annotator predict --tta MODE --uncertainty`) -----------------------------
 * Every argument up to out_hw means what it means for dnnca_lesion_table (the size query with rows == NULL included), and rows,
 * totals, mask and out_hw are bit-identical to that call's.  The spread plane is resized like the probabilities (the same bilinear
 * resize: resize_factor != 1 analyses the same plane); a pixel's spread' enters every sum as rint(max(spread', 0) * 2^24) and every
 * maximum through the float's bits, so all of this is bit-identical from run to run too.
 *   srows[i]     belongs to rows[i]: slice, row, area (the pixels that added to it: rows[i].area), max_spread, sum_spread_q24
 *                (mean = sum / area / 2^24)
 *   stotals[b]   pixels (oh * ow), max_spread and sum_spread_q24 over EVERY pixel of the analysed plane of slice b, lesion or not
 * srows holds rows_capacity records, stotals `batch`.  spread_hw == NULL: the model's own plane, which must be valid
 * (dnnca_forward_tta_spread) for at least `batch` slices -- DNNCA_ESTATE otherwise -- and prob_hw must be NULL as well; otherwise
 * spread_hw is a host plane [batch, h, w] beside prob_hw, which must then be given too.
 * DNNCA_EINVAL, with nothing launched and no output touched: everything dnnca_lesion_table refuses, one of prob_hw / spread_hw given
 * without the other, srows == NULL or stotals == NULL beside rows.  Synchronises. */
typedef struct dnnca_lesion_spread {
    int32_t slice, row, area;
    float max_spread;
    uint64_t sum_spread_q24;
} dnnca_lesion_spread;                              /* 24 bytes, no padding */
typedef struct dnnca_slice_spread {
    int32_t pixels;
    float max_spread;
    uint64_t sum_spread_q24;
} dnnca_slice_spread;                               /* 16 bytes, no padding */
int dnnca_lesion_table_spread(void* model, const float* prob_hw, int batch, int h, int w, float threshold, float resize_factor,
                              int filter_size, int min_area, int max_lesions, dnnca_lesion_row* rows, int64_t rows_capacity,
                              int64_t* n_rows, int32_t* totals, uint8_t* mask, int64_t mask_capacity, int32_t* out_hw,
                              const float* spread_hw, dnnca_lesion_spread* srows, dnnca_slice_spread* stotals);

/* ---- the same table plus what each lesion looks like in the input channels (`annotator predict --lesion_features`) -----------------
 * Every argument up to out_hw means what it means for dnnca_lesion_table (the size query with rows == NULL included), and rows,
 * totals, mask and out_hw are bit-identical to that call's.  Every lesion that has a row gets a shape record, and per channel a
 * body record, a ring record (ring > 0) and a histogram (bins > 0).
 * The value of a pixel in channel c is x', the channel read through the bilinear resize the probabilities went through
 * (resize_factor 1: the pixel itself), as v = min(max(x', 0), 1) with NaN = 0.  It enters every sum as q = rint(v * 2^16) in
 * float32: q16, not the q24 of the probabilities, so that q^2 fits 33 bits and a sum of q^2 over the up to 2^31 pixels of a plane
 * fits one uint64.  Extrema go through the float's bits.  All sums are integers: everything is bit-identical from run to run.
 *   shape[i]        belongs to rows[i]: slice, row, area (rows[i].area); boundary: its pixels with at least one of the four
 *                   neighbours outside the lesion or outside the plane (the BOUNDARY rule of dnnca_surface_distances); edges: the
 *                   (pixel, direction) pairs that face out, i.e. the crack length of its outline, the plane's border included;
 *                   sum_xx, sum_yy, sum_xy: sums of the coordinate products (sum_x, sum_y are in the row)
 *   body[i * channels + c]       slice, row, channel, n (the area), min and max of v, sum_q16 = sum q, sum_sq_q16 = sum q^2
 *   ring_out[i * channels + c]   the same over the lesion's ring.  A background pixel -- one in no kept component: what the opening
 *                   removed and components below min_area are background, kept components beyond max_lesions are not and own no
 *                   ring -- belongs to the ring of the smallest row number among the numbered lesions at (y + dy, x + dx), |dy| <=
 *                   ring, |dx| <= ring, inside the plane; to none if there is none.  n == 0: min = max = 0
 *   hist[(i * channels + c) * bins + k]   the body pixels with min(bins - 1, (int) floor(v * (float) bins)) == k, the product in
 *                   float32 (the bin rule of dnnca_calibration).  The ring has no histogram
 * shape holds rows_capacity records, body and ring_out rows_capacity * channels, hist rows_capacity * channels * bins counts.
 * ring == 0: nothing of the ring launch runs, ring_out is not touched and may be NULL; bins == 0: the same for hist.
 * x_hwc == NULL: the staged batch of the last forward (under dnnca_forward_tta* the untransformed batch) with the model's input
 * channels (`channels` is then 0 or that number); prob_hw must be NULL too; DNNCA_ESTATE when the last forward staged fewer than
 * `batch` slices or the model's output size is not its input size.  Otherwise x_hwc is a host plane [batch, h, w, channels],
 * channels in 1..16, beside a host prob_hw.
 * DNNCA_EINVAL, with nothing launched and no output touched: everything dnnca_lesion_table refuses, one of prob_hw / x_hwc given
 * without the other, channels outside 1..16, bins outside 0..256, ring outside 0..8, shape or body NULL beside rows, ring_out NULL
 * with ring > 0, hist NULL with bins > 0, an analysed plane with a side above 65535 (the moment sums must fit 64 bits), records of
 * one slice (min(max_lesions, (oh * ow + 1) / 2) rows) above 2^30 bytes.  Variables, state, the probabilities of the last forward
 * and the carry planes of the linked and matched calls are untouched.  Synchronises. */
typedef struct dnnca_lesion_shape {
    int32_t slice, row, area, boundary, edges, reserved;
    uint64_t sum_xx, sum_yy, sum_xy;
} dnnca_lesion_shape;                               /* 48 bytes, no padding */
typedef struct dnnca_lesion_intensity {
    int32_t slice, row, channel, n;
    float min, max;
    uint64_t sum_q16, sum_sq_q16;
} dnnca_lesion_intensity;                           /* 40 bytes, no padding */
int dnnca_lesion_table_features(void* model, const float* prob_hw, int batch, int h, int w, float threshold, float resize_factor,
                                int filter_size, int min_area, int max_lesions, dnnca_lesion_row* rows, int64_t rows_capacity,
                                int64_t* n_rows, int32_t* totals, uint8_t* mask, int64_t mask_capacity, int32_t* out_hw,
                                const float* x_hwc, int channels, int bins, int ring, dnnca_lesion_shape* shape,
                                dnnca_lesion_intensity* body, dnnca_lesion_intensity* ring_out, uint32_t* hist);

/* ---- is the spread larger where the model is wrong? (`annotator evaluate --tta MODE --uncertainty`) ---------------------------------
 * Per threshold t and slice b every pixel falls into the class 2 (y > 0.5) + (prob >= thresholds[t]): TN 0, FP 1, FN 2, TP 3 (the
 * label rule of dnnca_lesion_table_matched); out[t * batch + b] receives the pixels n[c] and the sums sum_q24[c] of
 * rint(max(spread, 0) * 2^24) of every class.  Raw planes: no resize, no opening.  prob_hw and spread_hw: both NULL -- the model's
 * probabilities and its spread plane, which must be valid for at least `batch` slices (DNNCA_ESTATE otherwise); h and w are then 0
 * or the model's output size -- or both host planes [batch, h, w] of any size.  y_hw: host [batch, h, w], required.
 * DNNCA_EINVAL, with nothing launched and no output touched: batch outside [1, max_batch], n_thresholds outside 1..64, a NaN
 * threshold, a NULL thresholds / y_hw / out, one of prob_hw / spread_hw given without the other, a plane that is empty or has 2^31
 * pixels or more, more than 65535 slices.  Exact integers: bit-identical from run to run.  Synchronises. */
typedef struct dnnca_spread_outcome {
    uint64_t n[4], sum_q24[4];
} dnnca_spread_outcome;                             /* 64 bytes, no padding */
int dnnca_spread_by_outcome(void* model, const float* prob_hw, const float* spread_hw, const float* y_hw, int batch, int h, int w,
                            const float* thresholds, int n_thresholds, dnnca_spread_outcome* out /* [n_thresholds][batch] */);

/* ---- can the probability be believed? (`annotator evaluate --calibration`, `--temperature`) ---------------------------------------
 * dnnca_calibration: the reliability table of a probability plane against its labels and its negative log-likelihood at a set of
 * temperatures.  A pixel is of class 1 when y > 0.5, else 0 (the rule above); its probability is clamped, p' = min(max(p, 0), 1) (a NaN
 * counts as 0), enters every sum as q = rint(p' * 2^24) (float32 product) and falls into bin k = min(n_bins - 1, (int) floor(p' *
 * (float) n_bins)) (float32 product).  bins[b * n_bins + k]: the pixels n[c] and the sums sum_q24[c] of q of slice b, bin k and class
 * c.  totals[b]: the same over all bins, and the sum of q^2 per class as two exact words, sq_lo = sum (q^2 & 0xffffffff) and sq_hi =
 * sum (q^2 >> 32): sum q^2 = sq_hi * 2^32 + sq_lo (the Brier score).  Integers: bit-identical from run to run.
 * nll[b * n_temperatures + t]: the sum over the pixels of slice b of softplus(-a) (class 1) or softplus(a) (class 0) in double, with
 * a = z * (1 / (double) temperatures[t]), z = log(pc) - log1p(-pc), pc = p' clamped to [2^-24, 1 - 2^-24] (an exact 0 or 1 counts as
 * z = -+16.64) and softplus(a) = max(a, 0) + log1p(exp(-|a|)).  Block partials summed in a fixed order: bit-identical from run to
 * run.  With n_temperatures == 0 nothing of it runs and nll is not touched.
 * prob_hw == NULL: the model's own probabilities (the last forward's, or the mean dnnca_forward_tta left); h and w are then 0 or the
 * output size, and DNNCA_ESTATE is returned when the last forward had fewer than `batch` slices.  Otherwise prob_hw is a host plane
 * [batch, h, w] of any size.  y_hw: host [batch, h, w], required.
 * DNNCA_EINVAL, with nothing launched and no output touched: batch outside [1, max_batch], n_bins outside 1..256, n_temperatures
 * outside 0..64, n_temperatures > 0 with a NULL temperatures or nll, a temperature that is NaN or outside [0.05, 20], a NULL y_hw /
 * bins / totals, a plane that is empty or has 2^31 pixels or more, more than 65535 slices.  Variables and state stay untouched.
 * Synchronises. */
typedef struct dnnca_calib_bin { uint64_t n[2], sum_q24[2]; } dnnca_calib_bin;                          /* 32 bytes */
typedef struct dnnca_calib_total { uint64_t n[2], sum_q24[2], sq_lo[2], sq_hi[2]; } dnnca_calib_total;  /* 64 bytes */
int dnnca_calibration(void* model, const float* prob_hw, const float* y_hw, int batch, int h, int w, int n_bins,
                      const float* temperatures, int n_temperatures, dnnca_calib_bin* bins /* [batch][n_bins] */,
                      dnnca_calib_total* totals /* [batch] */, double* nll /* [batch][n_temperatures] */);
/* dnnca_prob_temperature: p -> (float) (1 / (1 + exp(-z / T))) with z as above, in double, rounded once to float32.  0.5 stays 0.5
 * and the rounded map is non-decreasing: a mask at threshold 0.5 changes at most where a probability lay within a rounding of 0.5.  prob_hw == NULL: the model's probability buffer is scaled IN
 * PLACE for `batch` slices (DNNCA_ESTATE when the last forward had fewer) -- every later consumer of it reads the scaled values, the
 * spread plane of dnnca_forward_tta_spread stays what it is and stays valid, and a second call scales the scaled values again: call
 * it once per forward; out_hw may be NULL, or receives a copy.  With a host plane prob_hw [batch, h, w] out_hw is required and the
 * model's buffer stays untouched.  DNNCA_EINVAL, with nothing launched and nothing touched: batch outside [1, max_batch], a
 * temperature that is NaN or outside [0.05, 20], a host plane without out_hw, a plane that is empty or has 2^31 pixels or more.
 * Variables and state stay untouched.  Synchronises. */
int dnnca_prob_temperature(void* model, const float* prob_hw, int batch, int h, int w, float temperature, float* out_hw);

/* ---- the detection map: ranked lesion candidates without a fixed threshold (`evaluate --detection`, `predict --detection_map`) ---
 * The dynamic candidate extraction of PI-CAI's extract_lesion_candidates, per slice of h x w float32 values p:
 *     w = min(max(p, 0), 1), a NaN counts as 0;  D = 0;  n = 0
 *     for round = 1 .. rounds:
 *         m = max(w);  s = the smallest pixel index with w == m;  if m < min_confidence: stop
 *         t = (float32) m * (float32) factor                       (one float32 product)
 *         C = the 4-connected component of { w >= t } that contains s
 *         if |C| >= min_area: D[C] = m, candidate n = (seed s, area |C|, confidence m), n += 1;  else dropped += 1
 *         w[C] = 0;  if n == max_candidates: stop
 * Candidates never overlap and nothing depends on a thread order: map, rows and slice records are bit-identical from run to run.
 * slices[b] = (candidates, rounds spent, regions dropped below min_area, exhausted); exhausted = 1 says that all `rounds` rounds
 * are spent, fewer than max_candidates were found and a value >= min_confidence is still left.  rows receives *n_rows records
 * sorted by (slice, number); a slice's numbers run from 0 in the order of the rounds, i.e. in descending confidence.
 * prob_hw == NULL: the model's probability buffer (the last forward's, the mean of dnnca_forward_tta, scaled by
 * dnnca_prob_temperature) is replaced IN PLACE by D for `batch` slices (DNNCA_ESTATE when the last forward had fewer) -- every
 * later consumer of "the last forward" reads the detection map; out_hw may be NULL, or receives a copy.  With a host plane prob_hw
 * [batch, h, w] of any size out_hw is required and the model's buffer stays untouched.
 * DNNCA_EINVAL, with nothing launched and nothing touched: batch outside [1, max_batch], min_confidence outside [0.001, 1], factor
 * outside [0.01, 1], max_candidates outside 1..64, min_area outside 1..2^30, rounds outside max_candidates..256, a NaN, a NULL cfg /
 * rows / slices / n_rows, a host plane without out_hw, a plane that is empty or has 2^31 pixels or more.  Variables, state and the
 * carried rows of dnnca_lesion_table_linked / _matched stay untouched.  Synchronises. */
typedef struct dnnca_detection_cfg { float min_confidence, factor; int32_t max_candidates, min_area, rounds; } dnnca_detection_cfg;
typedef struct dnnca_detection_row { int32_t slice, number, seed, area; float confidence; } dnnca_detection_row;   /* 20 bytes */
typedef struct dnnca_detection_slice { int32_t candidates, rounds, dropped, exhausted; } dnnca_detection_slice;  /* 16 bytes */
int dnnca_detection_map(void* model, const float* prob_hw, int batch, int h, int w, const dnnca_detection_cfg* cfg,
                        float* out_hw, dnnca_detection_row* rows /* [batch * max_candidates] */, int64_t* n_rows,
                        dnnca_detection_slice* slices /* [batch] */);

/* ---- bootstrap over exams: confidence intervals of the detection and exam-lesion figures (`evaluate --bootstrap`) ------------------
 * The resampling, the same for both calls: the exams of a pass are numbered 0 .. E-1; pool [E] is a permutation of them ordered by
 * stratum, strata [S] (1 <= S <= 8) the positive sizes n_s of the strata, summing to E, o_s their offsets into pool.  Replicate r in
 * [0, R) makes E draws; draw j lies in the stratum s with o_s <= j < o_s + n_s and picks pool[o_s + ((uint64) x * n_s >> 32)], x
 * being word j & 3 of Philox4x32-10 on the counter (j >> 2, r, 0, 0) under the key (seed & 0xffffffff, seed >> 32).  The
 * multiply-shift maps the 2^32 values of x onto n_s exams with a bias below n_s / 2^32 (under 2^-18 at the largest E).  m_r[e] is the
 * number of draws that picked exam e: it sums to E, and to n_s within stratum s.  The draws depend on (seed, E, strata) alone, not on
 * what is resampled: two calls with the same three resample identically and can be differenced replicate by replicate.
 * mult_out (NULL, or [R, E]) receives m_r.  One workgroup per replicate builds m_r in LDS; everything is integers but ap, whose terms
 * are added in an order fixed by (N, the block size): both calls are bit-identical from run to run.
 *
 * dnnca_bootstrap_sums: out[r][k] = sum_e m_r[e] * cols[e][k], exact, for 1 <= K <= 64 columns of int32.
 *
 * dnnca_bootstrap_detection: exams[e] = (tumours >= 0, score_rank >= 0: the dense rank of the exam's score among all exams, 0 the
 * lowest, equal scores equal ranks); cands [N] sorted by descending confidence, each (exam, hit 0 / 1, level: the index of its
 * distinct confidence, 0 the highest, non-decreasing without gaps).  The device never sees a float.  With w_c = m_r[exam_c] and
 * cumulative weighted counts TP_k, FP_k at the end of level k, out[r] holds
 *     positive_exams = sum m [tumours > 0],  tumours T = sum m tumours,  candidates = sum w,  tp = sum w hit,  fp = sum w (1 - hit)
 *     auroc_pairs = positive_exams * (E - positive_exams)
 *     auroc_twice = sum over positive p, negative n of m_p m_n (2 [rank_p > rank_n] + [rank_p == rank_n])
 *     tp_at[i]    = TP_k of the last level with FP_k * 8 <= (1 << i) * E   (false positives per exam 1/8 .. 8), 0 when none
 *     ap          = sum_k (TP_k - TP_{k-1}) * TP_k / (T * (TP_k + FP_k)) in double; a level with TP_k + FP_k == 0 adds 0; 0.0 when
 *                   T == 0 (told by tumours == 0) or nothing is drawn
 * DNNCA_EINVAL, with nothing launched and the outputs untouched: E outside 1..16384, N outside 0..2^22, R outside 1..2^20, K outside
 * 1..64, S outside 1..8, a size that is not positive or sizes that do not sum to E, a pool that is no permutation of 0..E-1, an exam
 * index out of range, a hit that is not 0 / 1, a level that decreases or skips (the first is 0), negative tumours or rank, a NULL
 * cols / exams / cands (with N > 0) / pool / strata / out.  The model gives its stream and a scratch of the calls' own: no variable,
 * state, probability buffer or carried lesion rows are touched.  Synchronises. */
#define DNNCA_BOOTSTRAP_TILE 1024                    /* candidates a workgroup of dnnca_bootstrap_detection takes per step */
typedef struct dnnca_bootstrap_exam { int32_t tumours, score_rank; } dnnca_bootstrap_exam;                      /* 8 bytes */
typedef struct dnnca_bootstrap_candidate { int32_t exam, hit, level; } dnnca_bootstrap_candidate;               /* 12 bytes */
typedef struct dnnca_bootstrap_detection_row {                                                                    /* 120 bytes */
    int64_t positive_exams, tumours, candidates, tp, fp, auroc_pairs, auroc_twice, tp_at[7];
    double ap;
} dnnca_bootstrap_detection_row;
int dnnca_bootstrap_sums(void* model, const int32_t* cols /* [E, K] */, int E, int K, const int32_t* pool, const int32_t* strata,
                         int S, int R, uint64_t seed, int64_t* out /* [R, K] */, uint16_t* mult_out /* [R, E] or NULL */);
int dnnca_bootstrap_detection(void* model, const dnnca_bootstrap_exam* exams /* [E] */, int E,
                              const dnnca_bootstrap_candidate* cands /* [N] */, int N, const int32_t* pool, const int32_t* strata,
                              int S, int R, uint64_t seed, dnnca_bootstrap_detection_row* out /* [R] */, uint16_t* mult_out);

/* ---- the same table plus the links between neighbouring slices of an exam (`annotator predict --link_slices`) ------------------
 * Every argument up to out_hw means what it means for dnnca_lesion_table (the size query with rows == NULL included), and rows,
 * totals and mask are bit-identical to that call's.  continues [batch]: continues[b] != 0 says that slice b is the next slice of
 * the exam of slice b - 1; for b == 0 the predecessor is the last slice of the previous successful dnnca_lesion_table_linked call
 * on this model (its row numbers are kept on the device, whatever else the model was used for in between).  For every such slice
 * and every pair of a lesion of the predecessor (row_prev: its number there) and a lesion of slice `slice` (row) that share
 * pixels, links receives one entry with the number of common pixels; lesions beyond max_lesions or below min_area link to nothing.
 * *n_links entries, sorted by (slice, row_prev, row); links_capacity must be at least batch * min(cap * cap, (oh * ow + 1) / 2)
 * with cap = min(max_lesions, (oh * ow + 1) / 2).
 * DNNCA_EINVAL, with nothing launched and the kept predecessor untouched: everything dnnca_lesion_table refuses, continues ==
 * NULL, a links buffer that is too small, continues[0] set while no linked call has succeeded on this model or the last one
 * analysed planes of another oh x ow.  Synchronises. */
typedef struct dnnca_lesion_link { int32_t slice, row_prev, row, overlap; } dnnca_lesion_link;   /* 16 bytes */
int dnnca_lesion_table_linked(void* model, const float* prob_hw, int batch, int h, int w, float threshold, float resize_factor,
                              int filter_size, int min_area, int max_lesions, dnnca_lesion_row* rows, int64_t rows_capacity,
                              int64_t* n_rows, int32_t* totals, uint8_t* mask, int64_t mask_capacity, int32_t* out_hw,
                              const uint8_t* continues, dnnca_lesion_link* links, int64_t links_capacity, int64_t* n_links);

/* ---- both planes at once: predicted and labelled lesions and their common pixels (`annotator evaluate --exam_lesions`) ----------
 * prob_hw (NULL: the last forward's probabilities) and every argument from batch to continues mean what they mean for
 * dnnca_lesion_table_linked; `pred` (rows, totals, links), `mask` and out_hw receive bit for bit what that call writes.
 * y_hw: the labels, host [batch, h, w], required.  The label plane is resized by the same resize_factor; foreground is
 * y' > 0.5 (utils/metrics.py:125), there is no opening and no area filter; its 4-connected components are numbered in the same
 * way under the same max_lesions.  `truth` receives their rows (the sums and the maximum taken on y'), totals and the links
 * between neighbouring slices under the same continues flags -- what dnnca_lesion_table_linked gives for y_hw with threshold
 * nextafterf(0.5, 1), filter_size 1 and min_area 0.
 * pairs: for every slice, whatever its flag, and every pair of a labelled lesion (row_true) and a predicted lesion (row) of that
 * slice that share pixels, one entry with the number of common pixels, sorted by (slice, row_true, row); lesions beyond
 * max_lesions or below min_area pair with nothing.
 * A plane group carries the caller's buffers and their capacities in, and the counts out: rows_capacity at least batch * cap,
 * links_capacity and pairs->capacity at least batch * min(cap * cap, (oh * ow + 1) / 2), cap = min(max_lesions, (oh * ow + 1) / 2).
 * pred == NULL or pred->rows == NULL only queries out_hw.
 * continues[0] refers to the last slice of the previous successful dnnca_lesion_table_matched call on this model: the call keeps
 * the row numbers of both planes of its last slice on the device.  It neither reads nor writes what dnnca_lesion_table_linked
 * keeps, and that call neither reads nor writes this.
 * DNNCA_EINVAL, with nothing launched and both kept planes untouched: everything dnnca_lesion_table_linked refuses, y_hw ==
 * NULL, truth == NULL or pairs == NULL or one of their buffers NULL, one of the three new capacities too small, continues[0] set
 * while no matched call has succeeded on this model or the last one analysed planes of another oh x ow.
 * Variables, state and the probabilities of the last forward are untouched.  Every output is an integer or an extremum:
 * bit-identical from run to run.  Synchronises. */
typedef struct dnnca_lesion_pair { int32_t slice, row_true, row, overlap; } dnnca_lesion_pair;   /* 16 bytes */
typedef struct dnnca_lesion_plane_out {
    dnnca_lesion_row* rows;      /* in: host buffer of rows_capacity records */
    int64_t rows_capacity;
    int64_t n_rows;              /* out */
    int32_t* totals;             /* in: host [batch] */
    dnnca_lesion_link* links;    /* in: host buffer of links_capacity records */
    int64_t links_capacity;
    int64_t n_links;             /* out */
} dnnca_lesion_plane_out;
typedef struct dnnca_lesion_pairs_out {
    dnnca_lesion_pair* pairs;    /* in: host buffer of `capacity` records */
    int64_t capacity;
    int64_t n_pairs;             /* out */
} dnnca_lesion_pairs_out;
int dnnca_lesion_table_matched(void* model, const float* prob_hw, const float* y_hw, int batch, int h, int w, float threshold,
                               float resize_factor, int filter_size, int min_area, int max_lesions, const uint8_t* continues,
                               dnnca_lesion_plane_out* pred, uint8_t* mask, int64_t mask_capacity, dnnca_lesion_plane_out* truth,
                               dnnca_lesion_pairs_out* pairs, int32_t* out_hw);

/* ---- how far the predicted outline lies from the labelled one (`annotator evaluate --surface_distances`) -------------------------
 * Two masks per slice, on the analysed (resized) plane of oh x ow pixels.  Side 0 is the prediction mask: bit for bit the `mask`
 * that dnnca_lesion_table writes for the same prob_hw (NULL: the last forward's probabilities), threshold, resize_factor,
 * filter_size and min_area -- every kept component, whatever max_lesions would be.  Side 1 is the label foreground of
 * dnnca_lesion_table_matched: y_hw (host [batch, h, w], required) resized by the same factor, y' > 0.5, no opening, no area filter.
 * A BOUNDARY pixel of a mask is a foreground pixel with at least one of its four neighbours in the background or outside the plane.
 * For a boundary pixel a of side s, d2 is the smallest (ax - bx)^2 + (ay - by)^2 over the boundary pixels b of the OTHER side: an
 * exact integer, boundary to boundary (a pixel deep inside the other mask is not at distance 0).
 *   counts [batch][5]      area_pred, area_true, common (pixels in both masks), edge_pred, edge_true (boundary pixels); always exact
 *   samples                one entry (slice, side, pixel = y * ow + x, d2) per boundary pixel of either side, sorted by (slice,
 *                          side, pixel), *n_samples of them.  A slice gives samples only when edge_pred > 0, edge_true > 0 and both
 *                          are at most max_samples; otherwise it gives none, for neither side (never a subset).  capacity must be at
 *                          least batch * 2 * min(max_samples, oh * ow)
 *   edges                  NULL, or host uint8 [batch, oh, ow] of edges_capacity bytes: bit 0 on the prediction's boundary pixels,
 *                          bit 1 on the label's, truncated or not
 * out_hw receives (oh, ow); counts == NULL only queries it.  Everything is an integer: bit-identical from run to run.
 * DNNCA_EINVAL, with nothing launched: everything dnnca_lesion_table refuses, y_hw == NULL, max_samples < 1, samples == NULL or
 * n_samples == NULL, a buffer that is too small, an analysed plane of more than 16384 pixels a side (d2 would leave int32).
 * Variables, state and the probabilities of the last forward are untouched; so is what dnnca_lesion_table_linked and
 * dnnca_lesion_table_matched keep of their last slice: a chain of either continues as if this call had not happened.
 * Synchronises. */
typedef struct dnnca_surface_sample { int32_t slice, side, pixel, d2; } dnnca_surface_sample;   /* 16 bytes */
int dnnca_surface_distances(void* model, const float* prob_hw, const float* y_hw, int batch, int h, int w, float threshold,
                            float resize_factor, int filter_size, int min_area, int max_samples, int32_t* counts /* [batch][5] */,
                            dnnca_surface_sample* samples, int64_t capacity, int64_t* n_samples, uint8_t* edges,
                            int64_t edges_capacity, int32_t* out_hw);

/* ---- channel sensitivity of `annotator evaluate --visualize_sensitivity` (utils/callbacks.py:290-313) ---------------------------
 * With the model in inference mode (BatchNorm on its moving statistics, sigmoid output):
 *     sums[b * in_channels + c] = sum over H, W of | d (sum of all probabilities of slice b) / d x[b, h, w, c] |
 * The caller normalises a slice's row by its sum (an all-zero row gives the reference's 0 / 0 = NaN).  x_nhwc: host [batch, H, W,
 * in_channels], or NULL for the batch the last dnnca_forward of the same size left on the device.  One inference forward that keeps
 * every tensor plus the data gradients alone: no weight gradient, no optimizer step; variables, optimizer slots, BatchNorm state,
 * the iteration count and the probabilities / logits of the last forward are untouched (the gradient vector and the tensors'
 * gradient views are scratch, as between any two train steps).  The sums are float64 and bit-identical from run to run.
 * dtype f32 models only: a DNNCA_BF16 model returns DNNCA_EINVAL; so do a batch outside [1, max_batch] and sums == NULL.
 * Synchronises. */
int dnnca_input_sensitivity(void* model, const float* x_nhwc, int batch, double* sums /* [batch * in_channels] */);

/* ---- integrated-gradients attribution of `annotator evaluate --visualize_attribution` (Sundararajan et al. 2017) ------------------
 * The plain gradient of dnnca_input_sensitivity vanishes where the sigmoid saturates; this pass integrates it along the straight
 * path from a baseline image to the slice.  With the model in inference mode and F_b(x) = sum over H, W of sigmoid(logits_b(x)):
 *     baseline  x0[b, :, :, c] is a constant plane: 0 (baseline = 0, black) or the mean of x[b, :, :, c] (baseline = 1), the mean
 *               formed on the device in double in a fixed order and rounded once to float32
 *     path      x(alpha) = x0 + alpha (x - x0), alpha_k = (k + 0.5) / steps for k = 0 .. steps - 1 (midpoint rule), steps in 1..256
 *     attr[b, h, w, c] = (x - x0)[b, h, w, c] * (1 / steps) * sum over k of (d F_b / d x)(x(alpha_k))[b, h, w, c]
 *     signed_sums[b * C + c] = sum over H, W of attr;  abs_sums[b * C + c] = sum over H, W of |attr|
 *     endpoints[2 b] = F_b(x), endpoints[2 b + 1] = F_b(x0), from two more forwards
 * The attributions of a slice sum to F_b(x) - F_b(x0) up to the error of the quadrature (completeness): the caller forms the gap
 * sum over c of signed_sums[b, c] - (endpoints[2 b] - endpoints[2 b + 1]).  map: NULL, or host [batch, H, W, C] for attr itself.
 * x_nhwc as in dnnca_input_sensitivity (NULL: the slices the last forward left staged; DNNCA_ESTATE when `batch` is not that
 * forward's).  Cost: steps + 2 inference forwards and `steps` data-gradient backward passes.  Untouched: variables, BatchNorm state,
 * optimizer slots, the staged slices and the last forward's logits and probabilities (scratch: the gradient views and four buffers
 * of the pass's own, allocated for max_batch by the first call).  All sums are float64; sums and map are bit-identical from run
 * to run (no atomics: every element has one writer, every sum a fixed order).  dtype f32 U-Net / mulmo models only: a DNNCA_BF16 or
 * MultiResUnet model returns DNNCA_EINVAL; so do a batch outside [1, max_batch], steps outside [1, 256], a baseline other than 0 / 1
 * and a NULL signed_sums, abs_sums or endpoints.  Synchronises. */
int dnnca_integrated_gradients(void* model, const float* x_nhwc /* NULL: the slices the last forward left */, int batch,
                               int steps, int baseline /* 0 black, 1 slice mean */,
                               double* signed_sums /* [B,C] */, double* abs_sums /* [B,C] */, double* endpoints /* [B,2] */,
                               float* map /* [B,H,W,C] or NULL */);

/* ---- data parallel: tf.distribute.MirroredStrategy (engine.py:260-263) re-done as one process per GPU + RCCL ---- */
int dnnca_comm_unique_id(void* id_out /* DNNCA_UNIQUE_ID_BYTES */);
int dnnca_comm_init(void* model, int rank, int world, const void* unique_id, size_t id_len);   /* world == 1: no-op */
int dnnca_comm_world(void* model, int* rank, int* world);
/* gradient all-reduce calls the last train step issued: 1, or several when a gradient vector above 1 MB was sent in buckets
 * (reverse layer order, second stream) while the backward pass was still running -- bit-identical to the single call */
int dnnca_comm_collectives(void* model, int* count);
/* floats the last of those calls covered: dnnca_num_trainable + 1 (gradients and the loss slot) for the single call, 1 for a
 * micro-step of gradient accumulation that ends in no update, the last bucket's length for a bucketed step; 0 before any */
int dnnca_comm_collective_floats(void* model, int64_t* count);
/* weights, BN statistics and Adam slots of `root` on every rank; with a weight average (on every rank or on none) it and its count too */
int dnnca_comm_broadcast_weights(void* model, int root);
int dnnca_comm_average_state(void* model);          /* BN moving statistics: mean over ranks before a checkpoint */
/* small host-side reductions (validation loss sums, metric counts: MirroredStrategy's metric aggregation); doubles, any length */
int dnnca_comm_allreduce_host(void* model, double* values, int64_t n, int op /* 0 sum, 1 max */);

/* ---- measurement: HIP events on the model's stream ------------------------------------------------------------- */
int dnnca_timer_start(void* model);
int dnnca_timer_stop(void* model, float* elapsed_ms);  /* synchronises */
/* per-kernel accounting: when enabled every launch is bracketed by HIP events on the model's stream */
int dnnca_profile_enable(void* model, int mode /* 0 off, 1 all kernels, 2 only the kernel named by dnnca_profile_focus */);
int dnnca_profile_focus(void* model, const char* kernel_name);
/* mode 2 only: bracket the focus kernel in one train step out of `period` (>= 1), so that the brackets of a timed region cost
   next to nothing; every bracketed launch is a full HIP-event measurement on the launch stream */
int dnnca_profile_sample(void* model, int period);
int dnnca_profile_reset(void* model);
int dnnca_profile_count(void* model, int* count);
int dnnca_profile_get(void* model, int index, char* name, size_t name_cap, int64_t* launches, double* total_ms,
                      double* algorithmic_bytes, double* flops);   /* bytes/flops are per launch (mean) */
/* the launch schedule of one train step: name + algorithmic bytes/flops per launch (for DESIGN.md and bench.py) */
int dnnca_plan_dump(void* model, char* buf, size_t cap);
/* the same for one pass at one batch size in [1, max_batch]: the train step (dnnca_plan_dump is this at max_batch), an evaluation
   step (dnnca_eval_step / dnnca_eval_step_staged: inference forward + loss), or a prediction (dnnca_forward with training = 0:
   inference forward + sigmoid), or dnnca_input_sensitivity, or dnnca_lesion_table on the last forward's probabilities with the
   resize factor, filter size and mask choice of the last dnnca_lesion_table / dnnca_lesion_table_linked call (before any: 1.0, 5,
   with mask), or dnnca_lesion_table_linked with the same three values, or dnnca_lesion_table_matched with the three values of the
   last dnnca_lesion_table_matched call (before any: the same defaults), or dnnca_surface_distances with the resize factor and
   filter size of the last dnnca_surface_distances call (before any: 1.0, 5), or dnnca_integrated_gradients with the steps and
   baseline of the last dnnca_integrated_gradients call (before any: 32, black) and the map requested, or
   dnnca_lesion_table_features on the staged batch with the resize factor, filter size, mask choice, bins and ring of the last
   dnnca_lesion_table_features call (before any: 1.0, 5, with mask, 32, 3), or dnnca_detection_map in place with the parameters
   of the last dnnca_detection_map call (before any: 0.1, 0.4, 5, 10, 16).  A dry run: nothing is launched and the model is left
   as it was. */
enum { DNNCA_PLAN_TRAIN = 0, DNNCA_PLAN_EVAL = 1, DNNCA_PLAN_FORWARD = 2, DNNCA_PLAN_SENSITIVITY = 3, DNNCA_PLAN_LESION = 4,
       DNNCA_PLAN_LESION_LINKED = 5, DNNCA_PLAN_LESION_MATCHED = 6, DNNCA_PLAN_SURFACE = 7, DNNCA_PLAN_ATTRIBUTION = 8,
       DNNCA_PLAN_LESION_FEATURES = 9, DNNCA_PLAN_DETECTION = 10 };
int dnnca_plan_dump_pass(void* model, int pass, int batch, char* buf, size_t cap);
/* the small-channel launchers' size predicate (a host function, no model needed): 1 when one image of H x W pixels with C float
   channels stays below 2^31 bytes, so that the kernels can address it with a 32-bit byte offset through one buffer descriptor;
   0 otherwise (such a conv declines to the per-layer or generic path) */
int dnnca_store_image_fits(long long H, long long W, long long C);

#ifdef __cplusplus
}
#endif
#endif /* DNNCA_H */
