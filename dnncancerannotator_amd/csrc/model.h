// model.h -- the layer plan of one annotator model and its device state.
#pragma once
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "kernels.h"                     // DNNCA_CONF_MAX_THR

typedef struct ncclComm* ncclComm_t;

namespace dnnca {

struct OptChunk;    // optim.h

struct T {          // a tensor = data view + gradient view of identical geometry
    View d, g;
};

inline T tslice(const T& t, int c0, int c) { return T{slice(t.d, c0, c), slice(t.g, c0, c)}; }

// OP_JOIN (MultiResUnet): out = relu(inA + inB), the residual join of a MultiRes block / ResPath unit; the BatchNorm behind it is an OP_BN
enum OpType { OP_CONV = 0, OP_BN, OP_POOL, OP_TCONV, OP_HEAD, OP_JOIN };

struct Op {
    OpType type;
    std::string name;
    T inA, inB, out;
    int64_t w_off = -1, b_off = -1;      // trainable offsets: kernel/bias, or gamma/beta for BN
    int64_t mm_off = -1, mv_off = -1;    // state offsets (BN moving mean / variance)
    float alpha = -1.f;                  // conv activation (MultiResUnet: of a BatchNorm's output): <0 none, 0 relu, >0 leaky
    int k = 0;                           // conv kernel size / pool+tconv rate
    // conv without bias: b_off < 0, no bias add and no dbias.  BatchNorm without gamma (Keras scale=False): w_off < 0, gamma is 1
    // and sum(dy xhat), which the data gradient still needs, goes to nogamma_sum instead of the gradient vector
    float* nogamma_sum = nullptr;        // C floats inside Model::nogamma_scratch (zeroed at the top of every backward pass)
    // BN, training forward: the launch that produced the input (join_fwd) left the channel sums in ws[0 .. C) and zeroed
    // ws[C .. 2C): no memset, no mean pass (set by that launch, consumed by the BatchNorm's forward)
    bool mean_ready = false;
    bool need_din = true;                // false for the convs that read the network input
    bool accA = false, accB = false;     // backward: accumulate into (instead of overwrite) the input gradients
    // activation-derivative fusion: the LAST gradient contributor of a conv+activation output multiplies the summed
    // gradient by act'(output) when it stores it (maskA/maskB on that consumer), and the producing conv is then
    // `premasked`: its backward takes out.g as the pre-activation gradient directly.
    bool maskA = false, maskB = false, premasked = false;
    float mask_alpha = 0.f;
    float* coef = nullptr;               // BN: [scale, shift, mean, inv] x C
    double* ws = nullptr;                // BN: [sum, centred sumsq] x C
    // BN batch statistics that rode in the producing conv's epilogue this step: rows of float partials waiting in the
    // model's partials table (0: none)
    int fused_stats_rows = 0;
    // BatchNorm apply elided (f32 dense path): when every reader of a BatchNorm's output is a 3x3 conv that normalises while it
    // stages its operands (k_ig_conv3 forward, k_ig_wgrad2), the apply pass and the normalised tensor are skipped for the step
    // (`elided`, decided by the forward pass, valid until the next one); the convs read the BatchNorm's INPUT and its coefficients.
    // src_bn[k]: the BatchNorm op that produces conv input k (-1: none); out_readers: the ops that read this op's output tensor
    bool elided = false;
    // BN: the max-pool behind this BatchNorm handed its backward pass over (fast_pool_into_bn): the BatchNorm's backward passes route
    // the pooled gradient themselves; pool_grad_acc: dy already holds another reader's gradient (a skip connection)
    const Op* pool_grad = nullptr;
    bool pool_grad_acc = false;
    // BN: this step's dgamma / dbeta sums rode in the data-gradient launch that produced dy (bn_bwd_fold_args): no reduction pass
    bool bwd_sums_rode = false;
    int src_bn[2] = {-1, -1};
    std::vector<int> out_readers;
    // pool: position (0..3, row-major in the 2x2 window) of each output's first maximum, written by the fused BN-apply + pool
    // pass of this step; the backward pass routes by it instead of re-reading the input and output tensors
    unsigned char* pool_idx = nullptr;
    bool pool_idx_valid = false;
};

struct ParamInfo {
    std::string name;
    int64_t shape[4];
    int ndim;
    int trainable;
    int64_t offset;
    int64_t size;
};

struct KStat {
    std::string name;
    int64_t launches = 0;
    double total_ms = 0, bytes = 0, flops = 0;
};

constexpr float kBnMomentum = 0.99f;   // Keras BatchNormalization defaults [TF-2.6]
constexpr float kBnEps = 1e-3f;

struct RegionState;                      // kernels_region.hip
struct PgPlan; struct IgPlan; struct Ig3xPlan;      // kernels_mfma.hip, kernels_igemm.hip, kernels_ig3x.hip

// the thresholds of a pixel-confusion histogram: sorted ascending on the device (the kernel bins by binary search); the counts go
// back to the caller's order through `order`
struct ConfThresholds {
    float* dev = nullptr;                // DNNCA_CONF_MAX_THR floats
    std::vector<int> order;              // sorted position -> the caller's position
    int n = 0;                           // 0: none
};

// Switch table of the small-channel step: every DNNCA_ variable that the pixel-group, column-strip and block-fused
// launchers and the model's own passes consult.  Read ONCE PER MODEL, at the top of Model::build(); a variable set after
// dnnca_model_create does not affect that model, and no two decisions of one model can see different values.  A field is named
// after its variable (DNNCA_NO_TAIL3 -> no_tail3).
struct StepSwitches {
    // fallbacks: the fused / riding launch is off and the launches it replaced run
    bool no_fused = false, no_fused_bwd = false, no_first3 = false, no_first3f = false, no_up3f = false, no_tail3 = false;
    bool no_tcf = false, no_tcm = false, no_tconv_ride = false, no_prep_ride = false, no_fold_adam = false, no_pool_fold = false;
    bool no_fold_acc = false;      // gradient accumulation: pg_fold + grad_accumulate instead of the fused pg_fold_acc
    bool no_bwd3v = false, no_vw = false, no_head_in_conv = false, no_label_fusion = false, no_wg_stream = false;
    bool pgbwd_old = false;      // pgbwd_tc_3x2_3 without the counted waits (the kernel the A/B of that change compares against)
    // opt-in
    bool fz_up2 = false, fz_all = false, lockstep = false, force_rccl = false;
    // tuning aids.  fz_only / fzb_only: the one block that fuses ("down1", "up2", ...; empty: all); stamp_*: (C, NSRC, CO) of the
    // backward kernel that writes in-kernel stamps (0: none), stamps_pf: its pool-fold launch; nblocks > 0 replaces the
    // occupancy-derived grids of the pixel-group kernels, pg_maxocc caps their blocks per CU (2: -0.3 %, 4: same)
    std::string fz_only, fzb_only;
    int stamp_c = 0, stamp_ns = 0, stamp_co = 0;
    bool stamps_pf = false;
    int dbg = 0, fzb_dbg = 0, f3f_abl = 0, abl = 0, tail3_variant = 0;      // (abl, tail3_variant: DNNCA_TUNING builds only)
    int nblocks = 0, pg_maxocc = 3;
    int tail3_slots = 2048, tail3_lds = 0;      // k_tail3: task budget, dynamic LDS bytes (limits blocks per CU)
    int lockstep_maxh = 128;
    int wg_prio = 1;                            // side stream: 0 normal, 1 least urgent, 2 most urgent
    size_t bucket_bytes = 8u << 20;             // gradient all-reduce bucket (at least 4096)
    // MultiResUnet: the residual joins run as g_join_fwd / g_join_bwd + the generic BatchNorm passes instead of kernels_join.hip
    bool no_join = false;
};
StepSwitches step_switches();                   // model.hip: fills the table from the environment

// What a train step asks of its forward pass (dnnca_train_step and its plan dump; the default asks for nothing).  An argument of
// forward(), never model state: head_in_conv_requested (model.hip) is the one place that decides `head_in_conv`
struct StepRequest {
    const float* y = nullptr;        // the step's labels and loss configuration (the head-in-conv launches read them)
    dnnca_loss_cfg cfg{};
    bool defer_head = false;         // a backward pass follows: the head runs fused with the loss and its backward
    bool head_in_conv = false;       // pixel-group plan: the head may ride in the epilogue of the conv that feeds it (fast_conv_fwd_head)
};

// How a small host array of an augmentation call reaches the device (kernels_aug.hip): the pieces are laid out back to back in a
// pinned row of a ring of kAugRing rows and go to the one device row in one asynchronous copy on Model::stream, with an event
// recorded right behind it.  The caller's buffers are free when upload() returns, and upload() does not wait for the stream (the
// exam-file train loop keeps a step queued behind the running one): a pinned row is only waited for when it comes round again,
// kAugRing calls later.  A call that outgrows the pinned rows drains the stream (uploads from the old rows are complete) and
// replaces them; a device row that is outgrown stays in Model::allocs until the model closes -- a queued kernel may still read it.
struct Model;
struct HostRowRing {
    static constexpr int kAugRing = 4;
    struct Piece { const void* host; size_t bytes; };
    char* dev = nullptr;                 // the device row: the pieces of the last upload, then extra_dev bytes
    size_t dev_bytes = 0;
    char* pin = nullptr;                 // kAugRing x pin_bytes, pinned
    size_t pin_bytes = 0;
    hipEvent_t ev[kAugRing] = {nullptr, nullptr, nullptr, nullptr};      // recorded behind the upload that read row k
    int k = 0;
    // min_row: rows are at least this long (sized for max_batch, a ragged last batch does not grow them); extra_dev: device bytes
    // behind the uploaded part that the call's kernels use (zeroed when the row is allocated, not by an upload)
    int upload(Model* M, std::initializer_list<Piece> pieces, size_t extra_dev = 0, size_t min_row = 0);
    void release();                      // ~Model: the pinned rows and the events (the device row goes with Model::allocs)
};

struct Model {
    dnnca_model_desc desc;
    StepSwitches sw;
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<ParamInfo> params;
    std::vector<Op> ops;
    std::vector<void*> allocs;
    int64_t nT = 0, nS = 0;
    float *p = nullptr, *g = nullptr, *m = nullptr, *v = nullptr, *state = nullptr;
    double* scalars = nullptr;           // kScalars doubles
    float* out5 = nullptr;               // = g + nT : [loss, positive_rate, weight, ymin, ymax]
    float *x_stage = nullptr, *y_stage = nullptr, *logits = nullptr, *dlogits = nullptr, *prob = nullptr;
    bool head_defer_ok = false;           // set by the pixel-group plan when a k_pg_fold launch exists
    float* y_smooth = nullptr;           // smoothed labels of the step (label_smoothing, utils/losses.py:62-67)
    // region (Tversky) term of the loss (dnnca_model_set_region_loss, kernels_region_loss.hip).  ws: per image kRlStat doubles
    // (I, P, Y, A, C of the last step), then the block partials of the step's sums; sums_batch: images of the last step that wrote it
    struct RegionLoss { bool on = false; dnnca_region_loss cfg{}; double* ws = nullptr; int sums_batch = 0; } region_loss;
    // boundary term of the loss (dnnca_model_set_boundary_loss): weight > 0 is on, and only beside the region loss, whose launches
    // it rides.  phi [max_batch, outH, outW]: the signed distance map of the last step's raw labels (kernels_boundary.hip), cols its
    // column pass; both allocated once.  batch: images of the last step that wrote phi; sums_batch: ... that wrote S into region_loss.ws
    struct Boundary { float weight = 0.f; float* phi = nullptr; uint32_t* cols = nullptr; int batch = 0, sums_batch = 0; } boundary;
    // top-k (hard-pixel) cross-entropy (dnnca_model_set_topk_loss): fraction > 0 is on, and only beside the region loss, whose
    // launches it rides.  plane [max_batch, outH, outW]: the pixel losses of the last step; ws: the selection's workspace (topk.h:
    // TopkImage per image, histograms, block partials); both allocated once.  batch: images of the last step that wrote them.
    // select_ws: the workspace of dnnca_topk_select_of, which touches nothing of a step
    struct Topk { double fraction = 0.0; float* plane = nullptr; void* ws = nullptr; int batch = 0; void* select_ws = nullptr; } topk;
    // the host arrays of the augmentation entry points (kernels_aug.hip), one ring per entry point: dnnca_augment_u8's draws (+ the
    // channel sums behind them on the device), dnnca_warp_f32's and dnnca_warp_groups_f32's control points, spline weights (and
    // group table), dnnca_affine_f32's [batch, 2, 3] matrices, dnnca_intensity_f32's [batch, c, 32] records
    HostRowRing aug_ring, warp_ring, warpg_ring, affine_ring, intensity_ring;
    float* first_slabs = nullptr;        // bucket copies of the first-layer weight gradient (kernels_first.hip; kept zeroed)
    // bucket rows of the BN reductions that fold themselves (bn_dev.h): kBnTab doubles, then the ticket counter; kept zeroed
    static constexpr int kBnTab = 4096;
    double* bn_tab = nullptr;
    float* extra_zero = nullptr;         // buffer the tuned kernels need zeroed at the top of every backward pass
    size_t extra_zero_n = 0;
    // MultiResUnet: sum(dy xhat) of the BatchNorms without gamma (Op::nogamma_sum), zeroed with the gradient vector by g_step_init;
    // block partials [grid][C] + ticket of join_fwd's channel sums (kernels_join.hip; the ticket is left zeroed by every launch)
    float* nogamma_scratch = nullptr;
    size_t nogamma_n = 0;
    double* join_part = nullptr;
    unsigned* join_ticket = nullptr;
    bool multires() const { return desc.arch == DNNCA_ARCH_MULTIRES; }
    float* head_partials = nullptr;      // [2048][8] block partials of the fused head kernel
    double* conf_dev = nullptr;
    T xin;                               // network input view (points at the current batch)
    int outH = 0, outW = 0;
    int64_t iterations = 0;
    float beta1 = 0.9f, beta2 = 0.999f, eps = 1e-7f;
    int last_batch = 0;
    // exponential moving average of the trainable variables (dnnca_model_set_ema; tf.train.ExponentialMovingAverage with
    // num_updates): e [nT] rides every Adam launch (k_adam<true>, k_pg_fold<true>), one thread per element, nothing crosses to the
    // host.  e == nullptr: off, and every launch is the one it was.  in_use: dnnca_ema_exchange has put the average into `p` (and
    // the raw weights into `e`) -- contents, never pointers: kernel plans and prepared operands hold addresses derived from `p`,
    // and every forward pass rebuilds its weight-derived operands from `p` (fast_prepare, ig_prepare, ig3x_prepare, ig_flip)
    struct Ema { float* e = nullptr; float decay = 0.f; bool warmup = true; int64_t num_updates = 0; bool in_use = false; } ema;
    float ema_next_om();                 // counts one update (never in a dry plan run) and returns (float)(1 - d_n) for it
    int ema_refuse(const char* what);    // DNNCA_ESTATE while the averaged weights are in use, else DNNCA_OK
    // configurable optimizer (dnnca_model_set_optimizer, optim.h).  on == false: plain Adam, no table, every launch is the one it
    // was (pg_fold_adam / g_adam).  on: fast_finish_backward declines the deferred fold and optimizer_step runs
    // [grad_sqnorm, grad_clip_scale,] opt_* on the chunk table.  One device allocation `table`: chunks [nchunks], var_first
    // [nvars + 1], partials [nchunks] doubles, norms [1 + nvars] doubles (the global norm first), scales [nvars] floats.
    // beta1 / beta2 / eps stay the model's own fields above, which dnnca_set_adam feeds too
    struct Optim {
        bool on = false;
        dnnca_optimizer_cfg cfg{};
        void* table = nullptr;
        OptChunk* chunks = nullptr; int* var_first = nullptr; double* partials = nullptr; double* norms = nullptr; float* scales = nullptr;
        int nchunks = 0, nvars = 0;
        bool norm_clip() const { return on && (cfg.clipnorm > 0.f || cfg.global_clipnorm > 0.f); }
    } opt;
    int opt_launches(const float* grad, float lr, float lr_t, float gscale, float om);      // optimizer_step's launches while opt.on
    // gradient accumulation (dnnca_model_set_accumulation, accum.h): one optimizer update per `steps` micro-steps.  a [nT + 4]: the
    // float32 sum of the cycle's gradients (a <- g on its first micro-step, a <- a + g after; slot nT carries the loss through the
    // all-reduce under data parallel); pos: micro-steps in `a` (0: between cycles, `a` then holds the sum that was last applied).
    // steps == 1: off, a == nullptr, and every launch is the one it was.  `g` is never overwritten by the sum
    struct Accum { float* a = nullptr; int steps = 1; int pos = 0; } accum;
    int accumulate(bool reduce);         // optimizer_step's first part while accum.a: the launch (unless the fold did it) and the reduction
    // What one step hands from launch to launch (and from forward() to loss_and_backward() to optimizer_step()).  forward() begins
    // a pass with `step = Step{}`, in front of fast_prepare: nothing of an earlier step, finished or stopped on an error, survives
    // it.  Every other write is a launch setting a hand-over or the launch it is meant for consuming it.  (The hand-overs inside a
    // kernel family live in its plan: PgPlan::prep / pending_head, IgPlan::fold_pending; the per-op ones in Op.)
    struct Step {
        // the fused head's partial sums wait for the launch that ends the backward pass (k_pg_fold reduces them: one launch less)
        struct HeadPending { const float* partials = nullptr; int nblocks = 0, C = 0; float* dw = nullptr; float* dbias = nullptr; } head_pending;
        bool step_init_done = false;      // train step: the launch that prepares the pixel-group B operands already zeroed scalars / gradients / slabs
        // single-replica training steps: the step outputs are written by the Adam launch instead of a launch of their own
        struct FinalizePending { bool on = false; dnnca_loss_cfg cfg; double n_label = 0, inv_batch_hw = 0; } fin_pending;
        bool head_deferred = false;       // train step: the head runs fused with the loss and its backward
        // label statistics of a train step as per-block partials (sum, min, max, -) written into Model::label_part by the first
        // encoder block's fused launch (kernels_fused.hip) and consumed by the head-in-conv kernel: no launch and no atomics of their own
        int label_part_nblk = 0; bool label_part_valid = false;
        const Op* tconv_done = nullptr;      // the transposed conv whose backward rode in the launch of the conv behind it (k_pgbwd TCF)
        const Op* first_done = nullptr;      // the first conv whose weight gradient rode in the backward launch of the conv behind it (k_first3)
        // the step's operand preparation (k_pg_prep: B operands + zeroing) waits for the first launch of the forward pass: the first
        // encoder block's strip kernel takes it along as extra blocks; any other launch flushes it first (LAUNCH)
        void (*prep_flush)(Model*) = nullptr;
        bool fold_deferred = false;          // the slab fold waits for optimizer_step: fold + Adam + step outputs in one launch (fast_fold_adam)
        bool fold_accumulated = false;       // gradient accumulation: the fold has added this micro-step's gradient to Model::accum (pg_fold_acc)
        const Op* tail_done = nullptr;       // the conv whose backward already ran inside the forward pass (fast_tail3)
        struct PoolFold { const Op* conv = nullptr; const Op* pool = nullptr; } pool_fold;     // fast_pool_fold -> fast_conv_bwd hand-over
        // the forward pass of a train step ran the label statistics (labels_done) and maybe the head (done) on the labels y
        struct HeadInConv { const float* y = nullptr; bool done = false, labels_done = false; } head_in_conv;
        bool wg_pending = false;             // the side stream holds work of this backward pass
        bool bucketing = false;              // this step's backward pass sends buckets
        int64_t bucket_hi = 0, bucket_fin = 0;   // [bucket_fin, bucket_hi) is final and not yet sent
        std::vector<char> op_done;           // per pass: this op's work rode in an earlier launch of the pass
    } step;
    float* label_part = nullptr;         // the table behind Step::label_part_valid
    // data parallel
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
    // Gradient vectors above 1 MB (unet_big: 63 MB, mulmo_unet: 6.9 MB) are all-reduced in buckets while the backward pass is
    // still running: the backward pass finalises the flat gradient vector from its END (head, decoder ... first encoder), so
    // a bucket is the newest finalised suffix; it goes to RCCL on a second stream behind an event.  Sums over ranks are
    // elementwise, so the result is bit-identical to the single call.
    hipStream_t comm_stream = nullptr;
    // Weight gradients of the dense (igemm) convs are leaves of the backward pass: nothing reads them before the optimizer step.
    // Train steps launch them on a second, low-priority stream (fork: an event behind the kernel that produced
    // the conv's output gradient; join: one event at the end of the backward pass), where they run beside the HBM-bound
    // BatchNorm passes and data-gradient convs of the main chain instead of in front of them.
    hipStream_t wg_stream = nullptr;
    hipEvent_t wg_fork = nullptr, wg_join = nullptr, wg_bucket = nullptr;
    bool wg_side_begin();                // fork: later launches on `stream` go to the side stream; false: not in this mode
    void wg_side_end(hipStream_t main);  // back to the main stream
    int wg_side_join();                  // the main stream waits for the side stream (end of the backward pass)
    hipEvent_t ev_bucket = nullptr, ev_comm_done = nullptr;
    int bucket_state = 0;                // 0 undecided, 1 the op order finalises a suffix (bucketing possible), -1 it does not
    int collectives_last_step = 0;       // gradient all-reduce calls issued by the last train step
    int64_t collective_floats_last_step = 0;      // floats the last of them covered (the single-call arms; a bucketed step: its last bucket)
    int send_bucket(int64_t lo, int64_t hi);
    // Input pipeline (dnnca_stage_*): a batch travels host -> HBM on its own copy stream into one of a ring of staging slots
    // while the main stream is still working on the previous step; the main stream waits for the slot's `uploaded` event, runs
    // the step, sends the step outputs to a pinned host ring and records `done` (the next upload into the slot waits for it,
    // and the host reads the outputs behind it -- normally one step late, so that it never stalls the launch queue).
    static constexpr int kStageSlots = 8;     // e.g. four for the train feeder + four for the validation inside train()
    struct StageSlot {
        float *x = nullptr, *y = nullptr;
        hipEvent_t uploaded = nullptr, done = nullptr;
        bool has_done = false;           // `done` has been recorded at least once (main thread; handed over with the slot)
        bool is_eval = false;            // the step that last ran on the slot was an evaluation step (rank-local loss)
        int batch = 0;
    } stage[kStageSlots];
    int stage_slots = 0;
    size_t stage_bytes = 0;              // capacity of one slot
    hipStream_t copy_stream = nullptr;
    // staged evaluation (dnnca_eval_begin .. dnnca_eval_end): the pixel-confusion histogram stays on the device and keeps adding
    // up over the batches (exact integer counts); it is read once, at the end
    bool eval_active = false;
    ConfThresholds eval_thr;             // also the one-shot dnnca_pixel_confusion* (never inside an evaluation); counts in conf_dev
    // region metrics (kernels_region.hip): specs, accumulators and workspace; region_eval: the staged eval steps add region counts
    RegionState* region = nullptr;
    // mask refinement of the lesion tables and the boundary distances (dnnca_model_set_lesion_refine, refine.h); all zero: off
    dnnca_lesion_refine refine = {0.f, 0, 0};
    // the kernel families' plans, built by the first forward pass (fast_prepare, ig_prepare, ig3x_prepare), dropped by fast_release /
    // ig_release / ig3x_release; nullptr: none (force_generic, or no forward pass yet)
    PgPlan* plan_pg = nullptr; IgPlan* plan_ig = nullptr; Ig3xPlan* plan_ig3x = nullptr;
    bool region_eval = false;
    float* out_ring = nullptr;           // pinned host memory: kStageSlots x 8 floats (out5 of the step that used the slot)
    // per-step training metrics (dnnca_train_metrics): the fused head kernels store the step's probabilities into `prob` (their
    // PROB variants), one histogram launch counts them against the raw labels at the thresholds tm_thr (a table of its own:
    // validation's staged evaluation runs between train steps) into the step's own row of tm_hist (row kStageSlots: the unstaged
    // entry points), and the row goes to the same row of the pinned tm_pin behind it.
    // tm_scratch: the launch's accumulator + ticket; its last block moves the counts out and leaves it zeroed (no memset launch)
    static constexpr int kTmRow = 2 * (DNNCA_CONF_MAX_THR + 1);      // u64 per histogram row
    ConfThresholds tm_thr;               // n = 0: off
    unsigned long long *tm_scratch = nullptr, *tm_hist = nullptr, *tm_pin = nullptr;
    int tm_ran[kStageSlots + 1] = {};    // thresholds counted by the step that last ran on the row (0: none)
    bool train_metrics_on() const { return tm_thr.n > 0; }
    // measurement
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int prof_mode = 0;                   // 0 off, 1 every launch, 2 only `focus`, 3 every launch keyed by kernel@layer
    const std::string* cur_op = nullptr;
    int prof_period = 1;                 // mode 2: bracket the focus kernel in one train step out of prof_period
    // launches that ride in another kernel's launch keep doing so -- the profile table of mode 1 is the schedule that really runs
    // (their work is then inside the carrying launch's row) -- except in the per-layer table of mode 3
    bool merged_launches() const { return prof_mode != 3; }
    bool dry = false;
    std::string focus, plan_text;
    // the template variant of the next launch ("n4w8", "m2n4w4", ...): appended to the launch name as `name#variant` in the dry
    // plan only (dnnca_plan_dump) -- the kernel-coverage test tells variants apart, the profile tables keep aggregating by name
    std::string variant;
    void set_variant(const char* fmt, ...);
    std::map<std::string, int> kid;
    std::vector<KStat> kstats;
    struct Rec {
        int id;
        hipEvent_t a, b;
    };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> evpool;

    // mulmo: the encoders (unet.py:152-165) are identical in shape and independent until the bottleneck concat; their ops sit one
    // encoder after the other in `ops` (enc_ops each, n_enc of them, from index 0).  Both passes walk them in LOCKSTEP (op j of every
    // encoder, then op j + 1, ...) so that one launch can serve the twin ops of all encoders (fast_bn_bwd_mp, ...): at op j of the
    // first encoder visited, the inputs of every encoder's op j are ready.  enc_ops = 0: no such structure.
    int enc_ops = 0, n_enc = 0;
    bool lockstep() const;
    std::vector<int> pass_order(bool backward) const;      // op indices in the order a pass visits them

    // input sensitivity (dnnca_input_sensitivity): while sens_pass is set the inference forward keeps every tensor a backward pass
    // reads (no fused, elided or riding op) and leaves its logits in `dlogits`; the tensors' .g views are the pass's scratch.
    // sens_descs: the first-layer table (sens.h SensFirst x sens_nz, static per model); sens_part: block partials; sens_ticket: one
    // counter per (image, table entry), kept zeroed; sens_sums: [max_batch, in_channels] doubles
    bool sens_pass = false;
    void* sens_descs = nullptr;
    int sens_nz = 0;
    double *sens_part = nullptr, *sens_sums = nullptr;
    unsigned* sens_ticket = nullptr;
    int input_sensitivity(const float* x_dev, int B);      // enqueues the pass; the sums are in sens_sums behind it
    int sens_refusal(const char* what);                    // the models neither input-gradient pass takes
    int sens_backward(const float* x_dev, int B);          // the part both passes share: forward + data gradients down to the first convs
    void sens_first_cost(int B, double* bytes, double* flops) const;

    // integrated gradients (dnnca_integrated_gradients): scratch allocated for max_batch by the first call.  attr_acc: the
    // accumulator / map [max_batch, H, W, C]; attr_in: the path input the steps' forwards read (x_stage stays as it is); attr_x0:
    // the baseline table [max_batch, C]; attr_part: block partials; attr_out: the sums and endpoints (Model::integrated_gradients).
    // attr_steps_last / attr_baseline_last: what DNNCA_PLAN_ATTRIBUTION replays (before any call: 32, black)
    static constexpr int kAttrMaxSteps = 256;
    float *attr_acc = nullptr, *attr_in = nullptr, *attr_x0 = nullptr;
    double *attr_part = nullptr, *attr_out = nullptr;
    int attr_steps_last = 32, attr_baseline_last = 0;
    int integrated_gradients(const float* x_dev, int B, int steps, int baseline, bool want_map);

    // test-time augmentation (dnnca_forward_tta): the flipped / transposed copy of the batch that a view's forward reads, allocated
    // for max_batch by the first call (x_stage keeps the untransformed batch); tta_io: the device buffers of dnnca_tta_view_of /
    // dnnca_tta_mean_of (input, then output), grown on demand
    float* tta_view = nullptr;
    float* tta_io = nullptr;
    size_t tta_io_n = 0;
    // the spread of the views (dnnca_forward_tta_spread): the plane [max_batch, H, W] and the three planes of running moments, both
    // allocated by the first call of that function; valid from such a call (for its batch) until anything else rewrites `prob`
    float* tta_spread = nullptr;
    float* tta_mom = nullptr;
    bool tta_spread_valid = false;
    int tta_spread_batch = 0;
    // the ensemble (dnnca_model_set_members, dnnca_forward_ensemble; kernels_ensemble.hip).  w: n + 1 slots of nT + nS floats, one
    // per member (its trainable vector, then its BatchNorm state) and the spare that keeps the model's own (p, state) while a call
    // has a member's in their place -- contents, never pointers, as with Ema; stored: bit m set once slot m was filled.  planes:
    // seven planes [max_batch, H, W] allocated by the first dnnca_forward_ensemble: the running sum es, the first member's mean e0,
    // sum d, sum d^2 (d = mean_m - e0), sum s_m^2 (written by every member but the last, read by every member but the first), then
    // between and within (written by the last member alone).  spread_valid: the last call that wrote tta_spread was an ensemble's
    // (the two components are then valid as long as tta_spread_valid is).  n == 0: off, nothing allocated, no launch differs
    struct Members { float* w = nullptr; int n = 0; unsigned stored = 0; float* planes = nullptr; bool spread_valid = false; } members;
    // calibration (dnnca_calibration): the device tables, the temperatures and the block partials of the NLL, grown on demand
    void* calib_ws = nullptr;
    size_t calib_ws_bytes = 0;
    // the detection map (dnnca_detection_map, kernels_detect.hip): scratch plane, parents, slice states and records, grown on
    // demand; detect_last: the parameters of the last call (what DNNCA_PLAN_DETECTION replays)
    void* detect_ws = nullptr;
    size_t detect_ws_bytes = 0;
    dnnca_detection_cfg detect_last = {0.1f, 0.4f, 5, 10, 16};
    // the bootstrap (dnnca_bootstrap_sums / _detection, kernels_bootstrap.hip): inputs and a chunk of outputs, grown on demand
    void* boot_ws = nullptr;
    size_t boot_ws_bytes = 0;

    ~Model();
    int build();
    int64_t add_param(const std::string& name, std::initializer_list<int64_t> shape, int trainable);      // appends to `params`; returns the offset
    T new_tensor(int H, int W, int C, int* rc);      // data + gradient buffers for max_batch images (no-op once *rc is an error)
    int build_multires();                // the MultiResUnet plan (desc.arch == DNNCA_ARCH_MULTIRES)
    int build_buffers();                 // flat parameter / gradient / optimizer vectors, staging and output buffers, Keras defaults
    int alloc(void** ptr, size_t bytes);
    int forward(const float* x_dev, int B, bool training, const StepRequest& req = StepRequest());
    int loss_and_backward(const float* y_dev, int B, const dnnca_loss_cfg& cfg, bool backward);
    int optimizer_step(float lr, bool reduce = true);      // reduce == false: no all-reduce (dnnca_apply_gradients)
    int flush_profile();

    // launch accounting ------------------------------------------------------------------------------------
    bool begin(const char* name, double bytes, double flops);
    void end();
};

}  // namespace dnnca

// A launch is only "open" for profiling between begin() and end(); focus mode leaves other launches untouched.
#define LAUNCH(m, name, bytes, flops, call)                \
    do {                                                   \
        if ((m)->step.prep_flush) {      /* a deferred operand preparation that no launch has taken along: it goes first */ \
            auto flush_ = (m)->step.prep_flush;                 \
            (m)->step.prep_flush = nullptr;                     \
            flush_(m);                                     \
        }                                                  \
        bool prof_open_ = false;                           \
        if ((m)->dry || (m)->prof_mode) {                  \
            size_t before_ = (m)->recs.size();             \
            bool go_ = (m)->begin(name, bytes, flops);     \
            prof_open_ = (m)->recs.size() != before_;      \
            if (!go_) break;                               \
        }                                                  \
        call;                                              \
        if (prof_open_) (m)->end();                        \
        (m)->variant.clear();                              \
    } while (0)

