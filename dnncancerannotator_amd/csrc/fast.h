// fast.h -- hooks through which model.hip routes an op to a tuned gfx950 kernel.  Each returns false when it has no
// specialisation for the op's shape, in which case the caller falls through to the generic kernel.
#pragma once
#include "model.h"

namespace dnnca {

// per-pass operand preparation (weights -> MFMA B operands); train_step: a backward pass follows (StepRequest::defer_head) -- the
// launch then also zeroes scalars, gradients and slabs (Step::step_init_done) and may wait for the first launch (Step::prep_flush)
int fast_prepare(Model* m, bool train_step);
int fast_finish_backward(Model* m);   // folds the weight-gradient slabs into the flat gradient vector (or defers: Step::fold_deferred)
int fast_fold_adam(Model* m, float lr_t, float ema_om, const dnnca_loss_cfg& cfg, double n_label, double inv_batch_hw);   // the deferred fold + Adam + step outputs in one launch
int fast_fold_acc(Model* m, bool first, const dnnca_loss_cfg& cfg, double n_label, double inv_batch_hw);   // gradient accumulation: the deferred fold + accumulate + step outputs in one launch
void fast_release(Model* m);    // drop the model's pixel-group plan (Model::plan_pg)
unsigned long long* fast_debug_stamps(const Model* m);   // tuning aid: in-kernel s_memtime stamps (DNNCA_STAMPS); nullptr: none (asking creates nothing)
// `pool`: a max-pool op fused into the conv's epilogue (fast_pool_fusable), or nullptr
bool fast_conv_fwd(Model* m, int B, Op& o, double bytes, double flops, Op* pool);
bool fast_pool_fusable(const Model* m, const Op& conv, const Op& pool);
// the conv that feeds the head, training step: head + loss + head backward ride in its epilogue (labels' statistics already on the stream)
bool fast_conv_fwd_head(Model* m, int B, Op& o, Op& head, const float* y, const dnnca_loss_cfg& cfg, float gscale, double bytes, double flops);
// kernels_fused.hip: a whole Downsample / Upsample block (components.py:77-81, 158-166) of configs/unet.yaml in one launch;
// ops[oi .. oi+2] are consumed when these return true.  store_mid: also write the block's intermediate tensors (a backward pass follows)
bool fused_down_fwd(Model* m, int B, size_t oi, bool store_mid, const float* labels = nullptr);   // labels: also reduce them (first block only)
// ... or, where the shape allows, that conv's forward, the head, the loss and the conv's whole backward in one launch (sets Step::tail_done)
bool fast_tail3(Model* m, int B, Op& o, Op& head, const float* y, const dnnca_loss_cfg& cfg, float gscale);
bool fast_first3_fwd(Model* m, int B, Op& c1, Op& c2, Op& pool, float* y0, unsigned char* pool_idx, const float* labels, float* label_part,
                     double bytes, double flops, int* nblocks);      // first encoder block forward as one column-strip launch
bool fast_up3_fwd(Model* m, int B, size_t oi);     // last decoder block: transposed conv + two-source conv forward in one column-strip launch
bool fast_head_in_conv_possible(Model* m);      // would fast_conv_fwd_head take the conv that feeds the head?
bool fused_up_fwd(Model* m, int B, size_t oi, bool store_mid, int* consumed = nullptr);
bool fused_up2_fwd(Model* m, int B, size_t oi, bool store_mid);     // the two convs of a decoder block whose transposed conv has already run: ops[oi], ops[oi + 1]
// kernels_fused_bwd.hip: the whole BACKWARD of a Downsample / Upsample block of configs/unet.yaml (6- and 12-channel levels) in one
// launch; `oi` is the block's LAST op (the max-pool / the second conv): ops[oi - 2 .. oi] are consumed when these return true
bool fused_down_bwd(Model* m, int B, size_t oi);
bool fused_up_bwd(Model* m, int B, size_t oi);
// kernels_mfma.hip: what the block-fused kernels need from the pixel-group plan
constexpr int kPgBuckets = 16;                                 // partial-sum slabs per weight gradient
bool fast_pg_conv_supported(const Model* m, const Op& o);      // a 3x3 conv of the pixel-group plan
const float* fast_conv_bmat_dgrad(const Model* m, const Op& o);      // prepared data-gradient B operands (all passes), or nullptr
float* fast_wgrad_slabs(const Model* m, const Op& o, int source);    // weight-gradient slabs of (op, source) -- transposed convs: source 0 -- or nullptr
bool fast_conv_bwd(Model* m, int B, Op& o, double out_bytes, double in_bytes, double flops);
// kernels_first.hip: the one-channel-input 3x3 convs (first layer of every encoder)
bool fast_first_conv_fwd(Model* m, int B, Op& o, double bytes, double flops, Op* bn_next);   // bn_next as for ig_conv_fwd
bool fast_first_conv_bwd(Model* m, int B, Op& o, double out_bytes, double in_bytes, double flops);
bool fast_pool_fwd(Model* m, int B, Op& o, double bytes);
bool fast_pool_bwd(Model* m, int B, Op& o, double bytes);
bool fast_pool_fold(Model* m, Op& pool, Op& conv);      // the pool's backward rides in conv's backward launch (conv produced the pool's input)
bool fast_tconv_fwd(Model* m, int B, Op& o, double bytes, double flops);
bool fast_tconv_bwd(Model* m, int B, Op& o, double out_bytes, double in_bytes, double flops);
bool fast_pool_supported(const Model* m, const Op& o);
bool fast_tconv_supported(const Model* m, const Op& o);
bool fast_head_supported(const Model* m, const Op& o);
bool fast_head_train(Model* m, int B, Op& o, const float* y, const dnnca_loss_cfg& cfg, float gscale, double bytes);
void fast_head_partials_done(Model* m, int C, int blocks, float* dw, float* dbias);      // C in {3, 16, 64}: rows of C + 2 partials are in head_partials
// utils/losses.py:62-67 label_smoothing: Gaussian blur of the labels (false: unsupported filter size / image smaller than the pad)
bool fast_label_smooth(Model* m, int B, int H, int W, const float* y, float* out, int k, float sigma);
bool fast_label_stats(Model* m, size_t n, const float* y);
// pool: a 2x2 max-pool of the output that rides in the apply pass; pool_bn: the BatchNorm of the pooled tensor (its batch statistics ride along too)
bool fast_bn_fwd(Model* m, int B, Op& o, bool training, float momentum, float eps, Op* pool, Op* pool_bn);
bool fast_bn_pool_fusable(const Model* m, const Op& bn, const Op& pool);
bool fast_bn_bwd(Model* m, int B, Op& o);
bool fast_pool_into_bn(Model* m, Op& pool, Op& bn);      // the pool's backward rides in the backward passes of the BatchNorm in front of it
bool fast_bn_supported(const Model* m, const Op& o);
void fast_plan_masks(Model* m);
// Switch table of the dense path, read ONCE per process at its first use: the plan made at model creation (which
// BatchNorm apply passes are elided, which tensors are stored as bf16) and every later launch decision must see the same values -- a
// conv must never read a normalised tensor that was never written.  Deliberately NOT here, because tests flip them in-process:
// DNNCA_NO_HALF, _NO_HALF_Z, _NO_HALF_DY (read when a model is built, ig_plan_half) and DNNCA_FOLD_BATCH (read per step, ig_prepare).
// (The switches of the small-channel step are per MODEL: StepSwitches, model.h.)
struct DenseSwitches {
    // first-generation kernels (the fallbacks beyond the 32-bit offset limits)
    bool igconv1, wgrad1, tcwgrad1, tconv_fwd1;
    // the exact-fp32 MFMA kernels in place of the split-bf16 ones (fallbacks for more than 1024 output channels / oversized planes)
    bool no_x3, no_x3_wgrad;
    // weight-gradient slabs: float atomics instead of plain stores, no bucket copies, four-wave bf16 kernel for bf16-stored operands
    bool no_wg_plain, no_wg_buckets, wgrad64_narrow;
    // BatchNorm riders
    bool no_bn_fusion, no_pool_stats, no_norm_on_load, no_bn_bwd_ride, no_pool_bn_bwd;
    // tuning aids: waves per block (4 | 8; 0: by the eight-wave rule), split-bf16 channel tile cap / resident-block cap / no channel
    // split of the waves, grid caps of the BatchNorm and pool passes
    int ig_nw, igb_nw, x3_nn, x3_blocks;
    bool x3_no_split, x3_no_db;      // ... and no second LDS buffer
    int bn_blocks, pool_blocks;
};
const DenseSwitches& dense_switches();

// ---- the launch a dense layer gets.  Pure functions of the model description, the op, the batch size and the switch table: they touch
// no device memory and launch nothing.  The planners (ig_plan_half, ig_prepare, ig_norm_on_load_ok) ask them what WILL run; the
// launchers call the same functions and execute the answer.
enum DenseKernel {
    DK_NONE,
    // 3x3 conv forward / data gradient: split-bf16 persistent (ig3x::k_ig3x_conv3), exact-fp32 persistent (ig::k_ig_conv3),
    // first-generation fp32 (ig::k_ig_conv), bf16 persistent (igb::k_igb_conv3), first-generation bf16 (igb::k_igb_conv)
    DK_X3_CONV3, DK_F32_CONV3, DK_F32_CONV, DK_B16_CONV3, DK_B16_CONV,
    // 3x3 conv weight gradient of one source: split-bf16 (ig3x::k_ig3x_wgrad), second- / first-generation fp32 (ig::k_ig_wgrad2,
    // k_ig_wgrad), bf16 on 64-channel tiles with eight waves and bf16-stored operands (igb::k_igb_wgrad64w) / with four waves
    // (k_igb_wgrad64), first-generation bf16 (k_igb_wgrad)
    DK_X3_WGRAD, DK_F32_WGRAD2, DK_F32_WGRAD, DK_B16_WGRAD64W, DK_B16_WGRAD64, DK_B16_WGRAD,
    // transposed conv forward (bf16 / fp32, second / first generation), data gradient, weight gradient
    DK_B16_TCONV2, DK_B16_TCONV, DK_F32_TCONV2, DK_F32_TCONV, DK_B16_TCONV_DGRAD, DK_F32_TCONV_DGRAD,
    DK_B16_TCONV_WGRAD64, DK_F32_TCONV_WGRAD2, DK_F32_TCONV_WGRAD,
};
struct DenseLaunch {
    DenseKernel kern = DK_NONE;
    int nn = 0, mw = 0;             // channel tile: 16 nn output channels (N of the GEMM) x 16 mw (weight gradients: M)
    int nw = 4, wn = 1;             // waves per block; how many of them split the channel tile
    bool db = false;                // two LDS buffers
    bool a16 = false, x16 = false, g16 = false;      // bf16-stored conv source / weight-gradient activations / output gradient
    bool k64 = false;               // 64-channel K chunks (bf16 transposed-conv data gradient)
    bool plain = false, bucketed = false;            // weight-gradient slabs: one per pixel-split block / WG_BUCKETS shared copies
    // forward: the batch statistics of the BatchNorm behind it can ride in the epilogue; data gradient: the backward sums of the
    // BatchNorm in front of it can
    bool stats = false, bnb = false;
    int tiles_x = 0, tiles_y = 0, psplit = 0;
    unsigned units = 0, block = 256;          // units: work items of a persistent kernel (grid.x = min(units, resident blocks))
    dim3 grid;
};
DenseLaunch dense_conv_fwd(const Model* m, int B, const Op& o, const DenseSwitches& sw);
DenseLaunch dense_conv_dgrad(const Model* m, int B, const Op& o, const DenseSwitches& sw);
DenseLaunch dense_conv_wgrad(const Model* m, int B, const Op& o, int source, const DenseSwitches& sw);
DenseLaunch dense_tconv_fwd(const Model* m, int B, const Op& o, const DenseSwitches& sw);
DenseLaunch dense_tconv_dgrad(const Model* m, int B, const Op& o, const DenseSwitches& sw);
DenseLaunch dense_tconv_wgrad(const Model* m, int B, const Op& o, const DenseSwitches& sw);
// the three rules every dense launch shares
inline bool fits32(double bytes) { return bytes < 2.0e9; }          // the kernel's 32-bit byte offsets reach the whole tensor
inline int pixel_split(int combos, int ntiles, int blocks = 256) {  // pixel-split blocks per channel-block pair: `blocks` in all
    const int ps = (blocks + combos - 1) / combos;
    return ps > ntiles ? (ntiles < 1 ? 1 : ntiles) : ps;
}
// eight waves per block on 32 x 16-pixel tiles once that still gives every CU a unit
inline bool eight_waves(int B, int H, int W, int channel_tiles) {
    const long units8 = (long)((W + 15) / 16) * ((H + 31) / 32) * B * channel_tiles;
    return units8 >= 256;
}
// Grid of a persistent kernel of the small-channel step: one block per work item, at most the blocks that are resident at once on
// the 256 CUs -- what the occupancy calculator allows per CU, capped at per_cu_cap.  The calculator is asked once per kernel; the
// cap is applied per call (it may come from a model's switches).
template <auto Kernel, int Threads>
inline int resident_grid(int per_cu_cap, int items) {
    static const int occupancy = [] {
        int n = 0;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, Kernel, Threads, 0) == hipSuccess && n >= 1 ? n : 1;
    }();
    const int fit = 256 * (occupancy < per_cu_cap ? occupancy : per_cu_cap);
    return items < fit ? items : fit;
}
// implicit-GEMM MFMA path for channel counts that are multiples of 16 (kernels_igemm.hip)
bool ig_conv_supported(const Model* m, const Op& o);
int ig_prepare(Model* m);
int ig_finish_wgrad(Model* m);      // the backward pass's weight-gradient slab folds in one launch (before the streams join)
int ig_plan_half(Model* m);        // dtype bf16: decides View::h for every tensor (static per model; after fast_plan_masks)
int ig_begin_backward(Model* m);
void ig_release(Model* m);
bool ig_conv_fwd(Model* m, int B, Op& o, double bytes, double flops, Op* bn_next);   // bn_next: BatchNorm of the output whose statistics may ride in the epilogue
bool ig_conv_bwd(Model* m, int B, Op& o, double out_bytes, double in_bytes, double flops);
// the data gradient of a dense conv / transposed conv without its weight-gradient half, activation mask or BatchNorm sums (the
// input-sensitivity pass: o.out.g holds the pre-activation gradient); false: not a dense layer
bool ig_conv_dgrad_only(Model* m, int B, Op& o, double bytes, double flops);
bool ig_tconv_dgrad_only(Model* m, int B, Op& o, double bytes, double flops);
// will this conv's forward and weight-gradient launches (batch B) be the kernels that can normalise a BatchNorm's input while staging it?
// (Model::forward elides the BatchNorm's apply pass on this answer)
bool ig_norm_on_load_ok(const Model* m, int B, const Op& o);
struct BnSelfFold;
struct BnBwdFold;
// batch statistics of BatchNorm `bn` folded by the kernel that produces its input (bn_dev.h): fills *f and marks the statistics as
// taken care of (Op::fused_stats_rows); false: not available (the BatchNorm then runs its own reduction pass)
bool bn_self_fold_args(Model* m, Op& bn, int B, BnSelfFold* f);
bool bn_bwd_fold_args(Model* m, Op& bn, BnBwdFold* f);      // the BatchNorm backward sums ride in the launch that produces dy (ConvArgs::bnb)
// kernels_ig3x.hip: the fp32 3x3 convs on the bf16 matrix pipe (three bf16 planes per operand, fp32-accurate)
namespace ig { struct ConvArgs; struct WgArgs; }
bool ig3x_enabled(const Model* m);
int ig3x_prepare(Model* m);
void ig3x_release(Model* m);
// the split-bf16 part of dense_conv_fwd / _dgrad / _wgrad (pure): fills *d and returns true when these kernels take the launch.
// mode 0 forward / 1 data gradient; cin: all sources; nn: channel tile of the exact-fp32 kernel; any_half: a bf16-stored tensor takes part
bool ig3x_conv_decide(const Model* m, const DenseSwitches& sw, int mode, int B, int H, int W, int cin, int cout, int nn, bool any_half, DenseLaunch* d);
bool ig3x_wgrad_decide(const Model* m, const DenseSwitches& sw, int B, int H, int W, int cs, int co, DenseLaunch* d);
void ig3x_launch(Model* m, const DenseLaunch& d, int mode, const ig::ConvArgs& a, size_t w_off, const char* name, double bytes, double flops);
void ig3x_wgrad_launch(Model* m, const DenseLaunch& d, ig::WgArgs w, const char* name, double bytes, double flops);
// kernels_join.hip: the residual join of MultiResUnet, out = relu(a + b) in front of a BatchNorm, as streaming passes (float4 over
// the flat tensor when every view is dense and 16-byte aligned, else strided scalars).  ws != nullptr: also the per-channel sums of
// the output into ws[0 .. C) (and ws[C .. 2C) = 0), folded from block partials in `part` (join_part_doubles(C) doubles) by the block
// that draws the last `ticket` (kept zeroed).  force_grid > 0: that many blocks (tests)
void join_fwd(hipStream_t s, int B, View a, View b, View r, double* ws, double* part, unsigned* ticket, int force_grid = 0);
// y = relu(a + b) * coef[c] + coef[C + c]: join + the BatchNorm's inference affine, the joined tensor itself is not stored
void join_infer(hipStream_t s, int B, View a, View b, View y, const float* coef, int force_grid = 0);
void join_bwd(hipStream_t s, int B, View dr, View r, View dA, int accA, View dB, int accB, int force_grid = 0);
unsigned join_fwd_grid(size_t npix, const View& a, const View& b, const View& r, int force);
size_t join_part_doubles(int C);
bool ig_tconv_supported(const Model* m, const Op& o);
bool ig_tconv_fwd(Model* m, int B, Op& o, double bytes, double flops, Op* bn_next);
bool ig_tconv_bwd(Model* m, int B, Op& o, double out_bytes, double in_bytes, double flops);   // decides maskA/maskB/premasked for every op (static per model)

}  // namespace dnnca
