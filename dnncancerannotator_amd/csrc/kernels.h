// kernels.h -- host-side launchers of the HIP kernels.  All tensors are NHWC float32 views (common.h).
#pragma once
#include "common.h"

namespace dnnca {

#define DEVINL __device__ __forceinline__

// the model's output activation: the one expression behind every probability the library hands out for a logit (k_sigmoid and the
// test-time-augmentation mean), so that they agree bit for bit
DEVINL float sigmoid_of_logit(float x) {
    float e = expf(-fabsf(x));
    return x >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}

// ----------------------------------------------------------------------------- generic (any shape, untuned) kernels
// y = act(conv_kxk(concat(A, Bv)) + bias); Bv.C may be 0.  Weight layout HWIO with I = A.C + Bv.C.  bias / dbias may be null
// (a conv without bias); gamma may be null in g_bn_finalize / g_bn_bwd_apply (a BatchNorm without scale: gamma = 1).
// alpha < 0 -> no activation, alpha == 0 -> relu, alpha > 0 -> leaky relu.
void g_conv_fwd(hipStream_t s, int B, View A, View Bv, const float* w, const float* bias, View out, int K, float alpha);
// dz = dy * act'(y) in place on dy (dense tensors)
void g_act_bwd(hipStream_t s, size_t n, float* dy, const float* y, float alpha);
void g_act_bwd_view(hipStream_t s, int B, View dy, View y, float alpha);      // the same on views (channel slices)
// dA / dB (beta 0 = overwrite, 1 = accumulate) from dz (view of the conv output gradient, C = Cout)
void g_conv_dgrad(hipStream_t s, int B, View dz, const float* w, View dA, int accA, View dB, int accB, int K);
// dW (HWIO) += ..., dbias += ...   (atomic accumulation into pre-zeroed buffers)
void g_conv_wgrad(hipStream_t s, int B, View A, View Bv, View dz, float* dw, float* dbias, int K);

void g_pool_fwd(hipStream_t s, int B, View in, View out, int r);
// din = (acc ? din : 0) + route(dout) ; first maximum in row-major window order receives the gradient
void g_pool_bwd(hipStream_t s, int B, View in, View out, View dout, View din, int acc, int r);

// Conv2DTranspose k = s = r; weight [r, r, Cout, Cin]
void g_tconv_fwd(hipStream_t s, int B, View in, const float* w, const float* bias, View out, int r);
void g_tconv_dgrad(hipStream_t s, int B, View dout, const float* w, View din, int acc, int r);
void g_tconv_wgrad(hipStream_t s, int B, View in, View dout, float* dw, float* dbias, int r);

// BatchNormalization.  ws: 4*C doubles of scratch (sum, sumsq-centred, dgamma, dbeta) zeroed by the caller;
// coef: [scale(C), shift(C), mean(C), inv(C)] floats.
void g_bn_stats_mean(hipStream_t s, int B, View x, double* ws);
void g_bn_stats_var(hipStream_t s, int B, View x, double* ws);   // uses mean = ws[c]/n
void g_bn_finalize(hipStream_t s, int C, double n, const double* ws, const float* gamma, const float* beta,
                   float* mmean, float* mvar, float* coef, int training, float momentum, float eps);
// alpha: activation of the normalised value (as g_conv_fwd; MultiResUnet's conv -> BatchNorm -> ReLU)
void g_bn_apply(hipStream_t s, int B, View x, View y, const float* coef, float alpha = -1.f);
void g_bn_bwd_reduce(hipStream_t s, int B, View x, View dy, const float* coef, float* dgamma, float* dbeta);
void g_bn_bwd_apply(hipStream_t s, int B, View x, View dy, View dx, int acc, const float* coef, const float* gamma,
                    const float* dgamma, const float* dbeta, double n);

// residual join (MultiResUnet): out = relu(a + b); da, db (+)= dout * [out > 0].  The in-library cross-check of kernels_join.hip
void g_join_fwd(hipStream_t s, int B, View a, View b, View out);
void g_join_bwd(hipStream_t s, int B, View dout, View out, View da, int acca, View db, int accb);

// head: logits[b,y,x] = sum_c feat*w[c] + bias  (Conv2D(1, 1), unet.py:241-244)
void g_head_fwd(hipStream_t s, int B, View feat, const float* w, const float* bias, float* logits);
void g_head_bwd(hipStream_t s, int B, View feat, const float* w, const float* dlogits, View dfeat, float* dw, float* dbias);

// scalars layout (doubles): see model.hip kScalar*
void g_label_stats(hipStream_t s, size_t n, const float* y, double* scalars);
// loss + dlogits + probabilities.  inv_count = 1/(H*W*B*replicas) for dlogits; per-pixel loss summed into scalars.
void g_loss(hipStream_t s, size_t n, const float* logits, const float* y, const dnnca_loss_cfg cfg, double n_label,
            double* scalars, float* dlogits, float* prob, float grad_scale);
void g_sigmoid(hipStream_t s, size_t n, const float* logits, float* prob);

// ----------------------------------------------------------------------------- test-time augmentation (kernels_tta.hip)
// A view k = 4 t + 2 v + h of the dihedral group: flips first (v: rows, h: columns), then, with t, the transpose (H == W).
// dst[b,i,j,c] = view k of src [B,H,W,C]; dst must not alias src
void g_tta_view_in(hipStream_t s, const float* src, float* dst, int B, int H, int W, int C, int k);
// prob[b,i,j] (op)= p at the position of view k's plane `src` [B,H,W] that original pixel (i,j) went to; p = src or, with is_logits,
// sigmoid_of_logit(src).  first: prob = p, otherwise prob += p; last: the sum is then divided by n.  prob must not alias src
void g_tta_accumulate(hipStream_t s, const float* src, float* prob, int B, int H, int W, int k, bool is_logits, bool first, bool last,
                      int n);
// g_tta_accumulate plus the views' spread: view number `pos` (0 .. n - 1, in launch order) of n.  mom: three planes of `plane` floats
// of running state (the first view's value, the sums of the differences to it and of their squares); the last view writes the mean
// into prob (bit for bit g_tta_accumulate's) and sqrt((1/n) sum (p_k - mean)^2) into spread.  No buffer may alias another
void g_tta_moments(hipStream_t s, const float* src, float* prob, float* mom, float* spread, size_t plane, int B, int H, int W, int k,
                   bool is_logits, int pos, int n);

// ----------------------------------------------------------------------------- ensembles (kernels_ensemble.hip)
// Member number `pos` (0 .. n - 1, in launch order) of n joins the ensemble, per pixel of npix.  mean_in: the member's mean
// probability; within_in: its within-member spread, nullptr for 0.  run: the running planes, `pitch` floats apart: the sum es, the
// first member's mean e0, sum d, sum d^2 (d = mean_m - e0), sum s_m^2; every member but the last writes them, and without
// between_out only es is touched.  The last member writes mean_out = es / n (float32 sum in launch order, one division: the
// operations of g_tta_accumulate) and, with between_out, between = sqrt(max(0, (sum d^2 - (sum d)^2 / n) / n)), within =
// sqrt(sum s^2 / n) and total = sqrt of the sum of the two variances.  mean_out may be mean_in and total_out may be within_in (a
// pixel is read and written by one thread); no other buffer may alias another
void g_ens_join(hipStream_t s, size_t npix, const float* mean_in, const float* within_in, float* run, size_t pitch, int pos, int n,
                float* mean_out, float* between_out, float* within_out, float* total_out);

void g_l2(hipStream_t s, size_t n, const float* w, float* g, float l2, double* scalars);   // g += 2*l2*w ; penalty += l2*sum w^2
// writes [loss, positive_rate, weight, ymin, ymax] floats to out5 (device) from the scalar block
void g_finalize_scalars(hipStream_t s, double* scalars, const dnnca_loss_cfg cfg, double n_label, double inv_batch_hw,
                        float* out5);
// e != nullptr: the weight average rides the launch, e <- e - om * (e - p) with the p just written (Model::ema)
void g_adam(hipStream_t s, size_t n, float* p, const float* g, float* m, float* v, float lr_t, float b1, float b2,
            float eps, float gscale, float* e = nullptr, float om = 0.f);
void g_adam_finalize(hipStream_t s, size_t n, float* p, const float* g, float* m, float* v, float lr_t, float b1, float b2, float eps,
                     float gscale, double* scalars, const dnnca_loss_cfg cfg, double n_label, double inv_batch_hw, float* out5,
                     float* e = nullptr, float om = 0.f);
void g_ema_exchange(hipStream_t s, size_t n, float* a, float* b);      // a <-> b, exact (dnnca_ema_exchange)
constexpr int DNNCA_CONF_MAX_THR = 1024;
// pixel-confusion histogram.  out == nullptr: the bins add up in `hist` [2][nthr + 1] over launches (zeroed by the caller).
// out != nullptr (per-step training metrics): `hist` is scratch ([2][nthr + 1] + ticket, kept zeroed); the launch's last block
// moves the bins into `out` [2][nthr + 1] and zeroes the scratch again
void g_conf_hist(hipStream_t s, size_t n, const float* prob, const float* y, const float* thr_sorted, int nthr,
                 unsigned long long* hist, unsigned long long* out);
void g_scale(hipStream_t s, size_t n, float* p, float a);
// zeroes a[0..na) and b[0..nb) (either may be empty) and resets the scalar block, in one launch
void g_step_init(hipStream_t s, double* scalars, float* a, size_t na, float* b, size_t nb);

}  // namespace dnnca
