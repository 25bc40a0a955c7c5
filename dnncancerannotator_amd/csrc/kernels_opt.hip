// kernels_opt.hip -- the configurable optimizers (dnnca_model_set_optimizer): gradient norms for clipnorm / global_clipnorm and the
// Adam / AdamW / SGD updates with the clip scale read from device memory.  Every launch works on the chunk table of optim.h: block c
// owns chunk c, at most kOptChunk consecutive elements of one variable, thread t its elements t, t + 256, ...  (coalesced dwords:
// variable offsets are not 16-byte aligned in general, so nothing here loads wider).  No atomics, no tickets: a chunk's sum of squares
// goes through memory to the launch that adds them up, every sum has one fixed order, so norms, scales and weights are bit-identical
// from run to run.
#include "optim.h"

namespace dnnca {

static constexpr int kPerThread = kOptChunk / kOptThreads;
static_assert(kOptChunk % kOptThreads == 0 && kOptThreads % 64 == 0, "a chunk is a whole number of elements per thread");

// lanes 0..63 in a fixed tree, then the waves in ascending order; the total is valid in thread 0
__device__ __forceinline__ double block_sum_d(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kOptThreads / 64; ++w) t += red[w];
    return t;
}

// Keras' order: the gradient the optimizer receives (after the all-reduce: times 1 / world), then clipvalue
__device__ __forceinline__ float grad_in(float g, float gscale, float clipvalue) {
    float gi = g * gscale;
    if (clipvalue > 0.f) gi = fminf(fmaxf(gi, -clipvalue), clipvalue);
    return gi;
}

__global__ __launch_bounds__(kOptThreads) void k_grad_sqnorm(const OptChunk* __restrict__ chunks, const float* __restrict__ g,
                                                             float gscale, float clipvalue, double* __restrict__ partials) {
    __shared__ double red[kOptThreads / 64];
    const OptChunk c = chunks[blockIdx.x];
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const int i = j * kOptThreads + (int)threadIdx.x;
        if (i < c.n) {
            const double gi = (double)grad_in(g[c.off + i], gscale, clipvalue);      // squares of 1e30 stay finite
            acc += gi * gi;
        }
    }
    const double t = block_sum_d(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

void g_grad_sqnorm(hipStream_t s, const OptChunk* chunks, int nchunks, const float* g, float gscale, float clipvalue, double* partials) {
    hipLaunchKernelGGL(k_grad_sqnorm, dim3((unsigned)nchunks), dim3(kOptThreads), 0, s, chunks, g, gscale, clipvalue, partials);
}

// block v < nvars: variable v's partials (thread t adds chunks lo + t, lo + t + 256, ... in ascending order, then block_sum_d);
// block nvars: all of them, the same way.  The scale is c / max(norm, c) in double, rounded to float once: exactly 1 while norm <= c
__global__ __launch_bounds__(kOptThreads) void k_grad_clip_scale(const int* __restrict__ var_first, int nvars, int nchunks,
                                                                 const double* __restrict__ partials, float clipnorm,
                                                                 float global_clipnorm, float* __restrict__ scales,
                                                                 double* __restrict__ norms) {
    __shared__ double red[kOptThreads / 64];
    __shared__ float bcast;
    const int v = (int)blockIdx.x;
    const bool all = v == nvars;
    const int lo = all ? 0 : var_first[v], hi = all ? nchunks : var_first[v + 1];
    double acc = 0.0;
    for (int k = lo + (int)threadIdx.x; k < hi; k += kOptThreads) acc += partials[k];
    const double total = block_sum_d(acc, red);
    if (threadIdx.x == 0) {
        const double norm = sqrt(total);
        norms[all ? 0 : 1 + v] = norm;
        const double c = (double)(all ? global_clipnorm : clipnorm);
        bcast = (float)(c / fmax(norm, c));
    }
    if (!all) {
        if (threadIdx.x == 0 && clipnorm > 0.f) scales[v] = bcast;
        return;
    }
    if (clipnorm > 0.f) return;
    __syncthreads();
    const float s = bcast;          // global_clipnorm: the one scale, replicated
    for (int k = (int)threadIdx.x; k < nvars; k += kOptThreads) scales[k] = s;
}

void g_grad_clip_scale(hipStream_t s, const int* var_first, int nvars, int nchunks, const double* partials, float clipnorm,
                       float global_clipnorm, float* scales, double* norms) {
    hipLaunchKernelGGL(k_grad_clip_scale, dim3((unsigned)nvars + 1), dim3(kOptThreads), 0, s, var_first, nvars, nchunks, partials,
                       clipnorm, global_clipnorm, scales, norms);
}

// One pass over p, g, m[, v][, e].  The Adam arithmetic is k_adam's (kernels_generic.hip) expression for expression, on
// gi = g * gscale [clipped] * scale: with scale 1 the update is bit-identical to g_adam's.
// AdamW: decoupled decay first, p <- p - (lr * weight_decay) * p as one fused multiply-add, on the variables whose chunk carries
// the flag.
// SGD: momentum 0: p <- p - lr g; else a <- momentum a - lr g (the m slot), p <- p + a, Nesterov p <- p + momentum a - lr g.
// EMA: the thread that stores p[i] also moves the weight average towards it, as k_adam<true> does
template <int KIND, bool EMA>
__global__ __launch_bounds__(kOptThreads) void k_opt(const OptChunk* __restrict__ chunks, float* __restrict__ p,
                                                     const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                     float* __restrict__ e, OptArgs a, AdamFinalize fin) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && fin.out5) step_outputs(fin);
    const OptChunk c = chunks[blockIdx.x];
    const float scale = a.scales ? a.scales[c.var] : 1.f;
    const float lr_t = a.lr_t, b1 = a.b1, b2 = a.b2, eps = a.eps;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const int k = j * kOptThreads + (int)threadIdx.x;
        if (k >= c.n) break;
        const size_t i = (size_t)c.off + k;
        float gi = grad_in(g[i], a.gscale, a.clipvalue);
        gi = gi * scale;
        float pi;
        if (KIND == OPT_SGD) {
            if (a.momentum == 0.f) {
                pi = p[i] - a.lr * gi;
            } else {
                const float ai = a.momentum * m[i] - a.lr * gi;
                m[i] = ai;
                pi = a.nesterov ? p[i] + (a.momentum * ai - a.lr * gi) : p[i] + ai;
            }
        } else {
            float mi = m[i] * b1 + gi * (1.f - b1);
            float vi = v[i] * b2 + (gi * gi) * (1.f - b2);
            m[i] = mi;
            v[i] = vi;
            if (KIND == OPT_ADAMW) {
                float p0 = p[i];
                if (c.decay) p0 = fmaf(-a.lrwd, p0, p0);      // one rounding, whatever the compiler would contract
                pi = p0 - lr_t * mi / (sqrtf(vi) + eps);
            } else {
                pi = p[i] - lr_t * mi / (sqrtf(vi) + eps);
            }
        }
        p[i] = pi;
        if (EMA) {
            const float ei = e[i];
            e[i] = ei - a.om * (ei - pi);
        }
    }
}

template <int KIND>
static void launch_opt(hipStream_t s, const OptChunk* chunks, int nchunks, float* p, const float* g, float* m, float* v, float* e,
                       const OptArgs& a, const AdamFinalize& fin) {
    if (e) hipLaunchKernelGGL((k_opt<KIND, true>), dim3((unsigned)nchunks), dim3(kOptThreads), 0, s, chunks, p, g, m, v, e, a, fin);
    else hipLaunchKernelGGL((k_opt<KIND, false>), dim3((unsigned)nchunks), dim3(kOptThreads), 0, s, chunks, p, g, m, v, nullptr, a, fin);
}

void g_opt_step(hipStream_t s, int kind, const OptChunk* chunks, int nchunks, float* p, const float* g, float* m, float* v, float* e,
                const OptArgs& a, const AdamFinalize& fin) {
    if (kind == OPT_SGD) launch_opt<OPT_SGD>(s, chunks, nchunks, p, g, m, v, e, a, fin);
    else if (kind == OPT_ADAMW) launch_opt<OPT_ADAMW>(s, chunks, nchunks, p, g, m, v, e, a, fin);
    else launch_opt<OPT_ADAM>(s, chunks, nchunks, p, g, m, v, e, a, fin);
}

}  // namespace dnnca
