// kernels_sens.hip -- the kernels only the input-sensitivity pass needs (Model::input_sensitivity, model.hip):
//   k_sens_head     seed + head data gradient: d sum(sigmoid(logits)) / d feat = p (1 - p) w[c]
//   k_bn_infer_bwd  BatchNorm backward in inference mode: a per-channel scale by gamma / sqrt(moving_variance + eps)
//   k_sens_first    data gradient of the convs that read the network input, never stored: |dx| summed over the image per (b, channel)
// Everything else of the pass is a data-gradient launch the train step already has (kernels_generic.hip, kernels_igemm.hip).
#include "sens_first_dev.h"

namespace dnnca {

static constexpr int TB = 256;

static inline unsigned nblk(size_t n, int per = TB) { return (unsigned)((n + per - 1) / per); }

// ------------------------------------------------------------------------------------------------ seed + head
__global__ void k_sens_head(size_t npix, const float* __restrict__ logits, const float* __restrict__ w, View dfeat, int acc) {
    const int C = dfeat.C;
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= npix * C) return;
    const int c = (int)(i % C);
    const size_t p = i / C;
    const float e = expf(-fabsf(logits[p]));          // sigmoid'(x) = e / (1 + e)^2 with e = exp(-|x|), either sign
    const float d = e / ((1.0f + e) * (1.0f + e)) * w[c];
    float* o = dfeat.p + p * dfeat.ps + c;
    *o = acc ? *o + d : d;
}

void g_sens_head(hipStream_t s, int B, int H, int W, const float* logits, const float* w, View dfeat, int acc) {
    const size_t npix = (size_t)B * H * W;
    hipLaunchKernelGGL(k_sens_head, dim3(nblk(npix * dfeat.C)), dim3(TB), 0, s, npix, logits, w, dfeat, acc);
}

// ------------------------------------------------------------------------------------------------ BatchNorm, inference mode
// y = gamma (x - moving_mean) / sqrt(moving_variance + eps) + beta  =>  dx = dy gamma / sqrt(moving_variance + eps): the scale
// g_bn_finalize writes for training = 0, formed the same way
__global__ void k_bn_infer_bwd(size_t npix, View dy, View dx, int acc, const float* __restrict__ gamma, const float* __restrict__ mvar,
                               float eps) {
    const int C = dy.C;
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= npix * C) return;
    const int c = (int)(i % C);
    const size_t p = i / C;
    const float sc = gamma[c] * (1.0f / sqrtf(mvar[c] + eps));
    const float d = dy.p[p * dy.ps + c] * sc;
    float* o = dx.p + p * dx.ps + c;
    *o = acc ? *o + d : d;
}

void g_bn_infer_bwd(hipStream_t s, int B, View dy, View dx, int acc, const float* gamma, const float* mvar, float eps) {
    const size_t npix = (size_t)B * dy.H * dy.W;
    hipLaunchKernelGGL(k_bn_infer_bwd, dim3(nblk(npix * dy.C)), dim3(TB), 0, s, npix, dy, dx, acc, gamma, mvar, eps);
}

// ------------------------------------------------------------------------------------------------ first layer
// One block = `tpb` consecutive 16 x 16 tiles (row-major tile order) of image b for the input channels [ci0, ci0 + nci) of first conv
// blockIdx.z.  Per tile thread (ly, lx) gets its pixel's dx in registers (sens_first_tile, sens_first_dev.h: shared with
// k_attr_first), adds |dx| to its running sums and drops dx.  End of the block: the lane sums go through a wave reduction (__shfl_down)
// and a fixed-order sum of the waves to ONE double per channel, stored in the block's slot of the partial row of (b, channel).  The
// block that draws the last ticket of its (b, z) pair adds the row up in a fixed order, so two runs give the same bits whatever order
// the blocks finish in.  The partials travel as device-scope atomic stores / loads with the storing thread's vmcnt(0) wait in front
// of its ticket (the ordering argument of bn_dev.h; no device-scope fence).
__device__ __forceinline__ double sens_block_sum(double v, double* red) {
    // all threads of the block call it; result valid in thread 0.  Fixed order: lanes by shuffle tree, waves 0, 1, 2, 3
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double a = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < TB / 64; ++k) a += red[k];
    return a;
}

__global__ __launch_bounds__(TB) void k_sens_first(const SensFirst* __restrict__ descs, int H, int W, int K, int tiles_x, int ntiles, int tpb,
                                                   int c_total, double* part, unsigned* ticket, double* __restrict__ sums) {
    extern __shared__ float lds[];
    __shared__ double red[TB / 64];
    __shared__ unsigned is_last;
    const SensFirst d = descs[blockIdx.z];
    const int b = blockIdx.y, tid = threadIdx.x, lx = tid % kSensTile, ly = tid / kSensTile;
    const unsigned nblk_pair = gridDim.x;
    float tsum[kSensCi];
#pragma unroll
    for (int j = 0; j < kSensCi; ++j) tsum[j] = 0.f;
    const int t_end = min(ntiles, ((int)blockIdx.x + 1) * tpb);
    for (int t = (int)blockIdx.x * tpb; t < t_end; ++t) {
        const int ty0 = (t / tiles_x) * kSensTile, tx0 = (t % tiles_x) * kSensTile;
        float acc[kSensCi];
        sens_first_tile<TB>(d, b, H, W, K, ty0, tx0, lds, acc);
        if (ty0 + ly < H && tx0 + lx < W) {
#pragma unroll
            for (int j = 0; j < kSensCi; ++j) tsum[j] += fabsf(acc[j]);
        }
    }
    // block partials -> the block's slot of each channel's partial row
    const unsigned pair = (unsigned)b * gridDim.z + blockIdx.z;
#pragma unroll
    for (int j = 0; j < kSensCi; ++j) {
        const double a = sens_block_sum((double)tsum[j], red);
        if (tid == 0 && j < d.nci)
            __hip_atomic_store(part + ((size_t)b * c_total + d.chan + j) * nblk_pair + blockIdx.x, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid == 0) {
        __builtin_amdgcn_s_waitcnt(0x0070);            // vmcnt(0) lgkmcnt(0): this thread's partials have been performed
        unsigned last = 0u;
        if (__hip_atomic_fetch_add(ticket + pair, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nblk_pair - 1) {
            ticket[pair] = 0u;                         // left zeroed for the next launch
            last = 1u;
        }
        is_last = last;
    }
    __syncthreads();
    if (!is_last) return;
    for (int j = 0; j < d.nci; ++j) {
        const double* row = part + ((size_t)b * c_total + d.chan + j) * nblk_pair;
        double a = 0.0;
        for (unsigned k = tid; k < nblk_pair; k += TB) a += __hip_atomic_load(row + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a = sens_block_sum(a, red);
        if (tid == 0) sums[(size_t)b * c_total + d.chan + j] = a;
    }
}

size_t sens_first_lds(int K) {
    const int TH = kSensTile + K - 1, plane = (TH * TH) | 1;
    return ((size_t)kSensCo * plane + (size_t)K * K * kSensCi * kSensCo) * sizeof(float);
}

SensFirstGrid sens_first_grid(int B, int H, int W, int nz) {
    SensFirstGrid g;
    g.tiles_x = (W + kSensTile - 1) / kSensTile;
    g.ntiles = g.tiles_x * ((H + kSensTile - 1) / kSensTile);
    // about 2048 blocks in all: enough for every CU, few enough that a ticket counter meets a few dozen blocks
    const long total = (long)g.ntiles * B * nz;
    g.tpb = (int)((total + 2047) / 2048);
    if (g.tpb < 1) g.tpb = 1;
    g.nblk = (g.ntiles + g.tpb - 1) / g.tpb;
    return g;
}

void g_sens_first(hipStream_t s, const SensFirst* descs_dev, int nz, int B, int H, int W, int K, int c_total, const SensFirstGrid& g,
                  double* part, unsigned* ticket, double* sums) {
    hipLaunchKernelGGL(k_sens_first, dim3((unsigned)g.nblk, (unsigned)B, (unsigned)nz), dim3(TB), sens_first_lds(K), s, descs_dev, H, W, K,
                       g.tiles_x, g.ntiles, g.tpb, c_total, part, ticket, sums);
}

}  // namespace dnnca
