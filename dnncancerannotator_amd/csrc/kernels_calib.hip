// kernels_calib.hip -- can the probability be believed?  The reliability table of a probability plane against its labels, the
// negative log-likelihood of the plane at a set of temperatures, and the temperature scaling of the plane itself
// (dnnca_calibration, dnnca_prob_temperature; `evaluate --calibration`, `--temperature`).
//
// Shared by the kernels and by tests/calib_oracle.py:
//   class  1 when y > 0.5f, else 0 (the label rule of spread_outcome)
//   clamp  p' = fminf(fmaxf(p, 0), 1): a NaN becomes 0
//   q24    q = (uint64) rintf(p' * 2^24)
//   bin    k = min(n_bins - 1, (int) floorf(p' * (float) n_bins)): one float32 product
//   logit  z = log(pc) - log1p(-pc) in double, pc = (double) p' clamped to [2^-24, 1 - 2^-24]: an exact 0 or 1 is -+16.64
//   nll    at temperature T: a = z * (1 / (double) T); class 1 adds softplus(-a), class 0 softplus(a);
//          softplus(a) = max(a, 0) + log1p(exp(-|a|))
//
//   calib_bins        per slice, bin and class the pixels and the sum of q; per slice and class the sum of q^2 as two words
//                     (sum of the low 32 bits, sum of the bits above: one uint64 overflows at 512 x 512).  Integers only: bit-identical
//                     from run to run.  The histogram of a block lives in LDS and only its non-zero entries go to HBM
//   calib_nll         per slice, block and temperature the block's sum in double, into a scratch row of its own: no float atomics
//   calib_nll_sum     adds the rows in ascending block order: bit-identical from run to run
//   prob_temperature  p -> (float) (1 / (1 + exp(-z / T))), in double, rounded once; in place or from one buffer to another
#include <algorithm>

#include "calib.h"
#include "kernels.h"

namespace dnnca {

namespace {

constexpr int CB = 256;                  // threads per block
constexpr int kBinsU = 16;               // calib_bins: runs of CB pixels per block (as spread_outcome's kOutcomeU)
constexpr int kCountShift = 40;          // calib_bins: an LDS entry is pixels << 40 | sum of q (a block adds at most 2^12 pixels, 2^36)

DEVINL float clamp01(float p) { return fminf(fmaxf(p, 0.f), 1.f); }

DEVINL double logit_of(float p01) {
    const double pc = fmin(fmax((double)p01, 0x1p-24), 1.0 - 0x1p-24);
    return log(pc) - log1p(-pc);
}

DEVINL double softplus(double a) { return fmax(a, 0.0) + log1p(exp(-fabs(a))); }

DEVINL unsigned long long wave_sum_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the same tree in every run: lane l ends with the sum in the order the butterfly fixes
DEVINL double wave_sum_f64(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid (ceil(hw / (CB kBinsU)), slices).  A block walks kBinsU runs of CB pixels of ONE slice.  Key = 2 bin + class; a pixel is ONE
// 64-bit LDS add of (1 << 40) + q to its key's entry.  A real prediction plane puts almost every pixel of a wave on key 0, but the
// lanes are NOT grouped by key first: measured at 8 x 512 x 512 (profiles/lesion_rate.txt) the plain add takes 17 - 18 us on a
// uniform plane and 17 - 19 us on a plane with 99 % of its pixels on key 0, a fast path for a wave of one key 19 - 20 and 22 - 23 us,
// the ballot loop of lesion_spread over up to four keys 28 and 26 us -- the wave reduction of q costs more than the LDS saves.
// bins: [slices][n_bins] x (n[2], sum_q24[2]); sq: [slices] x (sq_lo[2], sq_hi[2]); both zeroed by the caller.
__global__ __launch_bounds__(CB) void k_calib_bins(const float* __restrict__ prob, const float* __restrict__ y, size_t hw, int n_bins,
                                                   unsigned long long* __restrict__ bins, unsigned long long* __restrict__ sq) {
#pragma clang fp contract(off)
    __shared__ unsigned long long hist[2 * kCalibMaxBins];
    __shared__ unsigned long long part[CB / 64][4];
    for (int i = threadIdx.x; i < 2 * n_bins; i += CB) hist[i] = 0ull;
    __syncthreads();
    const size_t base = (size_t)blockIdx.y * hw, p0 = (size_t)blockIdx.x * CB * kBinsU + threadIdx.x;
    const float fb = (float)n_bins;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long lo0 = 0, lo1 = 0, hi0 = 0, hi1 = 0;
    for (int u = 0; u < kBinsU; ++u) {
        const size_t p = p0 + (size_t)u * CB;
        if (p - threadIdx.x >= hw) break;                 // the whole run lies behind the slice: the same for every thread of the block
        if (p < hw) {
            const float pc = clamp01(prob[base + p]);
            const bool pos = y[base + p] > 0.5f;
            const unsigned long long q = (unsigned long long)rintf(pc * 16777216.f);
            const unsigned key = 2u * (unsigned)min(n_bins - 1, (int)floorf(pc * fb)) + (pos ? 1u : 0u);
            const unsigned long long q2 = q * q, lo = q2 & 0xffffffffull, hi = q2 >> 32;
            lo0 += pos ? 0ull : lo;
            lo1 += pos ? lo : 0ull;
            hi0 += pos ? 0ull : hi;
            hi1 += pos ? hi : 0ull;
            atomicAdd(&hist[key], (1ull << kCountShift) + q);
        }
    }
    const unsigned long long v[4] = {wave_sum_u64(lo0), wave_sum_u64(lo1), wave_sum_u64(hi0), wave_sum_u64(hi1)};
    if (lane == 0)
        for (int c = 0; c < 4; ++c) part[wv][c] = v[c];
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long s = 0;
        for (int w = 0; w < CB / 64; ++w) s += part[w][threadIdx.x];
        if (s) atomicAdd(sq + (size_t)blockIdx.y * 4 + threadIdx.x, s);
    }
    for (int i = threadIdx.x; i < 2 * n_bins; i += CB) {
        const unsigned long long e = hist[i], n = e >> kCountShift, sum = e & ((1ull << kCountShift) - 1);
        if (n) {
            unsigned long long* b = bins + ((size_t)blockIdx.y * n_bins + (i >> 1)) * 4 + (i & 1);
            atomicAdd(b, n);
            if (sum) atomicAdd(b + 2, sum);
        }
    }
}

// grid (blocks per slice, slices, ceil(nt / kNllChunk)).  A block walks `runs` runs of CB pixels of one slice for kNllChunk
// temperatures: a thread computes a pixel's logit once and keeps one double sum per temperature of the chunk (with eight the kernel
// takes 83 VGPRs, five waves per SIMD; all 64 at once would hold 128 for the sums alone).  inv_t: 1 / (double) T per temperature.
// part: [slices][gridDim.x][nt].  The wave's butterfly and the ascending sum over the waves are the same in every run.
constexpr int kNllChunk = 8;
__global__ __launch_bounds__(CB) void k_calib_nll(const float* __restrict__ prob, const float* __restrict__ y, size_t hw, int runs,
                                                  const double* __restrict__ inv_t, int nt, double* __restrict__ part) {
    __shared__ double wpart[CB / 64][kNllChunk];
    const int t0 = blockIdx.z * kNllChunk, tn = min(kNllChunk, nt - t0);
    double it[kNllChunk], acc[kNllChunk];
#pragma unroll
    for (int j = 0; j < kNllChunk; ++j) {
        it[j] = j < tn ? inv_t[t0 + j] : 0.0;
        acc[j] = 0.0;
    }
    const size_t base = (size_t)blockIdx.y * hw, p0 = (size_t)blockIdx.x * CB * (size_t)runs + threadIdx.x;
    for (int u = 0; u < runs; ++u) {
        const size_t p = p0 + (size_t)u * CB;
        if (p >= hw) break;
        const double z = logit_of(clamp01(prob[base + p]));
        const double zs = y[base + p] > 0.5f ? -z : z;     // class 1: softplus(-a); (-z) * inv_t is -(z * inv_t) exactly
#pragma unroll
        for (int j = 0; j < kNllChunk; ++j)
            if (j < tn) acc[j] += softplus(zs * it[j]);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < kNllChunk; ++j) {
        const double s = wave_sum_f64(acc[j]);
        if (lane == 0) wpart[wv][j] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < tn) {
        double s = wpart[0][threadIdx.x];
        for (int w = 1; w < CB / 64; ++w) s += wpart[w][threadIdx.x];
        part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * nt + t0 + threadIdx.x] = s;
    }
}

// one thread per (slice, temperature): the partial sums of the slice's blocks in ascending order
__global__ __launch_bounds__(CB) void k_calib_nll_sum(const double* __restrict__ part, int slices, int nblk, int nt,
                                                      double* __restrict__ out) {
    const int i = blockIdx.x * CB + threadIdx.x;
    if (i >= slices * nt) return;
    const int b = i / nt, t = i - b * nt;
    double s = 0.0;
#pragma unroll 16                        // the loads do not wait for the sum: sixteen of them in flight
    for (int k = 0; k < nblk; ++k) s += part[((size_t)b * nblk + k) * nt + t];
    out[i] = s;
}

// grid-stride over n pixels; dst may be src
__global__ __launch_bounds__(CB) void k_prob_temperature(const float* src, float* dst, size_t n, double t) {
    for (size_t i = (size_t)blockIdx.x * CB + threadIdx.x; i < n; i += (size_t)gridDim.x * CB) {
        const double z = logit_of(clamp01(src[i]));
        dst[i] = (float)(1.0 / (1.0 + exp(-z / t)));
    }
}

}  // namespace

void g_calib_bins(hipStream_t s, const float* prob, const float* y, int slices, size_t hw, int n_bins, unsigned long long* bins,
                  unsigned long long* sq) {
    const size_t per_block = (size_t)CB * kBinsU;
    hipLaunchKernelGGL(k_calib_bins, dim3((unsigned)((hw + per_block - 1) / per_block), slices), dim3(CB), 0, s, prob, y, hw, n_bins, bins,
                       sq);
}

void calib_nll_shape(size_t hw, int* runs, int* blocks) {
    // four runs per block (1024 pixels: 256 blocks a slice at 512 x 512); more on planes that would take more than 1024 blocks
    size_t r = 4;
    while ((hw + CB * r - 1) / (CB * r) > 1024) r *= 2;
    *runs = (int)r;
    *blocks = (int)((hw + CB * r - 1) / (CB * r));
}

void g_calib_nll(hipStream_t s, const float* prob, const float* y, int slices, size_t hw, const double* inv_t, int nt, double* part) {
    int runs = 0, blocks = 0;
    calib_nll_shape(hw, &runs, &blocks);
    hipLaunchKernelGGL(k_calib_nll, dim3(blocks, slices, (nt + kNllChunk - 1) / kNllChunk), dim3(CB), 0, s, prob, y, hw, runs, inv_t, nt,
                       part);
}

void g_calib_nll_sum(hipStream_t s, const double* part, int slices, size_t hw, int nt, double* out) {
    int runs = 0, blocks = 0;
    calib_nll_shape(hw, &runs, &blocks);
    hipLaunchKernelGGL(k_calib_nll_sum, dim3((slices * nt + CB - 1) / CB), dim3(CB), 0, s, part, slices, blocks, nt, out);
}

void g_prob_temperature(hipStream_t s, const float* src, float* dst, size_t n, float temperature) {
    const size_t blocks = std::min<size_t>((n + CB - 1) / CB, size_t(1) << 20);
    hipLaunchKernelGGL(k_prob_temperature, dim3((unsigned)blocks), dim3(CB), 0, s, src, dst, n, (double)temperature);
}

// workspace: the bin table, the squares (both zeroed), 1 / T, the sums per slice and temperature, the block partials
int calibration(Model* M, const float* prob, const float* y, int batch, size_t hw, int n_bins, const float* temperatures, int nt,
                dnnca_calib_bin* bins, dnnca_calib_total* totals, double* nll) {
    const size_t n = (size_t)batch * hw;
    int runs = 0, blocks = 0;
    calib_nll_shape(hw, &runs, &blocks);
    auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t bins_bytes = (size_t)batch * n_bins * sizeof(dnnca_calib_bin), sq_bytes = (size_t)batch * 32;
    const size_t zero_bytes = up(bins_bytes) + up(sq_bytes), it_bytes = up((size_t)kCalibMaxTemps * 8);
    const size_t sum_bytes = up((size_t)batch * nt * 8), part_bytes = up((size_t)batch * blocks * nt * 8);
    const size_t need = zero_bytes + it_bytes + sum_bytes + part_bytes;
    if (need > M->calib_ws_bytes) {
        if (M->calib_ws) HIP_TRY(hipFree(M->calib_ws));
        M->calib_ws = nullptr;
        M->calib_ws_bytes = 0;
        HIP_TRY(hipMalloc(&M->calib_ws, need));
        M->calib_ws_bytes = need;
    }
    char* ws = (char*)M->calib_ws;
    unsigned long long* bins_dev = (unsigned long long*)ws;
    unsigned long long* sq_dev = (unsigned long long*)(ws + up(bins_bytes));
    double* it_dev = (double*)(ws + zero_bytes);
    double* sum_dev = (double*)(ws + zero_bytes + it_bytes);
    double* part_dev = (double*)(ws + zero_bytes + it_bytes + sum_bytes);
    hipStream_t s = M->stream;
    HIP_TRY(hipMemsetAsync(ws, 0, zero_bytes, s));
    LAUNCH(M, "calib_bins", 8.0 * n, 0, g_calib_bins(s, prob, y, batch, hw, n_bins, bins_dev, sq_dev));
    HIP_TRY(hipGetLastError());
    double inv_t[kCalibMaxTemps];
    if (nt) {
        for (int t = 0; t < nt; ++t) inv_t[t] = 1.0 / (double)temperatures[t];
        HIP_TRY(hipMemcpyAsync(it_dev, inv_t, (size_t)nt * 8, hipMemcpyHostToDevice, s));
        // per pixel and temperature one exp and one log1p in double beside the product and the sum; the logit once per pixel and chunk
        LAUNCH(M, "calib_nll", 8.0 * n * ((nt + 7) / 8), 60.0 * n * nt, g_calib_nll(s, prob, y, batch, hw, it_dev, nt, part_dev));
        HIP_TRY(hipGetLastError());
        LAUNCH(M, "calib_nll_sum", 8.0 * batch * blocks * nt, (double)batch * blocks * nt, g_calib_nll_sum(s, part_dev, batch, hw, nt, sum_dev));
        HIP_TRY(hipGetLastError());
    }
    std::vector<unsigned long long> sq((size_t)batch * 4);
    std::vector<double> sums((size_t)batch * nt);
    HIP_TRY(hipMemcpyAsync(bins, bins_dev, bins_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(sq.data(), sq_dev, sq_bytes, hipMemcpyDeviceToHost, s));
    if (nt) HIP_TRY(hipMemcpyAsync(sums.data(), sum_dev, (size_t)batch * nt * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));      // inv_t, sq and sums are read and written by the copies up to here
    // a slice's pixels and q sums per class are those of its bins
    for (int b = 0; b < batch; ++b) {
        dnnca_calib_total t = {};
        for (int k = 0; k < n_bins; ++k)
            for (int c = 0; c < 2; ++c) {
                t.n[c] += bins[(size_t)b * n_bins + k].n[c];
                t.sum_q24[c] += bins[(size_t)b * n_bins + k].sum_q24[c];
            }
        for (int c = 0; c < 2; ++c) t.sq_lo[c] = sq[(size_t)b * 4 + c], t.sq_hi[c] = sq[(size_t)b * 4 + 2 + c];
        totals[b] = t;
    }
    for (size_t i = 0; i < sums.size(); ++i) nll[i] = sums[i];
    return DNNCA_OK;
}

int prob_temperature(Model* M, const float* src, float* dst, size_t n, float temperature, float* out_hw) {
    LAUNCH(M, "prob_temperature", 8.0 * n, 40.0 * n, g_prob_temperature(M->stream, src, dst, n, temperature));
    HIP_TRY(hipGetLastError());
    if (out_hw) HIP_TRY(hipMemcpyAsync(out_hw, dst, n * 4, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    return DNNCA_OK;
}

}  // namespace dnnca
