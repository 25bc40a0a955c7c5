// kernels_tta.hip -- test-time augmentation: the eight flip / transpose views of a slice (the dihedral group of the square) and the
// mean of the probabilities the network gives for them, mapped back to the original pixels.
//   view k = 4 t + 2 v + h:  xf[b,i,j,c] = x[b, v ? H-1-i : i, h ? W-1-j : j, c];  with t: xk[b,i,j,c] = xf[b,j,i,c]  (H == W)
// tta_moments (at the end of the file) is tta_accumulate's sibling that also carries the running state of the views' spread.
// The kernels stream a few MB beside forwards of 100 us and more: dword accesses, no atomics, every output element has one writer
// (bit-identical from run to run).  Non-transposed views: a wave reads one contiguous run of a row and writes the mirrored run.
// Transposed views: a 32 x 32 pixel tile goes through LDS, so that the global reads run along source rows and the global writes
// along output rows; the LDS row pitch is 33 pixels (33 * cc dwords for cc channels), which makes the column reads of 32 consecutive
// lanes land on 32 consecutive banks (bank = (jj * 33 cc + ii cc + c) mod 32 = (jj cc + c + const) mod 32).
#include "kernels.h"

namespace dnnca {

static constexpr int TTA_TB = 256;      // threads per block
static constexpr int TTA_T = 32;        // tile side in pixels
static constexpr int TTA_CC = 8;        // channels staged per pass of the transposed gather (more channels: several passes)

// ---------------------------------------------------------------------------------------------------------------- tta_view_in
// grid (ceil(W C / TTA_TB), H, B): one thread per float of an output row
__global__ void k_tta_flip_in(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int C, int v, int h) {
    const int e = blockIdx.x * TTA_TB + threadIdx.x;
    if (e >= W * C) return;
    const int i = blockIdx.y, b = blockIdx.z;
    const int j = e / C, c = e - j * C;
    const int si = v ? H - 1 - i : i, sj = h ? W - 1 - j : j;
    dst[((size_t)b * H + i) * W * C + e] = src[(((size_t)b * H + si) * W + sj) * C + c];
}

// grid (tiles along j, tiles along i, B); N = H = W.  dst[b,i,j,c] = src[b, v ? N-1-j : j, h ? N-1-i : i, c]
__global__ void __launch_bounds__(TTA_TB) k_tta_tr_in(const float* __restrict__ src, float* __restrict__ dst, int N, int C, int v, int h) {
    __shared__ float t[TTA_T * (TTA_T + 1) * TTA_CC];
    const int j0 = blockIdx.x * TTA_T, i0 = blockIdx.y * TTA_T, b = blockIdx.z;
    const int ti = min(TTA_T, N - i0), tj = min(TTA_T, N - j0);      // partial tiles at the right and bottom edges
    const size_t img = (size_t)b * N * N;
    for (int c0 = 0; c0 < C; c0 += TTA_CC) {
        const int cc = min(TTA_CC, C - c0), P = (TTA_T + 1) * cc;
        // source row jj of the tile: ti pixels of cc channels, read along the row (mirrored per pixel with h)
        const int run_in = ti * cc;
        for (int idx = threadIdx.x; idx < tj * run_in; idx += TTA_TB) {
            const int jj = idx / run_in, e = idx - jj * run_in, ii = e / cc, c = e - ii * cc;
            const int sr = v ? N - 1 - (j0 + jj) : j0 + jj, sc = h ? N - 1 - (i0 + ii) : i0 + ii;
            t[jj * P + e] = src[(img + (size_t)sr * N + sc) * C + c0 + c];
        }
        __syncthreads();
        // output row ii of the tile: tj pixels of cc channels, written along the row; the LDS read walks a column
        const int run_out = tj * cc;
        for (int idx = threadIdx.x; idx < ti * run_out; idx += TTA_TB) {
            const int ii = idx / run_out, e = idx - ii * run_out, jj = e / cc, c = e - jj * cc;
            dst[(img + (size_t)(i0 + ii) * N + j0 + jj) * C + c0 + c] = t[jj * P + ii * cc + c];
        }
        __syncthreads();
    }
}

void g_tta_view_in(hipStream_t s, const float* src, float* dst, int B, int H, int W, int C, int k) {
    const int h = k & 1, v = (k >> 1) & 1;
    if (k & 4)
        hipLaunchKernelGGL(k_tta_tr_in, dim3((W + TTA_T - 1) / TTA_T, (H + TTA_T - 1) / TTA_T, B), dim3(TTA_TB), 0, s, src, dst, H, C, v, h);
    else
        hipLaunchKernelGGL(k_tta_flip_in, dim3((W * C + TTA_TB - 1) / TTA_TB, H, B), dim3(TTA_TB), 0, s, src, dst, H, W, C, v, h);
}

// ------------------------------------------------------------------------------------------------------------- tta_accumulate
// the value of one view at one original pixel joins that pixel's sum: the first view writes, later ones add in place, the last one
// also divides (fp32 sum in the order of the launches, fp32 division)
template <bool IS_LOGITS>
DEVINL void tta_join(float* __restrict__ prob, size_t o, float p, int first, int last, float n) {
    if (IS_LOGITS) p = sigmoid_of_logit(p);
    if (!first) p = prob[o] + p;
    prob[o] = last ? p / n : p;
}

// grid (ceil(W / TTA_TB), H, B): one thread per output pixel, the source run mirrored
template <bool IS_LOGITS>
__global__ void k_tta_acc_flip(const float* __restrict__ src, float* __restrict__ prob, int H, int W, int v, int h, int first, int last,
                               float n) {
    const int j = blockIdx.x * TTA_TB + threadIdx.x;
    if (j >= W) return;
    const int i = blockIdx.y, b = blockIdx.z;
    const int si = v ? H - 1 - i : i, sj = h ? W - 1 - j : j;
    tta_join<IS_LOGITS>(prob, ((size_t)b * H + i) * W + j, src[((size_t)b * H + si) * W + sj], first, last, n);
}

// grid (tiles along j, tiles along i, B); N = H = W.  Original pixel (i, j) reads the view's plane at (h ? N-1-j : j, v ? N-1-i : i)
template <bool IS_LOGITS>
__global__ void __launch_bounds__(TTA_TB) k_tta_acc_tr(const float* __restrict__ src, float* __restrict__ prob, int N, int v, int h,
                                                       int first, int last, float n) {
    __shared__ float t[TTA_T * (TTA_T + 1)];
    const int j0 = blockIdx.x * TTA_T, i0 = blockIdx.y * TTA_T, b = blockIdx.z;
    const int ti = min(TTA_T, N - i0), tj = min(TTA_T, N - j0);
    const size_t img = (size_t)b * N * N;
    for (int idx = threadIdx.x; idx < tj * ti; idx += TTA_TB) {          // along the source rows
        const int jj = idx / ti, ii = idx - jj * ti;
        const int sr = h ? N - 1 - (j0 + jj) : j0 + jj, sc = v ? N - 1 - (i0 + ii) : i0 + ii;
        t[jj * (TTA_T + 1) + ii] = src[img + (size_t)sr * N + sc];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < ti * tj; idx += TTA_TB) {          // along the output rows
        const int ii = idx / tj, jj = idx - ii * tj;
        tta_join<IS_LOGITS>(prob, img + (size_t)(i0 + ii) * N + j0 + jj, t[jj * (TTA_T + 1) + ii], first, last, n);
    }
}

template <bool IS_LOGITS>
static void tta_accumulate(hipStream_t s, const float* src, float* prob, int B, int H, int W, int k, bool first, bool last, int n) {
    const int h = k & 1, v = (k >> 1) & 1;
    if (k & 4)
        hipLaunchKernelGGL(k_tta_acc_tr<IS_LOGITS>, dim3((W + TTA_T - 1) / TTA_T, (H + TTA_T - 1) / TTA_T, B), dim3(TTA_TB), 0, s, src, prob,
                           H, v, h, (int)first, (int)last, (float)n);
    else
        hipLaunchKernelGGL(k_tta_acc_flip<IS_LOGITS>, dim3((W + TTA_TB - 1) / TTA_TB, H, B), dim3(TTA_TB), 0, s, src, prob, H, W, v, h,
                           (int)first, (int)last, (float)n);
}

void g_tta_accumulate(hipStream_t s, const float* src, float* prob, int B, int H, int W, int k, bool is_logits, bool first, bool last,
                      int n) {
    if (is_logits) tta_accumulate<true>(s, src, prob, B, H, W, k, first, last, n);
    else tta_accumulate<false>(s, src, prob, B, H, W, k, first, last, n);
}

// ---------------------------------------------------------------------------------------------------------------- tta_moments
// tta_accumulate plus the running state of the views' spread (their population standard deviation).  Shifted form: with p0 the first
// view's value at the pixel and d_k = p_k - p0,  var = (sum d^2 - (sum d)^2 / n) / n  -- the differences are small where the views
// agree, so nothing cancels as it does in E[p^2] - E[p]^2, and equal views give d = 0 and an exact 0.  mom: three planes of `plane`
// floats (p0, sum d, sum d^2); view 0 writes p0 alone, view 1 writes the sums, later views add to them, the last view writes neither
// but the mean (the operations of tta_join, in its order) and the spread.  Every product and sum is rounded on its own: the pragma
// sits inside the function body, so nothing else in this file inherits it.
template <bool IS_LOGITS>
DEVINL void tta_moments_join(float* __restrict__ prob, float* __restrict__ mom, float* __restrict__ spread, size_t plane, size_t o, float p,
                             int pos, int last, float n) {
#pragma clang fp contract(off)
    if (IS_LOGITS) p = sigmoid_of_logit(p);
    float sd = 0.f, sq = 0.f;
    if (pos == 0) {
        if (!last) mom[o] = p;
    } else {
        const float d = p - mom[o];
        sd = d;
        sq = d * d;
        if (pos > 1) {
            sd = mom[plane + o] + sd;
            sq = mom[2 * plane + o] + sq;
        }
        if (!last) {
            mom[plane + o] = sd;
            mom[2 * plane + o] = sq;
        }
    }
    if (pos) p = prob[o] + p;
    prob[o] = last ? p / n : p;
    if (last) {
        const float var = (sq - (sd * sd) / n) / n;
        spread[o] = var > 0.f ? sqrtf(var) : 0.f;
    }
}

// grid (ceil(W / TTA_TB), H, B): one thread per output pixel, the source run mirrored
template <bool IS_LOGITS>
__global__ void k_tta_mom_flip(const float* __restrict__ src, float* __restrict__ prob, float* __restrict__ mom, float* __restrict__ spread,
                               size_t plane, int H, int W, int v, int h, int pos, int last, float n) {
    const int j = blockIdx.x * TTA_TB + threadIdx.x;
    if (j >= W) return;
    const int i = blockIdx.y, b = blockIdx.z;
    const int si = v ? H - 1 - i : i, sj = h ? W - 1 - j : j;
    tta_moments_join<IS_LOGITS>(prob, mom, spread, plane, ((size_t)b * H + i) * W + j, src[((size_t)b * H + si) * W + sj], pos, last, n);
}

// grid (tiles along j, tiles along i, B); N = H = W.  The tile of k_tta_acc_tr: 32 x 32 pixels, pitch 33
template <bool IS_LOGITS>
__global__ void __launch_bounds__(TTA_TB) k_tta_mom_tr(const float* __restrict__ src, float* __restrict__ prob, float* __restrict__ mom,
                                                       float* __restrict__ spread, size_t plane, int N, int v, int h, int pos, int last,
                                                       float n) {
    __shared__ float t[TTA_T * (TTA_T + 1)];
    const int j0 = blockIdx.x * TTA_T, i0 = blockIdx.y * TTA_T, b = blockIdx.z;
    const int ti = min(TTA_T, N - i0), tj = min(TTA_T, N - j0);
    const size_t img = (size_t)b * N * N;
    for (int idx = threadIdx.x; idx < tj * ti; idx += TTA_TB) {          // along the source rows
        const int jj = idx / ti, ii = idx - jj * ti;
        const int sr = h ? N - 1 - (j0 + jj) : j0 + jj, sc = v ? N - 1 - (i0 + ii) : i0 + ii;
        t[jj * (TTA_T + 1) + ii] = src[img + (size_t)sr * N + sc];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < ti * tj; idx += TTA_TB) {          // along the output rows
        const int ii = idx / tj, jj = idx - ii * tj;
        tta_moments_join<IS_LOGITS>(prob, mom, spread, plane, img + (size_t)(i0 + ii) * N + j0 + jj, t[jj * (TTA_T + 1) + ii], pos, last, n);
    }
}

template <bool IS_LOGITS>
static void tta_moments(hipStream_t s, const float* src, float* prob, float* mom, float* spread, size_t plane, int B, int H, int W, int k,
                        int pos, int n) {
    const int h = k & 1, v = (k >> 1) & 1, last = pos == n - 1;
    if (k & 4)
        hipLaunchKernelGGL(k_tta_mom_tr<IS_LOGITS>, dim3((W + TTA_T - 1) / TTA_T, (H + TTA_T - 1) / TTA_T, B), dim3(TTA_TB), 0, s, src, prob,
                           mom, spread, plane, H, v, h, pos, last, (float)n);
    else
        hipLaunchKernelGGL(k_tta_mom_flip<IS_LOGITS>, dim3((W + TTA_TB - 1) / TTA_TB, H, B), dim3(TTA_TB), 0, s, src, prob, mom, spread,
                           plane, H, W, v, h, pos, last, (float)n);
}

void g_tta_moments(hipStream_t s, const float* src, float* prob, float* mom, float* spread, size_t plane, int B, int H, int W, int k,
                   bool is_logits, int pos, int n) {
    if (is_logits) tta_moments<true>(s, src, prob, mom, spread, plane, B, H, W, k, pos, n);
    else tta_moments<false>(s, src, prob, mom, spread, plane, B, H, W, k, pos, n);
}

}  // namespace dnnca
