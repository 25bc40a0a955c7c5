// kernels_refine.hip -- mask refinement (dnnca_model_set_lesion_refine): the prediction plane's mask of one chunk of the lesion
// tables and the boundary distances, between its threshold and the numbering of its components.  Bit 0 of a pixel's word is its
// mask throughout (bit 1: the high-threshold plane of the hysteresis, straight after region_prep only).
//   region_prep          (kernels_region.hip) with T = 2: bit 0 = prob' >= low, bit 1 = prob' >= threshold, one read of the plane
//   region_ccl_*         (kernels_region.hip) label bit 0
//   region_hyst_seed     a pixel with bit 1 flags its root: every writer stores 1, no order dependence
//   region_hyst_keep     word = its root is flagged
//   region_open          (kernels_region.hip) the opening, unchanged
//   region_close         dilation then erosion over the (2 c + 1)^2 window, out-of-plane pixels ignored in both: the dual of
//                        region_open, the same 32 x 32 LDS tile with a halo of 2 c, row and column passes
//   region_complement    word = !mask, which region_ccl_* label: the 4-connected components of the background, per slice
//   region_hole_border   a background pixel in the first or last row or column of its slice flags its root (stores 1)
//   region_hole_fill     word = mask | (background && root not flagged)
// Labels and flags live in the parents and sizes planes of the chunk, which lesion_plane writes only after the stage.  A root is a
// pixel index of the chunk (ccl_dev.h), so the flags need no table; the tile / merge kernels never unite across a slice's edge.
#include "refine.h"

namespace dnnca {

namespace {

constexpr int RB = 256;
constexpr int kTile = 32;
constexpr int kCloseE = kTile + 2 * (kRefineMaxClose - 1);      // closing: input tile edge with the halo of dilation + erosion

inline unsigned nblocks(size_t n) { return (unsigned)((n + RB - 1) / RB); }

__global__ __launch_bounds__(RB) void k_region_hyst_seed(const uint32_t* __restrict__ words, const int* __restrict__ L, size_t n,
                                                         unsigned* __restrict__ flag) {
    const size_t q = (size_t)blockIdx.x * RB + threadIdx.x;
    if (q >= n) return;
    const int r = L[q];
    if ((words[q] & 2u) && r >= 0) flag[r] = 1u;
}

__global__ __launch_bounds__(RB) void k_region_hyst_keep(const int* __restrict__ L, const unsigned* __restrict__ flag, size_t n,
                                                         uint32_t* __restrict__ out) {
    const size_t q = (size_t)blockIdx.x * RB + threadIdx.x;
    if (q >= n) return;
    const int r = L[q];
    out[q] = (r >= 0 && flag[r]) ? 1u : 0u;
}

// closing of kTile x kTile output pixels of one word plane: dilation (OR; out-of-plane input = 0, i.e. ignored), then erosion
// (AND; out-of-plane dilated pixels = all ones, i.e. ignored), each as a row pass and a column pass in LDS.  The window of pixel
// y is [y - c, y + c] for both, k = 2 c + 1.
__global__ __launch_bounds__(RB) void k_region_close(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int H, int W, int k) {
    __shared__ uint32_t A[kCloseE * kCloseE], Bf[kCloseE * kCloseE];
    const int c = (k - 1) / 2;
    const int E = kTile + 2 * (k - 1), E2 = kTile + k - 1;
    const size_t base = (size_t)blockIdx.z * H * W;
    const int y0 = blockIdx.y * kTile, x0 = blockIdx.x * kTile;
    const int ey0 = y0 - 2 * c, ex0 = x0 - 2 * c;
    for (int i = threadIdx.x; i < E * E; i += RB) {
        const int r = i / E, cc = i - r * E, gy = ey0 + r, gx = ex0 + cc;
        A[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? in[base + (size_t)gy * W + gx] : 0u;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < E * E2; i += RB) {           // dilation, rows: Bf[E][E2]
        const int r = i / E2, cc = i - r * E2;
        uint32_t v = 0u;
        for (int d = 0; d < k; ++d) v |= A[r * E + cc + d];
        Bf[r * E2 + cc] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < E2 * E2; i += RB) {          // dilation, columns: A[E2][E2]; dilated pixels outside the slice -> ones
        const int r = i / E2, cc = i - r * E2, gy = y0 - c + r, gx = x0 - c + cc;
        uint32_t v = 0u;
        for (int d = 0; d < k; ++d) v |= Bf[(r + d) * E2 + cc];
        A[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? v : ~0u;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < E2 * kTile; i += RB) {       // erosion, rows: Bf[E2][kTile]
        const int r = i / kTile, cc = i - r * kTile;
        uint32_t v = ~0u;
        for (int d = 0; d < k; ++d) v &= A[r * E2 + cc + d];
        Bf[r * kTile + cc] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTile * kTile; i += RB) {    // erosion, columns -> out
        const int r = i / kTile, cc = i - r * kTile, gy = y0 + r, gx = x0 + cc;
        if (gy >= H || gx >= W) continue;
        uint32_t v = ~0u;
        for (int d = 0; d < k; ++d) v &= Bf[(r + d) * kTile + cc];
        out[base + (size_t)gy * W + gx] = v;
    }
}

__global__ __launch_bounds__(RB) void k_region_complement(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out) {
    const size_t q = (size_t)blockIdx.x * RB + threadIdx.x;
    if (q >= n) return;
    out[q] = ~in[q] & 1u;
}

// thread i of slice blockIdx.y looks at one pixel of the slice's outer border: the first row, the last row, the first column,
// the last column (corners twice: the stores are idempotent)
__global__ __launch_bounds__(RB) void k_region_hole_border(const int* __restrict__ L, int H, int W, unsigned* __restrict__ flag) {
    const int i = blockIdx.x * RB + threadIdx.x;
    if (i >= 2 * (H + W)) return;
    int y, x;
    if (i < W) y = 0, x = i;
    else if (i < 2 * W) y = H - 1, x = i - W;
    else if (i < 2 * W + H) y = i - 2 * W, x = 0;
    else y = i - 2 * W - H, x = W - 1;
    const int r = L[(size_t)blockIdx.y * H * W + (size_t)y * W + x];
    if (r >= 0) flag[r] = 1u;
}

__global__ __launch_bounds__(RB) void k_region_hole_fill(const uint32_t* __restrict__ fg, const int* __restrict__ L,
                                                         const unsigned* __restrict__ flag, size_t n, uint32_t* __restrict__ out) {
    const size_t q = (size_t)blockIdx.x * RB + threadIdx.x;
    if (q >= n) return;
    const int r = L[q];
    out[q] = (fg[q] & 1u) | ((r >= 0 && !flag[r]) ? 1u : 0u);
}

}  // namespace

const char* refine_invalid(const dnnca_lesion_refine& c) {
    if (c.hysteresis_low != 0.f && !(c.hysteresis_low > 0.f && c.hysteresis_low < 1.f)) return "hysteresis_low outside (0, 1)";
    if (c.closing_size < 0) return "closing_size is negative";
    if (c.closing_size > kRefineMaxClose) return "closing_size above 15";
    if (c.closing_size > 1 && c.closing_size % 2 == 0) return "closing_size is even (its window is asymmetric)";
    if (c.fill_holes != 0 && c.fill_holes != 1) return "fill_holes is neither 0 nor 1";
    return nullptr;
}

int refine_chunk(Model* M, const dnnca_lesion_refine& cfg, const float* src, const Resize& rz, int nb, const float* thr_host, int k,
                 const RefineWs& ws, const uint32_t** fg) {
    hipStream_t s = M->stream;
    const int oh = rz.out_h, ow = rz.out_w;
    const size_t hw = (size_t)oh * ow, n = (size_t)nb * hw;
    const bool hyst = cfg.hysteresis_low != 0.f;
    uint32_t *cur = ws.w0, *other = ws.w1;
    if (!M->dry) HIP_TRY(hipMemcpyAsync(ws.thr, hyst ? thr_host : thr_host + 1, hyst ? 8 : 4, hipMemcpyHostToDevice, s));
    region_prep_launch(M, src, rz, nb, ws.thr, hyst ? 2 : 1, cur);
    if (hyst) {
        region_ccl(M, cur, 1, nb, oh, ow, ws.lab);
        if (!M->dry) HIP_TRY(hipMemsetAsync(ws.flag, 0, n * 4, s));
        LAUNCH(M, "region_hyst_seed", n * 8.0, 0,
               hipLaunchKernelGGL(k_region_hyst_seed, dim3(nblocks(n)), dim3(RB), 0, s, (const uint32_t*)cur, (const int*)ws.lab, n, ws.flag));
        LAUNCH(M, "region_hyst_keep", n * 12.0, 0,
               hipLaunchKernelGGL(k_region_hyst_keep, dim3(nblocks(n)), dim3(RB), 0, s, (const int*)ws.lab, (const unsigned*)ws.flag, n, other));
        std::swap(cur, other);
    }
    const dim3 tiles((ow + kTile - 1) / kTile, (oh + kTile - 1) / kTile, nb);
    if (k > 1) {
        region_open_launch(M, cur, other, oh, ow, k, nb);
        std::swap(cur, other);
    }
    if (cfg.closing_size > 1) {
        LAUNCH(M, "region_close", n * 8.0, 0,
               hipLaunchKernelGGL(k_region_close, tiles, dim3(RB), 0, s, (const uint32_t*)cur, other, oh, ow, cfg.closing_size));
        std::swap(cur, other);
    }
    if (cfg.fill_holes) {
        LAUNCH(M, "region_complement", n * 8.0, 0,
               hipLaunchKernelGGL(k_region_complement, dim3(nblocks(n)), dim3(RB), 0, s, (const uint32_t*)cur, n, other));
        region_ccl(M, other, 1, nb, oh, ow, ws.lab);
        if (!M->dry) HIP_TRY(hipMemsetAsync(ws.flag, 0, n * 4, s));
        LAUNCH(M, "region_hole_border", (double)nb * 2 * (oh + ow) * 8.0, 0,
               hipLaunchKernelGGL(k_region_hole_border, dim3(nblocks((size_t)2 * (oh + ow)), nb), dim3(RB), 0, s, (const int*)ws.lab, oh, ow,
                                  ws.flag));
        // `other` held the complement, which only the labelling read: the filled mask takes its place
        LAUNCH(M, "region_hole_fill", n * 16.0, 0,
               hipLaunchKernelGGL(k_region_hole_fill, dim3(nblocks(n)), dim3(RB), 0, s, (const uint32_t*)cur, (const int*)ws.lab,
                                  (const unsigned*)ws.flag, n, other));
        std::swap(cur, other);
    }
    *fg = cur;
    return DNNCA_OK;
}

}  // namespace dnnca
