// kernels_region.hip -- region-based (lesion-level) metrics of the reference (annotator/utils/metrics.py:80-510) on the device.
//
// Per batch of slices and per spec (thresholds[T], IoU threshold, resize factor, morphological filter size k):
//   region_prep     resize (tf.image.resize bilinear, half-pixel centres, no antialias; metrics.py:196-204) and threshold:
//                   label' > 0.5 -> one bit; prob' >= thresholds[t] -> bit t of the pixel's mask words (T <= 64: two words)
//   region_open     morphological opening of every prediction mask (utils/image.py:12-26: erosion2d + dilation2d, zero filter,
//                   SAME, out-of-bounds pixels ignored): AND / OR over the k x k window of the bit words, all thresholds at once;
//                   row and column passes through one LDS tile with a halo of 2 (k - 1)
//   region_ccl_*    4-connected components (tfa.image.connected_components) by union-find on int32 parents in HBM: a 32 x 32
//                   tile is labelled in LDS (ccl_tile), the pixels on tile borders unite across tiles with atomicMin (ccl_merge),
//                   every pixel then points at its root (ccl_compress).  A root is the smallest pixel index of its component:
//                   parents only ever point to smaller indices.  The label plane is labelled once per slice and resized size.
//   region_sizes    component sizes: per-root atomicAdd (a root is a pixel index: no hashing)
//   region_pairs    intersections |L_i n P_j|: a per-(slice, threshold) open-addressing table keyed by (label root, prediction
//                   root), 64-bit CAS.  Overlap pixels of two different pairs are never 4-adjacent, so a slice of HW pixels has
//                   at most ceil(HW / 2) pairs: HW + 1 slots per table keep the load below one half
//   region_match    IoU = float(I) / float(|L| + |P| - I) > theta marks both roots (idempotent stores: no order dependence)
//   region_count    roots -> tp_label / fn / tp_pred / fp: wave and block reductions, one uint64 atomicAdd per block and counter;
//                   summed over the chunk's slices (grid z = 1), or per slice (grid z = slice: the Visualizer's casewise counts)
// Every count is an integer sum, so results are bit-exact and independent of which thread wins a race.
//
// The Visualizer's composite image (utils/callbacks.py generate_image + make_summary_constructor) is rendered here too:
//   region_render   [features | label | probability] panels side by side, resized bilinear by `ratio` (the same float32 arithmetic
//                   as region_prep), * 255 truncated to uint8; the panels are read in place through an index map, four output
//                   bytes per thread and one 32-bit store
//
// The lesion table of `annotator predict` (lesion_scan / lesion_stats / lesion_mask), its links and pairs (lesion_link, lesion_match),
// the spread of the test-time-augmentation views per lesion, slice and pixel outcome (lesion_spread, spread_outcome),
// what a lesion looks like in the input channels (lesion_features, lesion_ring)
// and the boundary distances of `evaluate --surface_distances` (surface_edges / surface_cols / surface_sample) start from the same
// prep / open / ccl / sizes launches; each is described above its kernels.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <tuple>

#include "ccl_dev.h"
#include "refine.h"
#include "region.h"

namespace dnnca {

namespace {

constexpr int RB = 256;
constexpr int kTile = 32;                                  // opening and LDS-labelling tile (kTile x kTile pixels)
constexpr int kOpenE = kTile + 2 * (kRegionMaxK - 1);      // opening: input tile edge with the halo of erosion + dilation
constexpr unsigned long long kEmpty = ~0ull;

#pragma clang fp contract(off)
// tf.image.resize(method=bilinear, antialias=False) [TF-2.6 resize_bilinear_op.cc, restated]: half-pixel centres, float32,
// each product and sum rounded on its own (no FMA contraction: the >= comparisons downstream must see the oracle's values)
__device__ __forceinline__ float resize_at(const float* __restrict__ src, const Resize& r, int i, int j) {
    if (r.identity) return src[(size_t)i * r.in_w + j];
    const float fy = ((float)i + 0.5f) * r.sy - 0.5f;
    const float fx = ((float)j + 0.5f) * r.sx - 0.5f;
    const float fy0 = floorf(fy), fx0 = floorf(fx);
    const int y0 = max((int)fy0, 0), y1 = min((int)ceilf(fy), r.in_h - 1);
    const int x0 = max((int)fx0, 0), x1 = min((int)ceilf(fx), r.in_w - 1);
    const float ly = fy - fy0, lx = fx - fx0;
    const float tl = src[(size_t)y0 * r.in_w + x0], tr = src[(size_t)y0 * r.in_w + x1];
    const float bl = src[(size_t)y1 * r.in_w + x0], br = src[(size_t)y1 * r.in_w + x1];
    const float top = tl + (tr - tl) * lx;
    const float bot = bl + (br - bl) * lx;
    return top + (bot - top) * ly;
}

// label mode (T = 0): word = label' > 0.5.  Otherwise words[w][q] bit (t - 32 w) = prob' >= thr[t]
__global__ __launch_bounds__(RB) void k_region_prep(const float* __restrict__ src, Resize r, int nb, const float* __restrict__ thr,
                                                    int T, uint32_t* __restrict__ words) {
    __shared__ float sthr[kRegionMaxThr];
    if (threadIdx.x < T) sthr[threadIdx.x] = thr[threadIdx.x];
    __syncthreads();
    const size_t hw = (size_t)r.out_h * r.out_w, n = (size_t)nb * hw;
    const size_t q = (size_t)blockIdx.x * RB + threadIdx.x;
    if (q >= n) return;
    const int b = (int)(q / hw);
    const int p = (int)(q - (size_t)b * hw);
    const int i = p / r.out_w, j = p - i * r.out_w;
    const float v = resize_at(src + (size_t)b * r.in_h * r.in_w, r, i, j);
    if (T == 0) {
        words[q] = v > 0.5f ? 1u : 0u;
        return;
    }
    uint32_t lo = 0, hi = 0;
    for (int t = 0; t < T && t < 32; ++t) lo |= (v >= sthr[t] ? 1u : 0u) << t;
    for (int t = 32; t < T; ++t) hi |= (v >= sthr[t] ? 1u : 0u) << (t - 32);
    words[q] = lo;
    if (T > 32) words[n + q] = hi;
}

// opening of kTile x kTile output pixels of one word plane: erosion (AND; out-of-bounds input = all ones, i.e. ignored), then
// dilation (OR; out-of-bounds eroded pixels = 0, i.e. ignored), each as a row pass and a column pass in LDS.  TF SAME offsets:
// the window of pixel y is [y - (k - 1) / 2, y + k / 2] for both (erosion2d = -dilation2d(-x, reversed zero filter)).
__global__ __launch_bounds__(RB) void k_region_open(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int H, int W, int k,
                                                    size_t plane, int nb) {
    __shared__ uint32_t A[kOpenE * kOpenE], Bf[kOpenE * kOpenE];
    const int lo = (k - 1) / 2;
    const int E = kTile + 2 * (k - 1), E2 = kTile + k - 1;
    const int w = blockIdx.z / nb, b = blockIdx.z - w * nb;
    const size_t base = (size_t)w * plane + (size_t)b * H * W;
    const int y0 = blockIdx.y * kTile, x0 = blockIdx.x * kTile;
    const int ey0 = y0 - 2 * lo, ex0 = x0 - 2 * lo;
    for (int i = threadIdx.x; i < E * E; i += RB) {
        const int r = i / E, c = i - r * E, gy = ey0 + r, gx = ex0 + c;
        A[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? in[base + (size_t)gy * W + gx] : ~0u;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < E * E2; i += RB) {           // erosion, rows: Bf[E][E2]
        const int r = i / E2, c = i - r * E2;
        uint32_t v = ~0u;
        for (int d = 0; d < k; ++d) v &= A[r * E + c + d];
        Bf[r * E2 + c] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < E2 * E2; i += RB) {          // erosion, columns: A[E2][E2]; eroded pixels outside the slice -> 0
        const int r = i / E2, c = i - r * E2, gy = y0 - lo + r, gx = x0 - lo + c;
        uint32_t v = ~0u;
        for (int d = 0; d < k; ++d) v &= Bf[(r + d) * E2 + c];
        A[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? v : 0u;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < E2 * kTile; i += RB) {       // dilation, rows: Bf[E2][kTile]
        const int r = i / kTile, c = i - r * kTile;
        uint32_t v = 0u;
        for (int d = 0; d < k; ++d) v |= A[r * E2 + c + d];
        Bf[r * kTile + c] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTile * kTile; i += RB) {    // dilation, columns -> out
        const int r = i / kTile, c = i - r * kTile, gy = y0 + r, gx = x0 + c;
        if (gy >= H || gx >= W) continue;
        uint32_t v = 0u;
        for (int d = 0; d < k; ++d) v |= Bf[(r + d) * kTile + c];
        out[base + (size_t)gy * W + gx] = v;
    }
}

// ---- connected components.  Plane t of the mask words (bit t & 31 of word plane t >> 5) holds T x nb slices of H x W; a pixel's
// global index is g = t * n + q (n = nb * H * W, q = b * H * W + y * W + x), its parent L[g] (-1: background).
__device__ __forceinline__ bool fg_at(const uint32_t* __restrict__ words, size_t n, int t, size_t q) {
    return (words[(size_t)(t >> 5) * n + q] >> (t & 31)) & 1u;
}

// ld_agent, find_root, unite (union by atomicMin on roots) and lds_find: ccl_dev.h, shared with kernels_detect.hip

// one kTile x kTile tile of one plane labelled in LDS; L[g] = the global index of the pixel's root inside the tile (the tile's
// row-major order is the global order, so that root is the smallest global index of the tile-local component)
__global__ __launch_bounds__(RB) void k_region_ccl_tile(const uint32_t* __restrict__ words, int nb, int H, int W, int* __restrict__ L) {
    __shared__ int l[kTile * kTile];
    const int t = blockIdx.z / nb, b = blockIdx.z - t * nb;
    const size_t hw = (size_t)H * W, n = (size_t)nb * hw;
    const size_t qb = (size_t)b * hw;
    const int y0 = blockIdx.y * kTile, x0 = blockIdx.x * kTile;
    for (int i = threadIdx.x; i < kTile * kTile; i += RB) {
        const int y = y0 + i / kTile, x = x0 + (i & (kTile - 1));
        l[i] = (y < H && x < W && fg_at(words, n, t, qb + (size_t)y * W + x)) ? i : -1;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTile * kTile; i += RB) {
        if (l[i] < 0) continue;
        const int c = i & (kTile - 1);
        for (int side = 0; side < 2; ++side) {
            const int nbr = side == 0 ? (c > 0 ? i - 1 : -1) : (i >= kTile ? i - kTile : -1);
            if (nbr < 0 || l[nbr] < 0) continue;
            int a = i, bb = nbr;
            for (;;) {
                a = lds_find(l, a);
                bb = lds_find(l, bb);
                if (a == bb) break;
                if (a > bb) { const int s = a; a = bb; bb = s; }
                const int old = atomicMin(&l[bb], a);
                if (old == bb) break;
                bb = old;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTile * kTile; i += RB) {
        const int y = y0 + i / kTile, x = x0 + (i & (kTile - 1));
        if (y >= H || x >= W) continue;
        const size_t g = (size_t)t * n + qb + (size_t)y * W + x;
        int v = -1;
        if (l[i] >= 0) {
            const int r = lds_find(l, i);
            v = (int)((size_t)t * n + qb + (size_t)(y0 + r / kTile) * W + x0 + (r & (kTile - 1)));
        }
        L[g] = v;
    }
}

// pixels on a tile's left / top border unite with their neighbour across it
__global__ __launch_bounds__(RB) void k_region_ccl_merge(int* __restrict__ L, size_t total, int H, int W) {
    const size_t g = (size_t)blockIdx.x * RB + threadIdx.x;
    if (g >= total) return;
    const size_t p = g % ((size_t)H * W);
    const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
    const bool bx = x > 0 && (x & (kTile - 1)) == 0, by = y > 0 && (y & (kTile - 1)) == 0;
    if (!(bx || by) || L[g] < 0) return;
    if (bx && L[g - 1] >= 0) unite(L, (int)g, (int)(g - 1));
    if (by && L[g - W] >= 0) unite(L, (int)g, (int)(g - W));
}

__global__ __launch_bounds__(RB) void k_region_ccl_compress(int* __restrict__ L, size_t total) {
    const size_t g = (size_t)blockIdx.x * RB + threadIdx.x;
    if (g >= total) return;
    const int v = L[g];
    if (v >= 0 && v != (int)g) L[g] = find_root(L, v);
}

// lanes of a wave that carry the same key are summed into one atomic by the first of them (usually one or two keys per wave)
template <typename Fn>
__device__ __forceinline__ void wave_grouped(bool active, unsigned long long key, Fn&& fn) {
    const int lane = threadIdx.x & 63;
    unsigned long long pending = __ballot(active);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const unsigned long long k0 = __shfl(key, leader);
        const unsigned long long same = __ballot(active && key == k0);
        if (lane == leader) fn(k0, (unsigned)__popcll(same));
        if (key == k0) active = false;
        pending &= ~same;
    }
}

__global__ __launch_bounds__(RB) void k_region_sizes(const int* __restrict__ L, size_t total, unsigned* __restrict__ S) {
    const size_t g = (size_t)blockIdx.x * RB + threadIdx.x;
    const int r = g < total ? L[g] : -1;
    wave_grouped(r >= 0, (unsigned long long)(unsigned)r, [&](unsigned long long k, unsigned c) { atomicAdd(S + k, c); });
}

__device__ __forceinline__ size_t slot_hash(unsigned long long key, size_t cap) {
    key ^= key >> 33;
    key *= 0xff51afd7ed558ccdull;
    key ^= key >> 33;
    return (size_t)(key % cap);
}

// wave_grouped over several tables: lanes that carry the same (table, key) are summed into one call by the first of them
template <typename Fn>
__device__ __forceinline__ void wave_grouped_at(bool on, size_t tb, unsigned long long key, Fn&& fn) {
    const int lane = threadIdx.x & 63;
    unsigned long long pending = __ballot(on);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const unsigned long long key0 = __shfl(key, leader);
        const size_t tb0 = __shfl(tb, leader);
        const bool mine = on && key == key0 && tb == tb0;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) fn(tb0, key0, (unsigned)__popcll(same));
        if (mine) on = false;
        pending &= ~same;
    }
}

// `c` added to the count of `key` in one open-addressing table of `cap` slots (keys kEmpty, counts 0 before the first insert)
__device__ __forceinline__ void table_add(unsigned long long* kt, unsigned* ct, size_t cap, unsigned long long key, unsigned c) {
    size_t h = slot_hash(key, cap);
    for (size_t probe = 0; probe < cap; ++probe) {
        const unsigned long long old = atomicCAS(kt + h, kEmpty, key);
        if (old == kEmpty || old == key) {
            atomicAdd(ct + h, c);
            break;
        }
        h = h + 1 == cap ? 0 : h + 1;
    }
}

// overlap pixels of label root rl and prediction root rp (slice-local indices) -> table (t, b): key rl << 32 | rp, count
__global__ __launch_bounds__(RB) void k_region_pairs(const int* __restrict__ LL, const int* __restrict__ LP, int T, int nb, size_t hw,
                                                     size_t cap, unsigned long long* __restrict__ keys, unsigned* __restrict__ cnt) {
    const size_t n = (size_t)nb * hw;
    const size_t g = (size_t)blockIdx.x * RB + threadIdx.x;
    bool on = false;
    unsigned long long key = 0;
    size_t tb = 0;
    if (g < (size_t)T * n) {
        const size_t t = g / n, q = g - t * n, b = q / hw;
        const int rp = LP[g], rl = LL[q];
        // roots lie in the pixel's own plane and slice; the range check only guards the table indices against a broken label
        if (rp >= 0 && rl >= 0 && (size_t)rl - b * hw < hw && (size_t)rp - t * n - b * hw < hw) {
            on = true;
            tb = t * nb + b;
            key = ((unsigned long long)((size_t)rl - b * hw) << 32) | (unsigned long long)((size_t)rp - t * n - b * hw);
        }
    }
    wave_grouped_at(on, tb, key, [&](size_t tb0, unsigned long long key0, unsigned c) {
        table_add(keys + tb0 * cap, cnt + tb0 * cap, cap, key0, c);
    });
}

__global__ __launch_bounds__(RB) void k_region_match(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ cnt,
                                                     size_t slots, size_t cap, int nb, size_t hw, const unsigned* __restrict__ SL,
                                                     const unsigned* __restrict__ SP, float theta, uint32_t* __restrict__ ML,
                                                     unsigned char* __restrict__ MP) {
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i >= slots) return;
    const unsigned long long key = keys[i];
    if (key == kEmpty) return;
    const size_t tb = i / cap, t = tb / nb, b = tb - t * nb, n = (size_t)nb * hw;
    const size_t rl = (size_t)(key >> 32), rp = (size_t)(key & 0xffffffffu);
    if (rl >= hw || rp >= hw || t >= 64) return;
    const size_t ql = b * hw + rl, gp = t * n + b * hw + rp;
    const unsigned inter = cnt[i];
    const float iou = (float)inter / (float)(SL[ql] + SP[gp] - inter);
    if (iou > theta) {
        atomicOr(ML + (t >> 5) * n + ql, 1u << (t & 31));
        MP[gp] = 1;
    }
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid (blocks, T, Z): acc[z * acc_z + t * 4 + 0..3] += tp_label, fn, tp_pred, fp of plane t over pixels [z * per_z, (z + 1) * per_z)
// of the chunk (Z = 1, per_z = n: the whole chunk; Z = slices, per_z = H W: one slice each)
__global__ __launch_bounds__(RB) void k_region_count(const int* __restrict__ LL, const int* __restrict__ LP, const uint32_t* __restrict__ ML,
                                                     const unsigned char* __restrict__ MP, size_t n, size_t per_z, size_t acc_z,
                                                     unsigned long long* __restrict__ acc) {
    __shared__ unsigned part[RB / 64][4];
    const int t = blockIdx.y;
    unsigned c[4] = {0u, 0u, 0u, 0u};
    const size_t stride = (size_t)gridDim.x * RB;
    const size_t q1 = (size_t)(blockIdx.z + 1) * per_z;
    for (size_t q = (size_t)blockIdx.z * per_z + (size_t)blockIdx.x * RB + threadIdx.x; q < q1; q += stride) {
        if (LL[q] == (int)q) {
            const unsigned m = (ML[(size_t)(t >> 5) * n + q] >> (t & 31)) & 1u;
            c[0] += m;
            c[1] += 1u - m;
        }
        const size_t g = (size_t)t * n + q;
        if (LP[g] == (int)g) {
            const unsigned m = MP[g];
            c[2] += m;
            c[3] += 1u - m;
        }
    }
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int j = 0; j < 4; ++j) {
        const unsigned s = wave_sum(c[j]);
        if (lane == 0) part[wv][j] = s;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long s = 0;
        for (int k = 0; k < RB / 64; ++k) s += part[k][threadIdx.x];
        if (s) atomicAdd(acc + (size_t)blockIdx.z * acc_z + (size_t)t * 4 + threadIdx.x, s);
    }
}

// ---- composite image.  Composite column cc of a slice lies in panel cc / W: features 0 .. C-1, then the label (C), then the
// probability (C + 1).  Overlay (3 channels): a feature panel is grey (the feature in every channel); the label / probability
// panels are stack([label or prob, f0, f0]).  Without overlay there is one channel.
struct Composite {
    int H, W, C, Wc;                     // slices H x W with C feature channels; composite width Wc = W (C + 2)
    int oh, ow, nch;                     // resized size; channels per pixel (1, overlay 3)
    float sy, sx;                        // H / oh, Wc / ow as float (TF's CalculateResizeScale)
};

__device__ __forceinline__ float composite_at(const float* __restrict__ x, const float* __restrict__ lab, const float* __restrict__ prob,
                                              const Composite& g, size_t slice, int r, int cc, int ch) {
    const int panel = cc / g.W, col = cc - panel * g.W;
    const size_t p = slice + (size_t)r * g.W + col;          // pixel index over [B, H, W]
    if (panel < g.C) return x[p * g.C + panel];
    if (ch > 0) return x[p * g.C];                            // overlay: green and blue of the label / probability panels = f0
    return panel == g.C ? lab[p] : prob[p];
}

// out: uint8 [nb, oh, ow, nch] padded to whole 32-bit words; thread = word (4 bytes, one store)
__global__ __launch_bounds__(RB) void k_region_render(const float* __restrict__ x, const float* __restrict__ lab, const float* __restrict__ prob,
                                                      Composite g, int nb, uint32_t* __restrict__ out) {
    const size_t total = (size_t)nb * g.oh * g.ow * g.nch;
    const size_t word = (size_t)blockIdx.x * RB + threadIdx.x;
    const size_t k0 = word * 4;
    if (k0 >= total) return;
    const size_t ohw = (size_t)g.oh * g.ow;
    uint32_t packed = 0;
    for (int e = 0; e < 4 && k0 + e < total; ++e) {
        const size_t k = k0 + e, pix = k / g.nch;
        const int ch = (int)(k - pix * g.nch);
        const size_t b = pix / ohw;
        const int q = (int)(pix - b * ohw), i = q / g.ow, j = q - i * g.ow;
        const size_t slice = b * g.H * g.W;
        // tf.image.resize bilinear, half-pixel centres, as resize_at (fp contract off: every product and sum rounded)
        const float fy = ((float)i + 0.5f) * g.sy - 0.5f;
        const float fx = ((float)j + 0.5f) * g.sx - 0.5f;
        const float fy0 = floorf(fy), fx0 = floorf(fx);
        const int y0 = max((int)fy0, 0), y1 = min((int)ceilf(fy), g.H - 1);
        const int x0 = max((int)fx0, 0), x1 = min((int)ceilf(fx), g.Wc - 1);
        const float ly = fy - fy0, lx = fx - fx0;
        const float tl = composite_at(x, lab, prob, g, slice, y0, x0, ch), tr = composite_at(x, lab, prob, g, slice, y0, x1, ch);
        const float bl = composite_at(x, lab, prob, g, slice, y1, x0, ch), br = composite_at(x, lab, prob, g, slice, y1, x1, ch);
        const float top = tl + (tr - tl) * lx;
        const float bot = bl + (br - bl) * lx;
        const float v = (top + (bot - top) * ly) * 255.f;
        // tf.cast(image * 255, uint8) truncates; values outside [0, 255] (and NaN) are clamped, where the cast is undefined
        const float s = v > 0.f ? (v < 255.f ? v : 255.f) : 0.f;
        packed |= (uint32_t)(int)s << (8 * e);
    }
    out[word] = packed;
}

// ---- lesion table (dnnca_lesion_table).  One prediction plane (T = 1): a pixel's index over the chunk is g = b * hw + p and its
// parent L[g]; S[g] is the size of the component rooted at g.
constexpr int kScanU = 16;               // lesion_scan: pixels per thread and pass (kScanU x RB / 64 = 64 wave counts: one wave scans them)
static_assert(kScanU * (RB / 64) == 64, "lesion_scan scans its wave counts with one wave");

// Kept roots (L[g] == g, S[g] >= min_area) numbered per slice in raster order: row[g] = the number at a kept root, -1 at every other
// pixel; total[b] = kept roots of slice b.  One block per slice walks it in passes of kScanU * RB pixels: a ballot per wave and 64
// pixels, the pass's 64 wave counts scanned by every wave on its own (shuffles, no second barrier; the count buffer alternates
// between passes), and the running count carried from pass to pass in a register.  No atomic: the order is the data's.
__global__ __launch_bounds__(RB) void k_lesion_scan(const int* __restrict__ L, const unsigned* __restrict__ S, int hw, unsigned min_area,
                                                    int* __restrict__ row, int* __restrict__ total) {
    __shared__ int cnt[2][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t g0 = (size_t)blockIdx.x * hw;
    const unsigned long long below = (1ull << lane) - 1ull;
    int carry = 0, buf = 0;
    for (int base = 0; base < hw; base += kScanU * RB, buf ^= 1) {
        unsigned keep = 0;               // bit u: this thread's pixel u of the pass is a kept root
        int pre[kScanU];                 // kept roots of the same wave and u on lower lanes
#pragma unroll
        for (int u = 0; u < kScanU; ++u) {
            const int p = base + u * RB + (int)threadIdx.x;
            bool k = false;
            if (p < hw) {
                const size_t g = g0 + p;
                k = L[g] == (int)g && S[g] >= min_area;
            }
            const unsigned long long bal = __ballot(k);
            pre[u] = __popcll(bal & below);
            keep |= (k ? 1u : 0u) << u;
            if (lane == 0) cnt[buf][u * (RB / 64) + wv] = __popcll(bal);
        }
        __syncthreads();
        // inclusive scan of the 64 counts over the lanes (count u * 4 + wave in lane u * 4 + wave: raster order)
        const int c = cnt[buf][lane];
        int inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        const int exc = inc - c, pass_total = __shfl(inc, 63);
#pragma unroll
        for (int u = 0; u < kScanU; ++u) {
            const int off = __shfl(exc, u * (RB / 64) + wv);
            const int p = base + u * RB + (int)threadIdx.x;
            if (p < hw) row[g0 + p] = ((keep >> u) & 1u) ? carry + off + pre[u] : -1;
        }
        carry += pass_total;
    }
    if (threadIdx.x == 0) total[blockIdx.x] = carry;
}

struct LesionAcc {                       // one row of the device table, zeroed by a memset: nx0 / ny0 hold max(~x) = ~min(x)
    unsigned long long sx, sy, sq;
    unsigned area, nx0, ny0, x1, y1, mp;
};

__device__ __forceinline__ unsigned wave_max(unsigned v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// every foreground pixel adds itself to the row of its root (rows below `cap` only).  The lanes of a wave that carry the same row
// are reduced first -- wave_grouped's loop over the distinct keys of the wave, here with sums and extrema instead of a count -- and
// the group's first lane issues the atomics: a lesion of 260 k pixels is 4 k groups, not 260 k atomics per field.  The probability
// is the one region_prep thresholded (resize_at); max through the bits (non-negative floats order like their bits).
__global__ __launch_bounds__(RB) void k_lesion_stats(const float* __restrict__ src, Resize r, int nb, const int* __restrict__ L,
                                                     const int* __restrict__ row, int cap, LesionAcc* __restrict__ acc) {
    const size_t hw = (size_t)r.out_h * r.out_w, n = (size_t)nb * hw;
    const size_t g = (size_t)blockIdx.x * RB + threadIdx.x;
    bool on = false;
    unsigned long long key = 0;
    unsigned x = 0, y = 0, bits = 0;
    unsigned long long q = 0;
    if (g < n) {
        const int root = L[g];
        if (root >= 0) {
            const int rw = row[root];
            if (rw >= 0 && rw < cap) {
                const size_t b = g / hw;
                const int p = (int)(g - b * hw);
                y = (unsigned)(p / r.out_w);
                x = (unsigned)(p - (int)y * r.out_w);
                const float v = resize_at(src + b * (size_t)r.in_h * r.in_w, r, (int)y, (int)x);
                on = true;
                key = (unsigned long long)b * (unsigned)cap + (unsigned)rw;
                bits = v > 0.f ? __float_as_uint(v) : 0u;
                q = (unsigned long long)rintf(v * 16777216.f);
            }
        }
    }
    const int lane = threadIdx.x & 63;
    unsigned long long pending = __ballot(on);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const unsigned long long k0 = __shfl(key, leader);
        const bool mine = on && key == k0;
        const unsigned long long same = __ballot(mine);
        const unsigned sx = wave_sum(mine ? x : 0u), sy = wave_sum(mine ? y : 0u);
        const unsigned long long sq = wave_sum64(mine ? q : 0ull);
        const unsigned nx0 = wave_max(mine ? ~x : 0u), ny0 = wave_max(mine ? ~y : 0u);
        const unsigned x1 = wave_max(mine ? x : 0u), y1 = wave_max(mine ? y : 0u), mp = wave_max(mine ? bits : 0u);
        if (lane == leader) {
            LesionAcc* a = acc + k0;
            atomicAdd(&a->area, (unsigned)__popcll(same));
            atomicAdd(&a->sx, (unsigned long long)sx);
            atomicAdd(&a->sy, (unsigned long long)sy);
            atomicAdd(&a->sq, sq);
            atomicMax(&a->nx0, nx0);
            atomicMax(&a->ny0, ny0);
            atomicMax(&a->x1, x1);
            atomicMax(&a->y1, y1);
            atomicMax(&a->mp, mp);
        }
        if (mine) on = false;
        pending &= ~same;
    }
}

// out: uint8 [nb, oh, ow] padded to whole 32-bit words: 255 where the pixel's component is kept; thread = word (4 bytes, one store)
__global__ __launch_bounds__(RB) void k_lesion_mask(const int* __restrict__ L, const int* __restrict__ row, size_t total,
                                                    uint32_t* __restrict__ out) {
    const size_t word = (size_t)blockIdx.x * RB + threadIdx.x;
    const size_t k0 = word * 4;
    if (k0 >= total) return;
    int root[4] = {-1, -1, -1, -1};
    if (k0 + 4 <= total) {
        const int4 v = *reinterpret_cast<const int4*>(L + k0);       // L is 256-byte aligned and k0 a multiple of 4
        root[0] = v.x, root[1] = v.y, root[2] = v.z, root[3] = v.w;
    } else {
        for (int e = 0; k0 + e < total; ++e) root[e] = L[k0 + e];
    }
    uint32_t packed = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (root[e] >= 0 && row[root[e]] >= 0) packed |= 0xffu << (8 * e);
    out[word] = packed;
}

// ---- the spread of the test-time-augmentation views under the lesion table (dnnca_lesion_table_spread) and per pixel outcome
// (dnnca_spread_by_outcome).  A spread enters every sum as rint(max(spread', 0) * 2^24) and every maximum through its bits.
struct SpreadAcc {                       // a lesion's row or a slice's total, zeroed by a memset
    unsigned long long sq;
    unsigned area, mx;
};

// lesion_stats for the spread plane.  grid (ceil(hw / (RB kSpreadU)), slices): a block walks kSpreadU runs of RB pixels of ONE slice.
// Every pixel of a kept, numbered component adds its spread -- read through the resize_at that the probability went through -- to its
// row, the lanes of a wave grouped by row as in lesion_stats; and EVERY pixel adds to the slice's total, kept in registers over the
// block's runs and reduced over the wave and the block: three atomics per block (64 blocks per slice at 512 x 512; one block per
// 256 pixels had 1024 blocks queue up on a slice's one cache line and took 232 us at 8 x 512 x 512).
constexpr int kSpreadU = 16;
__global__ __launch_bounds__(RB) void k_lesion_spread(const float* __restrict__ src, Resize r, const int* __restrict__ L,
                                                      const int* __restrict__ row, int cap, SpreadAcc* __restrict__ acc,
                                                      SpreadAcc* __restrict__ tot) {
    __shared__ unsigned long long wsq[RB / 64];
    __shared__ unsigned wmx[RB / 64];
    const int hw = r.out_h * r.out_w, b = blockIdx.y;
    const size_t g0 = (size_t)b * hw;
    const float* plane = src + (size_t)b * r.in_h * r.in_w;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int p0 = blockIdx.x * (RB * kSpreadU) + (int)threadIdx.x;
    unsigned long long tsq = 0;
    unsigned tmx = 0;
    for (int u = 0; u < kSpreadU; ++u) {
        const int p = p0 + u * RB;
        if (p - (int)threadIdx.x >= hw) break;           // the whole run lies behind the slice: the same for every thread of the block
        bool on = false;
        unsigned long long q = 0;
        unsigned key = 0, bits = 0;
        if (p < hw) {
            const int y = p / r.out_w, x = p - y * r.out_w;
            const float v = fmaxf(resize_at(plane, r, y, x), 0.f);
            bits = __float_as_uint(v);
            q = (unsigned long long)rintf(v * 16777216.f);
            tsq += q;
            tmx = max(tmx, bits);
            const int root = L[g0 + p];
            if (root >= 0) {
                const int rw = row[root];
                if (rw >= 0 && rw < cap) {
                    on = true;
                    key = (unsigned)rw;
                }
            }
        }
        unsigned long long pending = __ballot(on);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const unsigned k0 = __shfl(key, leader);
            const bool mine = on && key == k0;
            const unsigned long long same = __ballot(mine);
            const unsigned long long sq = wave_sum64(mine ? q : 0ull);
            const unsigned mx = wave_max(mine ? bits : 0u);
            if (lane == leader) {
                SpreadAcc* a = acc + (size_t)b * cap + k0;
                atomicAdd(&a->area, (unsigned)__popcll(same));
                atomicAdd(&a->sq, sq);
                atomicMax(&a->mx, mx);
            }
            if (mine) on = false;
            pending &= ~same;
        }
    }
    tsq = wave_sum64(tsq);
    tmx = wave_max(tmx);
    if (lane == 0) wsq[wv] = tsq, wmx[wv] = tmx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < RB / 64; ++w) tsq += wsq[w], tmx = max(tmx, wmx[w]);
        const int first = blockIdx.x * (RB * kSpreadU);
        SpreadAcc* a = tot + b;
        atomicAdd(&a->area, (unsigned)min(RB * kSpreadU, hw - first));
        atomicAdd(&a->sq, tsq);
        atomicMax(&a->mx, tmx);
    }
}

// grid (ceil(hw / (RB kOutcomeU)), thresholds, slices).  A pixel's class is 2 (y > 0.5) + (prob >= threshold): TN 0, FP 1, FN 2, TP 3.
// A thread keeps the four counts and the four q24 sums of its kOutcomeU pixels in registers, a wave and then the block reduce them,
// and eight threads add what is not zero to out [thresholds][slices][8] (n[4], then sum_q24[4]): at most eight atomics per block.
constexpr int kOutcomeU = 16;
__global__ __launch_bounds__(RB) void k_spread_outcome(const float* __restrict__ prob, const float* __restrict__ spread,
                                                       const float* __restrict__ y, const float* __restrict__ thr, size_t hw,
                                                       unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[RB / 64][8];
    const float th = thr[blockIdx.y];
    const size_t base = (size_t)blockIdx.z * hw, p0 = (size_t)blockIdx.x * RB * kOutcomeU + threadIdx.x;
    unsigned long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < kOutcomeU; ++u) {
        const size_t p = p0 + (size_t)u * RB;
        if (p < hw) {
            const int cls = (y[base + p] > 0.5f ? 2 : 0) + (prob[base + p] >= th ? 1 : 0);
            const unsigned long long q = (unsigned long long)rintf(fmaxf(spread[base + p], 0.f) * 16777216.f);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                v[c] += cls == c ? 1ull : 0ull;
                v[4 + c] += cls == c ? q : 0ull;
            }
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const unsigned long long s = wave_sum64(v[c]);
        if (lane == 0) part[wv][c] = s;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        unsigned long long s = 0;
        for (int w = 0; w < RB / 64; ++w) s += part[w][threadIdx.x];
        if (s) atomicAdd(out + ((size_t)blockIdx.y * gridDim.z + blockIdx.z) * 8 + threadIdx.x, s);
    }
}

// ---- what a lesion looks like in the input channels (dnnca_lesion_table_features): shape, body and ring records under the rows of
// the lesion table.  A pixel's value in channel c is x' (the channel read through the resize the probabilities went through) as
// v = min(max(x', 0), 1), NaN = 0.  It enters the sums as q = rint(v * 2^16): q16 and not the q24 of the probabilities, so that
// q^2 <= 2^32 and a sum of q^2 over the 2^31 pixels a plane can have stays below 2^64.  Extrema go through the float's bits.
struct FeatShapeAcc {                    // one lesion, zeroed by a memset
    unsigned long long sxx, syy, sxy;
    unsigned area, boundary, edges, pad;
};
struct FeatAcc {                         // one lesion and channel, body or ring, zeroed by a memset: nmn holds max(~bits) = ~min(bits)
    unsigned long long sq, ssq;
    unsigned n, nmn, mx, pad;
};

// resize_at on channel c of an interleaved plane [in_h, in_w, C]: the same operations in the same order
__device__ __forceinline__ float resize_at_c(const float* __restrict__ src, const Resize& r, int i, int j, int C, int c) {
    if (r.identity) return src[((size_t)i * r.in_w + j) * C + c];
    const float fy = ((float)i + 0.5f) * r.sy - 0.5f;
    const float fx = ((float)j + 0.5f) * r.sx - 0.5f;
    const float fy0 = floorf(fy), fx0 = floorf(fx);
    const int y0 = max((int)fy0, 0), y1 = min((int)ceilf(fy), r.in_h - 1);
    const int x0 = max((int)fx0, 0), x1 = min((int)ceilf(fx), r.in_w - 1);
    const float ly = fy - fy0, lx = fx - fx0;
    const float tl = src[((size_t)y0 * r.in_w + x0) * C + c], tr = src[((size_t)y0 * r.in_w + x1) * C + c];
    const float bl = src[((size_t)y1 * r.in_w + x0) * C + c], br = src[((size_t)y1 * r.in_w + x1) * C + c];
    const float top = tl + (tr - tl) * lx;
    const float bot = bl + (br - bl) * lx;
    return top + (bot - top) * ly;
}

// The lanes of a wave that are `on` add pixel (y, x) of every channel to the records of their row `key` (acc, hist: the slice's).
// Lanes are grouped by row as in lesion_stats; a lane loads its channels inside its own group's pass, so every value is read once.
// hist == nullptr: no histogram; else one count per pixel and channel (calibration's bin rule: a float32 product, floor, clamp).
// The counts of ONE row per block -- the first that a wave with all 64 lanes in one lesion claims in *lrow (-1: none yet) -- go to
// the block's LDS histogram lh [C][bins], which the caller adds to `hist` at its end; everything else goes to `hist` one atomic
// each.  A lesion that fills the block's 4096 pixels then costs C * bins global atomics per block, not 4096 C, and specks and
// outlines never ask.  Every lane of the wave must call this.
__device__ __forceinline__ void feat_intensity(bool on, unsigned key, int y, int x, const float* __restrict__ plane, const Resize& r, int C,
                                               int bins, FeatAcc* __restrict__ acc, unsigned* __restrict__ hist, unsigned* lh, int* lrow,
                                               int lane) {
    unsigned long long pending = __ballot(on);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const unsigned k0 = __shfl(key, leader);
        const bool mine = on && key == k0;
        const unsigned long long same = __ballot(mine);
        bool local = false;              // this group's row is the block's
        if (hist && same == ~0ull) {
            int held = (int)k0;
            if (lane == leader) {
                const int was = atomicCAS(lrow, -1, (int)k0);
                if (was != -1) held = was;
            }
            local = __shfl(held, leader) == (int)k0;
        }
        for (int c = 0; c < C; ++c) {
            unsigned q = 0, bits = 0, nbits = 0;
            if (mine) {
                const float xv = resize_at_c(plane, r, y, x, C, c);
                const float v = xv > 0.f ? (xv < 1.f ? xv : 1.f) : 0.f;      // a NaN compares false: 0
                bits = __float_as_uint(v);
                nbits = ~bits;
                q = (unsigned)rintf(v * 65536.f);
                if (hist) {
                    const int bin = min(bins - 1, (int)floorf(v * (float)bins));
                    if (local) atomicAdd(lh + c * bins + bin, 1u);
                    else atomicAdd(hist + ((size_t)k0 * C + c) * bins + bin, 1u);
                }
            }
            const unsigned sq = wave_sum(q);                                 // 64 lanes of at most 2^16
            const unsigned long long ssq = wave_sum64((unsigned long long)q * q);
            const unsigned mx = wave_max(bits), nmn = wave_max(nbits);
            if (lane == leader) {
                FeatAcc* a = acc + (size_t)k0 * C + c;
                atomicAdd(&a->n, (unsigned)__popcll(same));
                atomicAdd(&a->sq, (unsigned long long)sq);
                atomicAdd(&a->ssq, ssq);
                atomicMax(&a->nmn, nmn);
                atomicMax(&a->mx, mx);
            }
        }
        if (mine) on = false;
        pending &= ~same;
    }
}

// lesion_spread's grid, (ceil(hw / (RB kFeatU)), slices): a block walks kFeatU runs of RB pixels of ONE slice.  Every pixel of a
// numbered lesion adds to its shape record -- area, the second moments of its coordinates, the faces that look out of the lesion (a
// 4-neighbour with another root, or none: the plane's border) and whether it has one -- and to its body records.  No per-slice
// total is kept here, so no cache line is shared by every block of a slice (what lesion_spread's comment measured).
constexpr int kFeatU = 16;
constexpr int kFeatMaxC = 16, kFeatMaxBins = 256;        // what dnnca_lesion_table_features accepts: an LDS histogram of 16 KiB at most
__global__ __launch_bounds__(RB) void k_lesion_features(const float* __restrict__ x, Resize r, int C, int bins, const int* __restrict__ L,
                                                        const int* __restrict__ row, int cap, FeatShapeAcc* __restrict__ shp,
                                                        FeatAcc* __restrict__ body, unsigned* __restrict__ hist) {
    const int oh = r.out_h, ow = r.out_w, hw = oh * ow, b = blockIdx.y;
    const size_t g0 = (size_t)b * hw;
    const float* plane = x + (size_t)b * r.in_h * r.in_w * C;
    FeatShapeAcc* sh = shp + (size_t)b * cap;
    FeatAcc* bd = body + (size_t)b * cap * C;
    unsigned* hs = hist ? hist + (size_t)b * cap * C * bins : nullptr;
    extern __shared__ unsigned lh[];     // [C][bins] with a histogram, nothing without
    __shared__ int lrow;
    if (hs) {
        for (int i = threadIdx.x; i < C * bins; i += RB) lh[i] = 0;
        if (threadIdx.x == 0) lrow = -1;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int p0 = blockIdx.x * (RB * kFeatU) + (int)threadIdx.x;
    for (int u = 0; u < kFeatU; ++u) {
        const int p = p0 + u * RB;
        if (p - (int)threadIdx.x >= hw) break;           // the whole run lies behind the slice: the same for every thread of the block
        bool on = false;
        unsigned key = 0, faces = 0;
        int py = 0, px = 0;
        if (p < hw) {
            const int root = L[g0 + p];
            if (root >= 0) {
                const int rw = row[root];
                if (rw >= 0 && rw < cap) {
                    on = true;
                    key = (unsigned)rw;
                    py = p / ow, px = p - py * ow;
                    faces = (px == 0 || L[g0 + p - 1] != root) + (px == ow - 1 || L[g0 + p + 1] != root) +
                            (py == 0 || L[g0 + p - ow] != root) + (py == oh - 1 || L[g0 + p + ow] != root);
                }
            }
        }
        unsigned long long pending = __ballot(on);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const unsigned k0 = __shfl(key, leader);
            const bool mine = on && key == k0;
            const unsigned long long same = __ballot(mine), edge = __ballot(mine && faces);
            const unsigned long long ux = mine ? (unsigned long long)px : 0ull, uy = mine ? (unsigned long long)py : 0ull;
            const unsigned long long sxx = wave_sum64(ux * ux), syy = wave_sum64(uy * uy), sxy = wave_sum64(ux * uy);
            const unsigned nf = wave_sum(mine ? faces : 0u);
            if (lane == leader) {
                FeatShapeAcc* a = sh + k0;
                atomicAdd(&a->area, (unsigned)__popcll(same));
                atomicAdd(&a->boundary, (unsigned)__popcll(edge));
                atomicAdd(&a->edges, nf);
                atomicAdd(&a->sxx, sxx);
                atomicAdd(&a->syy, syy);
                atomicAdd(&a->sxy, sxy);
            }
            pending &= ~same;
        }
        feat_intensity(on, key, py, px, plane, r, C, bins, bd, hs, lh, &lrow, lane);
    }
    if (hs) {                            // every thread of the block gets here: the loop's break is the same for all of them
        __syncthreads();
        if (lrow >= 0)
            for (int i = threadIdx.x; i < C * bins; i += RB)
                if (lh[i]) atomicAdd(hs + (size_t)lrow * C * bins + i, lh[i]);
    }
}

// The tissue around every numbered lesion: a background pixel (in no kept component) belongs to the ring of the smallest row number
// among the numbered lesions in its (2R + 1)^2 window, clipped by the plane.  That minimum is separable.  grid (ceil(ow / kTile),
// ceil(oh / kTile), slices): a block loads the row numbers of its tile with a halo of R into LDS (kRingKept: a kept component
// that has no row; kRingNone: background or outside), takes the minimum along the rows, then along the columns, and adds its ring pixels
// like lesion_features adds body pixels.  A block whose tile and halo hold no numbered lesion leaves after the load: on a real slice
// that is nearly every block, and it has read 4 (1 + 2R / kTile)^2 bytes per pixel by then.
constexpr int kRingMaxR = 8;
constexpr int kRingE = kTile + 2 * kRingMaxR;
constexpr int kRingKept = 0x7ffffffe, kRingNone = 0x7fffffff;
__global__ __launch_bounds__(RB) void k_lesion_ring(const float* __restrict__ x, Resize r, int C, int R, const int* __restrict__ L,
                                                    const int* __restrict__ row, int cap, FeatAcc* __restrict__ ring) {
    __shared__ int m[kRingE * kRingE];
    __shared__ int hm[kRingE * kTile];
    const int oh = r.out_h, ow = r.out_w, b = blockIdx.z, E = kTile + 2 * R;
    const size_t g0 = (size_t)b * oh * ow;
    const int ty0 = blockIdx.y * kTile, tx0 = blockIdx.x * kTile;
    int any = 0;
    for (int i = threadIdx.x; i < E * E; i += RB) {
        const int ty = i / E, tx = i - ty * E;
        const int y = ty0 - R + ty, xx = tx0 - R + tx;
        int v = kRingNone;
        if (y >= 0 && y < oh && xx >= 0 && xx < ow) {
            const int root = L[g0 + (size_t)y * ow + xx];
            if (root >= 0) {
                const int rw = row[root];
                if (rw >= 0) v = rw < cap ? rw : kRingKept;
            }
        }
        any |= v < cap;
        m[i] = v;
    }
    if (!__syncthreads_or(any)) return;
    for (int i = threadIdx.x; i < E * kTile; i += RB) {
        const int ty = i / kTile, tx = i - ty * kTile;
        int v = kRingNone;
        for (int d = 0; d <= 2 * R; ++d) v = min(v, m[ty * E + tx + d]);
        hm[i] = v;
    }
    __syncthreads();
    const float* plane = x + (size_t)b * r.in_h * r.in_w * C;
    FeatAcc* rg = ring + (size_t)b * cap * C;
    const int lane = threadIdx.x & 63;
    const int tx = threadIdx.x & (kTile - 1);
    for (int ty = threadIdx.x / kTile; ty < kTile; ty += RB / kTile) {       // the same trip count for every thread
        const int y = ty0 + ty, xx = tx0 + tx;
        int owner = kRingNone;
        for (int d = 0; d <= 2 * R; ++d) owner = min(owner, hm[(ty + d) * kTile + tx]);
        const bool on = y < oh && xx < ow && m[(ty + R) * E + tx + R] == kRingNone && owner < cap;
        feat_intensity(on, (unsigned)owner, y, xx, plane, r, C, 0, rg, nullptr, nullptr, nullptr, lane);
    }
}

// ---- links between neighbouring slices (dnnca_lesion_table_linked).  A pixel's lesion is row[L[g]]: the row number of its root,
// taken as -1 on background, in a component below min_area and at rows >= cap (they are in no table).
__device__ __forceinline__ int lesion_row_at(const int* __restrict__ L, const int* __restrict__ row, size_t g, int cap) {
    const int root = L[g];
    if (root < 0) return -1;
    const int r = row[root];
    return r < cap ? r : -1;
}

// pixel p of slice b whose flag is set counts one towards key (prev << 32 | cur) of slice b's table when it lies in a lesion of
// the slice (cur) and pixel p of the slice before lies in one too (prev): the slice before is b - 1 of the chunk, or for b = 0
// the carry plane (the last slice of the chunk or of the call before).  Wave-grouped like region_pairs.
// A table has hw + 1 slots: distinct pairs of one slice number at most ceil(hw / 2).  Take one witness pixel per pair; two
// 4-adjacent pixels that both lie in lesions of both slices lie in the same lesion of either slice, i.e. in the same pair, so
// witnesses of different pairs are never 4-adjacent: they are an independent set of the hw-pixel grid, which has at most
// ceil(hw / 2) members.  hw + 1 slots keep the load below one half.
__global__ __launch_bounds__(RB) void k_lesion_link(const int* __restrict__ L, const int* __restrict__ row, const int* __restrict__ carry,
                                                    const unsigned char* __restrict__ cont, int nb, size_t hw, int cap, size_t slots,
                                                    unsigned long long* __restrict__ keys, unsigned* __restrict__ cnt) {
    const size_t g = (size_t)blockIdx.x * RB + threadIdx.x;
    bool on = false;
    unsigned long long key = 0;
    size_t b = 0;
    if (g < (size_t)nb * hw) {
        b = g / hw;
        if (cont[b]) {
            const int cur = lesion_row_at(L, row, g, cap);
            if (cur >= 0) {
                const int prev = b > 0 ? lesion_row_at(L, row, g - hw, cap) : carry[g];
                if (prev >= 0 && prev < cap) {
                    on = true;
                    key = ((unsigned long long)(unsigned)prev << 32) | (unsigned)cur;
                }
            }
        }
    }
    wave_grouped_at(on, b, key, [&](size_t b0, unsigned long long key0, unsigned c) {
        table_add(keys + b0 * slots, cnt + b0 * slots, slots, key0, c);
    });
}

struct LesionLink {                      // dnnca_lesion_link
    int slice, row_prev, row, overlap;
};
static_assert(sizeof(LesionLink) == sizeof(dnnca_lesion_link), "the device list is copied into the caller's records");

// one thread per slot of the chunk's tables: a filled slot appends its link to the list (in the order of the atomics: the host
// sorts).  One atomic per wave: its filled slots take consecutive places.  Grid y = 1 serves the linked call's one set of tables;
// the matched call's three sets (`total` slots each, one behind the other) go through one launch with grid y = 3: set y fills
// the list at list + y * list_cap and counts in n_list[y].  A wave lies in one set
__global__ __launch_bounds__(RB) void k_lesion_link_emit(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ cnt,
                                                         size_t total, size_t slots, int slice0, unsigned list_cap,
                                                         LesionLink* __restrict__ list, unsigned* __restrict__ n_list) {
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x, at0 = (size_t)blockIdx.y * total;
    const unsigned long long key = i < total ? keys[at0 + i] : kEmpty;
    const bool has = key != kEmpty;
    const unsigned long long bal = __ballot(has);
    if (!bal) return;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)bal) - 1;
    unsigned base = 0;
    if (lane == leader) base = atomicAdd(n_list + blockIdx.y, (unsigned)__popcll(bal));
    base = __shfl(base, leader);
    const unsigned at = base + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
    if (has && at < list_cap)
        list[(size_t)blockIdx.y * list_cap + at] =
            LesionLink{slice0 + (int)(i / slots), (int)(key >> 32), (int)(key & 0xffffffffu), (int)cnt[at0 + i]};
}

// the carry plane: the lesion (or -1) of every pixel of the chunk's last slice (L / row of that slice's first pixel at g0)
__global__ __launch_bounds__(RB) void k_lesion_carry(const int* __restrict__ L, const int* __restrict__ row, size_t g0, size_t hw, int cap,
                                                     int* __restrict__ carry) {
    const size_t p = (size_t)blockIdx.x * RB + threadIdx.x;
    if (p < hw) carry[p] = lesion_row_at(L, row, g0 + p, cap);
}

// ---- the matched call (dnnca_lesion_table_matched): the prediction plane (L / row) and the label plane (LT / rowT) of the same
// slices, each numbered by lesion_scan.  One pass over the pixels fills three sets of per-slice tables, `set` slots apart:
//   0  links of the prediction plane   key (prev << 32 | cur)        exactly what k_lesion_link counts
//   1  links of the label plane        key (prev_true << 32 | cur_true)
//   2  pairs of the slice itself       key (cur_true << 32 | cur)    whatever the slice's flag says
// A pixel reads its two rows once and, where the slice's flag is set, the two rows of the same pixel of the slice before: slice
// b - 1 of the chunk, or for b = 0 the two carry planes of the matched call.  Up to three wave-grouped table_adds per pixel.
// The bound of the pairs is the links' (above k_lesion_link), with the label map in the place of the slice before: take one
// witness pixel per pair (row_true, row); two 4-adjacent pixels that both lie in lesions of both maps lie in the same labelled
// lesion and in the same predicted lesion, i.e. in the same pair, so witnesses of different pairs are never 4-adjacent: they are
// an independent set of the hw-pixel grid, at most ceil(hw / 2) members.  Every table has hw + 1 slots: load below one half.
__global__ __launch_bounds__(RB) void k_lesion_match(const int* __restrict__ L, const int* __restrict__ row, const int* __restrict__ LT,
                                                     const int* __restrict__ rowT, const int* __restrict__ carry,
                                                     const int* __restrict__ carryT, const unsigned char* __restrict__ cont, int nb,
                                                     size_t hw, int cap, size_t slots, unsigned long long* __restrict__ keys,
                                                     unsigned* __restrict__ cnt) {
    const size_t g = (size_t)blockIdx.x * RB + threadIdx.x;
    bool on_link = false, on_true = false, on_pair = false;
    unsigned long long key_link = 0, key_true = 0, key_pair = 0;
    size_t b = 0;
    if (g < (size_t)nb * hw) {
        b = g / hw;
        const int cur = lesion_row_at(L, row, g, cap), curT = lesion_row_at(LT, rowT, g, cap);
        if (cur >= 0 && curT >= 0) {
            on_pair = true;
            key_pair = ((unsigned long long)(unsigned)curT << 32) | (unsigned)cur;
        }
        if (cont[b] && (cur >= 0 || curT >= 0)) {
            const size_t p = g - b * hw;
            if (cur >= 0) {
                const int prev = b > 0 ? lesion_row_at(L, row, g - hw, cap) : carry[p];
                if (prev >= 0 && prev < cap) {
                    on_link = true;
                    key_link = ((unsigned long long)(unsigned)prev << 32) | (unsigned)cur;
                }
            }
            if (curT >= 0) {
                const int prevT = b > 0 ? lesion_row_at(LT, rowT, g - hw, cap) : carryT[p];
                if (prevT >= 0 && prevT < cap) {
                    on_true = true;
                    key_true = ((unsigned long long)(unsigned)prevT << 32) | (unsigned)curT;
                }
            }
        }
    }
    auto add = [&](size_t tb, unsigned long long key0, unsigned c) { table_add(keys + tb * slots, cnt + tb * slots, slots, key0, c); };
    wave_grouped_at(on_link, b, key_link, add);                       // table b of set s is table s * nb + b
    wave_grouped_at(on_true, (size_t)nb + b, key_true, add);
    wave_grouped_at(on_pair, 2 * (size_t)nb + b, key_pair, add);
}

// the two carry planes of the matched call: grid y = 0 the prediction's rows, 1 the label's rows of the chunk's last slice
__global__ __launch_bounds__(RB) void k_lesion_match_carry(const int* __restrict__ L, const int* __restrict__ row, const int* __restrict__ LT,
                                                           const int* __restrict__ rowT, size_t g0, size_t hw, int cap,
                                                           int* __restrict__ carry, int* __restrict__ carryT) {
    const size_t p = (size_t)blockIdx.x * RB + threadIdx.x;
    if (p >= hw) return;
    if (blockIdx.y == 0) carry[p] = lesion_row_at(L, row, g0 + p, cap);
    else carryT[p] = lesion_row_at(LT, rowT, g0 + p, cap);
}

// ---- boundary distances (dnnca_surface_distances).  Side 0 is the prediction mask -- the mask of the lesion table: a foreground
// pixel of the opened words whose component has at least min_area pixels -- side 1 the label foreground (bit 0 of its words).
// A boundary pixel of a side is one of its pixels with a 4-neighbour off the side or off the plane.  A 4-neighbour that is
// foreground lies in the pixel's own component and is kept or dropped with it, so the neighbours are read from the words alone.
//   surface_edges   E[g] = bit 0: boundary of side 0, bit 1: boundary of side 1; counts[b] += {area_pred, area_true, common,
//                   edge_pred, edge_true}: one block reduction, one atomic per block and counter.  Grid y = slice
//   surface_cols    V[side][g] = rows between pixel g and the nearest boundary pixel of `side` in its column (kSurfaceFar: none):
//                   one launch for both sides and all slices, a thread per column and 32 rows
//   surface_sample  a boundary pixel (x, y) of side s takes d2 = min over x' of (x - x')^2 + V[1 - s][y][x']^2: the exact squared
//                   distance to the nearest boundary pixel of the other side (the lower envelope of the row's parabolas, evaluated at
//                   this pixel only).  It walks outward from x and stops where (x - x')^2 alone reaches the best so far.  The
//                   samples of a wave take consecutive places of the list behind one atomic (the host sorts).  A slice whose edge
//                   counts are 0 or above max_samples emits nothing: the counts are complete when this kernel starts
// kSurfaceFar^2 + (ow - 1)^2 < 2^31 for planes of up to kSurfaceMaxSide pixels a side, and every real distance is below it (region.h).

struct SurfaceSample {                   // dnnca_surface_sample
    int slice, side, pixel, d2;
};
static_assert(sizeof(SurfaceSample) == sizeof(dnnca_surface_sample), "the device list is copied into the caller's records");
static_assert((long long)kSurfaceFar * kSurfaceFar + (long long)(kSurfaceMaxSide - 1) * (kSurfaceMaxSide - 1) < (1ll << 31) &&
                  kSurfaceFar >= (unsigned)kSurfaceMaxSide,
              "the sentinel's square plus any offset fits an int32 and no real distance reaches it");

__global__ __launch_bounds__(RB) void k_surface_edges(const uint32_t* __restrict__ fg, const int* __restrict__ L,
                                                      const unsigned* __restrict__ S, unsigned min_area,
                                                      const uint32_t* __restrict__ yw, int H, int W, unsigned char* __restrict__ E,
                                                      unsigned* __restrict__ counts) {
    __shared__ unsigned part[RB / 64][5];
    const int hw = H * W, p = (int)(blockIdx.x * RB + threadIdx.x);
    const size_t g0 = (size_t)blockIdx.y * hw;
    unsigned c[5] = {0u, 0u, 0u, 0u, 0u};
    if (p < hw) {
        const size_t g = g0 + p;
        const int y = p / W, x = p - y * W;
        const bool l = x > 0, r = x + 1 < W, u = y > 0, d = y + 1 < H;
        unsigned pred = fg[g] & 1u;
        if (pred) {
            const int root = L[g];
            pred = root >= 0 && S[root] >= min_area ? 1u : 0u;
        }
        const unsigned lab = yw[g] & 1u;
        unsigned ep = 0, et = 0;
        if (pred) ep = !(l && (fg[g - 1] & 1u) && r && (fg[g + 1] & 1u) && u && (fg[g - W] & 1u) && d && (fg[g + W] & 1u));
        if (lab) et = !(l && (yw[g - 1] & 1u) && r && (yw[g + 1] & 1u) && u && (yw[g - W] & 1u) && d && (yw[g + W] & 1u));
        E[g] = (unsigned char)(ep | (et << 1));
        c[0] = pred, c[1] = lab, c[2] = pred & lab, c[3] = ep, c[4] = et;
    }
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int j = 0; j < 5; ++j) {
        const unsigned s = wave_sum(c[j]);
        if (lane == 0) part[wv][j] = s;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        unsigned s = 0;
        for (int k = 0; k < RB / 64; ++k) s += part[k][threadIdx.x];
        if (s) atomicAdd(counts + (size_t)blockIdx.y * 5 + threadIdx.x, s);
    }
}

// a block takes kColsX columns of one side of one slice; thread (column, lane) takes the 32-row pieces lane, lane + kColsL, ... of its
// column.  Pass 1 packs a piece's boundary bits into one word (32 independent loads) and leaves it in LDS; pass 2 finds the nearest
// boundary row above and below the piece in the column's words and every row's distance with bit counts, in registers
constexpr int kColsX = 16, kColsL = RB / kColsX;

__global__ __launch_bounds__(RB) void k_surface_cols(const unsigned char* __restrict__ E, int nb, int H, int W,
                                                     unsigned short* __restrict__ V) {
    extern __shared__ uint32_t words[];  // [pieces][kColsX]
    const int col = threadIdx.x & (kColsX - 1), lane = threadIdx.x / kColsX;
    const int x = (int)blockIdx.x * kColsX + col, side = (int)(blockIdx.y & 1u), b = (int)(blockIdx.y >> 1);
    const int pieces = (H + 31) / 32;
    const size_t hw = (size_t)H * W, at = (size_t)b * hw + x;
    const unsigned char* e = E + at;
    unsigned short* v = V + (size_t)side * nb * hw + at;
    for (int c = lane; c < pieces; c += kColsL) {
        uint32_t m = 0;
        if (x < W) {
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const int y = c * 32 + j;
                if (y < H) m |= (uint32_t)((e[(size_t)y * W] >> side) & 1u) << j;
            }
        }
        words[c * kColsX + col] = m;
    }
    __syncthreads();
    if (x >= W) return;
    for (int c = lane; c < pieces; c += kColsL) {
        const uint32_t m = words[c * kColsX + col];
        int above = -1, below = -1;      // the nearest boundary row before and behind the piece
        for (int cc = c - 1; cc >= 0; --cc) {
            const uint32_t o = words[cc * kColsX + col];
            if (o) { above = cc * 32 + 31 - __clz((int)o); break; }
        }
        for (int cc = c + 1; cc < pieces; ++cc) {
            const uint32_t o = words[cc * kColsX + col];
            if (o) { below = cc * 32 + __ffs((int)o) - 1; break; }
        }
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const int y = c * 32 + j;
            if (y >= H) break;
            const uint32_t upto = m & (0xffffffffu >> (31 - j)), from = m >> j;
            const int yu = upto ? c * 32 + 31 - __clz((int)upto) : above;
            const int yd = from ? y + __ffs((int)from) - 1 : below;
            const unsigned du = yu >= 0 ? (unsigned)(y - yu) : kSurfaceFar, dd = yd >= 0 ? (unsigned)(yd - y) : kSurfaceFar;
            v[(size_t)y * W] = (unsigned short)min(du, dd);
        }
    }
}

__global__ __launch_bounds__(RB) void k_surface_sample(const unsigned char* __restrict__ E, const unsigned short* __restrict__ V,
                                                       const unsigned* __restrict__ counts, int nb, int H, int W, unsigned max_samples,
                                                       int slice0, unsigned list_cap, SurfaceSample* __restrict__ list,
                                                       unsigned* __restrict__ n_list) {
    const int b = blockIdx.y, hw = H * W, p = (int)(blockIdx.x * RB + threadIdx.x);
    const unsigned np = counts[(size_t)b * 5 + 3], nt = counts[(size_t)b * 5 + 4];
    if (np == 0u || nt == 0u || np > max_samples || nt > max_samples) return;      // the whole block: its slice gives no samples
    const size_t n = (size_t)nb * hw;
    const unsigned bits = p < hw ? E[(size_t)b * hw + p] : 0u;
    const unsigned long long bal0 = __ballot(bits & 1u), bal1 = __ballot(bits & 2u);
    if (!(bal0 | bal1)) return;
    int d2[2] = {0, 0};
    if (bits) {
        const int y = p / W, x = p - y * W;
        const int reach = max(x, W - 1 - x);
        for (int side = 0; side < 2; ++side) {
            if (!((bits >> side) & 1u)) continue;
            const unsigned short* row = V + (size_t)(1 - side) * n + (size_t)b * hw + (size_t)y * W;
            int best = (int)row[x] * (int)row[x];
            for (int dx = 1; dx <= reach && dx * dx < best; ++dx) {
                if (x - dx >= 0) {
                    const int v = row[x - dx];
                    best = min(best, dx * dx + v * v);
                }
                if (x + dx < W) {
                    const int v = row[x + dx];
                    best = min(best, dx * dx + v * v);
                }
            }
            d2[side] = best;
        }
    }
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)(bal0 | bal1)) - 1;
    const unsigned n0 = (unsigned)__popcll(bal0);
    unsigned base = 0;
    if (lane == leader) base = atomicAdd(n_list, n0 + (unsigned)__popcll(bal1));
    base = __shfl(base, leader);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (bits & 1u) {
        const unsigned at = base + (unsigned)__popcll(bal0 & below);
        if (at < list_cap) list[at] = SurfaceSample{slice0 + b, 0, p, d2[0]};
    }
    if (bits & 2u) {
        const unsigned at = base + n0 + (unsigned)__popcll(bal1 & below);
        if (at < list_cap) list[at] = SurfaceSample{slice0 + b, 1, p, d2[1]};
    }
}

inline unsigned nblocks(size_t n) { return (unsigned)((n + RB - 1) / RB); }

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- host side
struct RegionState {
    std::vector<RegionSpecHost> specs;
    std::vector<int> order;              // specs by resized plane: the label plane is labelled once per size
    float* thr_dev = nullptr;            // [n_specs][kRegionMaxThr]
    unsigned long long* acc = nullptr;   // [n_specs][kRegionMaxThr][4]
    size_t acc_specs = 0;
    // workspace of one chunk of slices
    void* ws = nullptr;
    size_t ws_bytes = 0;
    int chunk = 0;                       // slices per chunk
    float* in_prob = nullptr;            // dnnca_region_confusion_of inputs
    float* in_y = nullptr;
    size_t in_n = 0;
    int label_batch = 0;                 // in_y holds the labels of dnnca_region_confusion_slices' `label_batch` slices (0: not)
    // per-slice counts (dnnca_region_confusion_slices): uint64 [slices][n_specs][kRegionMaxThr][4]
    unsigned long long* slice_acc = nullptr;
    size_t slice_acc_n = 0, slices = 0;
    uint32_t* viz = nullptr;             // rendered composites (dnnca_render_composite)
    size_t viz_bytes = 0;
    float lesion_rf = 1.f;               // the last dnnca_lesion_table(_linked): what DNNCA_PLAN_LESION(_LINKED) replays
    int lesion_k = 5;
    bool lesion_mask = true;
    float feat_rf = 1.f;                 // the last dnnca_lesion_table_features: what DNNCA_PLAN_LESION_FEATURES replays
    int feat_k = 5, feat_bins = 32, feat_ring = 3;
    bool feat_mask = true;
    // the carry plane of dnnca_lesion_table_linked: the row number (or -1) of every pixel of the last slice of the last linked
    // chunk.  A buffer of its own, not part of `ws`: it outlives every other call on the model
    int* carry = nullptr;
    size_t carry_n = 0;                  // allocated pixels
    bool carry_valid = false;            // written by a linked call that succeeded ...
    int carry_oh = 0, carry_ow = 0;      // ... on planes of this size ...
    dnnca_lesion_refine carry_refine = {0.f, 0, 0};      // ... under this mask refinement (a chain never mixes two)
    // dnnca_lesion_table_matched keeps all of this apart from the linked call's: two carry planes in one buffer (the prediction's
    // rows, then from mcarry + mcarry_n the label's rows) and what DNNCA_PLAN_LESION_MATCHED replays
    int* mcarry = nullptr;
    size_t mcarry_n = 0;                 // allocated pixels per plane
    bool mcarry_valid = false;
    int mcarry_oh = 0, mcarry_ow = 0;
    dnnca_lesion_refine mcarry_refine = {0.f, 0, 0};
    float match_rf = 1.f;
    int match_k = 5;
    bool match_mask = true;
    float surface_rf = 1.f;              // the last dnnca_surface_distances: what DNNCA_PLAN_SURFACE replays
    int surface_k = 5;
};

static constexpr size_t kRegionBudget = size_t(1) << 24;    // pixel-thresholds per chunk (~21 bytes each)
static constexpr size_t kFeatBudget = size_t(1) << 30;      // bytes of feature records per chunk (dnnca_lesion_table_features)

static size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

struct RegionWs {                        // carve-up of the workspace for nb slices of hw pixels and T thresholds
    uint32_t *wlab, *w0, *w1, *ml;
    int *ll, *lp;
    unsigned *sl, *sp, *cnt;
    unsigned char* mp;
    unsigned long long* keys;
    size_t bytes;
};

static RegionWs region_layout(void* base, size_t nb, size_t hw, size_t T) {
    const size_t n = nb * hw, cap = hw + 1;
    RegionWs w;
    char* p = (char*)base;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* r = p ? p + off : nullptr; off += align256(bytes); return (void*)r; };
    // the label plane first: its place depends on nb and hw only, so the specs of one resized size share it whatever their T
    w.wlab = (uint32_t*)take(n * 4);
    w.ll = (int*)take(n * 4);
    w.sl = (unsigned*)take(n * 4);
    w.keys = (unsigned long long*)take(T * nb * cap * 8);
    w.cnt = (unsigned*)take(T * nb * cap * 4);
    w.w0 = (uint32_t*)take(2 * n * 4);
    w.w1 = (uint32_t*)take(2 * n * 4);
    w.ml = (uint32_t*)take(2 * n * 4);
    w.lp = (int*)take(T * n * 4);
    w.sp = (unsigned*)take(T * n * 4);
    w.mp = (unsigned char*)take(T * n);
    w.bytes = off;
    return w;
}

static int fp16_scaled(int n, float rf) {
    const _Float16 a = (_Float16)(float)n, b = (_Float16)rf;
    const _Float16 c = (_Float16)(a * b);      // tf.cast(size, float16) * resize_factor: a float16 product (metrics.py:199-200)
    const float f = (float)c;
    if (!(f >= 1.f) || f > 1e9f) return 0;
    return (int)f;                             // tf.cast(..., int32) truncates
}

int region_spec_check(const dnnca_region_spec* s, int h, int w, RegionSpecHost& out) {
    if (!s) { set_error("null region spec"); return DNNCA_EINVAL; }
    if (s->n_thresholds < 1 || s->n_thresholds > kRegionMaxThr || !s->thresholds) {
        set_error("region spec: %d thresholds (1..%d)", s->n_thresholds, kRegionMaxThr);
        return DNNCA_EINVAL;
    }
    out.thr.assign(s->thresholds, s->thresholds + s->n_thresholds);
    for (int t = 0; t < s->n_thresholds; ++t)
        if (!(out.thr[t] >= 0.f)) {                // metrics.py:96 tf.debugging.assert_non_negative(thresholds); NaN too
            set_error("region spec: threshold %d is %g (must be >= 0)", t, (double)out.thr[t]);
            return DNNCA_EINVAL;
        }
    if (!(s->iou_threshold >= 0.f && s->iou_threshold < 1.f)) {
        set_error("region spec: IoU threshold %g outside [0, 1)", (double)s->iou_threshold);
        return DNNCA_EINVAL;
    }
    if (!(s->resize_factor > 0.f) || !std::isfinite(s->resize_factor)) {
        set_error("region spec: resize factor %g", (double)s->resize_factor);
        return DNNCA_EINVAL;
    }
    if (s->morph_filter_size < 1 || s->morph_filter_size > kRegionMaxK) {
        set_error("region spec: morph_filter_size %d outside 1..%d", s->morph_filter_size, kRegionMaxK);
        return DNNCA_EINVAL;
    }
    out.iou = s->iou_threshold;
    out.rf = s->resize_factor;
    out.k = s->morph_filter_size;
    out.oh = fp16_scaled(h, s->resize_factor);
    out.ow = fp16_scaled(w, s->resize_factor);
    if (out.oh < 1 || out.ow < 1) {
        set_error("region spec: resize factor %g maps %d x %d to an empty image", (double)s->resize_factor, h, w);
        return DNNCA_EINVAL;
    }
    return DNNCA_OK;
}

static int region_state(Model* M) {
    if (!M->region) M->region = new RegionState();
    return DNNCA_OK;
}

// slices per chunk: kRegionBudget pixel-thresholds, the grid z of the tile kernels (T x chunk) and int32 pixel indices
static size_t region_chunk(size_t T, size_t hw, int max_batch) {
    size_t chunk = std::max<size_t>(1, kRegionBudget / (T * hw));
    chunk = std::min(chunk, (size_t)std::max(max_batch, 1));
    chunk = std::min(chunk, (size_t)65535 / T);
    while (chunk > 1 && T * chunk * hw >= (size_t)INT32_MAX / 2) --chunk;
    return chunk;
}

// the one workspace of the region passes, grown on demand (its content is scratch between calls)
static int region_ws_reserve(RegionState& R, size_t need) {
    if (need <= R.ws_bytes) return DNNCA_OK;
    if (R.ws) HIP_TRY(hipFree(R.ws));
    R.ws = nullptr;
    R.ws_bytes = 0;
    HIP_TRY(hipMalloc(&R.ws, need));
    R.ws_bytes = need;
    return DNNCA_OK;
}

int region_prepare(Model* M, const std::vector<RegionSpecHost>& specs, int max_batch, int h, int w, int slices) {
    (void)h;
    (void)w;
    DN_TRY(region_state(M));
    RegionState& R = *M->region;
    R.specs = specs;
    R.slices = 0;
    R.order.resize(specs.size());
    for (size_t i = 0; i < specs.size(); ++i) R.order[i] = (int)i;
    std::stable_sort(R.order.begin(), R.order.end(), [&](int a, int b) {
        return std::make_pair(specs[a].oh, specs[a].ow) < std::make_pair(specs[b].oh, specs[b].ow);
    });
    size_t hw = 1, T = 1;
    for (const auto& s : specs) {
        hw = std::max(hw, (size_t)s.oh * s.ow);
        T = std::max(T, s.thr.size());
    }
    if ((size_t)T * hw * 2 >= (size_t)INT32_MAX) { set_error("region metrics: slices of %zu pixels are too large", hw); return DNNCA_EINVAL; }
    const size_t chunk = region_chunk(T, hw, max_batch);
    R.chunk = (int)chunk;
    DN_TRY(region_ws_reserve(R, region_layout(nullptr, chunk, hw, T).bytes));
    if (specs.size() > R.acc_specs) {
        if (R.acc) HIP_TRY(hipFree(R.acc));
        if (R.thr_dev) HIP_TRY(hipFree(R.thr_dev));
        R.acc = nullptr;
        R.thr_dev = nullptr;
        R.acc_specs = 0;
        HIP_TRY(hipMalloc((void**)&R.acc, specs.size() * kRegionMaxThr * 4 * 8));
        HIP_TRY(hipMalloc((void**)&R.thr_dev, specs.size() * kRegionMaxThr * 4));
        R.acc_specs = specs.size();
    }
    std::vector<float> thr(specs.size() * kRegionMaxThr, 0.f);
    for (size_t i = 0; i < specs.size(); ++i) std::copy(specs[i].thr.begin(), specs[i].thr.end(), thr.begin() + i * kRegionMaxThr);
    HIP_TRY(hipMemcpyAsync(R.thr_dev, thr.data(), thr.size() * 4, hipMemcpyHostToDevice, M->stream));
    HIP_TRY(hipMemsetAsync(R.acc, 0, specs.size() * kRegionMaxThr * 4 * 8, M->stream));
    if (slices > 0) {
        const size_t na = (size_t)slices * specs.size() * kRegionMaxThr * 4;
        if (na > R.slice_acc_n) {
            if (R.slice_acc) HIP_TRY(hipFree(R.slice_acc));
            R.slice_acc = nullptr;
            R.slice_acc_n = 0;
            HIP_TRY(hipMalloc((void**)&R.slice_acc, na * 8));
            R.slice_acc_n = na;
        }
        HIP_TRY(hipMemsetAsync(R.slice_acc, 0, na * 8, M->stream));
        R.slices = (size_t)slices;
    }
    HIP_TRY(hipStreamSynchronize(M->stream));        // `thr` is a local
    return DNNCA_OK;
}

// connected components of the T planes of `words` (nb slices of h x w) into L
void region_ccl(Model* M, const uint32_t* words, int T, int nb, int h, int w, int* L) {
    const size_t total = (size_t)T * nb * h * w;
    const dim3 tiles((w + kTile - 1) / kTile, (h + kTile - 1) / kTile, T * nb);
    LAUNCH(M, "region_ccl_tile", total * 8.0 / 32 * (T > 32 ? 2 : 1) + total * 4.0, 0,
           hipLaunchKernelGGL(k_region_ccl_tile, tiles, dim3(RB), 0, M->stream, words, nb, h, w, L));
    LAUNCH(M, "region_ccl_merge", total * 4.0, 0,
           hipLaunchKernelGGL(k_region_ccl_merge, dim3(nblocks(total)), dim3(RB), 0, M->stream, L, total, h, w));
    LAUNCH(M, "region_ccl_compress", total * 8.0, 0,
           hipLaunchKernelGGL(k_region_ccl_compress, dim3(nblocks(total)), dim3(RB), 0, M->stream, L, total));
}

// region_prep and region_open as the mask refinement launches them (refine.h): one word plane of nb slices
void region_prep_launch(Model* M, const float* src, const Resize& rz, int nb, const float* thr_dev, int T, uint32_t* words) {
    const size_t n = (size_t)nb * rz.out_h * rz.out_w;
    LAUNCH(M, "region_prep", n * 4.0 + (double)nb * rz.in_h * rz.in_w * 4, 0,
           hipLaunchKernelGGL(k_region_prep, dim3(nblocks(n)), dim3(RB), 0, M->stream, src, rz, nb, thr_dev, T, words));
}

void region_open_launch(Model* M, const uint32_t* in, uint32_t* out, int oh, int ow, int k, int nb) {
    const size_t n = (size_t)nb * oh * ow;
    const dim3 tiles((ow + kTile - 1) / kTile, (oh + kTile - 1) / kTile, nb);
    LAUNCH(M, "region_open", n * 8.0, 0, hipLaunchKernelGGL(k_region_open, tiles, dim3(RB), 0, M->stream, in, out, oh, ow, k, n, nb));
}

int region_accumulate(Model* M, const float* prob, const float* y, int batch, int h, int w, bool per_slice) {
    if (!M->region || M->region->specs.empty()) { set_error("region metrics: no specs prepared"); return DNNCA_ESTATE; }
    RegionState& R = *M->region;
    if (per_slice && (size_t)batch > R.slices) { set_error("region metrics: %d slices, %zu prepared", batch, R.slices); return DNNCA_ESTATE; }
    const size_t acc_slice = R.specs.size() * kRegionMaxThr * 4;       // per-slice accumulator stride
    hipStream_t s = M->stream;
    for (int b0 = 0; b0 < batch; b0 += R.chunk) {
        const int nb = std::min(R.chunk, batch - b0);
        const float* pb = prob + (size_t)b0 * h * w;
        const float* yb = y + (size_t)b0 * h * w;
        int lab_h = 0, lab_w = 0;
        for (int si : R.order) {
            const RegionSpecHost& sp = R.specs[si];
            const int T = (int)sp.thr.size(), oh = sp.oh, ow = sp.ow;
            const size_t hw = (size_t)oh * ow, n = (size_t)nb * hw, cap = hw + 1, slots = (size_t)T * nb * cap;
            const RegionWs ws = region_layout(R.ws, nb, hw, T);
            Resize rz{h, w, oh, ow, (float)h / (float)oh, (float)w / (float)ow, (oh == h && ow == w) ? 1 : 0};
            if (oh != lab_h || ow != lab_w) {              // the label plane of this size: once for every spec that shares it
                LAUNCH(M, "region_prep", n * 4.0 + (double)nb * h * w * 4, 0,
                       hipLaunchKernelGGL(k_region_prep, dim3(nblocks(n)), dim3(RB), 0, s, yb, rz, nb, (const float*)nullptr, 0, ws.wlab));
                region_ccl(M, ws.wlab, 1, nb, oh, ow, ws.ll);
                HIP_TRY(hipMemsetAsync(ws.sl, 0, n * 4, s));
                LAUNCH(M, "region_sizes", n * 4.0, 0,
                       hipLaunchKernelGGL(k_region_sizes, dim3(nblocks(n)), dim3(RB), 0, s, ws.ll, n, ws.sl));
                lab_h = oh;
                lab_w = ow;
            }
            const int nw = T > 32 ? 2 : 1;
            LAUNCH(M, "region_prep", n * 4.0 * nw + (double)nb * h * w * 4, 0,
                   hipLaunchKernelGGL(k_region_prep, dim3(nblocks(n)), dim3(RB), 0, s, pb, rz, nb, R.thr_dev + (size_t)si * kRegionMaxThr,
                                      T, ws.w0));
            const uint32_t* mask = ws.w0;
            if (sp.k > 1) {
                const dim3 tiles((ow + kTile - 1) / kTile, (oh + kTile - 1) / kTile, nw * nb);
                LAUNCH(M, "region_open", n * 8.0 * nw, 0,
                       hipLaunchKernelGGL(k_region_open, tiles, dim3(RB), 0, s, ws.w0, ws.w1, oh, ow, sp.k, n, nb));
                mask = ws.w1;
            }
            region_ccl(M, mask, T, nb, oh, ow, ws.lp);
            HIP_TRY(hipMemsetAsync(ws.sp, 0, (size_t)T * n * 4, s));
            LAUNCH(M, "region_sizes", (double)T * n * 4, 0,
                   hipLaunchKernelGGL(k_region_sizes, dim3(nblocks((size_t)T * n)), dim3(RB), 0, s, ws.lp, (size_t)T * n, ws.sp));
            HIP_TRY(hipMemsetAsync(ws.keys, 0xff, slots * 8, s));
            HIP_TRY(hipMemsetAsync(ws.cnt, 0, slots * 4, s));
            HIP_TRY(hipMemsetAsync(ws.ml, 0, (size_t)nw * n * 4, s));
            HIP_TRY(hipMemsetAsync(ws.mp, 0, (size_t)T * n, s));
            LAUNCH(M, "region_pairs", (double)T * n * 4 + n * 4.0, 0,
                   hipLaunchKernelGGL(k_region_pairs, dim3(nblocks((size_t)T * n)), dim3(RB), 0, s, ws.ll, ws.lp, T, nb, hw, cap, ws.keys,
                                      ws.cnt));
            LAUNCH(M, "region_match", slots * 12.0, 0,
                   hipLaunchKernelGGL(k_region_match, dim3(nblocks(slots)), dim3(RB), 0, s, ws.keys, ws.cnt, slots, cap, nb, hw, ws.sl,
                                      ws.sp, sp.iou, ws.ml, ws.mp));
            if (per_slice) {               // one z block row per slice, the counts of slice b0 + z into its own accumulator
                unsigned cb = nblocks(hw);
                if (cb > 32) cb = 32;
                LAUNCH(M, "region_count_slices", (double)T * n * 5 + n * 8.0, 0,
                       hipLaunchKernelGGL(k_region_count, dim3(cb, T, nb), dim3(RB), 0, s, ws.ll, ws.lp, ws.ml, ws.mp, n, hw, acc_slice,
                                          R.slice_acc + (size_t)b0 * acc_slice + (size_t)si * kRegionMaxThr * 4));
            } else {
                unsigned cb = nblocks(n);
                if (cb > 256) cb = 256;
                LAUNCH(M, "region_count", (double)T * n * 5 + n * 8.0, 0,
                       hipLaunchKernelGGL(k_region_count, dim3(cb, T), dim3(RB), 0, s, ws.ll, ws.lp, ws.ml, ws.mp, n, n, (size_t)0,
                                          R.acc + (size_t)si * kRegionMaxThr * 4));
            }
        }
    }
    HIP_TRY(hipGetLastError());
    return DNNCA_OK;
}

int region_read(Model* M, std::vector<std::vector<dnnca_region_counts>>& counts) {
    if (!M->region) { set_error("region metrics: no specs prepared"); return DNNCA_ESTATE; }
    RegionState& R = *M->region;
    std::vector<unsigned long long> h(R.specs.size() * kRegionMaxThr * 4);
    HIP_TRY(hipMemcpyAsync(h.data(), R.acc, h.size() * 8, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    counts.assign(R.specs.size(), {});
    for (size_t i = 0; i < R.specs.size(); ++i) {
        for (size_t t = 0; t < R.specs[i].thr.size(); ++t) {
            const unsigned long long* a = &h[(i * kRegionMaxThr + t) * 4];
            counts[i].push_back(dnnca_region_counts{(int64_t)a[0], (int64_t)a[1], (int64_t)a[2], (int64_t)a[3]});
        }
    }
    return DNNCA_OK;
}

int region_read_slices(Model* M, int batch, dnnca_region_counts* out) {
    if (!M->region || (size_t)batch > M->region->slices) { set_error("region metrics: no per-slice counts prepared"); return DNNCA_ESTATE; }
    RegionState& R = *M->region;
    const size_t ns = R.specs.size();
    std::vector<unsigned long long> h((size_t)batch * ns * kRegionMaxThr * 4);
    HIP_TRY(hipMemcpyAsync(h.data(), R.slice_acc, h.size() * 8, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    for (int b = 0; b < batch; ++b)
        for (size_t i = 0; i < ns; ++i)
            for (size_t t = 0; t < R.specs[i].thr.size(); ++t) {
                const unsigned long long* a = &h[(((size_t)b * ns + i) * kRegionMaxThr + t) * 4];
                *out++ = dnnca_region_counts{(int64_t)a[0], (int64_t)a[1], (int64_t)a[2], (int64_t)a[3]};
            }
    return DNNCA_OK;
}

int region_inputs(Model* M, size_t n, float** prob_dev, float** y_dev) {
    DN_TRY(region_state(M));
    RegionState& R = *M->region;
    R.label_batch = 0;
    if (n > R.in_n) {
        if (R.in_prob) HIP_TRY(hipFree(R.in_prob));
        if (R.in_y) HIP_TRY(hipFree(R.in_y));
        R.in_prob = R.in_y = nullptr;
        R.in_n = 0;
        HIP_TRY(hipMalloc((void**)&R.in_prob, n * 4));
        HIP_TRY(hipMalloc((void**)&R.in_y, n * 4));
        R.in_n = n;
    }
    *prob_dev = R.in_prob;
    *y_dev = R.in_y;
    return DNNCA_OK;
}

void region_set_label_batch(Model* M, int batch) {
    if (M->region) M->region->label_batch = batch;
}

const float* region_label_of(Model* M, int batch) {
    return M->region && batch > 0 && M->region->label_batch == batch ? M->region->in_y : nullptr;
}

int region_render(Model* M, const float* x, const float* lab, const float* prob, int batch, int h, int w, int c, float ratio,
                  int overlay, unsigned char* out, size_t capacity, int* out_hwc) {
    if (!(ratio > 0.f) || !std::isfinite(ratio)) { set_error("render: ratio %g", (double)ratio); return DNNCA_EINVAL; }
    Composite g;
    g.H = h;
    g.W = w;
    g.C = c;
    g.Wc = w * (c + 2);
    const float fh = (float)h * ratio, fw = (float)g.Wc * ratio;   // tf.cast(tf.cast(shape, float32) * ratio, int32)
    if (!(fh >= 1.f && fw >= 1.f) || fh > 65536.f || fw > 65536.f) {
        set_error("render: ratio %g maps %d x %d to %g x %g", (double)ratio, h, g.Wc, (double)fh, (double)fw);
        return DNNCA_EINVAL;
    }
    g.oh = (int)fh;
    g.ow = (int)fw;
    g.nch = overlay ? 3 : 1;
    g.sy = (float)g.H / (float)g.oh;
    g.sx = (float)g.Wc / (float)g.ow;
    out_hwc[0] = g.oh;
    out_hwc[1] = g.ow;
    out_hwc[2] = g.nch;
    const size_t total = (size_t)batch * g.oh * g.ow * g.nch;
    if (!out) return DNNCA_OK;                    // size query
    if (capacity < total) { set_error("render: %zu bytes needed, capacity %zu", total, capacity); return DNNCA_EINVAL; }
    DN_TRY(region_state(M));
    RegionState& R = *M->region;
    const size_t words = (total + 3) / 4;
    if (words * 4 > R.viz_bytes) {
        if (R.viz) HIP_TRY(hipFree(R.viz));
        R.viz = nullptr;
        R.viz_bytes = 0;
        HIP_TRY(hipMalloc((void**)&R.viz, words * 4));
        R.viz_bytes = words * 4;
    }
    LAUNCH(M, "region_render", (double)total + (double)batch * h * w * (c + 2) * 4, (double)total * 8,
           hipLaunchKernelGGL(k_region_render, dim3(nblocks(words)), dim3(RB), 0, M->stream, x, lab, prob, g, batch, R.viz));
    HIP_TRY(hipMemcpyAsync(out, R.viz, total, hipMemcpyDeviceToHost, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    return DNNCA_OK;
}

// ---- lesion table ----------------------------------------------------------------------------------------------------------
struct LesionWs {                        // carve-up of the workspace for nb slices of hw pixels and `cap` rows per slice
    uint32_t *w0, *w1, *mask;
    int *lp, *row, *tot;
    unsigned* sp;
    float* thr;                          // the one threshold (region_prep reads its thresholds from the device)
    LesionAcc* acc;
    // linked calls only, behind everything else: per-slice pair tables of hw + 1 slots, the chunk's flags, the link list
    unsigned long long* lkeys;
    unsigned* lcnt;
    unsigned char* cont;
    LesionLink* list;
    unsigned* n_list;
    // matched calls only: the label plane's own words, parents, sizes, rows, totals, threshold and table.  Their lkeys / lcnt hold
    // three sets of tables, list three lists of nb * links_per_slice entries and n_list three counts (lesion_match)
    uint32_t* yw;
    int *ylp, *yrow, *ytot;
    unsigned* ysp;
    float* ythr;
    LesionAcc* yacc;
    // spread calls only, behind everything else: the spread rows beside acc and the slices' totals
    SpreadAcc *sacc, *stot;
    // feature calls only, behind everything else: shape, body and ring records beside acc, the histograms [row][channel][bins]
    FeatShapeAcc* fshape;
    FeatAcc *fbody, *fring;
    unsigned* fhist;
    size_t bytes;
};

struct LesionFeatIO {                    // what a feature call adds: the channels (device [batch, h, w, channels]) and the host outputs
    const float* x;
    int channels, bins, ring;
    dnnca_lesion_shape* shape;
    dnnca_lesion_intensity *body, *ring_out;
    uint32_t* hist;
    // the feature records of one slice (cap rows) in the workspace
    size_t slice_bytes(size_t cap) const {
        return cap * (sizeof(FeatShapeAcc) + (size_t)channels * ((ring ? 2 : 1) * sizeof(FeatAcc) + (size_t)bins * 4));
    }
};

static LesionWs lesion_layout(void* base, size_t nb, size_t hw, size_t cap, size_t links_per_slice = 0, bool matched = false,
                              bool spread = false, const LesionFeatIO* ft = nullptr) {
    const size_t n = nb * hw;
    LesionWs w;
    char* p = (char*)base;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* r = p ? p + off : nullptr; off += align256(bytes); return (void*)r; };
    w.w0 = (uint32_t*)take(n * 4);
    w.w1 = (uint32_t*)take(n * 4);
    w.lp = (int*)take(n * 4);
    w.sp = (unsigned*)take(n * 4);
    w.row = (int*)take(n * 4);
    w.tot = (int*)take(nb * 4);
    w.thr = (float*)take(2 * 4);         // (two with the hysteresis of the mask refinement; a piece is 256 bytes at least)
    w.acc = (LesionAcc*)take(nb * cap * sizeof(LesionAcc));
    w.mask = (uint32_t*)take((n + 3) / 4 * 4);
    w.lkeys = nullptr, w.lcnt = nullptr, w.cont = nullptr, w.list = nullptr, w.n_list = nullptr;
    if (links_per_slice) {
        const size_t sets = matched ? 3 : 1;
        w.lkeys = (unsigned long long*)take(sets * nb * (hw + 1) * 8);
        w.lcnt = (unsigned*)take(sets * nb * (hw + 1) * 4);
        w.cont = (unsigned char*)take(nb);
        w.list = (LesionLink*)take(sets * nb * links_per_slice * sizeof(LesionLink));
        w.n_list = (unsigned*)take(sets * 4);
    }
    w.yw = nullptr, w.ylp = nullptr, w.yrow = nullptr, w.ytot = nullptr, w.ysp = nullptr, w.ythr = nullptr, w.yacc = nullptr;
    if (matched) {
        w.yw = (uint32_t*)take(n * 4);
        w.ylp = (int*)take(n * 4);
        w.ysp = (unsigned*)take(n * 4);
        w.yrow = (int*)take(n * 4);
        w.ytot = (int*)take(nb * 4);
        w.ythr = (float*)take(4);
        w.yacc = (LesionAcc*)take(nb * cap * sizeof(LesionAcc));
    }
    w.sacc = nullptr, w.stot = nullptr;
    if (spread) {
        w.sacc = (SpreadAcc*)take(nb * cap * sizeof(SpreadAcc));
        w.stot = (SpreadAcc*)take(nb * sizeof(SpreadAcc));
    }
    w.fshape = nullptr, w.fbody = nullptr, w.fring = nullptr, w.fhist = nullptr;
    if (ft) {
        const size_t rc = nb * cap * ft->channels;
        w.fshape = (FeatShapeAcc*)take(nb * cap * sizeof(FeatShapeAcc));
        w.fbody = (FeatAcc*)take(rc * sizeof(FeatAcc));
        if (ft->ring) w.fring = (FeatAcc*)take(rc * sizeof(FeatAcc));
        if (ft->bins) w.fhist = (unsigned*)take(rc * ft->bins * 4);
    }
    w.bytes = off;
    return w;
}

int lesion_check(LesionArgs& a, int h, int w) {
    if (h < 1 || w < 1) { set_error("lesion table: slices of %d x %d", h, w); return DNNCA_EINVAL; }
    if (!(a.threshold >= 0.f)) { set_error("lesion table: threshold %g (must be >= 0)", (double)a.threshold); return DNNCA_EINVAL; }
    if (!(a.rf > 0.f) || !std::isfinite(a.rf)) { set_error("lesion table: resize factor %g", (double)a.rf); return DNNCA_EINVAL; }
    if (a.k < 1 || a.k > kRegionMaxK) { set_error("lesion table: filter_size %d outside 1..%d", a.k, kRegionMaxK); return DNNCA_EINVAL; }
    if (a.min_area < 0) { set_error("lesion table: min_area %d (must be >= 0)", a.min_area); return DNNCA_EINVAL; }
    if (a.max_lesions < 1) { set_error("lesion table: max_lesions %d (must be >= 1)", a.max_lesions); return DNNCA_EINVAL; }
    a.oh = fp16_scaled(h, a.rf);
    a.ow = fp16_scaled(w, a.rf);
    if (a.oh < 1 || a.ow < 1) {
        set_error("lesion table: resize factor %g maps %d x %d to an empty image", (double)a.rf, h, w);
        return DNNCA_EINVAL;
    }
    const size_t hw = (size_t)a.oh * a.ow;
    if (hw * 2 >= (size_t)INT32_MAX) { set_error("lesion table: slices of %zu pixels are too large", hw); return DNNCA_EINVAL; }
    a.cap = (int)std::min<size_t>((size_t)a.max_lesions, (hw + 1) / 2);      // 4-connected components of hw pixels: at most ceil(hw / 2)
    return DNNCA_OK;
}

struct LesionLinkIO {                    // what a linked call adds to the chunk loop (host pointers)
    const uint8_t* continues;
    dnnca_lesion_link* links;
    int64_t* n_links;
};

struct LesionMatchIO {                   // what a matched call adds to a linked one: the labels (device) and the host outputs
    const float* y;
    dnnca_lesion_row* rows;
    int64_t* n_rows;
    int32_t* totals;
    dnnca_lesion_link* links;
    int64_t* n_links;
    dnnca_lesion_pair* pairs;
    int64_t* n_pairs;
};

struct LesionSpreadIO {                  // what a spread call adds: the spread plane (device [batch, h, w]) and the host outputs
    const float* spread;
    dnnca_lesion_spread* srows;
    dnnca_slice_spread* stotals;
};

static_assert(sizeof(LesionLink) == sizeof(dnnca_lesion_pair), "the device list is copied into the caller's records");

// label' > 0.5 as a >= threshold of region_prep (T = 1): the float32 after 0.5
static const float kLabelThreshold = nextafterf(0.5f, 1.f);

// one plane of nb slices from its thresholded words to its numbered components and their table: ccl, sizes, lesion_scan,
// lesion_stats (`src`: what was thresholded)
static int lesion_plane(Model* M, const float* src, const Resize& rz, int nb, const uint32_t* fg, int min_area, size_t cap, int* lp,
                        unsigned* sp, int* row, int* tot, LesionAcc* acc) {
    hipStream_t s = M->stream;
    const size_t hw = (size_t)rz.out_h * rz.out_w, n = (size_t)nb * hw;
    region_ccl(M, fg, 1, nb, rz.out_h, rz.out_w, lp);
    if (!M->dry) {
        HIP_TRY(hipMemsetAsync(sp, 0, n * 4, s));
        HIP_TRY(hipMemsetAsync(acc, 0, (size_t)nb * cap * sizeof(LesionAcc), s));
    }
    LAUNCH(M, "region_sizes", n * 4.0, 0, hipLaunchKernelGGL(k_region_sizes, dim3(nblocks(n)), dim3(RB), 0, s, lp, n, sp));
    LAUNCH(M, "lesion_scan", n * 12.0, 0,
           hipLaunchKernelGGL(k_lesion_scan, dim3(nb), dim3(RB), 0, s, lp, sp, (int)hw, (unsigned)min_area, row, tot));
    LAUNCH(M, "lesion_stats", n * 8.0 + (double)nb * rz.in_h * rz.in_w * 4, 0,
           hipLaunchKernelGGL(k_lesion_stats, dim3(nblocks(n)), dim3(RB), 0, s, src, rz, nb, lp, row, (int)cap, acc));
    return DNNCA_OK;
}

// the rows that the slices of a chunk filled (tot: their kept components, already on the host) from the device table to the
// caller's records; synchronises
static int lesion_rows_read(Model* M, const LesionAcc* acc_dev, const std::vector<int>& tot, int b0, size_t cap, std::vector<LesionAcc>& acc,
                            dnnca_lesion_row* rows, int64_t& out, int32_t* totals) {
    hipStream_t s = M->stream;
    const int nb = (int)tot.size();
    std::vector<size_t> first(nb + 1, 0);         // only the rows a slice filled come back
    for (int b = 0; b < nb; ++b) first[b + 1] = first[b] + std::min<size_t>((size_t)std::max(tot[b], 0), cap);
    acc.resize(first[nb]);
    for (int b = 0; b < nb; ++b)
        if (first[b + 1] > first[b])
            HIP_TRY(hipMemcpyAsync(acc.data() + first[b], acc_dev + (size_t)b * cap, (first[b + 1] - first[b]) * sizeof(LesionAcc),
                                   hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < nb; ++b) {
        totals[b0 + b] = tot[b];
        for (size_t r = 0; r < first[b + 1] - first[b]; ++r) {
            const LesionAcc& v = acc[first[b] + r];
            dnnca_lesion_row& o = rows[out++];
            o.slice = b0 + b;
            o.row = (int32_t)r;
            o.area = (int32_t)v.area;
            o.x0 = (int32_t)~v.nx0;
            o.y0 = (int32_t)~v.ny0;
            o.x1 = (int32_t)v.x1;
            o.y1 = (int32_t)v.y1;
            memcpy(&o.max_prob, &v.mp, 4);
            o.sum_x = v.sx;
            o.sum_y = v.sy;
            o.sum_prob_q24 = v.sq;
        }
    }
    return DNNCA_OK;
}

// the spread rows beside the rows that lesion_rows_read has just delivered (srows: the record of the chunk's first row) and the
// slices' totals; synchronises
static int lesion_spread_read(Model* M, const SpreadAcc* sacc_dev, const SpreadAcc* stot_dev, const std::vector<int>& tot, int b0, size_t cap,
                              dnnca_lesion_spread* srows, dnnca_slice_spread* stotals) {
    hipStream_t s = M->stream;
    const int nb = (int)tot.size();
    std::vector<size_t> first(nb + 1, 0);
    for (int b = 0; b < nb; ++b) first[b + 1] = first[b] + std::min<size_t>((size_t)std::max(tot[b], 0), cap);
    std::vector<SpreadAcc> acc(first[nb] + nb);          // the rows, then the totals
    for (int b = 0; b < nb; ++b)
        if (first[b + 1] > first[b])
            HIP_TRY(hipMemcpyAsync(acc.data() + first[b], sacc_dev + (size_t)b * cap, (first[b + 1] - first[b]) * sizeof(SpreadAcc),
                                   hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(acc.data() + first[nb], stot_dev, (size_t)nb * sizeof(SpreadAcc), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < nb; ++b) {
        for (size_t r = first[b]; r < first[b + 1]; ++r) {
            dnnca_lesion_spread& o = srows[r];
            o.slice = b0 + b;
            o.row = (int32_t)(r - first[b]);
            o.area = (int32_t)acc[r].area;
            memcpy(&o.max_spread, &acc[r].mx, 4);
            o.sum_spread_q24 = acc[r].sq;
        }
        const SpreadAcc& t = acc[first[nb] + b];
        dnnca_slice_spread& o = stotals[b0 + b];
        o.pixels = (int32_t)t.area;
        memcpy(&o.max_spread, &t.mx, 4);
        o.sum_spread_q24 = t.sq;
    }
    return DNNCA_OK;
}

static void feat_record(dnnca_lesion_intensity& o, const FeatAcc& v, int slice, int row, int channel) {
    const unsigned mn = v.n ? ~v.nmn : 0u, mx = v.n ? v.mx : 0u;      // no pixel (an empty ring): min = max = 0
    o.slice = slice, o.row = row, o.channel = channel, o.n = (int32_t)v.n;
    memcpy(&o.min, &mn, 4);
    memcpy(&o.max, &mx, 4);
    o.sum_q16 = v.sq, o.sum_sq_q16 = v.ssq;
}

// the feature records beside the rows that lesion_rows_read has just delivered (`first_row`: the chunk's first row in the caller's
// buffers); synchronises
static int lesion_feat_read(Model* M, const LesionWs& ws, const std::vector<int>& tot, int b0, size_t cap, const LesionFeatIO& ft,
                            int64_t first_row) {
    hipStream_t s = M->stream;
    const int nb = (int)tot.size();
    const size_t C = (size_t)ft.channels, bins = (size_t)ft.bins;
    std::vector<size_t> first(nb + 1, 0);
    for (int b = 0; b < nb; ++b) first[b + 1] = first[b] + std::min<size_t>((size_t)std::max(tot[b], 0), cap);
    std::vector<FeatShapeAcc> sh(first[nb]);
    std::vector<FeatAcc> bd(first[nb] * C), rg(ft.ring ? first[nb] * C : 0);
    for (int b = 0; b < nb; ++b) {
        const size_t cnt = first[b + 1] - first[b], at = first[b], dev = (size_t)b * cap;
        if (!cnt) continue;
        HIP_TRY(hipMemcpyAsync(sh.data() + at, ws.fshape + dev, cnt * sizeof(FeatShapeAcc), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(bd.data() + at * C, ws.fbody + dev * C, cnt * C * sizeof(FeatAcc), hipMemcpyDeviceToHost, s));
        if (ft.ring) HIP_TRY(hipMemcpyAsync(rg.data() + at * C, ws.fring + dev * C, cnt * C * sizeof(FeatAcc), hipMemcpyDeviceToHost, s));
        if (bins)                        // histograms are plain counts: straight into the caller's buffer
            HIP_TRY(hipMemcpyAsync(ft.hist + ((size_t)first_row + at) * C * bins, ws.fhist + dev * C * bins, cnt * C * bins * 4,
                                   hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < nb; ++b)
        for (size_t r = first[b]; r < first[b + 1]; ++r) {
            const int slice = b0 + b, rw = (int)(r - first[b]);
            const FeatShapeAcc& v = sh[r];
            dnnca_lesion_shape& o = ft.shape[first_row + r];
            o.slice = slice, o.row = rw, o.area = (int32_t)v.area, o.boundary = (int32_t)v.boundary, o.edges = (int32_t)v.edges;
            o.reserved = 0;
            o.sum_xx = v.sxx, o.sum_yy = v.syy, o.sum_xy = v.sxy;
            for (size_t c = 0; c < C; ++c) {
                feat_record(ft.body[((size_t)first_row + r) * C + c], bd[r * C + c], slice, rw, (int)c);
                if (ft.ring) feat_record(ft.ring_out[((size_t)first_row + r) * C + c], rg[r * C + c], slice, rw, (int)c);
            }
        }
    return DNNCA_OK;
}

// the chunk loop of lesion_table, lesion_table_linked (link != nullptr: the three link launches behind every chunk's table) and
// lesion_table_matched (link and match: the label plane's table as well, then lesion_match / lesion_link_emit over the three
// sets of tables / lesion_match_carry in the place of the link launches).  A matched chunk holds two planes and three sets of
// tables and lists: its slices are a third of a linked chunk's (region_chunk with T = 3), which changes no result
static int lesion_run(Model* M, const float* prob, int batch, int h, int w, const LesionArgs& a, dnnca_lesion_row* rows, int64_t* n_rows,
                      int32_t* totals, uint8_t* mask, bool want_mask, const LesionLinkIO* link, const LesionMatchIO* match = nullptr,
                      const LesionSpreadIO* sp = nullptr, const LesionFeatIO* ft = nullptr) {
    DN_TRY(region_state(M));
    RegionState& R = *M->region;
    if (ft) {
        R.feat_rf = a.rf;
        R.feat_k = a.k;
        R.feat_mask = want_mask;
        R.feat_bins = ft->bins;
        R.feat_ring = ft->ring;
    } else if (match) {
        R.match_rf = a.rf;
        R.match_k = a.k;
        R.match_mask = want_mask;
    } else {
        R.lesion_rf = a.rf;
        R.lesion_k = a.k;
        R.lesion_mask = want_mask;
    }
    const int oh = a.oh, ow = a.ow;
    const size_t hw = (size_t)oh * ow, cap = (size_t)a.cap, slots = hw + 1;
    const size_t per_slice = link ? (size_t)a.links_per_slice() : 0;
    const int sets = match ? 3 : 1;
    int chunk = (int)region_chunk(match ? 3 : 1, hw, batch);
    if (ft) chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)chunk, kFeatBudget / ft->slice_bytes(cap)));
    if (!M->dry)
        DN_TRY(region_ws_reserve(R, lesion_layout(nullptr, chunk, hw, cap, per_slice, match != nullptr, sp != nullptr, ft).bytes));
    if (link && !match && !M->dry) {     // from here on the carry is this call's: valid again once every chunk has gone through
        R.carry_valid = false;
        if (hw > R.carry_n) {            // (a set continues[0] was checked against a carry of this size: that one is never regrown)
            if (R.carry) HIP_TRY(hipFree(R.carry));
            R.carry = nullptr;
            R.carry_n = 0;
            HIP_TRY(hipMalloc((void**)&R.carry, hw * 4));
            R.carry_n = hw;
        }
    }
    if (match && !M->dry) {              // the same for the two carry planes of the matched calls
        R.mcarry_valid = false;
        if (hw > R.mcarry_n) {
            if (R.mcarry) HIP_TRY(hipFree(R.mcarry));
            R.mcarry = nullptr;
            R.mcarry_n = 0;
            HIP_TRY(hipMalloc((void**)&R.mcarry, 2 * hw * 4));
            R.mcarry_n = hw;
        }
    }
    int* const carry_t = R.mcarry ? R.mcarry + R.mcarry_n : nullptr;
    hipStream_t s = M->stream;
    std::vector<LesionAcc> acc;
    std::vector<int> tot, ytot;
    std::vector<LesionLink> found[3];
    int64_t out = 0, out_true = 0, out_list[3] = {0, 0, 0};
    Resize rz{h, w, oh, ow, (float)h / (float)oh, (float)w / (float)ow, (oh == h && ow == w) ? 1 : 0};
    const bool refine = refine_on(M->refine);
    const float refine_thr[2] = {M->refine.hysteresis_low, a.threshold};     // outlives every chunk's sync
    for (int b0 = 0; b0 < batch; b0 += chunk) {
        const int nb = std::min(chunk, batch - b0);
        const size_t n = (size_t)nb * hw;
        const LesionWs ws = lesion_layout(R.ws, nb, hw, cap, per_slice, match != nullptr, sp != nullptr, ft);
        const float* pb = prob + (size_t)b0 * h * w;
        const float* yb = match ? match->y + (size_t)b0 * h * w : nullptr;
        if (!refine && !M->dry) HIP_TRY(hipMemcpyAsync(ws.thr, &a.threshold, 4, hipMemcpyHostToDevice, s));   // `a` outlives the chunk's sync
        if (link && !M->dry) HIP_TRY(hipMemcpyAsync(ws.cont, link->continues + b0, (size_t)nb, hipMemcpyHostToDevice, s));
        const uint32_t* fg = ws.w0;
        if (refine) {                    // the refined mask in the place of prep / open; lp and sp are written only behind it
            DN_TRY(refine_chunk(M, M->refine, pb, rz, nb, refine_thr, a.k, RefineWs{ws.w0, ws.w1, ws.lp, ws.sp, ws.thr}, &fg));
        } else {
            region_prep_launch(M, pb, rz, nb, ws.thr, 1, ws.w0);
            if (a.k > 1) {
                region_open_launch(M, ws.w0, ws.w1, oh, ow, a.k, nb);
                fg = ws.w1;
            }
        }
        DN_TRY(lesion_plane(M, pb, rz, nb, fg, a.min_area, cap, ws.lp, ws.sp, ws.row, ws.tot, ws.acc));
        if (want_mask)
            LAUNCH(M, "lesion_mask", n * 9.0, 0,
                   hipLaunchKernelGGL(k_lesion_mask, dim3(nblocks((n + 3) / 4)), dim3(RB), 0, s, ws.lp, ws.row, n, ws.mask));
        if (sp) {                        // the spread plane under the prediction plane's rows
            if (!M->dry) {
                HIP_TRY(hipMemsetAsync(ws.sacc, 0, (size_t)nb * cap * sizeof(SpreadAcc), s));
                HIP_TRY(hipMemsetAsync(ws.stot, 0, (size_t)nb * sizeof(SpreadAcc), s));
            }
            const dim3 grid((unsigned)((hw + RB * kSpreadU - 1) / (RB * kSpreadU)), nb);
            LAUNCH(M, "lesion_spread", n * 8.0 + (double)nb * h * w * 4, 0,
                   hipLaunchKernelGGL(k_lesion_spread, grid, dim3(RB), 0, s, sp->spread + (size_t)b0 * h * w, rz, ws.lp, ws.row, (int)cap,
                                      ws.sacc, ws.stot));
        }
        if (ft) {                        // the input channels under the prediction plane's rows, and around them
            const size_t rc = (size_t)nb * cap * ft->channels;
            const float* xb = ft->x + (size_t)b0 * h * w * ft->channels;
            if (!M->dry) {
                HIP_TRY(hipMemsetAsync(ws.fshape, 0, (size_t)nb * cap * sizeof(FeatShapeAcc), s));
                HIP_TRY(hipMemsetAsync(ws.fbody, 0, rc * sizeof(FeatAcc), s));
                if (ft->ring) HIP_TRY(hipMemsetAsync(ws.fring, 0, rc * sizeof(FeatAcc), s));
                if (ft->bins) HIP_TRY(hipMemsetAsync(ws.fhist, 0, rc * ft->bins * 4, s));
            }
            const dim3 grid((unsigned)((hw + RB * kFeatU - 1) / (RB * kFeatU)), nb);
            LAUNCH(M, "lesion_features", n * 8.0, 0,
                   hipLaunchKernelGGL(k_lesion_features, grid, dim3(RB), (size_t)ft->channels * ft->bins * 4, s, xb, rz, ft->channels, ft->bins, ws.lp, ws.row, (int)cap,
                                      ws.fshape, ws.fbody, ws.fhist));
            if (ft->ring) {
                const dim3 tiles((ow + kTile - 1) / kTile, (oh + kTile - 1) / kTile, nb);
                LAUNCH(M, "lesion_ring", n * 8.0, 0,
                       hipLaunchKernelGGL(k_lesion_ring, tiles, dim3(RB), 0, s, xb, rz, ft->channels, ft->ring, ws.lp, ws.row, (int)cap,
                                          ws.fring));
            }
        }
        if (match) {                     // the label plane: label' > 0.5, no opening, no area filter
            if (!M->dry) HIP_TRY(hipMemcpyAsync(ws.ythr, &kLabelThreshold, 4, hipMemcpyHostToDevice, s));
            LAUNCH(M, "region_prep", n * 4.0 + (double)nb * h * w * 4, 0,
                   hipLaunchKernelGGL(k_region_prep, dim3(nblocks(n)), dim3(RB), 0, s, yb, rz, nb, (const float*)ws.ythr, 1, ws.yw));
            DN_TRY(lesion_plane(M, yb, rz, nb, ws.yw, 0, cap, ws.ylp, ws.ysp, ws.yrow, ws.ytot, ws.yacc));
        }
        if (link) {                      // on every chunk, whatever the flags say: they are device data
            const size_t total = (size_t)nb * slots, list_cap = (size_t)nb * per_slice;
            if (!M->dry) {
                HIP_TRY(hipMemsetAsync(ws.lkeys, 0xff, sets * total * 8, s));
                HIP_TRY(hipMemsetAsync(ws.lcnt, 0, sets * total * 4, s));
                HIP_TRY(hipMemsetAsync(ws.n_list, 0, sets * 4, s));
            }
            if (match)
                LAUNCH(M, "lesion_match", n * 32.0 + (double)nb, 0,
                       hipLaunchKernelGGL(k_lesion_match, dim3(nblocks(n)), dim3(RB), 0, s, ws.lp, ws.row, ws.ylp, ws.yrow,
                                          (const int*)R.mcarry, (const int*)carry_t, ws.cont, nb, hw, (int)cap, slots, ws.lkeys, ws.lcnt));
            else
                LAUNCH(M, "lesion_link", n * 16.0 + (double)nb, 0,
                       hipLaunchKernelGGL(k_lesion_link, dim3(nblocks(n)), dim3(RB), 0, s, ws.lp, ws.row, (const int*)R.carry, ws.cont, nb,
                                          hw, (int)cap, slots, ws.lkeys, ws.lcnt));
            LAUNCH(M, "lesion_link_emit", sets * total * 12.0, 0,
                   hipLaunchKernelGGL(k_lesion_link_emit, dim3(nblocks(total), sets), dim3(RB), 0, s, ws.lkeys, ws.lcnt, total, slots, b0,
                                      (unsigned)list_cap, ws.list, ws.n_list));
            // after lesion_link / lesion_match on the same stream: that kernel of this chunk has read the carry of the chunk before
            if (match)
                LAUNCH(M, "lesion_match_carry", hw * 24.0, 0,
                       hipLaunchKernelGGL(k_lesion_match_carry, dim3(nblocks(hw), 2), dim3(RB), 0, s, ws.lp, ws.row, ws.ylp, ws.yrow,
                                          (size_t)(nb - 1) * hw, hw, (int)cap, R.mcarry, carry_t));
            else
                LAUNCH(M, "lesion_carry", hw * 12.0, 0,
                       hipLaunchKernelGGL(k_lesion_carry, dim3(nblocks(hw)), dim3(RB), 0, s, ws.lp, ws.row, (size_t)(nb - 1) * hw, hw,
                                          (int)cap, R.carry));
        }
        if (M->dry) continue;
        HIP_TRY(hipGetLastError());
        tot.resize(nb);
        unsigned n_found[3] = {0, 0, 0};
        HIP_TRY(hipMemcpyAsync(tot.data(), ws.tot, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
        if (match) {
            ytot.resize(nb);
            HIP_TRY(hipMemcpyAsync(ytot.data(), ws.ytot, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
        }
        if (mask) HIP_TRY(hipMemcpyAsync(mask + (size_t)b0 * hw, ws.mask, n, hipMemcpyDeviceToHost, s));
        if (link) HIP_TRY(hipMemcpyAsync(n_found, ws.n_list, sets * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int t = 0; t < sets && link; ++t) {     // only the counted entries come back; their order is the atomics': sorted below
            if ((size_t)n_found[t] > (size_t)nb * per_slice) {
                set_error("lesion table: %u %s in %d slices exceed the bound of %zu per slice", n_found[t], t == 2 ? "pairs" : "links", nb,
                          per_slice);
                return DNNCA_ESTATE;
            }
            found[t].resize(n_found[t]);
            if (n_found[t])
                HIP_TRY(hipMemcpyAsync(found[t].data(), ws.list + (size_t)t * nb * per_slice, (size_t)n_found[t] * sizeof(LesionLink),
                                       hipMemcpyDeviceToHost, s));
        }
        const int64_t out_before = out;
        DN_TRY(lesion_rows_read(M, ws.acc, tot, b0, cap, acc, rows, out, totals));
        if (sp) DN_TRY(lesion_spread_read(M, ws.sacc, ws.stot, tot, b0, cap, sp->srows + out_before, sp->stotals));
        if (ft) DN_TRY(lesion_feat_read(M, ws, tot, b0, cap, *ft, out_before));
        if (match) DN_TRY(lesion_rows_read(M, ws.yacc, ytot, b0, cap, acc, match->rows, out_true, match->totals));
        for (int t = 0; t < sets && link; ++t) {
            std::sort(found[t].begin(), found[t].end(), [](const LesionLink& x, const LesionLink& y) {
                return std::make_tuple(x.slice, x.row_prev, x.row) < std::make_tuple(y.slice, y.row_prev, y.row);
            });
            for (const LesionLink& v : found[t]) {
                if (t == 0) link->links[out_list[0]++] = dnnca_lesion_link{v.slice, v.row_prev, v.row, v.overlap};
                else if (t == 1) match->links[out_list[1]++] = dnnca_lesion_link{v.slice, v.row_prev, v.row, v.overlap};
                else match->pairs[out_list[2]++] = dnnca_lesion_pair{v.slice, v.row_prev, v.row, v.overlap};
            }
        }
    }
    if (!M->dry && n_rows) *n_rows = out;
    if (link && !M->dry) *link->n_links = out_list[0];
    if (link && !match && !M->dry) {
        R.carry_valid = true;
        R.carry_oh = oh;
        R.carry_ow = ow;
        R.carry_refine = M->refine;
    }
    if (match && !M->dry) {
        *match->n_rows = out_true;
        *match->n_links = out_list[1];
        *match->n_pairs = out_list[2];
        R.mcarry_valid = true;
        R.mcarry_oh = oh;
        R.mcarry_ow = ow;
        R.mcarry_refine = M->refine;
    }
    return DNNCA_OK;
}

int lesion_table(Model* M, const float* prob, int batch, int h, int w, const LesionArgs& a, dnnca_lesion_row* rows, int64_t* n_rows,
                 int32_t* totals, uint8_t* mask, bool want_mask) {
    return lesion_run(M, prob, batch, h, w, a, rows, n_rows, totals, mask, want_mask, nullptr);
}

int lesion_table_spread(Model* M, const float* prob, const float* spread, int batch, int h, int w, const LesionArgs& a,
                        dnnca_lesion_row* rows, int64_t* n_rows, int32_t* totals, uint8_t* mask, bool want_mask,
                        dnnca_lesion_spread* srows, dnnca_slice_spread* stotals) {
    const LesionSpreadIO io{spread, srows, stotals};
    return lesion_run(M, prob, batch, h, w, a, rows, n_rows, totals, mask, want_mask, nullptr, nullptr, &io);
}

int lesion_features_check(const LesionArgs& a, int channels, int bins, int ring) {
    if (channels < 1 || channels > kFeatMaxC) { set_error("lesion features: %d channels outside 1..%d", channels, kFeatMaxC); return DNNCA_EINVAL; }
    if (bins < 0 || bins > kFeatMaxBins) { set_error("lesion features: %d bins outside 0..%d", bins, kFeatMaxBins); return DNNCA_EINVAL; }
    if (ring < 0 || ring > kRingMaxR) { set_error("lesion features: ring %d outside 0..%d", ring, kRingMaxR); return DNNCA_EINVAL; }
    if (a.oh > 65535 || a.ow > 65535) {
        set_error("lesion features: an analysed plane of %d x %d (a side above 65535: the moment sums would not fit 64 bits)", a.oh, a.ow);
        return DNNCA_EINVAL;
    }
    const LesionFeatIO io{nullptr, channels, bins, ring, nullptr, nullptr, nullptr, nullptr};
    if (io.slice_bytes((size_t)a.cap) > kFeatBudget) {
        set_error("lesion features: %d rows x %d channels x %d bins per slice need more than %zu bytes of records (lower max_lesions)",
                  a.cap, channels, bins, kFeatBudget);
        return DNNCA_EINVAL;
    }
    return DNNCA_OK;
}

int lesion_table_features(Model* M, const float* prob, const float* x, int channels, int batch, int h, int w, const LesionArgs& a,
                          dnnca_lesion_row* rows, int64_t* n_rows, int32_t* totals, uint8_t* mask, bool want_mask, int bins, int ring,
                          dnnca_lesion_shape* shape, dnnca_lesion_intensity* body, dnnca_lesion_intensity* ring_out, uint32_t* hist) {
    const LesionFeatIO io{x, channels, bins, ring, shape, body, ring_out, hist};
    return lesion_run(M, prob, batch, h, w, a, rows, n_rows, totals, mask, want_mask, nullptr, nullptr, nullptr, &io);
}

void lesion_features_last(Model* M, float* rf, int* k, bool* want_mask, int* bins, int* ring) {
    RegionState def;
    const RegionState& R = M->region ? *M->region : def;
    *rf = R.feat_rf;
    *k = R.feat_k;
    *want_mask = R.feat_mask;
    *bins = R.feat_bins;
    *ring = R.feat_ring;
}

int spread_by_outcome(Model* M, const float* prob, const float* spread, const float* y, int batch, size_t hw, const float* thresholds,
                      int n_thresholds, dnnca_spread_outcome* out) {
    DN_TRY(region_state(M));
    RegionState& R = *M->region;
    hipStream_t s = M->stream;
    const size_t acc_bytes = align256((size_t)n_thresholds * batch * sizeof(dnnca_spread_outcome));
    DN_TRY(region_ws_reserve(R, acc_bytes + align256((size_t)n_thresholds * 4)));
    unsigned long long* acc = (unsigned long long*)R.ws;
    float* thr = (float*)((char*)R.ws + acc_bytes);
    HIP_TRY(hipMemsetAsync(acc, 0, acc_bytes, s));
    HIP_TRY(hipMemcpyAsync(thr, thresholds, (size_t)n_thresholds * 4, hipMemcpyHostToDevice, s));
    const size_t per_block = (size_t)RB * kOutcomeU;
    const dim3 grid((unsigned)((hw + per_block - 1) / per_block), n_thresholds, batch);
    LAUNCH(M, "spread_outcome", (double)n_thresholds * batch * hw * 12.0, 0,
           hipLaunchKernelGGL(k_spread_outcome, grid, dim3(RB), 0, s, prob, spread, y, (const float*)thr, hw, acc));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, acc, (size_t)n_thresholds * batch * sizeof(dnnca_spread_outcome), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return DNNCA_OK;
}

int lesion_table_linked(Model* M, const float* prob, int batch, int h, int w, const LesionArgs& a, dnnca_lesion_row* rows,
                        int64_t* n_rows, int32_t* totals, uint8_t* mask, bool want_mask, const uint8_t* continues,
                        dnnca_lesion_link* links, int64_t* n_links) {
    const LesionLinkIO io{continues, links, n_links};
    return lesion_run(M, prob, batch, h, w, a, rows, n_rows, totals, mask, want_mask, &io);
}

int lesion_table_matched(Model* M, const float* prob, const float* y, int batch, int h, int w, const LesionArgs& a,
                         const uint8_t* continues, dnnca_lesion_plane_out* pred, uint8_t* mask, bool want_mask,
                         dnnca_lesion_plane_out* truth, dnnca_lesion_pairs_out* pairs) {
    if (M->dry) {
        const LesionLinkIO io{nullptr, nullptr, nullptr};
        const LesionMatchIO mo{y, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        return lesion_run(M, prob, batch, h, w, a, nullptr, nullptr, nullptr, nullptr, want_mask, &io, &mo);
    }
    const LesionLinkIO io{continues, pred->links, &pred->n_links};
    const LesionMatchIO mo{y, truth->rows, &truth->n_rows, truth->totals, truth->links, &truth->n_links, pairs->pairs, &pairs->n_pairs};
    return lesion_run(M, prob, batch, h, w, a, pred->rows, &pred->n_rows, pred->totals, mask, want_mask, &io, &mo);
}

// ---- boundary distances ------------------------------------------------------------------------------------------------------
struct SurfaceWs {                       // carve-up of the workspace for nb slices of hw pixels and `per` samples per slice and side
    uint32_t *w0, *w1, *yw;
    int* lp;
    unsigned *sp, *counts, *n_list;
    float *thr, *ythr;
    unsigned char* edges;
    unsigned short* cols;
    SurfaceSample* list;
    size_t bytes;
};

static SurfaceWs surface_layout(void* base, size_t nb, size_t hw, size_t per) {
    const size_t n = nb * hw;
    SurfaceWs w;
    char* p = (char*)base;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* r = p ? p + off : nullptr; off += align256(bytes); return (void*)r; };
    w.w0 = (uint32_t*)take(n * 4);
    w.w1 = (uint32_t*)take(n * 4);
    w.lp = (int*)take(n * 4);
    w.sp = (unsigned*)take(n * 4);
    w.yw = (uint32_t*)take(n * 4);
    w.thr = (float*)take(2 * 4);         // (two with the hysteresis of the mask refinement)
    w.ythr = (float*)take(4);
    w.edges = (unsigned char*)take(n);
    w.cols = (unsigned short*)take(2 * n * 2);
    w.counts = (unsigned*)take(nb * 5 * 4);
    w.list = (SurfaceSample*)take(nb * 2 * per * sizeof(SurfaceSample));
    w.n_list = (unsigned*)take(4);
    w.bytes = off;
    return w;
}

int surface_distances(Model* M, const float* prob, const float* y, int batch, int h, int w, const LesionArgs& a, int max_samples,
                      int32_t* counts, dnnca_surface_sample* samples, int64_t* n_samples, uint8_t* edges) {
    DN_TRY(region_state(M));
    RegionState& R = *M->region;
    R.surface_rf = a.rf;
    R.surface_k = a.k;
    const int oh = a.oh, ow = a.ow;
    const size_t hw = (size_t)oh * ow, per = std::min<size_t>((size_t)max_samples, hw);
    const int chunk = (int)region_chunk(3, hw, batch);       // two word planes, the column planes and the list: a matched chunk's room
    if (!M->dry) DN_TRY(region_ws_reserve(R, surface_layout(nullptr, chunk, hw, per).bytes));
    hipStream_t s = M->stream;
    std::vector<SurfaceSample> found;
    int64_t out = 0;
    Resize rz{h, w, oh, ow, (float)h / (float)oh, (float)w / (float)ow, (oh == h && ow == w) ? 1 : 0};
    const bool refine = refine_on(M->refine);
    const float refine_thr[2] = {M->refine.hysteresis_low, a.threshold};     // outlives every chunk's sync
    for (int b0 = 0; b0 < batch; b0 += chunk) {
        const int nb = std::min(chunk, batch - b0);
        const size_t n = (size_t)nb * hw, list_cap = (size_t)nb * 2 * per;
        const SurfaceWs ws = surface_layout(R.ws, nb, hw, per);
        const float* pb = prob + (size_t)b0 * h * w;
        const float* yb = y + (size_t)b0 * h * w;
        if (!M->dry) {
            if (!refine) HIP_TRY(hipMemcpyAsync(ws.thr, &a.threshold, 4, hipMemcpyHostToDevice, s));       // `a` outlives the chunk's sync
            HIP_TRY(hipMemcpyAsync(ws.ythr, &kLabelThreshold, 4, hipMemcpyHostToDevice, s));
        }
        const uint32_t* fg = ws.w0;
        if (refine) {                    // the refined mask in the place of prep / open; lp and sp are written only behind it
            DN_TRY(refine_chunk(M, M->refine, pb, rz, nb, refine_thr, a.k, RefineWs{ws.w0, ws.w1, ws.lp, ws.sp, ws.thr}, &fg));
        } else {
            region_prep_launch(M, pb, rz, nb, ws.thr, 1, ws.w0);
            if (a.k > 1) {
                region_open_launch(M, ws.w0, ws.w1, oh, ow, a.k, nb);
                fg = ws.w1;
            }
        }
        region_ccl(M, fg, 1, nb, oh, ow, ws.lp);
        if (!M->dry) {
            HIP_TRY(hipMemsetAsync(ws.sp, 0, n * 4, s));
            HIP_TRY(hipMemsetAsync(ws.counts, 0, (size_t)nb * 5 * 4, s));
            HIP_TRY(hipMemsetAsync(ws.n_list, 0, 4, s));
        }
        LAUNCH(M, "region_sizes", n * 4.0, 0, hipLaunchKernelGGL(k_region_sizes, dim3(nblocks(n)), dim3(RB), 0, s, ws.lp, n, ws.sp));
        LAUNCH(M, "region_prep", n * 4.0 + (double)nb * h * w * 4, 0,
               hipLaunchKernelGGL(k_region_prep, dim3(nblocks(n)), dim3(RB), 0, s, yb, rz, nb, (const float*)ws.ythr, 1, ws.yw));
        LAUNCH(M, "surface_edges", n * 17.0, 0,
               hipLaunchKernelGGL(k_surface_edges, dim3(nblocks(hw), nb), dim3(RB), 0, s, fg, (const int*)ws.lp, (const unsigned*)ws.sp,
                                  (unsigned)a.min_area, (const uint32_t*)ws.yw, oh, ow, ws.edges, ws.counts));
        LAUNCH(M, "surface_cols", n * 6.0, 0,
               hipLaunchKernelGGL(k_surface_cols, dim3((ow + kColsX - 1) / kColsX, 2 * nb), dim3(RB), (size_t)((oh + 31) / 32) * kColsX * 4, s,
                                  (const unsigned char*)ws.edges, nb, oh, ow, ws.cols));
        LAUNCH(M, "surface_sample", n * 1.0 + (double)list_cap * 16, 0,
               hipLaunchKernelGGL(k_surface_sample, dim3(nblocks(hw), nb), dim3(RB), 0, s, (const unsigned char*)ws.edges,
                                  (const unsigned short*)ws.cols, (const unsigned*)ws.counts, nb, oh, ow, (unsigned)max_samples, b0,
                                  (unsigned)list_cap, ws.list, ws.n_list));
        if (M->dry) continue;
        HIP_TRY(hipGetLastError());
        unsigned n_found = 0;
        HIP_TRY(hipMemcpyAsync(counts + (size_t)b0 * 5, ws.counts, (size_t)nb * 5 * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&n_found, ws.n_list, 4, hipMemcpyDeviceToHost, s));
        if (edges) HIP_TRY(hipMemcpyAsync(edges + (size_t)b0 * hw, ws.edges, n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if ((size_t)n_found > list_cap) {
            set_error("surface distances: %u samples in %d slices exceed the bound of %zu per slice", n_found, nb, 2 * per);
            return DNNCA_ESTATE;
        }
        found.resize(n_found);           // only the counted entries come back; their order is the atomics': sorted below
        if (n_found) {
            HIP_TRY(hipMemcpyAsync(found.data(), ws.list, (size_t)n_found * sizeof(SurfaceSample), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        std::sort(found.begin(), found.end(), [](const SurfaceSample& x, const SurfaceSample& y) {
            return std::make_tuple(x.slice, x.side, x.pixel) < std::make_tuple(y.slice, y.side, y.pixel);
        });
        for (const SurfaceSample& v : found) samples[out++] = dnnca_surface_sample{v.slice, v.side, v.pixel, v.d2};
    }
    if (!M->dry) *n_samples = out;
    return DNNCA_OK;
}

void surface_last(Model* M, float* rf, int* k) {
    RegionState def;
    const RegionState& R = M->region ? *M->region : def;
    *rf = R.surface_rf;
    *k = R.surface_k;
}

bool lesion_match_carry_is(Model* M, int oh, int ow) {
    return M->region && M->region->mcarry_valid && M->region->mcarry_oh == oh && M->region->mcarry_ow == ow &&
           refine_same(M->region->mcarry_refine, M->refine);
}

void lesion_match_last(Model* M, float* rf, int* k, bool* want_mask) {
    RegionState def;
    const RegionState& R = M->region ? *M->region : def;
    *rf = R.match_rf;
    *k = R.match_k;
    *want_mask = R.match_mask;
}

bool lesion_carry_is(Model* M, int oh, int ow) {
    return M->region && M->region->carry_valid && M->region->carry_oh == oh && M->region->carry_ow == ow &&
           refine_same(M->region->carry_refine, M->refine);
}

void lesion_last(Model* M, float* rf, int* k, bool* want_mask) {
    RegionState def;
    const RegionState& R = M->region ? *M->region : def;
    *rf = R.lesion_rf;
    *k = R.lesion_k;
    *want_mask = R.lesion_mask;
}

void region_release(Model* M) {
    if (!M->region) return;
    RegionState& R = *M->region;
    for (void* p : {(void*)R.thr_dev, (void*)R.acc, R.ws, (void*)R.in_prob, (void*)R.in_y, (void*)R.slice_acc, (void*)R.viz, (void*)R.carry,
                    (void*)R.mcarry})
        if (p) (void)hipFree(p);
    delete M->region;
    M->region = nullptr;
}

}  // namespace dnnca
