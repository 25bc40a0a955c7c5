// kernels_detect.hip -- the detection map of dnnca_detection_map: ranked lesion candidates by the dynamic extraction of PI-CAI's
// extract_lesion_candidates, restated per slice (include/dnnca.h states the definition; tests/detection_oracle.py states it in numpy):
//   strongest remaining peak m at the lowest pixel index s; t = (float32) m * factor; the 4-connected component C of { w >= t } that
//   holds s; |C| >= min_area: D[C] = m and a candidate record, else dropped; w[C] = 0; until max_candidates, rounds or m < min_confidence.
// All slices of the batch go through a round in lock-step; a finished slice's blocks leave after one load of its state.  Per round:
//   det_peak        key = (value bits << 32) | ~pixel index per pixel (values are in [0, 1]: their bits order as unsigned integers),
//                   maximum in the wave, in the block, then one 64-bit atomicMax per block into the slice's state
//   det_seed        one thread per slice: m < min_confidence or the rounds used up -> done (exhausted when a peak is left);
//                   else t = m * factor formed here, once, and stored beside m and s
//   det_ccl_tile    a 32 x 32 tile of the mask bits(w) >= bits(t), thresholded as it loads, labelled in LDS (the scheme of
//   det_ccl_merge   region_ccl_*: union-find on int32 parents, atomicMin across tile borders, root = smallest index); parents are
//                   pixel indices inside the slice
//   det_area        every pixel points at its root; pixels whose root is the seed's root counted: ballot, block sum, one integer
//                   atomicAdd per block
//   det_commit      D = m (|C| >= min_area) and w = 0 over C; the first thread of the slice's first block writes the record and
//                   advances candidates / rounds / dropped / done and clears the key -- fields that no block of this launch reads
// One more det_peak + det_seed after the last round sets `exhausted`.  No float atomics: map, records and counters are bit-identical
// from run to run.  No host round-trip between rounds (an early-exit variant that reads the count of finished slices is not built).
#include <string.h>

#include <algorithm>
#include <vector>

#include "ccl_dev.h"
#include "detect.h"

namespace dnnca {

namespace {

constexpr int DB = 256;
constexpr int kDetTile = 32;

struct DetSlice {                        // one slice's state, zeroed by a memset
    unsigned long long key;              // det_peak's maximum; cleared by det_commit
    uint32_t m_bits, t_bits;             // the round's peak and threshold (det_seed)
    int seed;                            // the round's seed pixel
    unsigned area;                       // |C| (det_area)
    int active;                          // this round runs for the slice (det_seed)
    int done, n, rounds, dropped, exhausted;
};

struct DetRec { int seed; unsigned area; uint32_t m_bits; };

// w = min(max(p, 0), 1) with NaN and -0 -> +0; D = 0.  dst may be src: a pixel is read before it is written, by the same thread
__device__ __forceinline__ float det_clamp(float v) { return v > 0.f ? fminf(v, 1.f) : 0.f; }

__global__ __launch_bounds__(DB) void k_det_init(const float* src, float* wsp, float* dst, size_t n, int vec) {
    const size_t stride = (size_t)gridDim.x * DB, i0 = (size_t)blockIdx.x * DB + threadIdx.x;
    const size_t nq = vec ? n / 4 : 0;
    for (size_t q = i0; q < nq; q += stride) {
        const float4 v = reinterpret_cast<const float4*>(src)[q];
        reinterpret_cast<float4*>(wsp)[q] = make_float4(det_clamp(v.x), det_clamp(v.y), det_clamp(v.z), det_clamp(v.w));
        reinterpret_cast<float4*>(dst)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (size_t i = nq * 4 + i0; i < n; i += stride) {
        const float v = src[i];
        wsp[i] = det_clamp(v);
        dst[i] = 0.f;
    }
}

__device__ __forceinline__ unsigned long long det_key(float v, uint32_t i) {
    return ((unsigned long long)__float_as_uint(v) << 32) | (uint32_t)~i;
}

__global__ __launch_bounds__(DB) void k_det_peak(const float* __restrict__ wsp, size_t hw, DetSlice* __restrict__ st) {
    __shared__ unsigned long long sm[DB / 64];
    DetSlice* s = st + blockIdx.y;
    if (s->done) return;
    const float* p = wsp + (size_t)blockIdx.y * hw;
    const size_t stride = (size_t)gridDim.x * DB, i0 = (size_t)blockIdx.x * DB + threadIdx.x;
    unsigned long long best = 0;
    const size_t nq = (hw & 3) == 0 ? hw / 4 : 0;      // the slices of the workspace start 16-byte aligned when hw is a multiple of 4
    for (size_t q = i0; q < nq; q += stride) {
        const float4 v = reinterpret_cast<const float4*>(p)[q];
        const uint32_t i = (uint32_t)(q * 4);
        best = max(best, max(max(det_key(v.x, i), det_key(v.y, i + 1)), max(det_key(v.z, i + 2), det_key(v.w, i + 3))));
    }
    for (size_t i = nq * 4 + i0; i < hw; i += stride) best = max(best, det_key(p[i], (uint32_t)i));
    for (int off = 32; off > 0; off >>= 1) best = max(best, (unsigned long long)__shfl_xor(best, off));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < DB / 64; ++i) best = max(best, sm[i]);
        atomicMax(&s->key, best);
    }
}

__global__ __launch_bounds__(64) void k_det_seed(DetSlice* __restrict__ st, int nb, uint32_t c0_bits, float factor, int rounds) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nb) return;
    DetSlice* s = st + b;
    s->active = 0;
    if (s->done) return;
    const unsigned long long key = s->key;
    const uint32_t m_bits = (uint32_t)(key >> 32);
    if (m_bits < c0_bits) { s->done = 1; return; }
    if (s->rounds >= rounds) { s->done = 1; s->exhausted = 1; return; }
    s->m_bits = m_bits;
    s->t_bits = __float_as_uint(__fmul_rn(__uint_as_float(m_bits), factor));
    s->seed = (int)~(uint32_t)key;
    s->area = 0;
    s->active = 1;
}

// one kDetTile x kDetTile tile of one slice labelled in LDS; L[p] = the slice index of the pixel's root inside the tile, -1 off the mask
__global__ __launch_bounds__(DB) void k_det_ccl_tile(const float* __restrict__ wsp, const DetSlice* __restrict__ st, int H, int W,
                                                     int* __restrict__ L) {
    __shared__ int l[kDetTile * kDetTile];
    const DetSlice* s = st + blockIdx.z;
    if (!s->active) return;
    const uint32_t tb = s->t_bits;
    const size_t base = (size_t)blockIdx.z * H * W;
    const int y0 = blockIdx.y * kDetTile, x0 = blockIdx.x * kDetTile;
    for (int i = threadIdx.x; i < kDetTile * kDetTile; i += DB) {
        const int y = y0 + i / kDetTile, x = x0 + (i & (kDetTile - 1));
        l[i] = (y < H && x < W && __float_as_uint(wsp[base + (size_t)y * W + x]) >= tb) ? i : -1;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kDetTile * kDetTile; i += DB) {
        if (l[i] < 0) continue;
        const int c = i & (kDetTile - 1);
        for (int side = 0; side < 2; ++side) {
            const int nbr = side == 0 ? (c > 0 ? i - 1 : -1) : (i >= kDetTile ? i - kDetTile : -1);
            if (nbr < 0 || l[nbr] < 0) continue;
            int a = i, bb = nbr;
            for (;;) {
                a = lds_find(l, a);
                bb = lds_find(l, bb);
                if (a == bb) break;
                if (a > bb) { const int t = a; a = bb; bb = t; }
                const int old = atomicMin(&l[bb], a);
                if (old == bb) break;
                bb = old;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kDetTile * kDetTile; i += DB) {
        const int y = y0 + i / kDetTile, x = x0 + (i & (kDetTile - 1));
        if (y >= H || x >= W) continue;
        int v = -1;
        if (l[i] >= 0) {
            const int r = lds_find(l, i);
            v = (y0 + r / kDetTile) * W + x0 + (r & (kDetTile - 1));
        }
        L[base + (size_t)y * W + x] = v;
    }
}

// pixels on a tile's left / top border unite with their neighbour across it
__global__ __launch_bounds__(DB) void k_det_ccl_merge(int* __restrict__ L, const DetSlice* __restrict__ st, int H, int W) {
    if (!st[blockIdx.y].active) return;
    const size_t hw = (size_t)H * W, p = (size_t)blockIdx.x * DB + threadIdx.x;
    if (p >= hw) return;
    int* Lb = L + (size_t)blockIdx.y * hw;
    const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
    const bool bx = x > 0 && (x & (kDetTile - 1)) == 0, by = y > 0 && (y & (kDetTile - 1)) == 0;
    if (!(bx || by) || Lb[p] < 0) return;
    if (bx && Lb[p - 1] >= 0) unite(Lb, (int)p, (int)(p - 1));
    if (by && Lb[p - W] >= 0) unite(Lb, (int)p, (int)(p - W));
}

// every pixel points at its root; the pixels of the seed's component are counted
__global__ __launch_bounds__(DB) void k_det_area(int* __restrict__ L, DetSlice* __restrict__ st, size_t hw) {
    __shared__ int s_root;
    __shared__ unsigned s_cnt[DB / 64];
    DetSlice* s = st + blockIdx.y;
    if (!s->active) return;
    int* Lb = L + (size_t)blockIdx.y * hw;
    if (threadIdx.x == 0) {
        const int seed = s->seed;
        s_root = ld_agent(Lb + seed) >= 0 ? find_root(Lb, seed) : -2;      // (the seed is on the mask: t <= m)
    }
    __syncthreads();
    const int root = s_root;
    const size_t p = (size_t)blockIdx.x * DB + threadIdx.x;
    bool in = false;
    if (p < hw) {
        const int v = ld_agent(Lb + p);
        if (v >= 0) {
            const int r = v == (int)p ? v : find_root(Lb, v);
            if (r != v) Lb[p] = r;
            in = r == root;
        }
    }
    const unsigned long long mask = __ballot(in);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = (unsigned)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = 0;
        for (int i = 0; i < DB / 64; ++i) total += s_cnt[i];
        if (total) atomicAdd(&s->area, total);
    }
}

__global__ __launch_bounds__(DB) void k_det_commit(const int* __restrict__ L, DetSlice* __restrict__ st, size_t hw, float* __restrict__ wsp,
                                                   float* __restrict__ D, DetRec* __restrict__ rec, int max_candidates, unsigned min_area) {
    DetSlice* s = st + blockIdx.y;
    if (!s->active) return;
    const size_t base = (size_t)blockIdx.y * hw;
    const int seed = s->seed;
    const unsigned area = s->area;
    const uint32_t m_bits = s->m_bits;
    const int root = L[base + seed];                         // compressed by det_area
    const bool keep = area >= min_area;
    const size_t p = (size_t)blockIdx.x * DB + threadIdx.x;
    if (p < hw && L[base + p] == root) {
        if (keep) D[base + p] = __uint_as_float(m_bits);
        wsp[base + p] = 0.f;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {               // none of these fields is read by a block of this launch
        int n = s->n;
        if (keep) {
            rec[(size_t)blockIdx.y * max_candidates + n] = DetRec{seed, area, m_bits};
            s->n = ++n;
        } else {
            s->dropped += 1;
        }
        s->rounds += 1;
        if (n >= max_candidates) s->done = 1;
        s->key = 0;
    }
}

size_t up256(size_t b) { return (b + 255) & ~size_t(255); }

}  // namespace

int detection_check(const dnnca_detection_cfg& c) {
    if (!(c.min_confidence >= 0.001f && c.min_confidence <= 1.f)) { set_error("detection: min_confidence %g outside [0.001, 1]", (double)c.min_confidence); return DNNCA_EINVAL; }
    if (!(c.factor >= 0.01f && c.factor <= 1.f)) { set_error("detection: factor %g outside [0.01, 1]", (double)c.factor); return DNNCA_EINVAL; }
    if (c.max_candidates < 1 || c.max_candidates > 64) { set_error("detection: max_candidates %d outside 1..64", c.max_candidates); return DNNCA_EINVAL; }
    if (c.min_area < 1 || c.min_area > (1 << 30)) { set_error("detection: min_area %d outside 1..2^30", c.min_area); return DNNCA_EINVAL; }
    if (c.rounds < c.max_candidates || c.rounds > 256) { set_error("detection: rounds %d outside max_candidates (%d)..256", c.rounds, c.max_candidates); return DNNCA_EINVAL; }
    return DNNCA_OK;
}

int detection_map(Model* M, const float* src, float* dst, int batch, int h, int w, const dnnca_detection_cfg& c, float* out_hw,
                  dnnca_detection_row* rows, int64_t* n_rows, dnnca_detection_slice* slices) {
    const size_t hw = (size_t)h * w, n = (size_t)batch * hw;
    const int N = c.max_candidates;
    const size_t plane_bytes = up256(n * 4), st_bytes = up256((size_t)batch * sizeof(DetSlice));
    const size_t rec_bytes = up256((size_t)batch * N * sizeof(DetRec));
    const size_t need = 2 * plane_bytes + st_bytes + rec_bytes;
    if (!M->dry && need > M->detect_ws_bytes) {
        if (M->detect_ws) HIP_TRY(hipFree(M->detect_ws));
        M->detect_ws = nullptr;
        M->detect_ws_bytes = 0;
        HIP_TRY(hipMalloc(&M->detect_ws, need));
        M->detect_ws_bytes = need;
    }
    char* ws = (char*)M->detect_ws;
    float* wsp = (float*)ws;
    int* L = (int*)(ws + plane_bytes);
    DetSlice* st = (DetSlice*)(ws + 2 * plane_bytes);
    DetRec* rec = (DetRec*)(ws + 2 * plane_bytes + st_bytes);
    hipStream_t s = M->stream;
    if (!M->dry) {
        M->detect_last = c;
        HIP_TRY(hipMemsetAsync(st, 0, st_bytes, s));
    }
    const int vec = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    const unsigned init_blocks = (unsigned)std::min<size_t>((n / 4 + DB - 1) / DB + 1, size_t(1) << 16);
    LAUNCH(M, "det_init", 12.0 * n, 0, hipLaunchKernelGGL(k_det_init, dim3(init_blocks), dim3(DB), 0, s, src, wsp, dst, n, vec));
    const unsigned peak_blocks = (unsigned)std::min<size_t>((hw + 4 * DB - 1) / (4 * DB), 256);
    const unsigned px_blocks = (unsigned)((hw + DB - 1) / DB);
    const dim3 tiles((w + kDetTile - 1) / kDetTile, (h + kDetTile - 1) / kDetTile, batch);
    uint32_t c0_bits;
    memcpy(&c0_bits, &c.min_confidence, 4);
    for (int round = 0; round <= c.rounds; ++round) {
        LAUNCH(M, "det_peak", 4.0 * n, 0, hipLaunchKernelGGL(k_det_peak, dim3(peak_blocks, batch), dim3(DB), 0, s, (const float*)wsp, hw, st));
        LAUNCH(M, "det_seed", 48.0 * batch, 0,
               hipLaunchKernelGGL(k_det_seed, dim3((batch + 63) / 64), dim3(64), 0, s, st, batch, c0_bits, c.factor, c.rounds));
        if (round == c.rounds) break;    // the last pair only says whether a peak is left
        LAUNCH(M, "det_ccl_tile", 8.0 * n, 0,
               hipLaunchKernelGGL(k_det_ccl_tile, tiles, dim3(DB), 0, s, (const float*)wsp, (const DetSlice*)st, h, w, L));
        LAUNCH(M, "det_ccl_merge", 4.0 * n, 0,
               hipLaunchKernelGGL(k_det_ccl_merge, dim3(px_blocks, batch), dim3(DB), 0, s, L, (const DetSlice*)st, h, w));
        LAUNCH(M, "det_area", 4.0 * n, 0, hipLaunchKernelGGL(k_det_area, dim3(px_blocks, batch), dim3(DB), 0, s, L, st, hw));
        LAUNCH(M, "det_commit", 4.0 * n, 0,
               hipLaunchKernelGGL(k_det_commit, dim3(px_blocks, batch), dim3(DB), 0, s, (const int*)L, st, hw, wsp, dst, rec, N,
                                  (unsigned)c.min_area));
    }
    if (M->dry) return DNNCA_OK;
    HIP_TRY(hipGetLastError());
    std::vector<DetSlice> hst((size_t)batch);
    std::vector<DetRec> hrec((size_t)batch * N);
    HIP_TRY(hipMemcpyAsync(hst.data(), st, hst.size() * sizeof(DetSlice), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(hrec.data(), rec, hrec.size() * sizeof(DetRec), hipMemcpyDeviceToHost, s));
    if (out_hw) HIP_TRY(hipMemcpyAsync(out_hw, dst, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    int64_t out = 0;
    for (int b = 0; b < batch; ++b) {
        const DetSlice& v = hst[b];
        slices[b] = dnnca_detection_slice{v.n, v.rounds, v.dropped, v.exhausted};
        for (int k = 0; k < v.n; ++k) {
            const DetRec& r = hrec[(size_t)b * N + k];
            dnnca_detection_row o = {b, k, r.seed, (int32_t)r.area, 0.f};
            memcpy(&o.confidence, &r.m_bits, 4);
            rows[out++] = o;
        }
    }
    *n_rows = out;
    return DNNCA_OK;
}

}  // namespace dnnca
