// kernels_bootstrap.hip -- the bootstrap over exams of dnnca_bootstrap_sums / dnnca_bootstrap_detection (include/dnnca.h states the
// resampling and the statistics; tests/bootstrap_oracle.py states them in numpy and Python integers).  One workgroup of four waves
// per replicate r:
//   draw          the E draws of the replicate, four per Philox4x32-10 call on the counter (j >> 2, r, 0, 0); every draw adds one to
//                 its exam's counter in LDS.  The counters are 16 bits wide (a multiplicity is at most E <= 16384), two to a dword,
//                 and are raised by a 32-bit LDS atomic on the dword: 32 KiB at the largest E, so several workgroups share a CU.
//   boot_sums     out[r][k] = sum_e m[e] cols[e][k]: KP = the power of two >= K lanes across a row of cols, 256 / KP rows per pass,
//                 the row groups' partial sums added through LDS.  Integers: no order matters.
//   boot_detect   exam totals (block sums); the AUROC pair count as two weighted scans over the exams in score-rank order -- tied
//                 exams with the negatives first give sum [rank_p >= rank_n], with the positives first sum [rank_p > rank_n], their
//                 sum is auroc_twice; the two prefix sums of negative weights (each <= E < 2^16) ride one dword -- then the candidates
//                 in tiles of kBootTile, four consecutive ones per thread as one 16-byte load of packed dwords
//                     bits 0..13 exam | 14 hit | 15 last of its level | 16..25 min(size of the level, 1024) - 1
//                 A block-wide inclusive scan of (w hit, w (1 - hit)), both below 2^24 inside a tile and riding one 64-bit word, on
//                 top of the running 64-bit totals.  The thread that holds a level's last candidate forms the level's AP term and
//                 tests the seven false-positive bounds.  TP_{k-1} is the cumulative TP at the candidate `size of the level` places
//                 before it: read from the tile's LDS image of the scan when that place is inside the tile, else the value carried
//                 from the last level end of the tiles before (the host tells every tile where its last level end is).
// AP: every thread adds its own terms in candidate order; the 256 partial sums are combined by a butterfly inside each wave and the
// four wave sums in wave order: an order fixed by (N, the block size).  No float atomics and no global atomics: every output is
// bit-identical from run to run.  The device never sees a confidence: the host sorts once and sends exam, hit and level ends.
#include <string.h>

#include <algorithm>
#include <vector>

#include "bootstrap.h"
#include "philox_dev.h"

namespace dnnca {

namespace {

constexpr int BB = 256;                              // four whole waves
constexpr int kItems = kBootTile / BB;
static_assert(kItems == 4, "boot_detect loads a thread's candidates as one uint4");
constexpr unsigned kCandHit = 1u << 14, kCandLast = 1u << 15;
static_assert(kBootMaxExams <= (1 << 14) && kBootTile == 1024, "the packed candidate: 14 bits of exam, 10 bits of level size");

struct BootStrata { int S; int off[kBootMaxStrata]; int n[kBootMaxStrata]; };

__device__ __forceinline__ unsigned boot_mult(const uint32_t* s_m, int e) { return (s_m[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu; }

// the replicate's multiplicities into s_m [(E + 1) / 2]; every index is below E: o + umulhi(x, n) < o + n <= E, pool holds exams
__device__ __forceinline__ void boot_draw(uint32_t* s_m, const int* __restrict__ pool, const BootStrata& st, int E, unsigned r, unsigned k0,
                                          unsigned k1) {
    for (int i = threadIdx.x; i < (E + 1) / 2; i += BB) s_m[i] = 0u;
    __syncthreads();
    for (int q = threadIdx.x; q * 4 < E; q += BB) {
        unsigned x[4];
        philox4x32_10((unsigned)q, r, 0u, 0u, k0, k1, x);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = q * 4 + i;
            if (j < E) {
                int o = 0, n = st.n[0];
#pragma unroll
                for (int s = 1; s < kBootMaxStrata; ++s)
                    if (s < st.S && j >= st.off[s]) { o = st.off[s]; n = st.n[s]; }
                const int e = pool[o + (int)__umulhi(x[i], (unsigned)n)];
                atomicAdd(&s_m[e >> 1], 1u << ((e & 1) * 16));
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void boot_store_mult(const uint32_t* s_m, int E, unsigned short* __restrict__ row) {
    for (int e = threadIdx.x; e < E; e += BB) row[e] = (unsigned short)boot_mult(s_m, e);
}

// block-wide reductions over s_w [BB / 64]; the value comes back in every thread
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long* s_w) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();                                 // the use of s_w before this one has been read
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__device__ __forceinline__ unsigned long long block_max(unsigned long long v, unsigned long long* s_w) {
    for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned long long)__shfl_xor(v, off));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return max(max(s_w[0], s_w[1]), max(s_w[2], s_w[3]));
}

// the butterfly adds the same two values on both sides of every exchange: all lanes hold the same bits; then the waves in order
__device__ __forceinline__ double block_sum_ordered(double v, unsigned long long* s_w) {
    for (int off = 32; off > 0; off >>= 1) v = __dadd_rn(v, __shfl_xor(v, off));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = (unsigned long long)__double_as_longlong(v);
    __syncthreads();
    double t = __longlong_as_double((long long)s_w[0]);
    for (int w = 1; w < BB / 64; ++w) t = __dadd_rn(t, __longlong_as_double((long long)s_w[w]));
    return t;
}

__device__ __forceinline__ unsigned long long block_scan_inclusive(unsigned long long v, unsigned long long* s_w, unsigned long long* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    __syncthreads();
    if (lane == 63) s_w[wave] = v;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (int w = 0; w < BB / 64; ++w) {
        const unsigned long long x = s_w[w];
        if (w < wave) before += x;
        all += x;
    }
    *total = all;
    return v + before;
}

__global__ __launch_bounds__(BB) void k_boot_sums(const int* __restrict__ cols, int E, int K, int kp_log2, const int* __restrict__ pool,
                                                  BootStrata st, unsigned r0, unsigned k0, unsigned k1, long long* __restrict__ out,
                                                  unsigned short* __restrict__ mult_out) {
    __shared__ uint32_t s_m[kBootMaxExams / 2];
    __shared__ long long s_acc[BB];
    boot_draw(s_m, pool, st, E, r0 + blockIdx.x, k0, k1);
    if (mult_out) boot_store_mult(s_m, E, mult_out + (size_t)blockIdx.x * E);
    const int KP = 1 << kp_log2, k = threadIdx.x & (KP - 1), g = threadIdx.x >> kp_log2, G = BB >> kp_log2;
    long long acc = 0;
    if (k < K)
        for (int e = g; e < E; e += G) acc += (long long)boot_mult(s_m, e) * cols[(size_t)e * K + k];
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    if ((int)threadIdx.x < K) {
        long long t = 0;
        for (int i = 0; i < G; ++i) t += s_acc[(i << kp_log2) + threadIdx.x];
        out[(size_t)blockIdx.x * K + threadIdx.x] = t;
    }
}

struct BootDetectArgs {
    const uint32_t* cand;        // [tiles * kBootTile] packed candidates, zero behind N
    const int* tile_last;        // [tiles] the place of the tile's last level end inside it, -1 without one
    const int* tumours;          // [E]
    const uint32_t* ord_ge;      // [E] exam | positive << 16 by (rank, negatives first)
    const uint32_t* ord_gt;      // [E] the same by (rank, positives first)
    const int* pool;
    dnnca_bootstrap_detection_row* out;
    unsigned short* mult_out;
    int N, E;
    unsigned r0, k0, k1;
};

__global__ __launch_bounds__(BB) void k_boot_detect(BootDetectArgs a, BootStrata st) {
    __shared__ uint32_t s_m[kBootMaxExams / 2];
    __shared__ uint32_t s_tp[kBootTile];
    __shared__ unsigned long long s_w[BB / 64];
    const int E = a.E, N = a.N;
    boot_draw(s_m, a.pool, st, E, a.r0 + blockIdx.x, a.k0, a.k1);
    if (a.mult_out) boot_store_mult(s_m, E, a.mult_out + (size_t)blockIdx.x * E);

    unsigned long long t_sum = 0, p_sum = 0;
    for (int e = threadIdx.x; e < E; e += BB) {
        const unsigned m = boot_mult(s_m, e);
        const int t = a.tumours[e];
        t_sum += (unsigned long long)m * (unsigned)t;
        p_sum += t > 0 ? m : 0u;
    }
    const long long T = (long long)block_sum(t_sum, s_w), P = (long long)block_sum(p_sum, s_w);

    unsigned long long pairs = 0;
    unsigned before = 0;                             // negative weight so far: order ge in the low, order gt in the high 16 bits
    for (int base = 0; base < E; base += BB) {
        const int i = base + threadIdx.x;
        unsigned neg_ge = 0, pos_ge = 0, neg_gt = 0, pos_gt = 0;
        if (i < E) {
            const unsigned x = a.ord_ge[i], y = a.ord_gt[i];
            const unsigned mx = boot_mult(s_m, x & 0xFFFFu), my = boot_mult(s_m, y & 0xFFFFu);
            if (x >> 16) pos_ge = mx; else neg_ge = mx;
            if (y >> 16) pos_gt = my; else neg_gt = my;
        }
        const unsigned v = neg_ge | neg_gt << 16;
        unsigned long long all;
        const unsigned excl = (unsigned)block_scan_inclusive(v, s_w, &all) - v + before;
        pairs += (unsigned long long)pos_ge * (excl & 0xFFFFu) + (unsigned long long)pos_gt * (excl >> 16);
        before += (unsigned)all;
    }
    const long long twice = (long long)block_sum(pairs, s_w);

    long long base_tp = 0, base_fp = 0, prev_tp = 0;
    long long best[7] = {0, 0, 0, 0, 0, 0, 0};
    double ap = 0.0;
    const double Td = (double)T;
    const int tiles = (N + kBootTile - 1) / kBootTile;
    for (int t = 0; t < tiles; ++t) {
        const int q0 = threadIdx.x * kItems;
        const size_t g0 = (size_t)t * kBootTile + q0;
        const uint4 c4 = *reinterpret_cast<const uint4*>(a.cand + g0);
        const unsigned c[kItems] = {c4.x, c4.y, c4.z, c4.w};
        unsigned tp[kItems], fp[kItems], run_tp = 0, run_fp = 0;
#pragma unroll
        for (int i = 0; i < kItems; ++i) {
            const unsigned m = g0 + i < (size_t)N ? boot_mult(s_m, c[i] & 0x3FFFu) : 0u;
            if (c[i] & kCandHit) run_tp += m; else run_fp += m;
            tp[i] = run_tp;
            fp[i] = run_fp;
        }
        const unsigned long long v = (unsigned long long)run_tp << 32 | run_fp;
        unsigned long long all;
        const unsigned long long excl = block_scan_inclusive(v, s_w, &all) - v;
        const unsigned excl_tp = (unsigned)(excl >> 32), excl_fp = (unsigned)excl;
#pragma unroll
        for (int i = 0; i < kItems; ++i) s_tp[q0 + i] = excl_tp + tp[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kItems; ++i) {
            if (!(c[i] & kCandLast)) continue;       // (zero behind N)
            const long long tp_k = base_tp + excl_tp + tp[i], fp_k = base_fp + excl_fp + fp[i];
            const int p = q0 + i - (int)((c[i] >> 16 & 0x3FFu) + 1u);
            const long long tp_before = p >= 0 ? base_tp + s_tp[p] : prev_tp;
            if (T > 0 && tp_k > tp_before)           // tp_k > 0: the denominator is not 0
                ap = __dadd_rn(ap, __ddiv_rn(__dmul_rn((double)(tp_k - tp_before), (double)tp_k), __dmul_rn(Td, (double)(tp_k + fp_k))));
#pragma unroll
            for (int x = 0; x < 7; ++x)
                if (fp_k * 8 <= ((long long)E << x)) best[x] = max(best[x], tp_k);
        }
        const int last = a.tile_last[t];
        if (last >= 0) prev_tp = base_tp + s_tp[last];
        base_tp += (long long)(all >> 32);
        base_fp += (long long)(unsigned)all;
    }
    const double ap_all = block_sum_ordered(ap, s_w);
#pragma unroll
    for (int x = 0; x < 7; ++x) best[x] = (long long)block_max((unsigned long long)best[x], s_w);
    if (threadIdx.x == 0) {
        dnnca_bootstrap_detection_row o;
        o.positive_exams = P;
        o.tumours = T;
        o.candidates = base_tp + base_fp;
        o.tp = base_tp;
        o.fp = base_fp;
        o.auroc_pairs = P * (E - P);
        o.auroc_twice = twice;
        for (int x = 0; x < 7; ++x) o.tp_at[x] = best[x];
        o.ap = ap_all;
        a.out[blockIdx.x] = o;
    }
}

size_t up256(size_t b) { return (b + 255) & ~size_t(255); }

int boot_reserve(Model* M, size_t need) {
    if (need <= M->boot_ws_bytes) return DNNCA_OK;
    if (M->boot_ws) HIP_TRY(hipFree(M->boot_ws));
    M->boot_ws = nullptr;
    M->boot_ws_bytes = 0;
    HIP_TRY(hipMalloc(&M->boot_ws, need));
    M->boot_ws_bytes = need;
    return DNNCA_OK;
}

BootStrata strata_of(const int32_t* strata, int S) {
    BootStrata st = {};
    st.S = S;
    for (int s = 0, o = 0; s < S; ++s) {
        st.off[s] = o;
        st.n[s] = strata[s];
        o += strata[s];
    }
    return st;
}

// the replicates of one launch: the rows and, when asked for, the multiplicities of a chunk stay within 32 MiB each
int boot_chunk(int R, int E, size_t row_bytes, bool mult) {
    size_t n = std::min<size_t>((size_t)R, (size_t(32) << 20) / row_bytes);
    if (mult) n = std::min(n, (size_t(32) << 20) / ((size_t)E * 2));
    return (int)std::max<size_t>(n, 1);
}

}  // namespace

int bootstrap_check_resampling(int E, const int32_t* pool, const int32_t* strata, int S, int R) {
    if (E < 1 || E > kBootMaxExams) { set_error("bootstrap: %d exams outside 1..%d", E, kBootMaxExams); return DNNCA_EINVAL; }
    if (R < 1 || R > kBootMaxReplicates) { set_error("bootstrap: %d replicates outside 1..%d", R, kBootMaxReplicates); return DNNCA_EINVAL; }
    if (S < 1 || S > kBootMaxStrata) { set_error("bootstrap: %d strata outside 1..%d", S, kBootMaxStrata); return DNNCA_EINVAL; }
    if (!pool || !strata) { set_error("bootstrap: null pool / strata"); return DNNCA_EINVAL; }
    int64_t sum = 0;
    for (int s = 0; s < S; ++s) {
        if (strata[s] < 1) { set_error("bootstrap: stratum %d has size %d", s, strata[s]); return DNNCA_EINVAL; }
        sum += strata[s];
    }
    if (sum != E) { set_error("bootstrap: the strata hold %lld exams, not %d", (long long)sum, E); return DNNCA_EINVAL; }
    std::vector<char> seen((size_t)E, 0);
    for (int i = 0; i < E; ++i) {
        if (pool[i] < 0 || pool[i] >= E || seen[pool[i]]) { set_error("bootstrap: pool is no permutation of 0..%d (entry %d is %d)", E - 1, i, pool[i]); return DNNCA_EINVAL; }
        seen[pool[i]] = 1;
    }
    return DNNCA_OK;
}

int bootstrap_check_detection(const dnnca_bootstrap_exam* exams, int E, const dnnca_bootstrap_candidate* cands, int N) {
    if (N < 0 || N > kBootMaxCandidates) { set_error("bootstrap: %d candidates outside 0..%d", N, kBootMaxCandidates); return DNNCA_EINVAL; }
    if (!exams || (N > 0 && !cands)) { set_error("bootstrap: null exams / cands"); return DNNCA_EINVAL; }
    for (int e = 0; e < E; ++e)
        if (exams[e].tumours < 0 || exams[e].score_rank < 0) {
            set_error("bootstrap: exam %d has tumours %d, score_rank %d", e, exams[e].tumours, exams[e].score_rank);
            return DNNCA_EINVAL;
        }
    for (int i = 0; i < N; ++i) {
        const dnnca_bootstrap_candidate& c = cands[i];
        if (c.exam < 0 || c.exam >= E) { set_error("bootstrap: candidate %d belongs to exam %d of %d", i, c.exam, E); return DNNCA_EINVAL; }
        if (c.hit != 0 && c.hit != 1) { set_error("bootstrap: candidate %d has hit %d", i, c.hit); return DNNCA_EINVAL; }
        const int before = i ? cands[i - 1].level : 0;
        if (c.level != before && (i == 0 || c.level != before + 1)) {
            set_error("bootstrap: candidate %d has level %d after %d (levels start at 0, never decrease and skip nothing)", i, c.level, before);
            return DNNCA_EINVAL;
        }
    }
    return DNNCA_OK;
}

int bootstrap_sums(Model* M, const int32_t* cols, int E, int K, const int32_t* pool, const int32_t* strata, int S, int R, uint64_t seed,
                   int64_t* out, uint16_t* mult_out) {
    const int chunk = boot_chunk(R, E, (size_t)K * 8, mult_out != nullptr);
    const size_t cols_b = up256((size_t)E * K * 4), pool_b = up256((size_t)E * 4), out_b = up256((size_t)chunk * K * 8);
    const size_t mult_b = mult_out ? up256((size_t)chunk * E * 2) : 0;
    DN_TRY(boot_reserve(M, cols_b + pool_b + out_b + mult_b));
    char* ws = (char*)M->boot_ws;
    int* d_cols = (int*)ws;
    int* d_pool = (int*)(ws + cols_b);
    long long* d_out = (long long*)(ws + cols_b + pool_b);
    unsigned short* d_mult = mult_out ? (unsigned short*)(ws + cols_b + pool_b + out_b) : nullptr;
    hipStream_t s = M->stream;
    HIP_TRY(hipMemcpyAsync(d_cols, cols, (size_t)E * K * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_pool, pool, (size_t)E * 4, hipMemcpyHostToDevice, s));
    const BootStrata st = strata_of(strata, S);
    int kp_log2 = 0;
    while ((1 << kp_log2) < K) ++kp_log2;
    for (int r0 = 0; r0 < R; r0 += chunk) {
        const int n = std::min(chunk, R - r0);
        LAUNCH(M, "boot_sums", (double)n * E * (K * 4.0 + 2.0), 0,
               hipLaunchKernelGGL(k_boot_sums, dim3(n), dim3(BB), 0, s, (const int*)d_cols, E, K, kp_log2, (const int*)d_pool, st, (unsigned)r0,
                                  (unsigned)seed, (unsigned)(seed >> 32), d_out, d_mult));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out + (size_t)r0 * K, d_out, (size_t)n * K * 8, hipMemcpyDeviceToHost, s));
        if (mult_out) HIP_TRY(hipMemcpyAsync(mult_out + (size_t)r0 * E, d_mult, (size_t)n * E * 2, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));            // the chunk's buffers are the next chunk's
    }
    return DNNCA_OK;
}

int bootstrap_detection(Model* M, const dnnca_bootstrap_exam* exams, int E, const dnnca_bootstrap_candidate* cands, int N,
                        const int32_t* pool, const int32_t* strata, int S, int R, uint64_t seed, dnnca_bootstrap_detection_row* out,
                        uint16_t* mult_out) {
    // what the kernel reads: packed candidates, every tile's last level end, the exams in the two score-rank orders
    const int tiles = (N + kBootTile - 1) / kBootTile;
    std::vector<uint32_t> packed((size_t)tiles * kBootTile, 0u);
    std::vector<int> tile_last((size_t)std::max(tiles, 1), -1);
    for (int i = 0, start = 0; i < N; ++i) {
        const bool last = i + 1 == N || cands[i + 1].level != cands[i].level;
        uint32_t v = (uint32_t)cands[i].exam | (cands[i].hit ? kCandHit : 0u);
        if (last) {
            v |= kCandLast | (uint32_t)(std::min(i + 1 - start, kBootTile) - 1) << 16;
            tile_last[i / kBootTile] = i % kBootTile;
            start = i + 1;
        }
        packed[i] = v;
    }
    std::vector<int> tumours((size_t)E);
    std::vector<uint32_t> ord_ge((size_t)E), ord_gt((size_t)E);
    for (int e = 0; e < E; ++e) {
        tumours[e] = exams[e].tumours;
        ord_ge[e] = ord_gt[e] = (uint32_t)e | (exams[e].tumours > 0 ? 1u << 16 : 0u);
    }
    const auto rank = [&](uint32_t v) { return exams[v & 0xFFFFu].score_rank; };
    std::stable_sort(ord_ge.begin(), ord_ge.end(), [&](uint32_t x, uint32_t y) { return rank(x) != rank(y) ? rank(x) < rank(y) : (x >> 16) < (y >> 16); });
    std::stable_sort(ord_gt.begin(), ord_gt.end(), [&](uint32_t x, uint32_t y) { return rank(x) != rank(y) ? rank(x) < rank(y) : (x >> 16) > (y >> 16); });

    const int chunk = boot_chunk(R, E, sizeof(dnnca_bootstrap_detection_row), mult_out != nullptr);
    const size_t cand_b = up256(std::max<size_t>(packed.size(), 1) * 4), tile_b = up256(tile_last.size() * 4), e_b = up256((size_t)E * 4);
    const size_t out_b = up256((size_t)chunk * sizeof(dnnca_bootstrap_detection_row));
    const size_t mult_b = mult_out ? up256((size_t)chunk * E * 2) : 0;
    DN_TRY(boot_reserve(M, cand_b + tile_b + 4 * e_b + out_b + mult_b));
    char* ws = (char*)M->boot_ws;
    BootDetectArgs a;
    a.cand = (const uint32_t*)ws;
    a.tile_last = (const int*)(ws + cand_b);
    a.tumours = (const int*)(ws + cand_b + tile_b);
    a.ord_ge = (const uint32_t*)(ws + cand_b + tile_b + e_b);
    a.ord_gt = (const uint32_t*)(ws + cand_b + tile_b + 2 * e_b);
    a.pool = (const int*)(ws + cand_b + tile_b + 3 * e_b);
    a.out = (dnnca_bootstrap_detection_row*)(ws + cand_b + tile_b + 4 * e_b);
    a.mult_out = mult_out ? (unsigned short*)(ws + cand_b + tile_b + 4 * e_b + out_b) : nullptr;
    a.N = N;
    a.E = E;
    a.k0 = (unsigned)seed;
    a.k1 = (unsigned)(seed >> 32);
    hipStream_t s = M->stream;
    if (!packed.empty()) HIP_TRY(hipMemcpyAsync((void*)a.cand, packed.data(), packed.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync((void*)a.tile_last, tile_last.data(), tile_last.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync((void*)a.tumours, tumours.data(), (size_t)E * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync((void*)a.ord_ge, ord_ge.data(), (size_t)E * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync((void*)a.ord_gt, ord_gt.data(), (size_t)E * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync((void*)a.pool, pool, (size_t)E * 4, hipMemcpyHostToDevice, s));
    const BootStrata st = strata_of(strata, S);
    for (int r0 = 0; r0 < R; r0 += chunk) {
        const int n = std::min(chunk, R - r0);
        a.r0 = (unsigned)r0;
        LAUNCH(M, "boot_detect", (double)n * (N * 4.0 + E * 14.0), (double)n * N * 8.0,
               hipLaunchKernelGGL(k_boot_detect, dim3(n), dim3(BB), 0, s, a, st));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out + r0, a.out, (size_t)n * sizeof(dnnca_bootstrap_detection_row), hipMemcpyDeviceToHost, s));
        if (mult_out) HIP_TRY(hipMemcpyAsync(mult_out + (size_t)r0 * E, a.mult_out, (size_t)n * E * 2, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));            // the chunk's buffers are the next chunk's; the host vectors are still alive
    }
    return DNNCA_OK;
}

}  // namespace dnnca
