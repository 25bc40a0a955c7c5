// kernels_join.hip -- the residual join of MultiResUnet (multiresunet.py MultiResBlock / ResPath: add -> ReLU -> BatchNorm), which
// that network runs 19 times forward and 19 times backward per step, as streaming passes:
//   k_join_fwd    r = relu(a + b), and the per-channel sums of r that the BatchNorm behind it needs for its mean
//   k_join_infer  y = relu(a + b) * scale + shift with the BatchNorm's inference coefficients; r itself is never stored
//   k_join_bwd    dA, dB (+)= dr * [r > 0]
// Two walks over a tensor (template V): V = 4 when every view is dense (ps == C) and its base 16-byte aligned -- the tensor is one
// flat array read as float4 with a scalar tail, and the channel of flat element i is i % C (the widths, 51, 105, ..., are odd: a
// pixel is not 16-byte aligned, the flat array is); V = 1 for channel slices of wider tensors (element (pixel, c) at pixel * ps + c).
// Both are grid-stride loops over a grid sized from the CU count, not from the tensor.
//
// Channel sums (k_join_fwd): the stride of the grid-stride loop is a multiple of C, so each of a thread's V lanes stays on ONE channel
// and adds up in a double of its own.  A block covers 256 V consecutive flat positions per round, position q on channel
// (base + q) % C: thread u adds positions u, u + C, u + 2C, ... of the block's LDS row in that order and stores the block's partial
// for its channel into row blockIdx.x of `part` [grid][C] -- plain stores, no atomics.  The block that draws the last ticket adds
// the rows in block order into ws[c] (and zeroes ws[C + c] for the variance pass, which adds into it), so the sums are the same bits
// on every run, and it leaves the ticket zeroed: no memset launch.  Hand-over: plain stores, every thread waits for its own
// (vmcnt(0)), barrier, one agent-scope release fence by thread 0 in front of its ticket; the last block acquires once before it
// reads the rows.  The partial table is capped at kJoinPartBytes: the last block reads it alone (about 100 GB/s), which is what the
// cap trades against blocks in flight at the widest (deepest, smallest) tensors.
#include <algorithm>

#include "fast.h"

namespace dnnca {

namespace {

constexpr int JT = 256;                          // threads per block: four full waves
constexpr size_t kJoinPartBytes = 512u << 10;    // partial table of one launch at most (the fold reads it in ~5 us)

int cu_count() {
    static const int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1) v = 256;
        return v;
    }();
    return n;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool flat_ok(const View& v) { return v.ps == v.C && aligned16(v.p); }

// grid of a streaming pass over n elements, V per thread and round: eight rounds per thread before a second block per CU is worth
// its launch, two blocks (eight waves) per CU at most
unsigned stream_grid(size_t n, int V) {
    const size_t per_block = (size_t)JT * V * 8;
    size_t g = (n + per_block - 1) / per_block;
    const size_t cap = (size_t)2 * cu_count();
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}

__device__ __forceinline__ float relu(float v) { return v > 0.f ? v : 0.f; }

// flat walk: elements [4 i, 4 i + 4) by thread-round i < n4 = n / 4, the n % 4 tail elements by the threads tail_t .. tail_t + 3
template <int V, bool SUMS>
__global__ __launch_bounds__(JT) void k_join_fwd(size_t npix, View a, View b, View r, double* __restrict__ ws, double* __restrict__ part,
                                                 unsigned* __restrict__ ticket) {
    __shared__ double row[SUMS ? JT * V : 1];
    __shared__ unsigned last;
    const int C = r.C;
    const size_t n = npix * (size_t)C;
    // thread stride in units of V elements: a multiple of C (SUMS), so that lane j of a thread stays on one channel
    size_t T = (size_t)gridDim.x * JT;
    if (SUMS) T = (T / C) * C;
    const size_t tid = (size_t)blockIdx.x * JT + threadIdx.x;
    double acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.0;
    if (tid < T) {
        if (V == 4) {
            const size_t n4 = n / 4;
            const float4* a4 = reinterpret_cast<const float4*>(a.p);
            const float4* b4 = reinterpret_cast<const float4*>(b.p);
            float4* r4 = reinterpret_cast<float4*>(r.p);
            size_t i = tid;
            for (; i < n4; i += T) {
                const float4 x = a4[i], y = b4[i];
                float4 o;
                o.x = relu(x.x + y.x); o.y = relu(x.y + y.y); o.z = relu(x.z + y.z); o.w = relu(x.w + y.w);
                r4[i] = o;
                acc[0] += o.x; acc[1 % V] += o.y; acc[2 % V] += o.z; acc[3 % V] += o.w;
            }
            // scalar tail: the thread-round that would hold element 4 n4 takes the n % 4 leftovers, each in the lane of its position
            if (i == n4) {
                for (size_t e = 4 * n4; e < n; ++e) {
                    const float o = relu(a.p[e] + b.p[e]);
                    r.p[e] = o;
                    acc[(e - 4 * n4) % V] += o;
                }
            }
        } else {
            for (size_t i = tid; i < n; i += T) {
                const size_t p = i / C;
                const int c = (int)(i - p * C);
                const float o = relu(a.p[p * a.ps + c] + b.p[p * b.ps + c]);
                r.p[p * r.ps + c] = o;
                acc[0] += o;
            }
        }
    }
    if (!SUMS) return;
    // block reduction: position q of the block's 256 V positions is on channel (base + q) % C
#pragma unroll
    for (int j = 0; j < V; ++j) row[threadIdx.x * V + j] = acc[j];
    __syncthreads();
    const int base = (int)(((size_t)blockIdx.x * JT * V) % C);
    double* mine = part + (size_t)blockIdx.x * C;
    for (int u = threadIdx.x; u < C; u += JT) {
        double s = 0.0;
        for (int q = u; q < JT * V; q += C) s += row[q];
        int c = base + u;
        if (c >= C) c -= C;
        mine[c] = s;
    }
    // hand-over: this thread's stores have been performed; then the whole block's; thread 0 releases them to the device and draws
    __builtin_amdgcn_s_waitcnt(0x0070);          // vmcnt(0) lgkmcnt(0)
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __builtin_amdgcn_s_waitcnt(0x0070);
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned l = t == gridDim.x - 1 ? 1u : 0u;
        if (l) {
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            __builtin_amdgcn_s_waitcnt(0x0070);
        }
        last = l;
    }
    __syncthreads();
    if (!last) return;
    for (int c = threadIdx.x; c < C; c += JT) {
        double s = 0.0;
        for (unsigned g = 0; g < gridDim.x; ++g) s += __hip_atomic_load(part + (size_t)g * C + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ws[c] = s;
        ws[C + c] = 0.0;
    }
}

template <int V>
__global__ __launch_bounds__(JT) void k_join_infer(size_t npix, View a, View b, View y, const float* __restrict__ coef) {
    const int C = y.C;
    const size_t n = npix * (size_t)C;
    const size_t T = (size_t)gridDim.x * JT;
    const size_t tid = (size_t)blockIdx.x * JT + threadIdx.x;
    if (V == 4) {
        const size_t n4 = n / 4;
        const float4* a4 = reinterpret_cast<const float4*>(a.p);
        const float4* b4 = reinterpret_cast<const float4*>(b.p);
        float4* y4 = reinterpret_cast<float4*>(y.p);
        for (size_t i = tid; i < n4; i += T) {
            const float4 x = a4[i], z = b4[i];
            int c = (int)((4 * i) % C);
            float v[4] = {relu(x.x + z.x), relu(x.y + z.y), relu(x.z + z.z), relu(x.w + z.w)};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = fmaf(v[j], coef[c], coef[C + c]);
                if (++c == C) c = 0;
            }
            y4[i] = make_float4(v[0], v[1], v[2], v[3]);
        }
        for (size_t e = 4 * n4 + tid; e < n; e += T) {
            const int c = (int)(e % C);
            y.p[e] = fmaf(relu(a.p[e] + b.p[e]), coef[c], coef[C + c]);
        }
    } else {
        for (size_t i = tid; i < n; i += T) {
            const size_t p = i / C;
            const int c = (int)(i - p * C);
            y.p[p * y.ps + c] = fmaf(relu(a.p[p * a.ps + c] + b.p[p * b.ps + c]), coef[c], coef[C + c]);
        }
    }
}

template <int V>
__global__ __launch_bounds__(JT) void k_join_bwd(size_t npix, View dr, View r, View dA, int accA, View dB, int accB) {
    const int C = r.C;
    const size_t n = npix * (size_t)C;
    const size_t T = (size_t)gridDim.x * JT;
    const size_t tid = (size_t)blockIdx.x * JT + threadIdx.x;
    if (V == 4) {
        const size_t n4 = n / 4;
        const float4* g4 = reinterpret_cast<const float4*>(dr.p);
        const float4* r4 = reinterpret_cast<const float4*>(r.p);
        float4* da4 = reinterpret_cast<float4*>(dA.p);
        float4* db4 = reinterpret_cast<float4*>(dB.p);
        for (size_t i = tid; i < n4; i += T) {
            const float4 g = g4[i], o = r4[i];
            float4 d;
            d.x = o.x > 0.f ? g.x : 0.f; d.y = o.y > 0.f ? g.y : 0.f; d.z = o.z > 0.f ? g.z : 0.f; d.w = o.w > 0.f ? g.w : 0.f;
            float4 ua = d, ub = d;
            if (accA) { const float4 t = da4[i]; ua.x += t.x; ua.y += t.y; ua.z += t.z; ua.w += t.w; }
            if (accB) { const float4 t = db4[i]; ub.x += t.x; ub.y += t.y; ub.z += t.z; ub.w += t.w; }
            da4[i] = ua;
            db4[i] = ub;
        }
        for (size_t e = 4 * n4 + tid; e < n; e += T) {
            const float d = r.p[e] > 0.f ? dr.p[e] : 0.f;
            dA.p[e] = accA ? dA.p[e] + d : d;
            dB.p[e] = accB ? dB.p[e] + d : d;
        }
    } else {
        for (size_t i = tid; i < n; i += T) {
            const size_t p = i / C;
            const int c = (int)(i - p * C);
            const float d = r.p[p * r.ps + c] > 0.f ? dr.p[p * dr.ps + c] : 0.f;
            float* pa = dA.p + p * dA.ps + c;
            float* pb = dB.p + p * dB.ps + c;
            *pa = accA ? *pa + d : d;
            *pb = accB ? *pb + d : d;
        }
    }
}

}  // namespace

// blocks of join_fwd for a tensor of B x H x W x C: at least enough threads that the loop stride can be a multiple of C, at most
// what keeps the partial table within kJoinPartBytes; force > 0 (tests): that many blocks instead of the streaming rule
unsigned join_fwd_grid(size_t npix, const View& a, const View& b, const View& r, int force) {
    const int C = r.C;
    const bool vec = flat_ok(a) && flat_ok(b) && flat_ok(r);
    const unsigned minb = (unsigned)((C + JT - 1) / JT);
    unsigned g = force > 0 ? (unsigned)force : stream_grid(npix * (size_t)C, vec ? 4 : 1);
    const unsigned cap = (unsigned)(kJoinPartBytes / 8 / (size_t)C);
    if (force <= 0 && g > cap) g = cap;
    return g < minb ? minb : g;
}

size_t join_part_doubles(int C) {      // partial rows of the largest grid join_fwd_grid(.., force = 0) can choose
    const size_t minb = (size_t)((C + JT - 1) / JT);
    const size_t cap = std::max(kJoinPartBytes / 8 / (size_t)C, minb);
    return std::min(cap, (size_t)2 * cu_count() + minb) * C;
}

void join_fwd(hipStream_t s, int B, View a, View b, View r, double* ws, double* part, unsigned* ticket, int force_grid) {
    const size_t npix = (size_t)B * r.H * r.W;
    const bool vec = flat_ok(a) && flat_ok(b) && flat_ok(r);
    if (ws) {
        const unsigned g = join_fwd_grid(npix, a, b, r, force_grid);
        if (vec) hipLaunchKernelGGL((k_join_fwd<4, true>), dim3(g), dim3(JT), 0, s, npix, a, b, r, ws, part, ticket);
        else hipLaunchKernelGGL((k_join_fwd<1, true>), dim3(g), dim3(JT), 0, s, npix, a, b, r, ws, part, ticket);
    } else {
        const unsigned g = force_grid > 0 ? (unsigned)force_grid : stream_grid(npix * (size_t)r.C, vec ? 4 : 1);
        if (vec) hipLaunchKernelGGL((k_join_fwd<4, false>), dim3(g), dim3(JT), 0, s, npix, a, b, r, ws, part, ticket);
        else hipLaunchKernelGGL((k_join_fwd<1, false>), dim3(g), dim3(JT), 0, s, npix, a, b, r, ws, part, ticket);
    }
}

void join_infer(hipStream_t s, int B, View a, View b, View y, const float* coef, int force_grid) {
    const size_t npix = (size_t)B * y.H * y.W;
    const bool vec = flat_ok(a) && flat_ok(b) && flat_ok(y);
    const unsigned g = force_grid > 0 ? (unsigned)force_grid : stream_grid(npix * (size_t)y.C, vec ? 4 : 1);
    if (vec) hipLaunchKernelGGL(k_join_infer<4>, dim3(g), dim3(JT), 0, s, npix, a, b, y, coef);
    else hipLaunchKernelGGL(k_join_infer<1>, dim3(g), dim3(JT), 0, s, npix, a, b, y, coef);
}

void join_bwd(hipStream_t s, int B, View dr, View r, View dA, int accA, View dB, int accB, int force_grid) {
    const size_t npix = (size_t)B * r.H * r.W;
    const bool vec = flat_ok(dr) && flat_ok(r) && flat_ok(dA) && flat_ok(dB);
    const unsigned g = force_grid > 0 ? (unsigned)force_grid : stream_grid(npix * (size_t)r.C, vec ? 4 : 1);
    if (vec) hipLaunchKernelGGL(k_join_bwd<4>, dim3(g), dim3(JT), 0, s, npix, dr, r, dA, accA, dB, accB);
    else hipLaunchKernelGGL(k_join_bwd<1>, dim3(g), dim3(JT), 0, s, npix, dr, r, dA, accA, dB, accB);
}

}  // namespace dnnca
