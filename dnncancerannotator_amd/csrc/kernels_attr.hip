// kernels_attr.hip -- the kernels only the integrated-gradients pass needs (Model::integrated_gradients, model.hip):
//   k_attr_baseline_part / k_attr_baseline   the mean of every (slice, channel) plane in double, rounded once to float32
//   k_attr_path_in    the path input x0 + alpha (x - x0) of one step, for the whole batch (streaming)
//   k_attr_first      the sibling of k_sens_first: the signed first-layer dx, added into an accumulator [B, H, W, C]
//   k_attr_finish     attr = (x - x0) acc / steps, and the block partials of its sum and of the sum of |attr| per (slice, channel)
//   k_attr_sums       a row of block partials added up in ascending order
//   k_attr_prob_part  block partials of sum(sigmoid(logits)) per slice
// No atomics and no tickets anywhere: every output element has exactly one writer and every sum a fixed order.
#include "attr.h"
#include "sens_first_dev.h"

namespace dnnca {

namespace {

constexpr int TB = 256;

// the same tree in every run
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// A block walks the interleaved elements [e0, e1) of one slice (e0 a multiple of C) with the first L = (TB / C) C threads at stride
// L: thread t only ever meets channel t % C.  Afterwards thread c < C adds the lanes c, c + C, ... < L in ascending order.
__device__ __forceinline__ int lanes_of(int C) { return (TB / C) * C; }

__device__ __forceinline__ double channel_sum(double v, int C, double* red) {
    // every thread of the block calls it with its lane sum (0 beyond L); valid in threads c < C
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    double a = 0.0;
    if ((int)threadIdx.x < C)
        for (int t = threadIdx.x; t < lanes_of(C); t += C) a += red[t];
    return a;
}

// grid (blocks per slice, B)
__global__ __launch_bounds__(TB) void k_attr_baseline_part(const float* __restrict__ x, size_t hw, int C, double* __restrict__ part) {
    __shared__ double red[TB];
    const int L = lanes_of(C), tid = threadIdx.x, b = blockIdx.y;
    const size_t n = hw * C, e0 = (size_t)blockIdx.x * kAttrBlockPix * C, e1 = min(n, e0 + (size_t)kAttrBlockPix * C);
    const float* xs = x + (size_t)b * n;
    double v = 0.0;
    if (tid < L)
        for (size_t e = e0 + tid; e < e1; e += L) v += (double)xs[e];
    const double a = channel_sum(v, C, red);
    if (tid < C) part[((size_t)b * C + tid) * gridDim.x + blockIdx.x] = a;
}

// one thread per (slice, channel): the row in ascending block order, the division in double, ONE rounding to float32
__global__ __launch_bounds__(TB) void k_attr_baseline(const double* __restrict__ part, int rows, int n, double inv_hw, float* __restrict__ x0) {
    const int r = blockIdx.x * TB + threadIdx.x;
    if (r >= rows) return;
    double s = 0.0;
#pragma unroll 8
    for (int k = 0; k < n; ++k) s += part[(size_t)r * n + k];
    x0[r] = (float)(s * inv_hw);
}

__global__ __launch_bounds__(TB) void k_attr_sums(const double* __restrict__ part, int rows, int n, double* __restrict__ out) {
    const int r = blockIdx.x * TB + threadIdx.x;
    if (r >= rows) return;
    double s = 0.0;
#pragma unroll 8
    for (int k = 0; k < n; ++k) s += part[(size_t)r * n + k];
    out[r] = s;
}

__device__ __forceinline__ float path_point(float x, float x0, float alpha) {
#pragma clang fp contract(off)
    const float d = x - x0;
    return x0 + alpha * d;               // two roundings, as the float32 statement of the definition has them (no fma)
}

// grid-stride over the batch's float4s; n_slice = hw * C is a multiple of 4, so a float4 never straddles two slices
__global__ __launch_bounds__(TB) void k_attr_path_in_v4(const float4* __restrict__ x, const float* __restrict__ x0, float alpha, size_t n4,
                                                        size_t n_slice, int C, float4* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * TB + threadIdx.x; i < n4; i += (size_t)gridDim.x * TB) {
        const size_t e = i * 4, b = e / n_slice;
        int c = (int)((e - b * n_slice) % C);
        const float* t = x0 ? x0 + b * C : nullptr;
        const float4 v = x[i];
        float r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r[j] = path_point(r[j], t ? t[c] : 0.f, alpha);
            c = c + 1 == C ? 0 : c + 1;
        }
        out[i] = make_float4(r[0], r[1], r[2], r[3]);
    }
}

// the scalar form: any hw * C
__global__ __launch_bounds__(TB) void k_attr_path_in(const float* __restrict__ x, const float* __restrict__ x0, float alpha, size_t n,
                                                     size_t n_slice, int C, float* __restrict__ out) {
    for (size_t e = (size_t)blockIdx.x * TB + threadIdx.x; e < n; e += (size_t)gridDim.x * TB) {
        const size_t b = e / n_slice;
        const int c = (int)((e - b * n_slice) % C);
        out[e] = path_point(x[e], x0 ? x0[b * C + c] : 0.f, alpha);
    }
}

// The grid and the descriptors of k_sens_first.  A descriptor owns the channels [chan, chan + nci) of every pixel of its conv's
// image, a block a run of tiles, a thread one pixel of a tile: (pixel, channel) has ONE writer, which the host has checked
// (Model::integrated_gradients).  The C floats of a pixel are contiguous: a thread's nci = 4 channels go out as one 16-byte store
// when c_total and chan are multiples of 4 (then the address is 16-byte aligned), as nci scalars otherwise -- neighbouring lanes
// write neighbouring pixels, so a wave's scalar stores still fill whole lines at C = 3.
__global__ __launch_bounds__(TB) void k_attr_first(const SensFirst* __restrict__ descs, int H, int W, int K, int tiles_x, int ntiles, int tpb,
                                                   int c_total, float* __restrict__ accum, int first) {
    extern __shared__ float lds[];
    const SensFirst d = descs[blockIdx.z];
    const int b = blockIdx.y, tid = threadIdx.x, lx = tid % kSensTile, ly = tid / kSensTile;
    const bool vec = d.nci == 4 && (c_total & 3) == 0 && (d.chan & 3) == 0;
    const int t_end = min(ntiles, ((int)blockIdx.x + 1) * tpb);
    for (int t = (int)blockIdx.x * tpb; t < t_end; ++t) {
        const int ty0 = (t / tiles_x) * kSensTile, tx0 = (t % tiles_x) * kSensTile;
        float acc[kSensCi];
        sens_first_tile<TB>(d, b, H, W, K, ty0, tx0, lds, acc);
        const int iy = ty0 + ly, ix = tx0 + lx;
        if (iy < H && ix < W) {
            float* o = accum + (((size_t)b * H + iy) * W + ix) * c_total + d.chan;
            if (vec) {
                float4 v = make_float4(acc[0], acc[1], acc[2], acc[3]);
                if (!first) {
                    const float4 p = *(const float4*)o;
                    v = make_float4(p.x + v.x, p.y + v.y, p.z + v.z, p.w + v.w);
                }
                *(float4*)o = v;
            } else {
#pragma unroll
                for (int j = 0; j < kSensCi; ++j)
                    if (j < d.nci) o[j] = first ? acc[j] : o[j] + acc[j];
            }
        }
    }
}

// grid (blocks per slice, B)
__global__ __launch_bounds__(TB) void k_attr_finish(float* accum, const float* __restrict__ x, const float* __restrict__ x0, float steps,
                                                    size_t hw, int C, int write_map, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double red[TB];
    const int L = lanes_of(C), tid = threadIdx.x, b = blockIdx.y;
    const size_t n = hw * C, e0 = (size_t)blockIdx.x * kAttrBlockPix * C, e1 = min(n, e0 + (size_t)kAttrBlockPix * C);
    const float* xs = x + (size_t)b * n;
    float* as = accum + (size_t)b * n;
    double s = 0.0, sa = 0.0;
    if (tid < L) {
        const float base = x0 ? x0[(size_t)b * C + tid % C] : 0.f;
        for (size_t e = e0 + tid; e < e1; e += L) {
            const float a = (xs[e] - base) * (as[e] / steps);
            if (write_map) as[e] = a;
            s += (double)a;
            sa += (double)fabsf(a);
        }
    }
    const double r0 = channel_sum(s, C, red);
    const double r1 = channel_sum(sa, C, red);
    if (tid < C) {
        double* p = part + ((size_t)b * C + tid) * 2 * gridDim.x + blockIdx.x;
        p[0] = r0;
        p[gridDim.x] = r1;
    }
}

// grid (blocks per slice, B): kAttrBlockPix / TB pixels per thread
__global__ __launch_bounds__(TB) void k_attr_prob_part(const float* __restrict__ logits, size_t hw, double* __restrict__ part) {
    __shared__ double wpart[TB / 64];
    const size_t p0 = (size_t)blockIdx.x * kAttrBlockPix, p1 = min(hw, p0 + (size_t)kAttrBlockPix);
    const float* z = logits + (size_t)blockIdx.y * hw;
    double v = 0.0;
    for (size_t p = p0 + threadIdx.x; p < p1; p += TB) v += 1.0 / (1.0 + exp(-(double)z[p]));
    v = wave_sum_f64(v);
    if ((threadIdx.x & 63) == 0) wpart[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wpart[0];
        for (int w = 1; w < TB / 64; ++w) s += wpart[w];
        part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

unsigned stream_blocks(size_t n) { return (unsigned)std::min<size_t>((n + TB - 1) / TB, 256 * 16); }

}  // namespace

void g_attr_baseline_part(hipStream_t s, const float* x, int B, size_t hw, int C, double* part) {
    hipLaunchKernelGGL(k_attr_baseline_part, dim3(attr_blocks(hw), B), dim3(TB), 0, s, x, hw, C, part);
}

void g_attr_baseline(hipStream_t s, const double* part, int B, size_t hw, int C, float* x0) {
    hipLaunchKernelGGL(k_attr_baseline, dim3((B * C + TB - 1) / TB), dim3(TB), 0, s, part, B * C, attr_blocks(hw), 1.0 / (double)hw, x0);
}

void g_attr_path_in(hipStream_t s, const float* x, const float* x0, float alpha, int B, size_t hw, int C, float* out) {
    const size_t n_slice = hw * C, n = n_slice * B;
    if (n_slice % 4 == 0)
        hipLaunchKernelGGL(k_attr_path_in_v4, dim3(stream_blocks(n / 4)), dim3(TB), 0, s, (const float4*)x, x0, alpha, n / 4, n_slice, C,
                           (float4*)out);
    else
        hipLaunchKernelGGL(k_attr_path_in, dim3(stream_blocks(n)), dim3(TB), 0, s, x, x0, alpha, n, n_slice, C, out);
}

void g_attr_first(hipStream_t s, const SensFirst* descs_dev, int nz, int B, int H, int W, int K, int c_total, const SensFirstGrid& g,
                  float* acc, int first) {
    hipLaunchKernelGGL(k_attr_first, dim3((unsigned)g.nblk, (unsigned)B, (unsigned)nz), dim3(TB), sens_first_lds(K), s, descs_dev, H, W, K,
                       g.tiles_x, g.ntiles, g.tpb, c_total, acc, first);
}

void g_attr_finish(hipStream_t s, float* acc, const float* x, const float* x0, int steps, int B, size_t hw, int C, int write_map,
                   double* part) {
    hipLaunchKernelGGL(k_attr_finish, dim3(attr_blocks(hw), B), dim3(TB), 0, s, acc, x, x0, (float)steps, hw, C, write_map, part);
}

void g_attr_sums(hipStream_t s, const double* part, int rows, int n, double* out) {
    hipLaunchKernelGGL(k_attr_sums, dim3((rows + TB - 1) / TB), dim3(TB), 0, s, part, rows, n, out);
}

void g_attr_prob_part(hipStream_t s, const float* logits, int B, size_t hw, double* part) {
    hipLaunchKernelGGL(k_attr_prob_part, dim3(attr_blocks(hw), B), dim3(TB), 0, s, logits, hw, part);
}

}  // namespace dnnca
