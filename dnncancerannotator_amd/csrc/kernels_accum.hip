// kernels_accum.hip -- gradient accumulation (accum.h): one streaming launch over the flat gradient vector.  Memory-bound: 8 bytes
// per parameter when it starts a cycle (a = g), 12 when it adds (a += g).  16-byte loads and stores, at most kAccumMaxBlocks blocks
// with a grid-stride loop, no atomics and no LDS: every element has one owner and one float32 add per micro-step.
#include "accum.h"

namespace dnnca {

template <bool FIRST>
__global__ __launch_bounds__(kAccumThreads) void k_grad_accumulate(size_t n, float* __restrict__ a, const float* __restrict__ g,
                                                                   AdamFinalize fin, int loss_slot) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (fin.out5) step_outputs(fin);
        if (loss_slot) a[n] = g[n];
    }
    const size_t n4 = n / 4;
    const size_t stride = (size_t)gridDim.x * kAccumThreads;
    float4* __restrict__ a4 = reinterpret_cast<float4*>(a);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    for (size_t i = (size_t)blockIdx.x * kAccumThreads + threadIdx.x; i < n4; i += stride) {
        float4 x = g4[i];
        if (!FIRST) {
            const float4 y = a4[i];
            x.x = y.x + x.x; x.y = y.y + x.y; x.z = y.z + x.z; x.w = y.w + x.w;
        }
        a4[i] = x;
    }
    // the n % 4 elements behind the body: threads 0..2 of block 0
    const size_t k = 4 * n4 + threadIdx.x;
    if (blockIdx.x == 0 && k < n) a[k] = FIRST ? g[k] : a[k] + g[k];
}

void g_grad_accumulate(hipStream_t s, size_t n, float* a, const float* g, bool first, const AdamFinalize& fin, bool loss_slot) {
    const size_t need = (n / 4 + kAccumThreads - 1) / kAccumThreads;
    const unsigned grid = (unsigned)(need < 1 ? 1 : (need > (size_t)kAccumMaxBlocks ? (size_t)kAccumMaxBlocks : need));
    if (first) hipLaunchKernelGGL(k_grad_accumulate<true>, dim3(grid), dim3(kAccumThreads), 0, s, n, a, g, fin, loss_slot ? 1 : 0);
    else hipLaunchKernelGGL(k_grad_accumulate<false>, dim3(grid), dim3(kAccumThreads), 0, s, n, a, g, fin, loss_slot ? 1 : 0);
}

}  // namespace dnnca
