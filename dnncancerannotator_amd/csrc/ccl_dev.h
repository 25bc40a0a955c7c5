// ccl_dev.h -- the union-find device helpers of the connected-component kernels (kernels_region.hip region_ccl_*, kernels_detect.hip
// det_ccl_*): int32 parents, -1 = background, parents only ever point to smaller indices, so a root is the smallest index of its
// component.  Device code only: include it from a .hip file.
#pragma once
#include <hip/hip_runtime.h>

namespace dnnca {

namespace {

__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int find_root(const int* L, int x) {
    int y;
    while ((y = ld_agent(L + x)) != x) x = y;
    return x;
}

// union by atomicMin on roots (Playne & Hawick 2018): the larger root is linked to the smaller one; a lost race retries from the
// value atomicMin returned
__device__ void unite(int* L, int a, int b) {
    for (;;) {
        a = find_root(L, a);
        b = find_root(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(L + b, a);
        if (old == b) return;
        b = old;
    }
}

__device__ __forceinline__ int lds_find(volatile int* l, int x) {
    int y;
    while ((y = l[x]) != x) x = y;
    return x;
}

}  // namespace

}  // namespace dnnca
