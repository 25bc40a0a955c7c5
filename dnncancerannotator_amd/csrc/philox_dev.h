// philox_dev.h -- the Philox4x32-10 counter generator (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3, SC'11)
// as one device function, shared by the noise of aug_intensity (kernels_aug.hip) and the draws of the bootstrap (kernels_bootstrap.hip).
// tests/intensity_oracle.py::philox4x32_10 states the same rounds in numpy.
#pragma once
#include <hip/hip_runtime.h>

namespace dnnca {

// the four output words of the counter (c0, c1, c2, c3) under the key (k0, k1)
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&r)[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = c0;
    r[1] = c1;
    r[2] = c2;
    r[3] = c3;
}

}  // namespace dnnca
