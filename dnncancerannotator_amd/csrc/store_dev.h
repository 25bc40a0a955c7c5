// store_dev.h -- the one way the step's kernels store activations and activation gradients (device code).
//
// What a store instruction leaves behind in the XCD's L2 is a policy of its own: a plain store keeps the line there, dirty, and
// the next kernel on the stream starts only after those lines have been written back; a write-through store (cache policy sc1 =
// aux 16 of the buffer-store builtins) sends the bytes on as they are stored and drops the line, so a kernel ends with a clean L2.
// The same values go to the same addresses either way.  Narrow write-through stores are expensive (one fabric write per lane),
// so the helper has a 16-byte, a 12-byte and a 4-byte form and the callers pick the widest their layout allows.
//
// Buffer-store builtins only: hipcc counts them in its s_waitcnt vmcnt(N) bookkeeping (an inline-asm store would leave every later
// counted wait one short), and a lane that must not store gets a byte offset at or beyond the descriptor's num_records -- the
// hardware drops the store, no predicate or branch goes around it.
//
// DNNCA_STORE_AUX: the build's policy (a compile-time constant: a run-time flag would put a uniform branch around every store, and
// hipcc then waits vmcnt(0) on the joins).  Default 16; -DDNNCA_STORE_AUX=0 gives plain stores everywhere (the A/B partner).  The
// per-group constants below can be set one by one (DNNCA_BUILD_TAG=<tag> DNNCA_EXTRA_FLAGS="-D..." python -m dnncancerannotator_amd.build).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

#ifndef DNNCA_STORE_AUX
#define DNNCA_STORE_AUX 16
#endif
// The strip kernels' 12-byte-per-lane rows keep plain stores whatever DNNCA_STORE_AUX says: with write-through stores the step got
// slower (profiles/r06_store_policy.txt: forward strips +0.9 %, k_tail3 +0.5 %); their constants are set on their own.
#ifndef DNNCA_STORE_AUX_STRIP       // forward strip kernels: k_first3_fwd, k_up3_fwd
#define DNNCA_STORE_AUX_STRIP 0
#endif
#ifndef DNNCA_STORE_AUX_TAIL        // k_tail3's data gradient
#define DNNCA_STORE_AUX_TAIL 0
#endif
#ifndef DNNCA_STORE_AUX_MFMA_FWD    // k_pgfwd, k_fz_up, k_fz_down
#define DNNCA_STORE_AUX_MFMA_FWD DNNCA_STORE_AUX
#endif
#ifndef DNNCA_STORE_AUX_MFMA_BWD    // k_pgbwd, k_fzb
#define DNNCA_STORE_AUX_MFMA_BWD DNNCA_STORE_AUX
#endif

namespace dnnca {

constexpr unsigned kStoreRsrc = 0x00020000u;        // raw buffer, 32-bit data format
constexpr unsigned kStoreNowhere = 0x80000000u;     // a byte offset past every descriptor built here: the store is dropped
constexpr unsigned long long kStoreMaxBytes = 0x80000000ull;      // a tensor (or image) addressed through one descriptor stays below 2^31 bytes

typedef unsigned store_u4 __attribute__((ext_vector_type(4)));
typedef unsigned store_u3 __attribute__((ext_vector_type(3)));
typedef unsigned store_u2 __attribute__((ext_vector_type(2)));

// the launchers' predicate: can `bytes` bytes be addressed with a 32-bit offset that leaves kStoreNowhere out of range?
__host__ __device__ constexpr bool store_fits(unsigned long long bytes) { return bytes < kStoreMaxBytes; }

// descriptor over [base, base + bytes); base is wave-uniform (it lives in scalar registers)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t store_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, kStoreRsrc);
}

template <int AUX>
__device__ __forceinline__ void store16(__amdgpu_buffer_rsrc_t rs, unsigned byte_offset, float4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(store_u4, v), rs, byte_offset, 0, AUX);
}
template <int AUX>
__device__ __forceinline__ void store12(__amdgpu_buffer_rsrc_t rs, unsigned byte_offset, float x, float y, float z) {
    const store_u3 u = {__builtin_bit_cast(unsigned, x), __builtin_bit_cast(unsigned, y), __builtin_bit_cast(unsigned, z)};
    __builtin_amdgcn_raw_buffer_store_b96(u, rs, byte_offset, 0, AUX);
}
template <int AUX>
__device__ __forceinline__ void store8(__amdgpu_buffer_rsrc_t rs, unsigned byte_offset, float2 v) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(store_u2, v), rs, byte_offset, 0, AUX);
}
template <int AUX>
__device__ __forceinline__ void store4(__amdgpu_buffer_rsrc_t rs, unsigned byte_offset, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs, byte_offset, 0, AUX);
}

}  // namespace dnnca
