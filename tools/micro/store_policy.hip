// micro-benchmark: what does a streaming kernel's store flavour cost, and what does it leave behind for the next kernel?
// A writer streams N MB in the step's access shapes -- the strip kernels' row segments (60 of 64 lanes x 12 B per 720-B segment),
// the same segment as whole 16-byte stores (45 lanes x 16 B), the MFMA kernels' tile rows (48 lanes x 16 B = 768 B) -- with plain
// (aux 0) and write-through (aux 16 = sc1) buffer stores.  Timed: the writer alone, writer + a dependent trivial kernel, writer +
// a kernel that reads the bytes back.  Every figure is per iteration of a back-to-back chain on one stream, so "write" already holds
// one dependent boundary behind the writer (the next writer waits for its dirty lines like any other kernel would): the dirty tail's
// price is write(aux 0) - write(aux 16); "+read - write" is what the consumer pays for finding the lines in L2 or not.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
typedef float f3 __attribute__((ext_vector_type(3)));
typedef unsigned u3 __attribute__((ext_vector_type(3)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));
constexpr unsigned OOR = 0x40000000u;      // byte offset past every buffer here: the store is dropped

// SHAPE 0: 60 lanes x 12 B, 1: 45 lanes x 16 B (both: 720-B segments), 2: 48 lanes x 16 B (768-B segments), 3: 64 lanes x 16 B
template <int SHAPE, int AUX>
__global__ __launch_bounds__(256) void k_write(float* p, unsigned nbytes, unsigned nseg) {
    constexpr unsigned SEG = SHAPE == 2 ? 768u : (SHAPE == 3 ? 1024u : 720u);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, nbytes, 0x00020000u);
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned nw = gridDim.x * 4;
    unsigned col;
    if (SHAPE == 0) col = lane >= 2 && lane < 62 ? (lane - 2) * 12u : OOR;
    else col = lane * 16u < SEG ? lane * 16u : OOR;
    const float v = (float)lane;
    // a wave walks "rows": consecutive waves take adjacent segments (whole rows are in flight together), as the strip kernels do
    for (unsigned s = blockIdx.x * 4 + wave; s < nseg; s += nw) {
        const unsigned off = col + s * SEG;
        if (SHAPE == 0) __builtin_amdgcn_raw_buffer_store_b96(__builtin_bit_cast(u3, f3{v, v, v}), rs, off, 0, AUX);
        else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, make_float4(v, v, v, v)), rs, off, 0, AUX);
    }
}
__global__ void k_one(float* p) { if (threadIdx.x == 0 && blockIdx.x == 0) p[0] += 1.f; }
__global__ __launch_bounds__(256) void k_read(const float4* p, size_t n4, float* out) {
    float a = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) { const float4 v = p[i]; a += v.x + v.y + v.z + v.w; }
    if (a == -1.f) out[0] = a;
}

int main(int argc, char** argv) {
    float *buf, *out;
    hipMalloc(&buf, 256u << 20);
    hipMalloc(&out, 256);
    hipMemset(buf, 0, 256u << 20);
    hipStream_t s; hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    auto run = [&](int reps, auto body) {
        float best = 1e9;
        for (int r = 0; r < 5; ++r) {
            hipEventRecord(e0, s);
            for (int i = 0; i < reps; ++i) body();
            hipEventRecord(e1, s);
            hipEventSynchronize(e1);
            float ms; hipEventElapsedTime(&ms, e0, e1);
            if (ms < best) best = ms;
        }
        return best * 1e3f / reps;
    };
    const int R = 200;
    const float t_one = run(R, [&] { hipLaunchKernelGGL(k_one, dim3(1), dim3(64), 0, s, out); });
    printf("trivial kernel alone: %.2f us per launch (back to back)\n", t_one);
    printf("%-8s %-22s %-4s %9s %9s %9s %9s %9s %9s\n", "MB", "shape", "aux", "write", "GB/s", "+trivial", "tail", "+read", "read");
    const char* names[4] = {"60 lanes x 12 B", "45 lanes x 16 B", "48 lanes x 16 B", "64 lanes x 16 B"};
    const double mbs[4] = {6.0, 12.6, 25.0, 50.0};
    for (double mb : mbs) {
        for (int shape = 0; shape < 4; ++shape) {
            const unsigned seg = shape == 2 ? 768u : (shape == 3 ? 1024u : 720u);
            const unsigned nseg = (unsigned)(mb * 1e6 / seg);
            const unsigned nbytes = nseg * seg;
            const size_t n4 = nbytes / 16;
            const float t_read = run(R, [&] { hipLaunchKernelGGL(k_read, dim3(2048), dim3(256), 0, s, (const float4*)buf, n4, out); });
            for (int aux : {0, 16}) {
                auto wr = [&] {
#define W(S, A) hipLaunchKernelGGL((k_write<S, A>), dim3(2048), dim3(256), 0, s, buf, nbytes, nseg)
                    if (aux == 0) { if (shape == 0) W(0, 0); else if (shape == 1) W(1, 0); else if (shape == 2) W(2, 0); else W(3, 0); }
                    else { if (shape == 0) W(0, 16); else if (shape == 1) W(1, 16); else if (shape == 2) W(2, 16); else W(3, 16); }
#undef W
                };
                const float t_w = run(R, wr);
                const float t_w1 = run(R, [&] { wr(); hipLaunchKernelGGL(k_one, dim3(1), dim3(64), 0, s, out); });
                const float t_wr = run(R, [&] { wr(); hipLaunchKernelGGL(k_read, dim3(2048), dim3(256), 0, s, (const float4*)buf, n4, out); });
                // tail: what the pair costs beyond the writer chain and the trivial kernel chain
                printf("%-8.1f %-22s %-4d %9.2f %9.0f %9.2f %9.2f %9.2f %9.2f\n", mb, names[shape], aux, t_w, nbytes / t_w * 1e-3, t_w1, t_w1 - t_w - t_one,
                       t_wr, t_wr - t_w);
            }
            printf("%-8.1f %-22s %-4s read alone (cold, back to back) %9.2f us\n", mb, names[shape], "-", t_read);
        }
    }
    return 0;
}
