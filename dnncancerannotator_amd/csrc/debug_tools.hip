// debug_tools.hip -- development aids (NOT part of include/dnnca.h and not used by the product path):
// micro-benchmarks that calibrate what the conv kernels can expect from the f32 matrix pipe, a read-back of the BatchNorm
// reduction table for the tests, and the residual-join kernels on caller-supplied tensors.
#include "abi.h"
#include "fast.h"
#include "kernels.h"
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace dnnca;

// development aid: raw issue rate of v_mfma_f32_16x16x4_f32.  mode 0: operands in registers; mode 1: A operand from LDS
// (one ds_read_b32 per MFMA, stride-12 float pattern of the conv kernels); mode 2: A and B from LDS.
typedef float dbg_f32x4 __attribute__((ext_vector_type(4)));
template <int MODE, int NCH>
__global__ __launch_bounds__(512) void k_mfma_rate(float* out, int iters) {
    __shared__ float lds[16384];
    for (int i = threadIdx.x; i < 16384; i += 512) lds[i] = (float)(i & 7) * 0.125f;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    dbg_f32x4 acc[NCH];
    for (int c = 0; c < NCH; ++c) acc[c] = dbg_f32x4{0.f, 0.f, 0.f, 0.f};
    float a = 1.0f + lane * 0.001f, b = 0.5f;
    const int base = wave * 1024 + (lane & 15) * 12 + (lane >> 4);
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int k = 0; k < 16; ++k)
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                float av = MODE >= 1 ? lds[base + c * 200 + 4 * k + (it & 1) * 64] : a;
                float bv = MODE == 2 ? lds[8192 + base + 4 * k + (it & 1) * 64] : b;
                acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[c], 0, 0, 0);
            }
    }
    float s = 0.f;
    for (int c = 0; c < NCH; ++c) s += acc[c][0] + acc[c][1] + acc[c][2] + acc[c][3];
    out[blockIdx.x * 512 + threadIdx.x] = s;
}

extern "C" {

int dnnca_debug_mfma_rate(void* model, int mode, int nch, int blocks, int iters, float* tflops) {
    MODEL(model);
    float* buf = nullptr;
    HIP_TRY(hipMalloc(&buf, (size_t)blocks * 512 * 4));
    auto launch = [&]() {
        if (mode == 0 && nch == 1) hipLaunchKernelGGL((k_mfma_rate<0, 1>), dim3(blocks), dim3(512), 0, M->stream, buf, iters);
        if (mode == 0 && nch == 2) hipLaunchKernelGGL((k_mfma_rate<0, 2>), dim3(blocks), dim3(512), 0, M->stream, buf, iters);
        if (mode == 0 && nch == 4) hipLaunchKernelGGL((k_mfma_rate<0, 4>), dim3(blocks), dim3(512), 0, M->stream, buf, iters);
        if (mode == 1 && nch == 2) hipLaunchKernelGGL((k_mfma_rate<1, 2>), dim3(blocks), dim3(512), 0, M->stream, buf, iters);
        if (mode == 1 && nch == 4) hipLaunchKernelGGL((k_mfma_rate<1, 4>), dim3(blocks), dim3(512), 0, M->stream, buf, iters);
        if (mode == 2 && nch == 4) hipLaunchKernelGGL((k_mfma_rate<2, 4>), dim3(blocks), dim3(512), 0, M->stream, buf, iters);
    };
    launch();
    HIP_TRY(hipStreamSynchronize(M->stream));
    HIP_TRY(hipEventRecord(M->ev0, M->stream));
    launch();
    HIP_TRY(hipEventRecord(M->ev1, M->stream));
    HIP_TRY(hipEventSynchronize(M->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, M->ev0, M->ev1));
    double flops = (double)blocks * 8 * iters * 16 * nch * 2048.0;
    *tflops = (float)(flops / (ms * 1e-3) / 1e12);
    (void)hipFree(buf);
    return DNNCA_OK;
}

// test aid (tests/test_engine_gpu.py): what the self-folding BatchNorm reductions left in their table (csrc/bn_dev.h) -- the bucket
// rows and the ticket counters must read back as zero after every step.  Synchronises the stream.
int dnnca_debug_bn_table(void* model, double* abs_sum, unsigned* ticket_sum, int* allocated) {
    MODEL(model);
    *abs_sum = 0.0;
    *ticket_sum = 0u;
    *allocated = M->bn_tab != nullptr;
    if (!M->bn_tab) return DNNCA_OK;
    HIP_TRY(hipStreamSynchronize(M->stream));
    std::vector<double> h(Model::kBnTab + 32);
    HIP_TRY(hipMemcpy(h.data(), M->bn_tab, h.size() * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < Model::kBnTab; ++i) *abs_sum += h[i] < 0 ? -h[i] : h[i];
    const unsigned* t = reinterpret_cast<const unsigned*>(h.data() + Model::kBnTab);
    for (int i = 0; i < 64; ++i) *ticket_sum += t[i];
    return DNNCA_OK;
}

// test aid (tests/test_pgbwd_tc3_gpu.py): the two data gradients the backward launch of the last decoder block writes (k_pgbwd TCF),
// as they stand in their buffers after a train step of `batch` images: the gradient of the skip source of the two-source 3-channel conv
// [batch, H, W, 3] and the gradient of the 6 -> 3 transposed conv's input [batch, H/2, W/2, 6].  Sizes in floats; synchronises.
// (Every tensor of the plan has a data and a gradient buffer of its own for the life of the model -- nothing is reused within a step;
// later backward launches read these two buffers and do not write them, except the in-place act' of a conv that is not `premasked`.)
int dnnca_debug_tcf_dgrads(void* model, int batch, float* dskip, size_t n_skip, float* dtcin, size_t n_tcin) {
    MODEL(model);
    for (size_t i = M->ops.size(); i-- > 1;) {
        const Op& o = M->ops[i];
        const Op& tc = M->ops[i - 1];
        if (o.type != OP_CONV || !o.inB.d.C || o.inA.d.C != 3 || o.inB.d.C != 3 || o.out.d.C != 3) continue;
        if (tc.type != OP_TCONV || tc.inA.d.C != 6 || tc.out.d.p != o.inA.d.p) continue;
        const size_t ns = (size_t)batch * o.out.d.H * o.out.d.W * 3, nt = (size_t)batch * tc.inA.d.H * tc.inA.d.W * 6;
        if (ns != n_skip || nt != n_tcin || !o.inB.g.p || !tc.inA.g.p) { set_error("dnnca_debug_tcf_dgrads: sizes %zu / %zu expected", ns, nt); return DNNCA_EINVAL; }
        HIP_TRY(hipStreamSynchronize(M->stream));
        HIP_TRY(hipMemcpy(dskip, o.inB.g.p, ns * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(dtcin, tc.inA.g.p, nt * 4, hipMemcpyDeviceToHost));
        return DNNCA_OK;
    }
    set_error("dnnca_debug_tcf_dgrads: no two-source 3-channel conv behind a 6 -> 3 transposed conv");
    return DNNCA_EINVAL;
}

// test aid (tests/test_multires_gpu.py): the residual-join kernels (kernels_join.hip; generic != 0: g_join_fwd / g_join_bwd) alone.
// Every tensor is a host array of npix = B * H * W pixels with `ps` floats each, of which the kernels see channels [c0, c0 + C)
// (ps == C, c0 == 0: dense, the float4 walk; else the strided walk).  grid > 0 forces that many blocks.
//   what 0  forward, training: in0 = a, in1 = b -> io0 = relu(a + b) (channels outside the view keep what io0 held), sums[C] = channel sums
//   what 1  inference: coef[2 C] = scale, shift -> io0 = relu(a + b) * scale + shift
//   what 2  backward: in0 = dr, in1 = r; io0 = dA, io1 = dB in and out, acc0 / acc1: add to what they hold
int dnnca_debug_join(void* model, int what, int B, int H, int W, int C, int ps, int c0, int grid, int generic, const float* in0,
                     const float* in1, float* io0, float* io1, const float* coef, double* sums, int acc0, int acc1) {
    MODEL(model);
    if (what < 0 || what > 2 || B < 1 || H < 1 || W < 1 || C < 1 || c0 < 0 || c0 + C > ps || !in0 || !in1 || !io0 || (what == 2 && !io1) ||
        (what == 1 && !coef) || (generic && what == 1)) { set_error("dnnca_debug_join: bad arguments"); return DNNCA_EINVAL; }
    const size_t n = (size_t)B * H * W * ps;
    float* dev = nullptr;          // four tensors, each padded to a multiple of four floats so that every base stays 16-byte aligned
    const size_t n4 = (n + 3) / 4 * 4;
    double* dsum = nullptr;
    unsigned* ticket = nullptr;
    float* dcoef = nullptr;
    const unsigned rows = (unsigned)(grid > 0 ? grid : 0) + (unsigned)((C + 255) / 256);
    const size_t part = std::max(join_part_doubles(C), (size_t)rows * C);
    hipStream_t s = M->stream;
    int rc = DNNCA_OK;
    auto body = [&]() -> int {          // (whatever it allocated is freed behind it, on an error too)
        HIP_TRY(hipMalloc(&dev, 4 * n4 * 4));
        HIP_TRY(hipMalloc(&dsum, (2 * (size_t)C + part) * 8));
        HIP_TRY(hipMalloc(&ticket, 16));
        HIP_TRY(hipMalloc(&dcoef, 2 * (size_t)C * 4));
        HIP_TRY(hipMemsetAsync(ticket, 0, 16, s));
        HIP_TRY(hipMemsetAsync(dsum, 0xff, (2 * (size_t)C + part) * 8, s));          // NaN patterns: whatever is read must have been written
        HIP_TRY(hipMemcpyAsync(dev, in0, n * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(dev + n4, in1, n * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(dev + 2 * n4, io0, n * 4, hipMemcpyHostToDevice, s));
        if (io1) HIP_TRY(hipMemcpyAsync(dev + 3 * n4, io1, n * 4, hipMemcpyHostToDevice, s));
        if (coef) HIP_TRY(hipMemcpyAsync(dcoef, coef, 2 * (size_t)C * 4, hipMemcpyHostToDevice, s));
        View v[4];
        for (int k = 0; k < 4; ++k) { v[k].p = dev + k * n4 + c0; v[k].H = H; v[k].W = W; v[k].C = C; v[k].ps = ps; }
        if (what == 0) {
            if (generic) g_join_fwd(s, B, v[0], v[1], v[2]);
            else join_fwd(s, B, v[0], v[1], v[2], sums ? dsum : nullptr, dsum + 2 * C, ticket, grid);
        } else if (what == 1) {
            join_infer(s, B, v[0], v[1], v[2], dcoef, grid);
        } else {
            if (generic) g_join_bwd(s, B, v[0], v[1], v[2], acc0, v[3], acc1);
            else join_bwd(s, B, v[0], v[1], v[2], acc0, v[3], acc1, grid);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(io0, dev + 2 * n4, n * 4, hipMemcpyDeviceToHost, s));
        if (io1) HIP_TRY(hipMemcpyAsync(io1, dev + 3 * n4, n * 4, hipMemcpyDeviceToHost, s));
        if (sums && what == 0 && !generic) HIP_TRY(hipMemcpyAsync(sums, dsum, (size_t)C * 8, hipMemcpyDeviceToHost, s));
        unsigned t[4] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpyAsync(t, ticket, 16, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (t[0]) { set_error("dnnca_debug_join: the ticket reads %u after the launch, not 0", t[0]); return DNNCA_ESTATE; }
        return DNNCA_OK;
    };
    rc = body();
    (void)hipStreamSynchronize(s);
    (void)hipFree(dev);
    (void)hipFree(dsum);
    (void)hipFree(ticket);
    (void)hipFree(dcoef);
    return rc;
}

// test aids (tests/layerwise.py): what a pass left in the plan's own tensors, one launch at a time.  Every tensor of a plan has a data
// and a gradient buffer of its own for the life of the model, so after forward() / a train step the stored inputs and the stored
// output of every launch are still there.  These three only synchronise the stream and copy; bf16 storage is widened on the host.

// One text line per Op, `key=value` tokens separated by blanks.  A view is H,W,C,ps,h(data),h(gradient),id: the id is the same for
// equal data base pointers (1, 2, ... in order of first appearance; 0: no tensor), so the reader learns who reads and writes what
// without seeing an address.  Returns DNNCA_EINVAL (and the size needed in the message) when `cap` is too small.
int dnnca_debug_ops(void* model, char* buf, size_t cap) {
    MODEL(model);
    static const char* kType[] = {"CONV", "BN", "POOL", "TCONV", "HEAD", "JOIN"};
    std::map<const float*, int> ids;
    std::string s;
    char t[512];
    auto view = [&](const char* key, const T& v) {
        int id = 0;
        if (v.d.C) {
            const float* base = v.d.p;
            auto it = ids.find(base);
            id = it != ids.end() ? it->second : (ids[base] = (int)ids.size() + 1);
        }
        snprintf(t, sizeof t, " %s=%d,%d,%d,%d,%d,%d,%d", key, v.d.H, v.d.W, v.d.C, v.d.ps, v.d.h, v.g.h, id);
        s += t;
    };
    for (size_t i = 0; i < M->ops.size(); ++i) {
        const Op& o = M->ops[i];
        snprintf(t, sizeof t, "op=%zu type=%s name=%s k=%d alpha=%.9g w_off=%lld b_off=%lld mm_off=%lld mv_off=%lld need_din=%d accA=%d accB=%d "
                 "maskA=%d maskB=%d premasked=%d mask_alpha=%.9g elided=%d src_bn=%d,%d", i, kType[o.type], o.name.c_str(), o.k, (double)o.alpha,
                 (long long)o.w_off, (long long)o.b_off, (long long)o.mm_off, (long long)o.mv_off, (int)o.need_din, (int)o.accA, (int)o.accB,
                 (int)o.maskA, (int)o.maskB, (int)o.premasked, (double)o.mask_alpha, (int)o.elided, o.src_bn[0], o.src_bn[1]);
        s += t;
        view("inA", o.inA); view("inB", o.inB); view("out", o.out);
        s += "\n";
    }
    if (!buf || s.size() + 1 > cap) { set_error("dnnca_debug_ops: %zu bytes needed", s.size() + 1); return DNNCA_EINVAL; }
    memcpy(buf, s.c_str(), s.size() + 1);
    return DNNCA_OK;
}

// The view `slot` (0 inA, 1 inB, 2 out) of op `op`, data (grad == 0) or gradient, as dense float32 [batch, H, W, C]: channel slices
// (ps > C) are gathered, bf16 storage is converted exactly.  n: floats `out` holds.
int dnnca_debug_tensor(void* model, int op, int slot, int grad, int batch, float* out, size_t n) {
    MODEL(model);
    if (op < 0 || op >= (int)M->ops.size() || slot < 0 || slot > 2 || !out) { set_error("dnnca_debug_tensor: no op %d / slot %d", op, slot); return DNNCA_EINVAL; }
    DN_TRY(check_batch(M, batch));
    const Op& o = M->ops[op];
    const T& t = slot == 0 ? o.inA : (slot == 1 ? o.inB : o.out);
    const View& v = grad ? t.g : t.d;
    if (!v.C || !v.p) { set_error("dnnca_debug_tensor: %s has no %s buffer in slot %d", o.name.c_str(), grad ? "gradient" : "data", slot); return DNNCA_EINVAL; }
    const size_t npix = (size_t)batch * v.H * v.W;
    if (n != npix * v.C) { set_error("dnnca_debug_tensor: %zu floats expected, not %zu", npix * v.C, n); return DNNCA_EINVAL; }
    const size_t stored = (npix - 1) * v.ps + v.C;          // elements from the view's first to its last
    HIP_TRY(hipStreamSynchronize(M->stream));
    if (v.h) {
        std::vector<uint16_t> h(stored);
        HIP_TRY(hipMemcpy(h.data(), v.p, stored * 2, hipMemcpyDeviceToHost));
        for (size_t p = 0; p < npix; ++p)
            for (int c = 0; c < v.C; ++c) {
                const uint32_t u = (uint32_t)h[p * v.ps + c] << 16;
                memcpy(out + p * v.C + c, &u, 4);
            }
    } else if (v.ps == v.C) {
        HIP_TRY(hipMemcpy(out, v.p, stored * 4, hipMemcpyDeviceToHost));
    } else {
        std::vector<float> h(stored);
        HIP_TRY(hipMemcpy(h.data(), v.p, stored * 4, hipMemcpyDeviceToHost));
        for (size_t p = 0; p < npix; ++p) memcpy(out + p * v.C, h.data() + p * v.ps, (size_t)v.C * 4);
    }
    return DNNCA_OK;
}

// The coefficient table [scale, shift, mean, inv] x C of BatchNorm `op` as the last forward pass left it (out: 4 C floats).
int dnnca_debug_bn_coef(void* model, int op, float* out) {
    MODEL(model);
    if (op < 0 || op >= (int)M->ops.size() || M->ops[op].type != OP_BN || !M->ops[op].coef || !out) { set_error("dnnca_debug_bn_coef: op %d is no BatchNorm", op); return DNNCA_EINVAL; }
    HIP_TRY(hipStreamSynchronize(M->stream));
    HIP_TRY(hipMemcpy(out, M->ops[op].coef, (size_t)4 * M->ops[op].inA.d.C * 4, hipMemcpyDeviceToHost));
    return DNNCA_OK;
}

}  // extern "C"
