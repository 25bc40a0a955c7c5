// kernels_aug.hip -- train-time augmentation on the device: the reference's per-image tf.data maps
//   base():            centre crop to the stored size, cast to float32, / 255            (annotator/data.py:195-206)
//   random_crop():     crop to output_size at centre + clip(int(N(0, stddev)), min_, max_)  (data.py:677-689)
//   random_flip():     tf.image.random_flip_left_right                                     (data.py:620-625)
//   random_contrast(): (x - mean_hw(x)) * U[lower, upper) + mean_hw(x) on the feature channels (data.py:586-609)
//   to_feature_label() label channel -> y, the others in order -> x                        (data.py:766-788)
// in two launches over a uint8 batch that was uploaded as stored (a quarter of the float bytes over PCIe).  The random draws are
// made by the host (augment.py) and passed per image, so the arithmetic is checkable against the oracle draw for draw.
// random_warp (tfa.image.sparse_image_warp) follows below as dnnca_warp_f32, random_intrachannelwarp as dnnca_warp_groups_f32.
// random_affine (this project's own: rotation, zoom, shift and D4 view in one bilinear resampling) closes the file as dnnca_affine_f32.
#include <stdlib.h>
#include <string.h>
#include "fast.h"
#include "kernels.h"

namespace dnnca {

struct AugArgs {
    const unsigned char* src;    // [B, Hs, Ws, Cs] uint8
    const dnnca_aug_param* prm;  // [B] (device copy)
    unsigned* sums;              // [B, Cs] integer sums of the crop window (zeroed before the launch)
    float* x;                    // [B, Ho, Wo, Cs - 1]
    float* y;                    // [B, Ho, Wo]
    int B, Hs, Ws, Cs, Ho, Wo, label_index;
    unsigned contrast_mask;      // bit c set: source channel c is contrast-adjusted
};

constexpr int AUG_MAXC = 8;

__device__ __forceinline__ void aug_window(const AugArgs& p, int b, int& top, int& left, int& flip, float& f) {
    const dnnca_aug_param q = p.prm[b];
    top = (p.Hs - p.Ho) / 2 + q.dy;
    left = (p.Ws - p.Wo) / 2 + q.dx;
    flip = q.flip;
    f = q.contrast;
}

// integer sums of every source channel over the crop window of image blockIdx.y (exact: uint8 sums fit 32 bits up to 2^24 pixels)
__global__ __launch_bounds__(256) void k_aug_sums(AugArgs p) {
    __shared__ unsigned red[4][AUG_MAXC];
    const int b = blockIdx.y;
    int top, left, flip;
    float f;
    aug_window(p, b, top, left, flip, f);
    unsigned s[AUG_MAXC];
#pragma unroll
    for (int c = 0; c < AUG_MAXC; ++c) s[c] = 0;
    const int n = p.Ho * p.Wo;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int oy = i / p.Wo, ox = i - oy * p.Wo;
        const unsigned char* px = p.src + (((size_t)b * p.Hs + top + oy) * p.Ws + left + ox) * p.Cs;
#pragma unroll
        for (int c = 0; c < AUG_MAXC; ++c)
            if (c < p.Cs) s[c] += px[c];
    }
#pragma unroll
    for (int c = 0; c < AUG_MAXC; ++c) {
        unsigned v = s[c];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < p.Cs) atomicAdd(p.sums + b * p.Cs + threadIdx.x, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// one thread = one output pixel
__global__ __launch_bounds__(256) void k_aug_apply(AugArgs p) {
    const int n = p.Ho * p.Wo;
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (size_t)p.B * n) return;
    const int b = (int)(id / n), i = (int)(id - (size_t)b * n);
    const int oy = i / p.Wo, ox = i - oy * p.Wo;
    int top, left, flip;
    float f;
    aug_window(p, b, top, left, flip, f);
    const int sx = flip ? p.Wo - 1 - ox : ox;                       // flip of the cropped image
    const unsigned char* px = p.src + (((size_t)b * p.Hs + top + oy) * p.Ws + left + sx) * p.Cs;
    const float inv_n = 1.0f / (float)n;
    float* xo = p.x + id * (p.Cs - 1);
    int k = 0;
#pragma unroll
    for (int c = 0; c < AUG_MAXC; ++c) {
        if (c >= p.Cs) break;
        float v = (float)px[c] / 255.0f;
        if (c == p.label_index) {
            p.y[id] = v;
            continue;
        }
        if (((p.contrast_mask >> c) & 1u) && f != 1.0f) {      // factor 1 is the identity (and the host's "no contrast" value)
            const float mean = ((float)p.sums[b * p.Cs + c] * inv_n) / 255.0f;
            v = (v - mean) * f + mean;                                // tf.image.adjust_contrast (no clipping)
        }
        xo[k++] = v;
    }
}

}  // namespace dnnca

using namespace dnnca;

int dnnca_augment_u8(void* model, const void* src_dev, int batch, int hs, int ws, int cs, int label_index, unsigned contrast_mask,
                     const dnnca_aug_param* params_host, int ho, int wo, float* x_dev, float* y_dev) {
    Model* M = reinterpret_cast<Model*>(model);
    if (!M) { set_error("null model"); return DNNCA_EINVAL; }
    if (!src_dev || !params_host || !x_dev || !y_dev || batch < 1 || cs < 2 || cs > AUG_MAXC || label_index < 0 || label_index >= cs ||
        ho < 1 || wo < 1 || ho > hs || wo > ws) {
        set_error("dnnca_augment_u8: bad arguments (batch %d, %dx%dx%d -> %dx%d, label %d)", batch, hs, ws, cs, ho, wo, label_index);
        return DNNCA_EINVAL;
    }
    for (int b = 0; b < batch; ++b) {      // tf.image.crop_to_bounding_box asserts the window lies inside the image
        const int top = (hs - ho) / 2 + params_host[b].dy, left = (ws - wo) / 2 + params_host[b].dx;
        if (top < 0 || left < 0 || top + ho > hs || left + wo > ws) {
            set_error("dnnca_augment_u8: crop window of image %d leaves the %dx%d source (top %d, left %d, %dx%d)", b, hs, ws, top, left, ho, wo);
            return DNNCA_EINVAL;
        }
    }
    const size_t need = (size_t)batch * sizeof(dnnca_aug_param) + (size_t)batch * AUG_MAXC * 4;
    if (need > M->aug_scratch_bytes) {
        void* p = nullptr;
        DN_TRY(M->alloc(&p, need));
        M->aug_scratch = p;
        M->aug_scratch_bytes = need;
    }
    AugArgs a{};
    a.src = (const unsigned char*)src_dev;
    a.prm = (const dnnca_aug_param*)M->aug_scratch;
    a.sums = (unsigned*)((char*)M->aug_scratch + (size_t)batch * sizeof(dnnca_aug_param));
    a.x = x_dev; a.y = y_dev;
    a.B = batch; a.Hs = hs; a.Ws = ws; a.Cs = cs; a.Ho = ho; a.Wo = wo; a.label_index = label_index;
    a.contrast_mask = contrast_mask & ~(1u << label_index);
    // the draws travel through a pinned row of the model's ring: the caller's buffer is free when this call returns, and the call
    // does not wait for the stream (a row is only waited for when it comes round again, four calls later)
    const size_t prm_bytes = (size_t)batch * sizeof(dnnca_aug_param);
    if (prm_bytes > M->aug_pin_bytes) {
        HIP_TRY(hipStreamSynchronize(M->stream));         // uploads from the old rows are complete
        if (M->aug_pin) (void)hipHostFree(M->aug_pin);
        M->aug_pin = nullptr;
        M->aug_pin_bytes = 0;
        const size_t row = (size_t)M->desc.max_batch * sizeof(dnnca_aug_param) > prm_bytes ? (size_t)M->desc.max_batch * sizeof(dnnca_aug_param) : prm_bytes;
        HIP_TRY(hipHostMalloc(&M->aug_pin, row * Model::kAugRing, hipHostMallocDefault));
        M->aug_pin_bytes = row;
    }
    const int k = M->aug_k;
    M->aug_k = (k + 1) % Model::kAugRing;
    if (!M->aug_ev[k]) HIP_TRY(hipEventCreateWithFlags(&M->aug_ev[k], hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(M->aug_ev[k]));
    char* pin = (char*)M->aug_pin + (size_t)k * M->aug_pin_bytes;
    memcpy(pin, params_host, prm_bytes);
    HIP_TRY(hipMemcpyAsync((void*)a.prm, pin, prm_bytes, hipMemcpyHostToDevice, M->stream));
    HIP_TRY(hipEventRecord(M->aug_ev[k], M->stream));
    HIP_TRY(hipMemsetAsync(a.sums, 0, (size_t)batch * cs * 4, M->stream));
    const int n = ho * wo;
    int bx = (n + 256 * 16 - 1) / (256 * 16);
    if (bx > 64) bx = 64;
    if (a.contrast_mask)
        LAUNCH(M, "aug_sums", (double)batch * n * cs, 0, hipLaunchKernelGGL(k_aug_sums, dim3(bx, batch), dim3(256), 0, M->stream, a));
    LAUNCH(M, "aug_apply", (double)batch * n * (cs + 4.0 * cs), 0,
           hipLaunchKernelGGL(k_aug_apply, dim3((unsigned)(((size_t)batch * n + 255) / 256)), dim3(256), 0, M->stream, a));
    return DNNCA_OK;
}

// ------------------------------------------------------------------------------------------------ random_warp (dense part)
// annotator/data.py:725-763 random_warp -> tfa.image.sparse_image_warp(image, source = raw, dest = raw + diff), order 2:
//   flow(q) = sum_i phi(|q - c_i|^2) w_i + [q, 1] v        phi(r) = 0.5 r log(max(r, 1e-10))   (tfa interpolate_spline, order 2)
//   out(q)  = bilinear(image, q - flow(q))                  (tfa dense_image_warp / interpolate_bilinear, "ij" indexing)
// The (n+3) x (n+3) spline system is solved on the host (augment.solve_warp); here every output pixel evaluates its flow from the
// n control points c_i (the *destination* points) and the weights (w, v), and samples features and label with the same flow.
namespace dnnca {

// a launch gets 64 KB of dynamic LDS without opting in; the coefficients of one spline take n * 4 + 6 doubles of it
constexpr size_t WARP_LDS_MAX = 64u << 10;
constexpr int WARP_MAX_POINTS = (int)((WARP_LDS_MAX / 8 - 6) / 4);      // 2046

struct WarpArgs {
    const float* x;          // [B, H, W, C] source features
    const float* y;          // [B, H, W] source label
    const double* ctrl;      // [B, n, 2] control points (row, column)
    const double* wv;        // [B, n + 3, 2] spline weights w (n rows) then v (3 rows: row coefficient, column coefficient, constant)
    float* xo;
    float* yo;
    int B, H, W, C, n;
};

__global__ __launch_bounds__(256) void k_warp(WarpArgs p) {
    // The thin-plate weights cancel massively (|phi| ~ 1e4, flows ~ 1): the flow is evaluated in double (the float32 sum is only
    // good to ~1e-2 pixel, which is also all that tfa's own float32 evaluation is good for).
    extern __shared__ double sm[];         // control points + weights of this image: n * 4 + 6 doubles
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < p.n * 2; i += 256) {
        sm[i] = p.ctrl[(size_t)b * p.n * 2 + i];
        sm[p.n * 2 + i] = p.wv[(size_t)b * (p.n + 3) * 2 + i];
    }
    if (threadIdx.x < 6) sm[p.n * 4 + threadIdx.x] = p.wv[((size_t)b * (p.n + 3) + p.n) * 2 + threadIdx.x];
    __syncthreads();
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= p.H * p.W) return;
    const int qy = id / p.W, qx = id - qy * p.W;
    const float fqy = (float)qy, fqx = (float)qx;
    const double* v = sm + p.n * 4;
    double d0 = qy * v[0] + qx * v[2] + v[4];             // linear term [q, 1] v  (v rows: y, x, 1; columns: flow_y, flow_x)
    double d1 = qy * v[1] + qx * v[3] + v[5];
    for (int i = 0; i < p.n; ++i) {
        const double dy = qy - sm[2 * i], dx = qx - sm[2 * i + 1];
        const double r = dy * dy + dx * dx;
        const double ph = 0.5 * r * log(fmax(r, 1e-10));
        d0 = fma(ph, sm[p.n * 2 + 2 * i], d0);
        d1 = fma(ph, sm[p.n * 2 + 2 * i + 1], d1);
    }
    const float f0 = (float)d0, f1 = (float)d1;
    // interpolate_bilinear at (qy - f0, qx - f1): floor clamped to [0, size - 2], alpha clipped to [0, 1]
    const float sy = fqy - f0, sx = fqx - f1;
    const float fy = fminf(fmaxf(floorf(sy), 0.f), (float)(p.H - 2)), fx = fminf(fmaxf(floorf(sx), 0.f), (float)(p.W - 2));
    const float ay = fminf(fmaxf(sy - fy, 0.f), 1.f), ax = fminf(fmaxf(sx - fx, 0.f), 1.f);
    const int iy = (int)fy, ix = (int)fx;
    const size_t o00 = ((size_t)b * p.H + iy) * p.W + ix, o01 = o00 + 1, o10 = o00 + p.W, o11 = o10 + 1;
    const size_t oq = ((size_t)b * p.H + qy) * p.W + qx;
    auto lerp2 = [&](float tl, float tr, float bl, float br) {
        const float top = ax * (tr - tl) + tl, bot = ax * (br - bl) + bl;
        return ay * (bot - top) + top;
    };
    for (int c = 0; c < p.C; ++c)
        p.xo[oq * p.C + c] = lerp2(p.x[o00 * p.C + c], p.x[o01 * p.C + c], p.x[o10 * p.C + c], p.x[o11 * p.C + c]);
    p.yo[oq] = lerp2(p.y[o00], p.y[o01], p.y[o10], p.y[o11]);
}

}  // namespace dnnca

int dnnca_warp_f32(void* model, const float* x_dev, const float* y_dev, int batch, int h, int w, int c, int n_points,
                   const double* ctrl_host, const double* wv_host, float* x_out_dev, float* y_out_dev) {
    Model* M = reinterpret_cast<Model*>(model);
    if (!M) { set_error("null model"); return DNNCA_EINVAL; }
    if (!x_dev || !y_dev || !ctrl_host || !wv_host || !x_out_dev || !y_out_dev || batch < 1 || h < 2 || w < 2 || c < 1 || n_points < 1 ||
        x_out_dev == x_dev || y_out_dev == y_dev) {
        set_error("dnnca_warp_f32: bad arguments");
        return DNNCA_EINVAL;
    }
    if (n_points > WARP_MAX_POINTS) {
        set_error("dnnca_warp_f32: %d control points, at most %d (their %zu bytes of coefficients must fit %zu bytes of LDS)", n_points,
                  WARP_MAX_POINTS, (size_t)(n_points * 4 + 6) * 8, WARP_LDS_MAX);
        return DNNCA_EINVAL;
    }
    const size_t nc = (size_t)batch * n_points * 2 * 8, nw = (size_t)batch * (n_points + 3) * 2 * 8;
    if (nc + nw > M->warp_scratch_bytes) {
        void* p = nullptr;
        DN_TRY(M->alloc(&p, nc + nw));
        M->warp_scratch = p;
        M->warp_scratch_bytes = nc + nw;
    }
    WarpArgs a{};
    a.x = x_dev; a.y = y_dev; a.xo = x_out_dev; a.yo = y_out_dev;
    a.ctrl = (const double*)M->warp_scratch;
    a.wv = (const double*)((char*)M->warp_scratch + nc);
    a.B = batch; a.H = h; a.W = w; a.C = c; a.n = n_points;
    HIP_TRY(hipMemcpyAsync((void*)a.ctrl, ctrl_host, nc, hipMemcpyHostToDevice, M->stream));
    HIP_TRY(hipMemcpyAsync((void*)a.wv, wv_host, nw, hipMemcpyHostToDevice, M->stream));
    LAUNCH(M, "aug_warp", (double)batch * h * w * (c + 1) * 8.0, (double)batch * h * w * n_points * 8.0,
           hipLaunchKernelGGL(k_warp, dim3((h * w + 255) / 256, batch), dim3(256), (size_t)(n_points * 4 + 6) * 8, M->stream, a));
    HIP_TRY(hipStreamSynchronize(M->stream));
    return DNNCA_OK;
}

// ------------------------------------------------------------------------------------- random_intrachannelwarp (dense part)
// annotator/data.py:692-715 random_intrachannelwarp: the channels of a slice, label included, are split into groups (the `paired`
// lists, then every other channel on its own) and every group goes through a random_warp of its own (data.py:706), so the
// modalities slide against each other while a paired channel stays on its label.  The arithmetic per group is that of k_warp; here
// one launch serves every group of every image.
namespace dnnca {

struct WarpGroupsArgs {
    const float* x;          // [B, H, W, C] source features
    const float* y;          // [B, H, W] source label
    const double* ctrl;      // [B, G, n, 2] control points (row, column) of every group
    const double* wv;        // [B, G, n + 3, 2] spline weights of every group (rows as in WarpArgs)
    const int* group_of;     // [C + 1] group of feature channel c; entry C: the label
    float* xo;
    float* yo;
    int B, H, W, C, G, n;
};

// control points + weights of group g of image b into sm (n * 4 + 6 doubles, the layout of k_warp); the caller synchronises
__device__ __forceinline__ void warp_coeffs_to_lds(const WarpGroupsArgs& p, int b, int g, double* sm) {
    const size_t bg = (size_t)b * p.G + g;
    for (int i = threadIdx.x; i < p.n * 2; i += 256) {
        sm[i] = p.ctrl[bg * p.n * 2 + i];
        sm[p.n * 2 + i] = p.wv[bg * (p.n + 3) * 2 + i];
    }
    if (threadIdx.x < 6) sm[p.n * 4 + threadIdx.x] = p.wv[(bg * (p.n + 3) + p.n) * 2 + threadIdx.x];
}

// the bilinear taps of output pixel (qy, qx) under the spline in sm: flow in double (see k_warp), then tfa's interpolate_bilinear
// at q - flow with the floor clamped to [0, size - 2] and alpha clipped to [0, 1] -- the clamps keep every tap inside the image
// however far the flow throws the position (max_diff 100 in the shipped overlays)
struct WarpTaps {
    int iy, ix;
    float ay, ax;
    __device__ __forceinline__ float operator()(float tl, float tr, float bl, float br) const {
        const float top = ax * (tr - tl) + tl, bot = ax * (br - bl) + bl;
        return ay * (bot - top) + top;
    }
};

__device__ __forceinline__ WarpTaps warp_taps(const double* sm, int n, int H, int W, int qy, int qx) {
    const double* v = sm + n * 4;
    double d0 = qy * v[0] + qx * v[2] + v[4];
    double d1 = qy * v[1] + qx * v[3] + v[5];
    for (int i = 0; i < n; ++i) {
        const double dy = qy - sm[2 * i], dx = qx - sm[2 * i + 1];
        const double r = dy * dy + dx * dx;
        const double ph = 0.5 * r * log(fmax(r, 1e-10));
        d0 = fma(ph, sm[n * 2 + 2 * i], d0);
        d1 = fma(ph, sm[n * 2 + 2 * i + 1], d1);
    }
    const float sy = (float)qy - (float)d0, sx = (float)qx - (float)d1;
    const float fy = fminf(fmaxf(floorf(sy), 0.f), (float)(H - 2)), fx = fminf(fmaxf(floorf(sx), 0.f), (float)(W - 2));
    WarpTaps t;
    t.ay = fminf(fmaxf(sy - fy, 0.f), 1.f);
    t.ax = fminf(fmaxf(sx - fx, 0.f), 1.f);
    t.iy = (int)fy;
    t.ix = (int)fx;
    return t;
}

// the channels of group g (and the label when it is in g) of output pixel (qy, qx) of image b
__device__ __forceinline__ void warp_group_sample(const WarpGroupsArgs& p, int b, int g, int qy, int qx, const WarpTaps& t) {
    const size_t o00 = ((size_t)b * p.H + t.iy) * p.W + t.ix, o01 = o00 + 1, o10 = o00 + p.W, o11 = o10 + 1;
    const size_t oq = ((size_t)b * p.H + qy) * p.W + qx;
    for (int c = 0; c < p.C; ++c)
        if (p.group_of[c] == g)
            p.xo[oq * p.C + c] = t(p.x[o00 * p.C + c], p.x[o01 * p.C + c], p.x[o10 * p.C + c], p.x[o11 * p.C + c]);
    if (p.group_of[p.C] == g) p.yo[oq] = t(p.y[o00], p.y[o01], p.y[o10], p.y[o11]);
}

// PIXEL false: one group per block (blockIdx.z): n * 4 + 6 doubles of LDS, every lane of the block in the same n-term loop; a thread
//              writes only its group's channels of the pixel.
// PIXEL true:  one pixel per thread, the groups in a loop: G * (n * 4 + 6) doubles of LDS, the pixel is written by one thread.
template <bool PIXEL>
__global__ __launch_bounds__(256) void k_warp_groups(WarpGroupsArgs p) {
    extern __shared__ double sm[];
    const int b = blockIdx.y, stride = p.n * 4 + 6;
    if (PIXEL)
        for (int g = 0; g < p.G; ++g) warp_coeffs_to_lds(p, b, g, sm + g * stride);
    else
        warp_coeffs_to_lds(p, b, blockIdx.z, sm);
    __syncthreads();
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= p.H * p.W) return;
    const int qy = id / p.W, qx = id - qy * p.W;
    if (PIXEL) {
        for (int g = 0; g < p.G; ++g) warp_group_sample(p, b, g, qy, qx, warp_taps(sm + g * stride, p.n, p.H, p.W, qy, qx));
    } else {
        warp_group_sample(p, b, blockIdx.z, qy, qx, warp_taps(sm, p.n, p.H, p.W, qy, qx));
    }
}

}  // namespace dnnca

int dnnca_warp_groups_f32(void* model, const float* x_dev, const float* y_dev, int batch, int h, int w, int c, int n_groups,
                          const int* group_of, int n_points, const double* ctrl_host, const double* wv_host, float* x_out_dev,
                          float* y_out_dev) {
    Model* M = reinterpret_cast<Model*>(model);
    if (!M) { set_error("null model"); return DNNCA_EINVAL; }
    if (!x_dev || !y_dev || !group_of || !ctrl_host || !wv_host || !x_out_dev || !y_out_dev || batch < 1 || batch > 65535 || h < 2 || w < 2 ||
        c < 1 || n_points < 1 || x_out_dev == x_dev || y_out_dev == y_dev) {
        set_error("dnnca_warp_groups_f32: bad arguments");
        return DNNCA_EINVAL;
    }
    if (n_points > WARP_MAX_POINTS) {
        set_error("dnnca_warp_groups_f32: %d control points, at most %d (their %zu bytes of coefficients must fit %zu bytes of LDS)",
                  n_points, WARP_MAX_POINTS, (size_t)(n_points * 4 + 6) * 8, WARP_LDS_MAX);
        return DNNCA_EINVAL;
    }
    if (n_groups < 1 || n_groups > c + 1) {
        set_error("dnnca_warp_groups_f32: %d groups for %d channels + label", n_groups, c);
        return DNNCA_EINVAL;
    }
    for (int i = 0; i <= c; ++i)
        if (group_of[i] < 0 || group_of[i] >= n_groups) {
            set_error("dnnca_warp_groups_f32: group_of[%d] = %d is not one of %d groups", i, group_of[i], n_groups);
            return DNNCA_EINVAL;
        }
    // one row: control points, weights, group table -- the device copy has the same layout, so the row travels in one copy
    const size_t nc = (size_t)batch * n_groups * n_points * 2 * 8, nw = (size_t)batch * n_groups * (n_points + 3) * 2 * 8;
    const size_t row = nc + nw + (size_t)(c + 1) * 4;
    if (row > M->warpg_scratch_bytes) {
        void* p = nullptr;
        DN_TRY(M->alloc(&p, row));
        M->warpg_scratch = p;
        M->warpg_scratch_bytes = row;
    }
    // like the draws of dnnca_augment_u8 the coefficients wait for their upload in a ring of pinned rows: the caller's buffers are
    // free when this call returns and the call does not wait for the stream (a row is waited for when it comes round again)
    if (row > M->warpg_pin_bytes) {
        HIP_TRY(hipStreamSynchronize(M->stream));         // uploads from the old rows are complete
        if (M->warpg_pin) (void)hipHostFree(M->warpg_pin);
        M->warpg_pin = nullptr;
        M->warpg_pin_bytes = 0;
        HIP_TRY(hipHostMalloc(&M->warpg_pin, row * Model::kAugRing, hipHostMallocDefault));
        M->warpg_pin_bytes = row;
    }
    const int k = M->warpg_k;
    M->warpg_k = (k + 1) % Model::kAugRing;
    if (!M->warpg_ev[k]) HIP_TRY(hipEventCreateWithFlags(&M->warpg_ev[k], hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(M->warpg_ev[k]));
    char* pin = (char*)M->warpg_pin + (size_t)k * M->warpg_pin_bytes;
    memcpy(pin, ctrl_host, nc);
    memcpy(pin + nc, wv_host, nw);
    memcpy(pin + nc + nw, group_of, (size_t)(c + 1) * 4);
    HIP_TRY(hipMemcpyAsync(M->warpg_scratch, pin, row, hipMemcpyHostToDevice, M->stream));
    HIP_TRY(hipEventRecord(M->warpg_ev[k], M->stream));
    WarpGroupsArgs a{};
    a.x = x_dev; a.y = y_dev; a.xo = x_out_dev; a.yo = y_out_dev;
    a.ctrl = (const double*)M->warpg_scratch;
    a.wv = (const double*)((char*)M->warpg_scratch + nc);
    a.group_of = (const int*)((char*)M->warpg_scratch + nc + nw);
    a.B = batch; a.H = h; a.W = w; a.C = c; a.G = n_groups; a.n = n_points;
    const size_t lds = (size_t)(n_points * 4 + 6) * 8;
    const unsigned bx = (unsigned)(((size_t)h * w + 255) / 256);
    const double bytes = (double)batch * h * w * (c + 1) * 8.0, flops = (double)batch * h * w * n_groups * n_points * 8.0;
    // DNNCA_WARP_GROUPS_PIXEL (tuning aid, read per call: tools/intrawarp_rate.py flips it): the pixel-per-thread layout, where its
    // G coefficient sets fit the 64 KB of LDS a launch gets without opting in
    if (getenv("DNNCA_WARP_GROUPS_PIXEL") != nullptr && lds * n_groups <= WARP_LDS_MAX)
        LAUNCH(M, "aug_warp_groups", bytes, flops,
               hipLaunchKernelGGL(k_warp_groups<true>, dim3(bx, batch), dim3(256), lds * n_groups, M->stream, a));
    else
        LAUNCH(M, "aug_warp_groups", bytes, flops,
               hipLaunchKernelGGL(k_warp_groups<false>, dim3(bx, batch, n_groups), dim3(256), lds, M->stream, a));
    return DNNCA_OK;
}

// ---------------------------------------------------------------------------------------------------------- random_affine
// This project's own option (augment.py draw_affine; the reference has no rotation, zoom, up-down mirror or transpose): output
// pixel q of image b is sampled at s = L_b q + o_b (row, column), the host's composition of a rotation, a zoom, a shift and a
// flip / transpose of the plane about its centre.  Bilinear in the shape of k_warp's lerp2, features and label with the same taps
// and weights; OUTSIDE THE IMAGE IS ZERO (MRI background is black): a tap whose row or column is outside the plane contributes 0,
// its address is never formed (the indices are clamped first, the value is selected away), and whether it is outside is decided in
// double before anything is converted to int -- a position of 1e12 is an all-zero pixel.  H = 1 and W = 1 are valid.
namespace dnnca {

struct AffineArgs {
    const float* x;          // [B, H, W, C] source features
    const float* y;          // [B, H, W] source label
    const double* mat;       // [B, 2, 3] rows (L[r][0], L[r][1], o[r]): s_r = L[r][0] q_row + L[r][1] q_col + o[r]
    float* xo;
    float* yo;
    int B, H, W, C;
};

// one axis of the position: the cell floor(s) clamped to the two in-range tap indices, which of the two taps exist, the fraction
struct AffineAxis {
    int i0, i1;
    bool in0, in1;
    float a;
};

__device__ __forceinline__ AffineAxis affine_axis(double s, int size) {
    AffineAxis t;
    const double f = floor(s);
    // taps f and f + 1: at least one of them is in [0, size - 1] exactly when -1 <= f <= size - 1 (false for NaN and +-inf too)
    if (!(f >= -1.0 && f <= (double)(size - 1))) {
        t.i0 = t.i1 = 0;
        t.in0 = t.in1 = false;
        t.a = 0.f;
        return t;
    }
    const int i = (int)f;                  // -1 .. size - 1
    t.in0 = i >= 0;
    t.in1 = i + 1 <= size - 1;
    t.i0 = t.in0 ? i : 0;
    t.i1 = t.in1 ? i + 1 : size - 1;
    t.a = (float)(s - f);
    return t;
}

// grid (ceil(W / TX), ceil(H / TY), B), TX * TY threads: a block owns a TX x TY tile of output pixels, so that its source footprint
// is a compact (rotated, mirrored or transposed) patch of about the same area whatever the matrix is -- a linear run of 256 output
// pixels would read a 256-pixel COLUMN under the transposed D4 views, one cache line per lane.  One thread = one output pixel: the
// position once, then the C channels (contiguous per tap in NHWC) and the label.
template <int TX, int TY>
__global__ __launch_bounds__(TX * TY) void k_affine(AffineArgs p) {
    const int qx = blockIdx.x * TX + (int)(threadIdx.x % TX), qy = blockIdx.y * TY + (int)(threadIdx.x / TX), b = blockIdx.z;
    if (qx >= p.W || qy >= p.H) return;
    const double* m = p.mat + (size_t)b * 6;
    const double sy = m[0] * (double)qy + m[1] * (double)qx + m[2];
    const double sx = m[3] * (double)qy + m[4] * (double)qx + m[5];
    const AffineAxis r = affine_axis(sy, p.H), c = affine_axis(sx, p.W);
    const size_t img = (size_t)b * p.H * p.W;
    const size_t o00 = img + (size_t)r.i0 * p.W + c.i0, o01 = img + (size_t)r.i0 * p.W + c.i1;
    const size_t o10 = img + (size_t)r.i1 * p.W + c.i0, o11 = img + (size_t)r.i1 * p.W + c.i1;
    const bool k00 = r.in0 && c.in0, k01 = r.in0 && c.in1, k10 = r.in1 && c.in0, k11 = r.in1 && c.in1;
    const float ay = r.a, ax = c.a;
    auto lerp2 = [&](float tl, float tr, float bl, float br) {
        const float top = ax * (tr - tl) + tl, bot = ax * (br - bl) + bl;
        return ay * (bot - top) + top;
    };
    const size_t oq = img + (size_t)qy * p.W + qx;
    for (int ch = 0; ch < p.C; ++ch)
        p.xo[oq * p.C + ch] = lerp2(k00 ? p.x[o00 * p.C + ch] : 0.f, k01 ? p.x[o01 * p.C + ch] : 0.f,
                                    k10 ? p.x[o10 * p.C + ch] : 0.f, k11 ? p.x[o11 * p.C + ch] : 0.f);
    p.yo[oq] = lerp2(k00 ? p.y[o00] : 0.f, k01 ? p.y[o01] : 0.f, k10 ? p.y[o10] : 0.f, k11 ? p.y[o11] : 0.f);
}

static bool affine_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const char *pa = (const char*)a, *pb = (const char*)b;
    return pa < pb + nb && pb < pa + na;
}

}  // namespace dnnca

int dnnca_affine_f32(void* model, const float* x_dev, const float* y_dev, int batch, int h, int w, int c, const double* mat_host,
                     float* x_out_dev, float* y_out_dev) {
    Model* M = reinterpret_cast<Model*>(model);
    if (!M) { set_error("dnnca_affine_f32: null model"); return DNNCA_EINVAL; }
    if (!x_dev || !y_dev || !mat_host || !x_out_dev || !y_out_dev) {
        set_error("dnnca_affine_f32: null pointer");
        return DNNCA_EINVAL;
    }
    if (batch < 1 || batch > 65535 || h < 1 || w < 1 || c < 1) {
        set_error("dnnca_affine_f32: bad shape (batch %d in 1..65535, %d x %d x %d, each >= 1)", batch, h, w, c);
        return DNNCA_EINVAL;
    }
    const size_t ny = (size_t)batch * h * w * 4, nx = ny * c;
    if (affine_overlap(x_out_dev, nx, x_dev, nx) || affine_overlap(x_out_dev, nx, y_dev, ny) || affine_overlap(y_out_dev, ny, x_dev, nx) ||
        affine_overlap(y_out_dev, ny, y_dev, ny) || affine_overlap(x_out_dev, nx, y_out_dev, ny)) {
        set_error("dnnca_affine_f32: the outputs must not alias the inputs or each other");
        return DNNCA_EINVAL;
    }
    for (int i = 0; i < batch * 6; ++i)
        if (!(mat_host[i] - mat_host[i] == 0.0)) {         // NaN or +-inf
            set_error("dnnca_affine_f32: matrix entry %d of image %d is not finite", i % 6, i / 6);
            return DNNCA_EINVAL;
        }
    // DNNCA_AFFINE_TILE (tuning aid, read per call: tools/affine_rate.py walks it): the W x H tile of output pixels a block owns.
    // 32 x 8 is the shipped one: at 8 x 512 x 512 x 3 it is the fastest on d4 draws and on affine_augment.yaml's draws and within
    // 5 % of the fastest (64 x 4) on identity matrices; the linear 256 x 1 run is a third slower on d4 draws (profiles/affine_rate.txt)
    static const char* const kTiles[] = {"32x8", "16x16", "8x32", "64x4", "8x8", "256x1"};
    int tile = 0;
    if (const char* name = getenv("DNNCA_AFFINE_TILE")) {
        tile = -1;
        for (int i = 0; i < 6; ++i)
            if (!strcmp(name, kTiles[i])) tile = i;
        if (tile < 0) {
            set_error("dnnca_affine_f32: DNNCA_AFFINE_TILE=%s is none of 16x16, 32x8, 8x32, 64x4, 8x8, 256x1", name);
            return DNNCA_EINVAL;
        }
    }
    // one device row and a ring of pinned rows, as dnnca_warp_groups_f32: the caller's matrices are free when this call returns and
    // the call does not wait for the stream.  Rows are sized for max_batch, so a ragged last batch does not grow them.
    const size_t bytes_in = (size_t)batch * 6 * sizeof(double);
    const size_t row = (size_t)M->desc.max_batch > (size_t)batch ? (size_t)M->desc.max_batch * 6 * sizeof(double) : bytes_in;
    if (row > M->affine_scratch_bytes) {
        void* p = nullptr;
        DN_TRY(M->alloc(&p, row));
        M->affine_scratch = p;
        M->affine_scratch_bytes = row;
    }
    if (row > M->affine_pin_bytes) {
        HIP_TRY(hipStreamSynchronize(M->stream));         // uploads from the old rows are complete
        if (M->affine_pin) (void)hipHostFree(M->affine_pin);
        M->affine_pin = nullptr;
        M->affine_pin_bytes = 0;
        HIP_TRY(hipHostMalloc(&M->affine_pin, row * Model::kAugRing, hipHostMallocDefault));
        M->affine_pin_bytes = row;
    }
    const int k = M->affine_k;
    M->affine_k = (k + 1) % Model::kAugRing;
    if (!M->affine_ev[k]) HIP_TRY(hipEventCreateWithFlags(&M->affine_ev[k], hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(M->affine_ev[k]));
    char* pin = (char*)M->affine_pin + (size_t)k * M->affine_pin_bytes;
    memcpy(pin, mat_host, bytes_in);
    HIP_TRY(hipMemcpyAsync(M->affine_scratch, pin, bytes_in, hipMemcpyHostToDevice, M->stream));
    HIP_TRY(hipEventRecord(M->affine_ev[k], M->stream));
    AffineArgs a{};
    a.x = x_dev; a.y = y_dev; a.xo = x_out_dev; a.yo = y_out_dev;
    a.mat = (const double*)M->affine_scratch;
    a.B = batch; a.H = h; a.W = w; a.C = c;
    const double bytes = (double)batch * h * w * (c + 1) * 8.0;
#define AFFINE_GO(TX, TY)                                                                                                       \
    LAUNCH(M, "aug_affine", bytes, 0,                                                                                           \
           hipLaunchKernelGGL((k_affine<TX, TY>), dim3((w + TX - 1) / TX, (h + TY - 1) / TY, batch), dim3(TX * TY), 0, M->stream, a))
    switch (tile) {
        case 1: AFFINE_GO(16, 16); break;
        case 2: AFFINE_GO(8, 32); break;
        case 3: AFFINE_GO(64, 4); break;
        case 4: AFFINE_GO(8, 8); break;
        case 5: AFFINE_GO(256, 1); break;
        default: AFFINE_GO(32, 8); break;
    }
#undef AFFINE_GO
    return DNNCA_OK;
}
