// kernels_aug.hip -- train-time augmentation on the device: the reference's per-image tf.data maps
//   base():            centre crop to the stored size, cast to float32, / 255            (annotator/data.py:195-206)
//   random_crop():     crop to output_size at centre + clip(int(N(0, stddev)), min_, max_)  (data.py:677-689)
//   random_flip():     tf.image.random_flip_left_right                                     (data.py:620-625)
//   random_contrast(): (x - mean_hw(x)) * U[lower, upper) + mean_hw(x) on the feature channels (data.py:586-609)
//   to_feature_label() label channel -> y, the others in order -> x                        (data.py:766-788)
// in two launches over a uint8 batch that was uploaded as stored (a quarter of the float bytes over PCIe).  The random draws are
// made by the host (augment.py) and passed per image, so the arithmetic is checkable against the oracle draw for draw.
// random_warp (tfa.image.sparse_image_warp) follows below as dnnca_warp_f32, random_intrachannelwarp as dnnca_warp_groups_f32.
// random_affine (this project's own: rotation, zoom, shift and D4 view in one bilinear resampling) is dnnca_affine_f32;
// random_intensity (this project's own: gamma, bias field, blur and noise per image and channel) closes the file as dnnca_intensity_f32.
#include <stdlib.h>
#include <string.h>
#include "fast.h"
#include "kernels.h"
#include "philox_dev.h"

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
    // the draws, padded to max_batch, with room for the channel sums behind them on the device
    const size_t prm_bytes = (size_t)batch * sizeof(dnnca_aug_param);
    DN_TRY(M->aug_ring.upload(M, {{params_host, prm_bytes}}, (size_t)batch * AUG_MAXC * 4, (size_t)M->desc.max_batch * sizeof(dnnca_aug_param)));
    AugArgs a{};
    a.src = (const unsigned char*)src_dev;
    a.prm = (const dnnca_aug_param*)M->aug_ring.dev;
    a.sums = (unsigned*)(M->aug_ring.dev + prm_bytes);
    a.x = x_dev; a.y = y_dev;
    a.B = batch; a.Hs = hs; a.Ws = ws; a.Cs = cs; a.Ho = ho; a.Wo = wo; a.label_index = label_index;
    a.contrast_mask = contrast_mask & ~(1u << label_index);
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

// control points + weights of spline s (an image of k_warp, a group of an image of k_warp_groups) into sm (n * 4 + 6 doubles); the
// caller synchronises
__device__ __forceinline__ void warp_coeffs_to_lds(const double* ctrl, const double* wv, int n, size_t s, double* sm) {
    for (int i = threadIdx.x; i < n * 2; i += 256) {
        sm[i] = ctrl[s * n * 2 + i];
        sm[n * 2 + i] = wv[s * (n + 3) * 2 + i];
    }
    if (threadIdx.x < 6) sm[n * 4 + threadIdx.x] = wv[(s * (n + 3) + n) * 2 + threadIdx.x];
}

// the bilinear taps of output pixel (qy, qx) under the spline in sm, then tfa's interpolate_bilinear at q - flow with the floor
// clamped to [0, size - 2] and alpha clipped to [0, 1] -- the clamps keep every tap inside the image however far the flow throws
// the position (max_diff 100 in the shipped overlays).  The thin-plate weights cancel massively (|phi| ~ 1e4, flows ~ 1): the flow
// is evaluated in double (the float32 sum is only good to ~1e-2 pixel, which is also all that tfa's own float32 evaluation is good for).
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
    double d0 = qy * v[0] + qx * v[2] + v[4];             // linear term [q, 1] v  (v rows: y, x, 1; columns: flow_y, flow_x)
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

__global__ __launch_bounds__(256) void k_warp(WarpArgs p) {
    extern __shared__ double sm[];         // control points + weights of this image: n * 4 + 6 doubles
    const int b = blockIdx.y;
    warp_coeffs_to_lds(p.ctrl, p.wv, p.n, b, sm);
    __syncthreads();
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= p.H * p.W) return;
    const int qy = id / p.W, qx = id - qy * p.W;
    const WarpTaps t = warp_taps(sm, p.n, p.H, p.W, qy, qx);
    const size_t o00 = ((size_t)b * p.H + t.iy) * p.W + t.ix, o01 = o00 + 1, o10 = o00 + p.W, o11 = o10 + 1;
    const size_t oq = ((size_t)b * p.H + qy) * p.W + qx;
    for (int c = 0; c < p.C; ++c)
        p.xo[oq * p.C + c] = t(p.x[o00 * p.C + c], p.x[o01 * p.C + c], p.x[o10 * p.C + c], p.x[o11 * p.C + c]);
    p.yo[oq] = t(p.y[o00], p.y[o01], p.y[o10], p.y[o11]);
}

// dnnca_warp_f32 and dnnca_warp_groups_f32: the coefficients of one spline must fit the LDS of a launch
static bool warp_points_fit(const char* fn, int n_points) {
    if (n_points <= WARP_MAX_POINTS) return true;
    set_error("%s: %d control points, at most %d (their %zu bytes of coefficients must fit %zu bytes of LDS)", fn, n_points,
              WARP_MAX_POINTS, (size_t)(n_points * 4 + 6) * 8, WARP_LDS_MAX);
    return false;
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
    if (!warp_points_fit("dnnca_warp_f32", n_points)) return DNNCA_EINVAL;
    const size_t nc = (size_t)batch * n_points * 2 * 8, nw = (size_t)batch * (n_points + 3) * 2 * 8;
    DN_TRY(M->warp_ring.upload(M, {{ctrl_host, nc}, {wv_host, nw}}));
    WarpArgs a{};
    a.x = x_dev; a.y = y_dev; a.xo = x_out_dev; a.yo = y_out_dev;
    a.ctrl = (const double*)M->warp_ring.dev;
    a.wv = (const double*)(M->warp_ring.dev + nc);
    a.B = batch; a.H = h; a.W = w; a.C = c; a.n = n_points;
    LAUNCH(M, "aug_warp", (double)batch * h * w * (c + 1) * 8.0, (double)batch * h * w * n_points * 8.0,
           hipLaunchKernelGGL(k_warp, dim3((h * w + 255) / 256, batch), dim3(256), (size_t)(n_points * 4 + 6) * 8, M->stream, a));
    HIP_TRY(hipStreamSynchronize(M->stream));      // this call has always returned with its outputs complete: callers may rely on it
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
        for (int g = 0; g < p.G; ++g) warp_coeffs_to_lds(p.ctrl, p.wv, p.n, (size_t)b * p.G + g, sm + g * stride);
    else
        warp_coeffs_to_lds(p.ctrl, p.wv, p.n, (size_t)b * p.G + blockIdx.z, sm);
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
    if (!warp_points_fit("dnnca_warp_groups_f32", n_points)) return DNNCA_EINVAL;
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
    DN_TRY(M->warpg_ring.upload(M, {{ctrl_host, nc}, {wv_host, nw}, {group_of, (size_t)(c + 1) * 4}}));
    WarpGroupsArgs a{};
    a.x = x_dev; a.y = y_dev; a.xo = x_out_dev; a.yo = y_out_dev;
    a.ctrl = (const double*)M->warpg_ring.dev;
    a.wv = (const double*)(M->warpg_ring.dev + nc);
    a.group_of = (const int*)(M->warpg_ring.dev + nc + nw);
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

static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
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
    if (ranges_overlap(x_out_dev, nx, x_dev, nx) || ranges_overlap(x_out_dev, nx, y_dev, ny) || ranges_overlap(y_out_dev, ny, x_dev, nx) ||
        ranges_overlap(y_out_dev, ny, y_dev, ny) || ranges_overlap(x_out_dev, nx, y_out_dev, ny)) {
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
    DN_TRY(M->affine_ring.upload(M, {{mat_host, (size_t)batch * 6 * sizeof(double)}}, 0, (size_t)M->desc.max_batch * 6 * sizeof(double)));
    AffineArgs a{};
    a.x = x_dev; a.y = y_dev; a.xo = x_out_dev; a.yo = y_out_dev;
    a.mat = (const double*)M->affine_ring.dev;
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

// ------------------------------------------------------------------------------------------------------- random_intensity
// This project's own option (augment.py draw_intensity; the reference changes values only through random_contrast): what differs
// between scanners and sessions, per image AND feature channel -- a gamma, a smooth multiplicative bias field, an in-plane Gaussian
// blur and Gaussian or Rician noise.  The host draws one 128-byte record per (image, channel) (layout: include/dnnca.h); the device
// never sees a probability or a sigma of the blur, only flags, coefficients, taps and a Philox key.  Per active plane, in float32:
//   1. gamma   v <= 0 ? 0 : powf(v, g)
//   2. bias    v * expf(f),  f = sum a_ij P_i(u) P_j(v) over 1 <= i + j <= 3, Legendre P on the pixel's own coordinates in [-1, 1]
//   3. blur    rows, then columns, taps w[0..R]; a tap outside the image reads the nearest edge pixel (after steps 1 and 2)
//   4. noise   Philox4x32-10(counter (row * W + col, 0, 0, 0), the record's key) -> Box-Muller -> v + s z0, or sqrt((v + s z0)^2 + (s z1)^2)
//   5. clamp   to [0, 1]
// A plane whose flags are 0 is copied bit for bit.  Every address is a function of the thread's coordinates alone (clamped to the
// plane for the halo): nothing in a record or in the data moves one.  The label is not an argument.
namespace dnnca {

constexpr int INTENSITY_WORDS = 32, INTENSITY_RMAX = 8;
constexpr unsigned INTENSITY_GAMMA = 1u, INTENSITY_BIAS = 2u, INTENSITY_BLUR = 4u, INTENSITY_NOISE = 8u, INTENSITY_RICIAN = 16u;
constexpr unsigned INTENSITY_FLAGS = 31u;

struct IntensityArgs {
    const float* x;          // [B, H, W, C] source features
    const unsigned* rec;     // [B, C, 32] records (device copy)
    float* xo;
    int B, H, W, C;
};

// coordinate i of a size-n axis on [-1, 1] (0 where the axis has one point)
__device__ __forceinline__ float intensity_coord(int i, int n) {
#pragma clang fp contract(off)
    const float d = (float)(n - 1);
    return n > 1 ? ((float)i * 2.0f - d) / d : 0.0f;
}

// steps 1 and 2 on the pixel (row, col) of a plane with record r.  No contraction: the two instantiations of k_intensity, and the
// halo pixels of neighbouring tiles, must give the same bits for the same pixel.
__device__ __forceinline__ float intensity_point(float v, unsigned flags, const unsigned* __restrict__ r, int row, int col, int H, int W) {
#pragma clang fp contract(off)
    if (flags & INTENSITY_GAMMA) v = v <= 0.0f ? 0.0f : powf(v, __uint_as_float(r[1]));
    if (flags & INTENSITY_BIAS) {
        const float u = intensity_coord(row, H), t = intensity_coord(col, W);
        const float u2 = 1.5f * u * u - 0.5f, u3 = (2.5f * u * u - 1.5f) * u;
        const float t2 = 1.5f * t * t - 0.5f, t3 = (2.5f * t * t - 1.5f) * t;
        float f = __uint_as_float(r[2]) * u;
        f += __uint_as_float(r[3]) * t;
        f += __uint_as_float(r[4]) * u2;
        f += __uint_as_float(r[5]) * (u * t);
        f += __uint_as_float(r[6]) * t2;
        f += __uint_as_float(r[7]) * u3;
        f += __uint_as_float(r[8]) * (u2 * t);
        f += __uint_as_float(r[9]) * (u * t2);
        f += __uint_as_float(r[10]) * t3;
        v = v * expf(f);
    }
    return v;
}

// steps 4 and 5
__device__ __forceinline__ float intensity_finish(float v, unsigned flags, const unsigned* __restrict__ r, unsigned index) {
#pragma clang fp contract(off)
    if (flags & INTENSITY_NOISE) {
        unsigned word[4];                                             // the first two of the four words are used
        philox4x32_10(index, 0u, 0u, 0u, r[22], r[23], word);
        const unsigned r0 = word[0], r1 = word[1];
        const float u1 = (float)((r0 >> 9) + 1u) * 0x1p-23f;          // (0, 1], exact
        const float a2 = (float)(r1 >> 8) * 0x1p-23f;                  // 2 u2 in [0, 2), exact
        const float sigma = __uint_as_float(r[21]);
        const float rad = sqrtf(-2.0f * logf(u1));
        v = v + sigma * (rad * cospif(a2));
        if (flags & INTENSITY_RICIAN) {
            const float q = sigma * (rad * sinpif(a2));
            v = sqrtf(v * v + q * q);
        }
    }
    return fminf(fmaxf(v, 0.0f), 1.0f);
}

// grid (ceil(W / TX), ceil(H / TY), B), TX * TY threads, one thread = one output pixel, the channels in a loop (as k_affine).
// HALO false: no record of the batch blurs -- no LDS, no barrier.
// HALO true:  a blurred plane (a block-uniform property: the record belongs to blockIdx.z and the channel) is staged with a halo of
//   R pixels, after steps 1 and 2, as one float plane of row stride TX + 16, filtered along the rows into a second plane of row
//   stride TX and along the columns from there.  One plane at a time keeps the LDS independent of C (at most 15 KB, the 32 x 32
//   tile) and makes every pass read consecutive dwords with consecutive lanes.  By the bank rule of 4-byte LDS accesses (bank
//   (a / 4) % 32, lanes conflict within a 32-lane half of the wave): the column pass and the write of the row pass are linear in
//   the thread index -- no conflict at any TX; the row pass reads one staged row per half-wave when TX >= 32 -- no conflict -- and
//   two rows of 16 when TX = 16, which lie 32 dwords apart (stride 16 + 16) on the same banks: 2-way, the one tile that pays; the
//   staging write is linear where R = 8 and skips 16 - 2 R dwords at a row's end otherwise (2-way for the lanes behind the skip).
//   An interleaved [pixel][C] plane would have had odd lane strides (C = 3, 5: conflict-free too) but an LDS size that grows
//   with C.  Planes without blur take the pointwise route of the other instantiation, statement for statement.
template <int TX, int TY, bool HALO>
__global__ __launch_bounds__(TX * TY) void k_intensity(IntensityArgs p) {
    constexpr int NT = TX * TY, SW = TX + 2 * INTENSITY_RMAX, SH = TY + 2 * INTENSITY_RMAX;
    __shared__ float s_in[HALO ? SH * SW : 1];
    __shared__ float s_row[HALO ? SH * TX : 1];
    const int tx = (int)(threadIdx.x % TX), ty = (int)(threadIdx.x / TX);
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY, b = blockIdx.z;
    const int qx = x0 + tx, qy = y0 + ty;
    const bool inside = qx < p.W && qy < p.H;
    if (!HALO && !inside) return;
    const size_t img = (size_t)b * p.H * p.W;
    const size_t oq = img + (size_t)qy * p.W + qx;                     // formed for every thread, used by the inside ones
    const unsigned index = (unsigned)qy * (unsigned)p.W + (unsigned)qx;
    for (int c = 0; c < p.C; ++c) {
        const unsigned* __restrict__ r = p.rec + ((size_t)b * p.C + c) * INTENSITY_WORDS;
        const unsigned flags = r[0];
        float v;
        if (HALO && (flags & INTENSITY_BLUR)) {
            const int R = (int)min(r[11], (unsigned)INTENSITY_RMAX);      // (the host refuses more)
            const int sw = TX + 2 * R, sh = TY + 2 * R;
            __syncthreads();                                            // the passes of the channel before this one are over
            for (int i = threadIdx.x; i < sh * sw; i += NT) {
                const int ry = i / sw, rx = i - ry * sw;
                const int gy = min(max(y0 - R + ry, 0), p.H - 1), gx = min(max(x0 - R + rx, 0), p.W - 1);      // nearest edge pixel
                const float s = p.x[(img + (size_t)gy * p.W + gx) * p.C + c];
                s_in[ry * SW + rx] = intensity_point(s, flags, r, gy, gx, p.H, p.W);
            }
            __syncthreads();
            for (int i = threadIdx.x; i < sh * TX; i += NT) {
                const int ry = i / TX, rx = i - ry * TX;
                const float* s = s_in + ry * SW + rx + R;
                float acc = __uint_as_float(r[12]) * s[0];
                for (int k = 1; k <= R; ++k) acc = fmaf(__uint_as_float(r[12 + k]), s[-k] + s[k], acc);
                s_row[ry * TX + rx] = acc;
            }
            __syncthreads();
            const float* s = s_row + (ty + R) * TX + tx;
            v = __uint_as_float(r[12]) * s[0];
            for (int k = 1; k <= R; ++k) v = fmaf(__uint_as_float(r[12 + k]), s[-k * TX] + s[k * TX], v);
            if (!inside) continue;
        } else {
            if (!inside) continue;
            v = p.x[oq * p.C + c];
            if (flags == 0u) {                                          // nothing drawn, or not a target channel: the bits as they are
                p.xo[oq * p.C + c] = v;
                continue;
            }
            v = intensity_point(v, flags, r, qy, qx, p.H, p.W);
        }
        p.xo[oq * p.C + c] = intensity_finish(v, flags, r, index);
    }
}

static bool intensity_finite(unsigned bits) { return (bits & 0x7F800000u) != 0x7F800000u; }

}  // namespace dnnca

int dnnca_intensity_f32(void* model, const float* x_dev, int batch, int h, int w, int c, const unsigned* rec_host, float* x_out_dev) {
    Model* M = reinterpret_cast<Model*>(model);
    if (!M) { set_error("dnnca_intensity_f32: null model"); return DNNCA_EINVAL; }
    if (!x_dev || !rec_host || !x_out_dev) {
        set_error("dnnca_intensity_f32: null pointer");
        return DNNCA_EINVAL;
    }
    if (batch < 1 || batch > 65535 || h < 1 || w < 1 || c < 1 || (unsigned long long)h * (unsigned long long)w > 0xFFFFFFFFull) {
        set_error("dnnca_intensity_f32: bad shape (batch %d in 1..65535, %d x %d x %d, each >= 1, h * w < 2^32)", batch, h, w, c);
        return DNNCA_EINVAL;
    }
    const size_t nx = (size_t)batch * h * w * c * 4;
    if (ranges_overlap(x_out_dev, nx, x_dev, nx)) {
        set_error("dnnca_intensity_f32: the output must not alias the input");
        return DNNCA_EINVAL;
    }
    bool any_blur = false;
    for (int i = 0; i < batch * c; ++i) {
        const unsigned* r = rec_host + (size_t)i * INTENSITY_WORDS;
        auto f = [&](int k) { float v; memcpy(&v, r + k, 4); return v; };
        const int b = i / c, ch = i % c;
        if (r[0] & ~INTENSITY_FLAGS) {
            set_error("dnnca_intensity_f32: record (%d, %d) has unknown flag bits 0x%x", b, ch, r[0]);
            return DNNCA_EINVAL;
        }
        for (int k = 1; k <= 21; ++k)
            if (k != 11 && !intensity_finite(r[k])) {
                set_error("dnnca_intensity_f32: word %d of record (%d, %d) is not a finite float", k, b, ch);
                return DNNCA_EINVAL;
            }
        for (int k = 24; k < INTENSITY_WORDS; ++k)
            if (r[k]) {
                set_error("dnnca_intensity_f32: reserved word %d of record (%d, %d) is not 0", k, b, ch);
                return DNNCA_EINVAL;
            }
        if ((r[0] & INTENSITY_GAMMA) && !(f(1) > 0.0f)) {
            set_error("dnnca_intensity_f32: gamma %g of record (%d, %d) is not positive", (double)f(1), b, ch);
            return DNNCA_EINVAL;
        }
        if (r[11] > (unsigned)INTENSITY_RMAX) {
            set_error("dnnca_intensity_f32: blur radius %u of record (%d, %d) is above %d", r[11], b, ch, INTENSITY_RMAX);
            return DNNCA_EINVAL;
        }
        double sum = f(12);
        for (int k = 0; k <= INTENSITY_RMAX; ++k) {
            if (f(12 + k) < 0.0f) {
                set_error("dnnca_intensity_f32: tap %d of record (%d, %d) is negative", k, b, ch);
                return DNNCA_EINVAL;
            }
            if (k) sum += 2.0 * f(12 + k);
        }
        if ((r[0] & INTENSITY_BLUR) && !(sum - 1.0 <= 1e-5 && 1.0 - sum <= 1e-5)) {
            set_error("dnnca_intensity_f32: the taps of record (%d, %d) sum to %.9g, not 1", b, ch, sum);
            return DNNCA_EINVAL;
        }
        if (f(21) < 0.0f) {
            set_error("dnnca_intensity_f32: noise sigma %g of record (%d, %d) is negative", (double)f(21), b, ch);
            return DNNCA_EINVAL;
        }
        any_blur = any_blur || (r[0] & INTENSITY_BLUR);
    }
    // DNNCA_INTENSITY_TILE (tuning aid, read per call: tools/intensity_rate.py walks it): the W x H tile of output pixels a block owns.
    // 32 x 8 is the shipped one: at 8 x 512 x 512 x 3 it is the fastest or within the spread of the fastest on a copy, on pointwise
    // terms, on noise and on intensity_augment.yaml's draws; 32 x 16 is 20 % faster only where every plane blurs at R = 8 (its
    // halo is 3 x the tile, not 4.5 x) and 2 % slower on the overlay's draws (profiles/intensity_rate.txt)
    static const char* const kTiles[] = {"32x8", "16x16", "64x4", "32x16", "32x32"};
    int tile = 0;
    if (const char* name = getenv("DNNCA_INTENSITY_TILE")) {
        tile = -1;
        for (int i = 0; i < 5; ++i)
            if (!strcmp(name, kTiles[i])) tile = i;
        if (tile < 0) {
            set_error("dnnca_intensity_f32: DNNCA_INTENSITY_TILE=%s is none of 32x8, 16x16, 64x4, 32x16, 32x32", name);
            return DNNCA_EINVAL;
        }
    }
    const size_t rec_bytes = (size_t)c * INTENSITY_WORDS * 4;
    DN_TRY(M->intensity_ring.upload(M, {{rec_host, batch * rec_bytes}}, 0, M->desc.max_batch * rec_bytes));
    IntensityArgs a{};
    a.x = x_dev; a.xo = x_out_dev;
    a.rec = (const unsigned*)M->intensity_ring.dev;
    a.B = batch; a.H = h; a.W = w; a.C = c;
    const double bytes = (double)batch * h * w * c * 8.0;
#define INTENSITY_GO(TX, TY)                                                                                                    \
    do {                                                                                                                        \
        const dim3 grid((w + TX - 1) / TX, (h + TY - 1) / TY, batch);                                                           \
        if (any_blur) LAUNCH(M, "aug_intensity", bytes, 0, hipLaunchKernelGGL((k_intensity<TX, TY, true>), grid, dim3(TX * TY), 0, M->stream, a)); \
        else LAUNCH(M, "aug_intensity", bytes, 0, hipLaunchKernelGGL((k_intensity<TX, TY, false>), grid, dim3(TX * TY), 0, M->stream, a)); \
    } while (0)
    switch (tile) {
        case 1: INTENSITY_GO(16, 16); break;
        case 2: INTENSITY_GO(64, 4); break;
        case 3: INTENSITY_GO(32, 16); break;
        case 4: INTENSITY_GO(32, 32); break;
        default: INTENSITY_GO(32, 8); break;
    }
#undef INTENSITY_GO
    return DNNCA_OK;
}
