// sens_first_dev.h -- the tile body that k_sens_first (kernels_sens.hip) and k_attr_first (kernels_attr.hip) share: the data gradient
// of a conv that reads the network input, formed in registers and never stored as a tensor.
//
// One call = one 16 x 16 tile of image b for the input channels [d.ci0, d.ci0 + d.nci) of the conv of `d`.  Per chunk of kSensCo
// output channels the block stages dz = dy act'(y) with its halo (channel planes, odd plane stride: conflict-free reads) and the
// chunk's weights in LDS; thread (ly, lx) = (tid / 16, tid % 16) forms
//     dx[iy, ix, ci] = sum over ky, kx, co of dz[iy - ky + pad, ix - kx + pad, co] w[ky, kx, ci, co]
// for its pixel (ty0 + ly, tx0 + lx) into acc[0 .. kSensCi).  Every thread of the block calls it (it holds barriers); a thread whose
// pixel lies outside the image gets a value it must not use.  lds: sens_first_lds(K) bytes.
#pragma once
#include "sens.h"

namespace dnnca {

template <int kThreads>
__device__ __forceinline__ void sens_first_tile(const SensFirst& d, int b, int H, int W, int K, int ty0, int tx0, float* lds,
                                                float (&acc)[kSensCi]) {
    const int tid = threadIdx.x, lx = tid % kSensTile, ly = tid / kSensTile;
    const int pad = (K - 1) / 2, TH = kSensTile + K - 1, plane = (TH * TH) | 1;
    float* s_dz = lds;                                 // [kSensCo][plane]
    float* s_w = lds + kSensCo * plane;                // [K * K][kSensCi][kSensCo]
#pragma unroll
    for (int j = 0; j < kSensCi; ++j) acc[j] = 0.f;
    for (int co0 = 0; co0 < d.cout; co0 += kSensCo) {
        const int nco = min(kSensCo, d.cout - co0);
        __syncthreads();                           // the previous chunk's readers are done
        for (int i = tid; i < TH * TH * kSensCo; i += kThreads) {
            const int c = i % kSensCo, pix = i / kSensCo;
            const int gy = ty0 + pix / TH - pad, gx = tx0 + pix % TH - pad;
            float v = 0.f;
            if (c < nco && gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const size_t idx = (((size_t)b * H + gy) * W + gx) * d.cout + co0 + c;
                v = d.dy[idx];
                if (d.alpha >= 0.f) v *= d.y[idx] > 0.f ? 1.f : d.alpha;          // as g_act_bwd
            }
            s_dz[c * plane + pix] = v;
        }
        for (int i = tid; i < K * K * kSensCi * kSensCo; i += kThreads) {
            const int c = i % kSensCo, j = (i / kSensCo) % kSensCi, kk = i / (kSensCo * kSensCi);
            s_w[i] = (j < d.nci && c < nco) ? d.w[((size_t)kk * d.cin + d.ci0 + j) * d.cout + co0 + c] : 0.f;
        }
        __syncthreads();
        for (int ky = 0; ky < K; ++ky)
            for (int kx = 0; kx < K; ++kx) {
                const float* zp = s_dz + (ly + 2 * pad - ky) * TH + (lx + 2 * pad - kx);
                const float* wp = s_w + (ky * K + kx) * kSensCi * kSensCo;
#pragma unroll
                for (int c = 0; c < kSensCo; ++c) {
                    const float v = zp[c * plane];
#pragma unroll
                    for (int j = 0; j < kSensCi; ++j) acc[j] = fmaf(v, wp[j * kSensCo + c], acc[j]);
                }
            }
    }
}

}  // namespace dnnca
