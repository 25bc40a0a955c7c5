// sens.h -- launchers of the input-sensitivity pass's own kernels (kernels_sens.hip).
#pragma once
#include "common.h"

namespace dnnca {

// d sum(sigmoid(logits)) / d feat of the head (Conv2D(1, 1)): dfeat[p, c] = (acc ? dfeat : 0) + sigmoid'(logits[p]) w[c]
void g_sens_head(hipStream_t s, int B, int H, int W, const float* logits, const float* w, View dfeat, int acc);
// BatchNorm backward with the moving statistics (inference mode): dx = (acc ? dx : 0) + dy gamma / sqrt(moving_variance + eps)
void g_bn_infer_bwd(hipStream_t s, int B, View dy, View dx, int acc, const float* gamma, const float* mvar, float eps);

// first layer: one entry per (conv that reads the network input, group of up to kSensCi of its input channels)
constexpr int kSensTile = 16, kSensCo = 16, kSensCi = 4, kSensMaxK = 7;
struct SensFirst {
    const float* dy;         // gradient of the conv's output [B, H, W, cout] (dense), before the activation mask
    const float* y;          // the conv's output (the mask's argument)
    const float* w;          // HWIO kernel [K, K, cin, cout]
    int cin, ci0, nci, cout;
    int chan;                // network input channel of ci0
    float alpha;             // the conv's activation (<0 none, 0 relu, >0 leaky)
};
struct SensFirstGrid { int tiles_x, ntiles, tpb, nblk; };
SensFirstGrid sens_first_grid(int B, int H, int W, int nz);
size_t sens_first_lds(int K);
// sums[b * c_total + channel] = sum over the image of |d out / d x|.  part: B * c_total * g.nblk doubles of scratch; ticket: B * nz
// counters, zero before the first launch and left zeroed by every launch
void g_sens_first(hipStream_t s, const SensFirst* descs_dev, int nz, int B, int H, int W, int K, int c_total, const SensFirstGrid& g,
                  double* part, unsigned* ticket, double* sums);

}  // namespace dnnca
