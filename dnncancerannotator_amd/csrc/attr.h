// attr.h -- launchers of the integrated-gradients pass's own kernels (kernels_attr.hip; Model::integrated_gradients, model.hip).
// None of them uses an atomic: every sum is block partials in a scratch row, then one small launch that adds the row in ascending
// order, so two runs give the same bits.
#pragma once
#include "sens.h"

namespace dnnca {

// pixels of a slice that one block of attr_baseline_part / attr_finish / attr_prob_part covers
constexpr int kAttrBlockPix = 1024;
inline int attr_blocks(size_t hw) { return (int)((hw + kAttrBlockPix - 1) / kAttrBlockPix); }
constexpr int kAttrMaxC = 256;           // attr_finish: one thread per channel adds the block's lanes up

// mean baseline: part[(b * C + c) * nblk + k] = sum in double of x[b, pixels of block k, c]; then
// x0[b * C + c] = (float) (row sum / hw)
void g_attr_baseline_part(hipStream_t s, const float* x, int B, size_t hw, int C, double* part);
void g_attr_baseline(hipStream_t s, const double* part, int B, size_t hw, int C, float* x0);
// out = x0[b, c] + alpha (x - x0[b, c]) over [B, hw, C]; x0 == nullptr: the black baseline (0).  16-byte accesses when hw * C is a
// multiple of 4
void g_attr_path_in(hipStream_t s, const float* x, const float* x0, float alpha, int B, size_t hw, int C, float* out);
// the first-layer data gradient of k_sens_first, kept signed: acc[b, iy, ix, chan + j] = (first ? 0 : acc) + dx.  Same descriptors
// and grid as g_sens_first; every (pixel, channel) must belong to exactly one descriptor
void g_attr_first(hipStream_t s, const SensFirst* descs_dev, int nz, int B, int H, int W, int K, int c_total, const SensFirstGrid& g,
                  float* acc, int first);
// attr = (x - x0) * (acc / steps), written over acc when `write_map`; part[((b * C + c) * 2 + which) * nblk + k] = the block's sum
// of attr (which = 0) and |attr| (1) in double
void g_attr_finish(hipStream_t s, float* acc, const float* x, const float* x0, int steps, int B, size_t hw, int C, int write_map,
                   double* part);
// out[r] = sum over k < n, ascending, of part[r * n + k]
void g_attr_sums(hipStream_t s, const double* part, int rows, int n, double* out);
// part[b * nblk + k] = the block's sum of sigmoid(logits[b, pixel]) in double (sigmoid formed in double)
void g_attr_prob_part(hipStream_t s, const float* logits, int B, size_t hw, double* part);

}  // namespace dnnca
