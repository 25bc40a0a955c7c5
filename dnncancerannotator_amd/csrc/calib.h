// calib.h -- host-side launchers of kernels_calib.hip (reliability table, NLL at a set of temperatures, temperature scaling); the
// definitions the kernels share with tests/calib_oracle.py are at the top of that file.  All planes are device [slices, hw] float32.
#pragma once
#include "common.h"

namespace dnnca {

constexpr int kCalibMaxBins = 256;
constexpr int kCalibMaxTemps = 64;
constexpr float kCalibMinT = 0.05f, kCalibMaxT = 20.f;

// bins: [slices][n_bins] x (n[2], sum_q24[2]) and sq: [slices] x (sq_lo[2], sq_hi[2]) uint64, zeroed by the caller; the launch adds.
// slices <= 65535, hw < 2^31, 1 <= n_bins <= kCalibMaxBins
void g_calib_bins(hipStream_t s, const float* prob, const float* y, int slices, size_t hw, int n_bins, unsigned long long* bins,
                  unsigned long long* sq);
// the grid of calib_nll on slices of hw pixels: runs of 256 pixels per block, blocks per slice (at most 1024)
void calib_nll_shape(size_t hw, int* runs, int* blocks);
// part [slices][blocks][nt] (every entry written); inv_t: nt doubles on the device, 1 / (double) T
void g_calib_nll(hipStream_t s, const float* prob, const float* y, int slices, size_t hw, const double* inv_t, int nt, double* part);
// out [slices][nt] = the sum over the blocks of part, in ascending block order
void g_calib_nll_sum(hipStream_t s, const double* part, int slices, size_t hw, int nt, double* out);
// dst[i] = the probability src[i] at `temperature`; dst may be src
void g_prob_temperature(hipStream_t s, const float* src, float* dst, size_t n, float temperature);

}  // namespace dnnca
