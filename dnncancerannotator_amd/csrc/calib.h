// calib.h -- host-side launchers of kernels_calib.hip (reliability table, NLL at a set of temperatures, temperature scaling); the
// definitions the kernels share with tests/calib_oracle.py are at the top of that file.  All planes are device [slices, hw] float32.
#pragma once
#include "model.h"

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

// ---- the host side of dnnca_calibration and dnnca_prob_temperature: device planes in, host tables out -----------------------------
// prob, y: device [batch, hw], batch <= 65535.  calib_bins and, with nt > 0 host `temperatures`, calib_nll and calib_nll_sum in the
// model's calibration workspace (grown on demand).  bins (host [batch][n_bins]), totals (host [batch]: every slice's pixels and sums
// over its bins, and its squares) and nll (host [batch][nt]; not touched with nt == 0) are written.  Synchronises
int calibration(Model* M, const float* prob, const float* y, int batch, size_t hw, int n_bins, const float* temperatures, int nt,
                dnnca_calib_bin* bins, dnnca_calib_total* totals, double* nll);
// prob_temperature on n device floats, src -> dst (dst may be src); out_hw (host, or nullptr) receives a copy of dst.  Synchronises
int prob_temperature(Model* M, const float* src, float* dst, size_t n, float temperature, float* out_hw);

}  // namespace dnnca
