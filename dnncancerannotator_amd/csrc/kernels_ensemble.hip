// kernels_ensemble.hip -- the members of an ensemble (cross-validation folds, snapshots of one run) join per pixel: the mean of
// their mean probabilities and, with the spread, how much they disagree.  One level above kernels_tta.hip: a member's mean and its
// within-member spread are what tta_accumulate / tta_moments left for its weights.
//   mean    = (sum over the members, ascending, in float32, of mean_m) / n                     (tta_join's operations, in its order)
//   between = sqrt(max(0, (sum d^2 - (sum d)^2 / n) / n)),  d = mean_m - mean_0                (tta_moments' shifted form: nothing
//             cancels where the members agree; equal members and n == 1 give an exact 0)
//   within  = sqrt((sum s_m^2) / n),  s_m the member's spread over its views (0 for one view)
//   total   = sqrt(between^2 + within^2), from the two variances before their square roots     (the law of total variance over the
//             n x V forwards: every member has the same V views)
// A streaming kernel of a few MB beside forwards of 100 us and more: dword accesses (the planes of dnnca_ensemble_of lie npix floats
// apart in one allocation, so for an odd npix they are not 16-byte aligned), a grid-stride loop, no atomics, every output element
// has one writer (bit-identical from run to run).
#include "kernels.h"

namespace dnnca {

static constexpr int ENS_TB = 256;           // threads per block
static constexpr int ENS_MAX_BLOCKS = 2048;  // 256 CUs x 8 blocks; the loop strides over the rest

// Every product and sum is rounded on its own: the pragma sits inside the function body, so nothing else inherits it.
// mean_in / mean_out and within_in / total_out may be the same plane: the pixel's inputs are in registers before its first store.
__global__ void __launch_bounds__(ENS_TB) k_ens_join(size_t npix, const float* mean_in, const float* within_in, float* __restrict__ run,
                                                     size_t pitch, int pos, int last, float n, float* mean_out,
                                                     float* __restrict__ between_out, float* __restrict__ within_out, float* total_out) {
#pragma clang fp contract(off)
    const size_t stride = (size_t)gridDim.x * ENS_TB;
    for (size_t o = (size_t)blockIdx.x * ENS_TB + threadIdx.x; o < npix; o += stride) {
        const float p = mean_in[o];
        const float es = pos ? run[o] + p : p;
        if (between_out) {
            const float s = within_in ? within_in[o] : 0.f;
            float ss = s * s, sd = 0.f, sq = 0.f;
            if (pos == 0) {
                if (!last) run[pitch + o] = p;
            } else {
                const float d = p - run[pitch + o];
                sd = d;
                sq = d * d;
                ss = run[4 * pitch + o] + ss;
                if (pos > 1) {
                    sd = run[2 * pitch + o] + sd;
                    sq = run[3 * pitch + o] + sq;
                }
                if (!last) {
                    run[2 * pitch + o] = sd;
                    run[3 * pitch + o] = sq;
                }
            }
            if (!last) {
                run[4 * pitch + o] = ss;
            } else {
                const float vb0 = (sq - (sd * sd) / n) / n;
                const float vb = vb0 > 0.f ? vb0 : 0.f, vw = ss / n;
                between_out[o] = sqrtf(vb);
                within_out[o] = sqrtf(vw);
                total_out[o] = sqrtf(vb + vw);
            }
        }
        if (last) mean_out[o] = es / n;
        else run[o] = es;
    }
}

void g_ens_join(hipStream_t s, size_t npix, const float* mean_in, const float* within_in, float* run, size_t pitch, int pos, int n,
                float* mean_out, float* between_out, float* within_out, float* total_out) {
    const size_t blocks = (npix + ENS_TB - 1) / ENS_TB;
    const unsigned grid = (unsigned)(blocks < (size_t)ENS_MAX_BLOCKS ? blocks : (size_t)ENS_MAX_BLOCKS);
    hipLaunchKernelGGL(k_ens_join, dim3(grid), dim3(ENS_TB), 0, s, npix, mean_in, within_in, run, pitch, pos, (int)(pos == n - 1), (float)n,
                       mean_out, between_out, within_out, total_out);
}

}  // namespace dnnca
