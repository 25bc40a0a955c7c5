// refine.h -- mask refinement of the lesion tables and the boundary distances (dnnca_model_set_lesion_refine, kernels_refine.hip):
// hysteresis, then the opening, then closing and hole filling, on the prediction plane of one chunk, before its components are
// numbered.  lesion_run and surface_distances (kernels_region.hip) call refine_chunk in the place of their prep / open launches
// while the refinement is on; while it is off they never come here.
#pragma once
#include "region.h"

namespace dnnca {

constexpr int kRefineMaxClose = 15;      // closing_size: odd, 3 .. 15 (the LDS tile of region_close is sized for it)

inline bool refine_on(const dnnca_lesion_refine& c) { return c.hysteresis_low != 0.f || c.closing_size > 1 || c.fill_holes != 0; }
// do two configurations make the same masks?  (closing sizes 0 and 1 are both "off")
inline bool refine_same(const dnnca_lesion_refine& a, const dnnca_lesion_refine& b) {
    return a.hysteresis_low == b.hysteresis_low && std::max(a.closing_size, 1) == std::max(b.closing_size, 1) && a.fill_holes == b.fill_holes;
}
// nullptr, or why dnnca_model_set_lesion_refine refuses the configuration
const char* refine_invalid(const dnnca_lesion_refine& c);

// what the stage borrows from the chunk's workspace: two word planes, the parents and sizes planes that lesion_plane writes only
// afterwards (labels and flags here), and room for two thresholds on the device.  n = nb * out_h * out_w elements each
struct RefineWs {
    uint32_t *w0, *w1;
    int* lab;
    unsigned* flag;
    float* thr;
};

// The refined mask of `nb` slices of src (device [nb, rz.in_h, rz.in_w]) in bit 0 of *fg (w0 or w1): region_prep at
// thr_host = {hysteresis_low, threshold} (host, alive until the chunk's synchronisation; without hysteresis only [1] is read),
// the hysteresis launches, region_open with filter size k, region_close, the hole-filling launches.  Every launch goes through
// LAUNCH; a dry run touches no memory
int refine_chunk(Model* M, const dnnca_lesion_refine& cfg, const float* src, const Resize& rz, int nb, const float* thr_host, int k,
                 const RefineWs& ws, const uint32_t** fg);

// the launches of kernels_region.hip that the stage reuses
void region_prep_launch(Model* M, const float* src, const Resize& rz, int nb, const float* thr_dev, int T, uint32_t* words);
void region_open_launch(Model* M, const uint32_t* in, uint32_t* out, int oh, int ow, int k, int nb);
void region_ccl(Model* M, const uint32_t* words, int T, int nb, int h, int w, int* L);

}  // namespace dnnca
