// detect.h -- the detection map of dnnca_detection_map (kernels_detect.hip): ranked lesion candidates by the dynamic extraction
// (strongest peak, region at a fraction of the peak's height, erase, repeat), all slices of a batch in lock-step on the device.
#pragma once
#include "model.h"

namespace dnnca {

// the ranges of dnnca_detection_cfg (a NaN fails); DNNCA_EINVAL with the reason otherwise
int detection_check(const dnnca_detection_cfg& c);
// src: device [batch, h, w] probabilities; dst: device [batch, h, w] receives the map (dst may be src: every pixel is read before it
// is written, by the same thread).  h * w below 2^31, batch <= 65535.  rows (host [batch * c.max_candidates]) receives *n_rows records
// sorted by (slice, number), slices (host [batch]) every slice's record, out_hw (host, or nullptr) a copy of dst.  The workspace is
// the model's own detection scratch (grown on demand): no plane, variable, state or carry of another call is touched.  Synchronises.
// In a dry run (M->dry) nothing is allocated and none of the host pointers is touched
int detection_map(Model* M, const float* src, float* dst, int batch, int h, int w, const dnnca_detection_cfg& c, float* out_hw,
                  dnnca_detection_row* rows, int64_t* n_rows, dnnca_detection_slice* slices);

}  // namespace dnnca
