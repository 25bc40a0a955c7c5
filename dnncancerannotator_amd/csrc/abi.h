// abi.h -- what the translation units of the C ABI share (model.hip: model, steps, staging, parameters, data parallel, measurement,
// plan dump; abi_analysis.hip: test-time augmentation and every analysis entry point; debug_tools.hip).  Internal.
#pragma once
#include "model.h"

#define MODEL(h)                                             \
    Model* M = reinterpret_cast<Model*>(h);                  \
    if (!M) { set_error("null model handle"); return DNNCA_EINVAL; }

namespace dnnca {

inline int check_batch(Model* M, int batch) {
    if (batch < 1 || batch > M->desc.max_batch) { set_error("batch %d outside [1, %d]", batch, M->desc.max_batch); return DNNCA_EINVAL; }
    return DNNCA_OK;
}

inline int check_slot(Model* M, int slot) {
    if (slot < 0 || slot >= M->stage_slots) { set_error("staging slot %d outside [0, %d)", slot, M->stage_slots); return DNNCA_EINVAL; }
    return DNNCA_OK;
}

// ---- defined in model.hip, used by abi_analysis.hip too -------------------------------------------------------------------------
// a host batch -> x_stage and, with `labels`, y_stage
int stage_inputs(Model* M, int batch, const float* x_nhwc, const float* y_hw, bool labels);
// evaluation and the one-shot counts: eval_thr + the histogram conf_dev, which keeps adding up until it is read
int confusion_begin(Model* M, const float* thresholds, int n);
void confusion_add(Model* M, size_t npix, const float* y_dev);
int confusion_finish(Model* M, dnnca_confusion* out);

}  // namespace dnnca
