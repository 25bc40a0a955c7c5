// optim.h -- the configurable optimizers (dnnca_model_set_optimizer): the chunk table, the kernel arguments and the launchers of
// kernels_opt.hip, and what those kernels share with k_adam (kernels_generic.hip): the step-output finalize and the class weight.
#pragma once
#include "common.h"

namespace dnnca {

// the positive-class weight of the step (utils/losses.py:24-29)
__device__ __forceinline__ float loss_weight(const dnnca_loss_cfg cfg, double label_sum, double n_label) {
    float w;
    if (cfg.has_weight) {
        w = cfg.weight;
    } else {
        float pr = (float)(label_sum / n_label);           // utils/losses.py:100
        w = pr > 0.f ? 1.0f / pr : 1.0f;                   // utils/losses.py:27
    }
    return cfg.weight_mul * w + cfg.weight_add;            // utils/losses.py:29
}

// out5 != nullptr: block 0 / thread 0 of the launch that applies the optimizer also turns the step's scalar block into the five step
// outputs (k_finalize_scalars' job; single-replica steps only -- under data parallel the loss slot must be final before the all-reduce)
struct AdamFinalize {
    double* scalars;
    dnnca_loss_cfg cfg;
    double n_label, inv_batch_hw;
    float* out5;
};

__device__ __forceinline__ void step_outputs(const AdamFinalize& fin) {
    fin.out5[0] = (float)(fin.scalars[3] * fin.inv_batch_hw + fin.scalars[4]);
    fin.out5[1] = (float)(fin.scalars[0] / fin.n_label);
    fin.out5[2] = loss_weight(fin.cfg, fin.scalars[0], fin.n_label);
    fin.out5[3] = (float)fin.scalars[1];
    fin.out5[4] = (float)fin.scalars[2];
}

// One block of every optimizer launch works on one chunk: at most kOptChunk consecutive elements of ONE trainable variable (a chunk
// never straddles two), so that the variable's clip scale and decay flag are uniform over the block.  Built on the host when the
// optimizer is set and uploaded once.
constexpr int kOptChunk = 1024;
constexpr int kOptThreads = 256;
struct OptChunk {
    int off;        // first element in the flat vectors
    int n;          // 1 .. kOptChunk
    int var;        // index among the trainable variables (param_infos() order)
    int decay;      // AdamW: the variable takes weight decay
};

enum { OPT_ADAM = DNNCA_OPT_ADAM, OPT_ADAMW = DNNCA_OPT_ADAMW, OPT_SGD = DNNCA_OPT_SGD };

struct OptArgs {
    float lr_t;          // Adam / AdamW: lr * sqrt(1 - beta2^t) / (1 - beta1^t), formed on the host in double
    float lr;            // SGD: this step's learning rate
    float lrwd;          // AdamW: (float)(lr * weight_decay), formed on the host in double
    float b1, b2, eps;
    float momentum;
    int nesterov;
    float gscale;        // 1 / world behind the all-reduce, else 1
    float clipvalue;     // 0: off
    const float* scales; // one clip scale per variable (grad_clip_scale), or nullptr: no clipping by norm
    float om;            // _ema twins: 1 - decay of this step's weight-average update
};

// partials[c] = sum over chunk c of (double)gh_i^2, gh = g * gscale after clipvalue; fixed summation order, no atomics
void g_grad_sqnorm(hipStream_t s, const OptChunk* chunks, int nchunks, const float* g, float gscale, float clipvalue, double* partials);
// var_first [nvars + 1]: the first chunk of every variable.  norms[0] = the norm over all of gh, norms[1 + v] = variable v's;
// scales[v] = c / max(norm, c): clipnorm > 0 with variable v's norm, else global_clipnorm with the norm over all
void g_grad_clip_scale(hipStream_t s, const int* var_first, int nvars, int nchunks, const double* partials, float clipnorm,
                       float global_clipnorm, float* scales, double* norms);
// kind OPT_*; e != nullptr: the _ema twin.  m: Adam's first moment or SGD's accumulator; v: Adam's second moment (SGD: untouched)
void g_opt_step(hipStream_t s, int kind, const OptChunk* chunks, int nchunks, float* p, const float* g, float* m, float* v, float* e,
                const OptArgs& a, const AdamFinalize& fin);

}  // namespace dnnca
