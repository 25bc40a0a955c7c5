// accum.h -- gradient accumulation (dnnca_model_set_accumulation): the launcher of kernels_accum.hip.  One optimizer update takes the
// float32 sum of k micro-batch gradients: a <- g on the first micro-step of a cycle, a <- a + g on the later ones, one add per element
// per micro-step in micro-step order, so the accumulator is bit-identical from run to run.
#pragma once
#include "optim.h"

namespace dnnca {

constexpr int kAccumMaxSteps = 4096;
constexpr int kAccumThreads = 256;
constexpr int kAccumMaxBlocks = 2048;      // grid = min(blocks needed, this); the rest is a grid-stride loop

// a[i] = first ? g[i] : a[i] + g[i] for i < n.  a and g start at allocation-aligned (16-byte) addresses: float4 over the body, one
// element per thread over the n % 4 tail.  fin.out5 != nullptr: block 0 / thread 0 also writes the step outputs (as k_opt does).
// loss_slot: block 0 / thread 0 also copies g[n] (the step's loss, final before this launch) to a[n] for the all-reduce of [a, loss]
void g_grad_accumulate(hipStream_t s, size_t n, float* a, const float* g, bool first, const AdamFinalize& fin, bool loss_slot);

}  // namespace dnnca
