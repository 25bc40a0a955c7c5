// bootstrap.h -- the bootstrap over exams of dnnca_bootstrap_sums / dnnca_bootstrap_detection (kernels_bootstrap.hip): one workgroup
// per replicate draws the exams' multiplicities into LDS and reduces the resampled statistics from them (include/dnnca.h states the
// resampling and the statistics; tests/bootstrap_oracle.py states them in numpy and Python integers).
#pragma once
#include "model.h"

namespace dnnca {

constexpr int kBootMaxExams = 16384;                 // the 16-bit counters of a replicate: 32 KiB of LDS
constexpr int kBootMaxCandidates = 1 << 22;
constexpr int kBootMaxReplicates = 1 << 20;
constexpr int kBootMaxColumns = 64;
constexpr int kBootMaxStrata = 8;
constexpr int kBootTile = DNNCA_BOOTSTRAP_TILE;      // candidates per step of boot_detect: four per thread

// E, R, the strata and the pool of both calls; DNNCA_EINVAL with the reason otherwise
int bootstrap_check_resampling(int E, const int32_t* pool, const int32_t* strata, int S, int R);
// everything else dnnca_bootstrap_detection refuses
int bootstrap_check_detection(const dnnca_bootstrap_exam* exams, int E, const dnnca_bootstrap_candidate* cands, int N);
// the two calls on checked arguments (host pointers in and out).  The workspace is the model's own bootstrap scratch, grown on
// demand; the replicates run in chunks that bound it.  Synchronise.
int bootstrap_sums(Model* M, const int32_t* cols, int E, int K, const int32_t* pool, const int32_t* strata, int S, int R, uint64_t seed,
                   int64_t* out, uint16_t* mult_out);
int bootstrap_detection(Model* M, const dnnca_bootstrap_exam* exams, int E, const dnnca_bootstrap_candidate* cands, int N,
                        const int32_t* pool, const int32_t* strata, int S, int R, uint64_t seed, dnnca_bootstrap_detection_row* out,
                        uint16_t* mult_out);

}  // namespace dnnca
