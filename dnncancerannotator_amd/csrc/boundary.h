// boundary.h -- the signed Euclidean distance map of a label plane (kernels_boundary.hip): the constant of the boundary term of the
// training loss (dnnca_model_set_boundary_loss) and what dnnca_signed_distance_of returns.
#pragma once
#include <cstdint>

#include "model.h"

namespace dnnca {

// y: device [B, H, W] labels, G = { y > 0.5 }.  boundary_cols writes cols[B, H, W]: per pixel the rows to the nearest pixel of G in
// its column (low half) and to the nearest pixel outside G (high half), kSurfaceFar where the column has none.  boundary_rows takes
// the lower envelope over the pixel's row and writes phi[B, H, W]: sqrt(d2) outside G, 1 - sqrt(d2) inside, 0 where the other set
// is empty; and, d2 != nullptr, the exact squared distance (0 where the other set is empty).  H, W <= kSurfaceMaxSide, B <= 65535.
// No atomics: every value is a function of the labels alone.
void boundary_transform(Model* m, const float* y, int B, int H, int W, uint32_t* cols, float* phi, int32_t* d2);

}  // namespace dnnca
