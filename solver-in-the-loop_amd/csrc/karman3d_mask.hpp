// karman-3d: the hard-BC face masks from the scene's `active` cell mask [Y][X][Z] ('boundary' extrapolation: outside the OPEN domain = edge
// value), shared by the step and its adjoint (karman3d.hip) and the buoyancy term (karman3d_buoyancy.hip).
#pragma once
#include "common.hpp"

__device__ __forceinline__ float acc_at(const float* act, int Y, int X, int Z, int j, int i, int k) {
    return act[((size_t)clampi(j, 0, Y - 1) * X + clampi(i, 0, X - 1)) * Z + clampi(k, 0, Z - 1)] != 0.f ? 1.f : 0.f;
}
// mask of the face of component AX (0: y, 1: x, 2: z) at (j, i, k): 1 where both adjacent cells are accessible
template <int AX>
__device__ __forceinline__ float face_mask(const float* act, int Y, int X, int Z, int j, int i, int k) {
    return acc_at(act, Y, X, Z, j - (AX == 0), i - (AX == 1), k - (AX == 2)) * acc_at(act, Y, X, Z, j, i, k);
}
