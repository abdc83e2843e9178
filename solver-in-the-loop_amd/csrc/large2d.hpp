// Device helpers of the large-grid karman-2d step, shared by the forward kernels (karman_large.hip) and the adjoint (karman_large_bwd.hip)
#pragma once
#include "common.hpp"

__device__ __forceinline__ float acc_at(const float* act, int Y, int X, int j, int i) {   // 'boundary' extrapolation of the active mask
    return act[clampi(j, 0, Y - 1) * X + clampi(i, 0, X - 1)] != 0.f ? 1.f : 0.f;
}
// hard-BC face masks: a face is open iff both cells it separates are accessible (outside the OPEN domain counts as accessible)
__device__ __forceinline__ float mask_y(const float* act, int Y, int X, int j, int i) {   // face between rows j-1 and j
    return acc_at(act, Y, X, j - 1, i) * acc_at(act, Y, X, j, i);
}
__device__ __forceinline__ float mask_x(const float* act, int Y, int X, int j, int i) {   // face between columns i-1 and i
    return acc_at(act, Y, X, j, i - 1) * acc_at(act, Y, X, j, i);
}
