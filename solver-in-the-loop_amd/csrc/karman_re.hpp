// karman-2d: what the Reynolds-number gradient (karman_re_bwd.hip) shares with the two adjoints that call it (karman_large_bwd.hip,
// karman_density_bwd.hip): the density path's cotangent at a face, and the launcher of the reduction.
#pragma once
#include "fixed_scatter.hpp"
#include "re_reduce.hpp"

// g' of the density path: the cell-to-face transpose of the back-trace term gU (a centre velocity is the mean of its two faces; out-of-range
// cells count as zero), times (1 - velBCyMask) on v_y.  k_kd_diffuse_adj applies (I + alpha L^T) to it, k_re_partial<RE_GU> sums it
// against L v_in: ONE spelling for both.
__device__ __forceinline__ float kd_face_y(const float* uy, const float* m, int Y, int X, int jf, int i) {
#pragma clang fp contract(off)
    const float lo = jf > 0 ? uy[(jf - 1) * X + i] : 0.f, hi = jf < Y ? uy[jf * X + i] : 0.f;
    return 0.5f * (lo + hi) * (1.f - m[jf * X + i]);
}
__device__ __forceinline__ float kd_face_x(const float* ux, int X, int j, int iF) {
#pragma clang fp contract(off)
    const float lo = iF > 0 ? ux[j * X + iF - 1] : 0.f, hi = iF < X ? ux[j * X + iF] : 0.f;
    return 0.5f * (lo + hi);
}

// Where g' of the reduction comes from
enum ReSrc {
    RE_FIXED = 0,       // the velocity adjoint's int64 fixed-point g_c (between k_lb_advect_adj* and k_lb_diffuse_adj), gmax = max|g_a| slots
    RE_GU = 1,          // the density adjoint's back-trace term gU per cell (k_kd_advect_adj*), gmax = max|g_d_out| slots
};

struct ReIn {
    ReSrc src;
    const long long *gcy, *gcx;          // RE_FIXED: [B][(Y+1) X], [B][Y (X+1)]
    const float *gUy, *gUx;              // RE_GU:    [B][Y X] each
    const unsigned* gmax;                // [B][FX_SLOTS]: the scale of the fixed-point values; a poisoned simulation (non-finite cotangent) gets g_re = NaN
    const float *bcm;                    // velBCyMask
    long bc_stride;
    const float *vy_in, *vx_in, *re;     // the step's INPUT velocity and Reynolds numbers
    double* partial;                     // [B][re_nblk(faces)] scratch, sol_re_partial_take
    float* g_re;                         // [B]
    int accumulate;                      // 1: one fp32 add onto g_re
};

// what an adjoint's _re entry point takes beyond the plain form's arguments
struct ReExtra {
    const float *vy_in, *vx_in;          // the step's input velocity
    float* g_re;                         // [B]
    int accumulate;
};

// the partial sums for cfg's grid and batch as the optional last member of an adjoint's layout (carve.hpp)
double* sol_re_partial_take(Carve& w, const sol_karman_cfg* c);
// the two launches (k_re_partial, k_re_final) on stream s: no synchronisation, no allocation, nothing read on the host
int sol_re_reduce(hipStream_t s, const sol_karman_cfg* c, const ReIn& in);
