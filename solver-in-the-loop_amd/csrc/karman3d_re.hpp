// karman-3d: what the Reynolds-number gradient (karman3d_re_bwd.hip) shares with the two adjoints that call it (karman3d.hip's
// sol_karman3d_step_bwd_re, karman3d_density_bwd.hip): the density path's cotangent at a face, and the launcher of the reduction.
// The 3-D twin of karman_re.hpp; re_reduce.hpp holds the dimension-independent part.
#pragma once
#include "fixed_scatter.hpp"
#include "re_reduce.hpp"

// g' of the density path: the cell-to-face transpose of the back-trace term gU [Y][X][Z] (a centre velocity is the mean of its two faces;
// out-of-range cells count as zero), times (1 - velBCyMask) on v_y.  k3d_diffuse_adj applies (I + alpha L^T) to it, k3_re_partial<RE3_GU>
// sums it against L v_in: ONE spelling for both.
__device__ __forceinline__ float k3d_face_y(const float* uy, const float* m, int Y, int X, int Z, int jf, int i, int k) {
#pragma clang fp contract(off)
    const size_t c = ((size_t)jf * X + i) * Z + k, sy = (size_t)X * Z;
    const float lo = jf > 0 ? uy[c - sy] : 0.f, hi = jf < Y ? uy[c] : 0.f;
    return 0.5f * (lo + hi) * (1.f - m[c]);
}
__device__ __forceinline__ float k3d_face_x(const float* ux, int X, int Z, int j, int iF, int k) {
#pragma clang fp contract(off)
    const size_t c = ((size_t)j * X + iF) * Z + k;           // cell (j, iF, k); the face's low neighbour is one cell column before it
    const float lo = iF > 0 ? ux[c - Z] : 0.f, hi = iF < X ? ux[c] : 0.f;
    return 0.5f * (lo + hi);
}
__device__ __forceinline__ float k3d_face_z(const float* uz, int X, int Z, int j, int i, int kF) {
#pragma clang fp contract(off)
    const size_t c = ((size_t)j * X + i) * Z + kF;
    const float lo = kF > 0 ? uz[c - 1] : 0.f, hi = kF < Z ? uz[c] : 0.f;
    return 0.5f * (lo + hi);
}

// Where g' of the reduction comes from
enum Re3Src {
    RE3_FIXED = 0,      // the velocity adjoint's int64 fixed-point g_c (what k3b_diffuse_adj reads), gmax = max|g_a| slots
    RE3_GU = 1,         // the density adjoint's back-trace term gU per cell (k3d_advect_adj*), gmax = max|g_d_out| slots
};

struct Re3In {
    Re3Src src;
    const long long *gcy, *gcx, *gcz;    // RE3_FIXED: [B][(Y+1) X Z], [B][Y (X+1) Z], [B][Y X (Z+1)]
    const float *gUy, *gUx, *gUz;        // RE3_GU:    [B][Y X Z] each
    const unsigned* gmax;                // [B][FX_SLOTS]: the scale of the fixed-point values; a poisoned simulation (non-finite cotangent) gets g_re = NaN
    const float* bcm;                    // velBCyMask
    long bc_stride;
    const float *vy_in, *vx_in, *vz_in, *re;      // the step's INPUT velocity and Reynolds numbers
    double* partial;                     // [B][re_nblk(faces)] scratch (sol_re3_partial_behind)
    float* g_re;                         // [B]
    int accumulate;                      // 1: one fp32 add onto g_re
};

// what an adjoint's _re entry point takes beyond the plain form's arguments
struct Re3Extra {
    const float *vy_in, *vx_in, *vz_in;  // the step's input velocity
    float* g_re;                         // [B]
    int accumulate;
};

// the partial sums for cfg's grid and batch as the optional last member of an adjoint's layout (carve.hpp): behind the plain call's
// part `plain`, on the next eight bytes past plain.bytes() of the caller's pointer; *bytes = the layout's bytes with them (256-byte
// granule; includes the eight bytes that align the doubles)
double* sol_re3_partial_behind(const Carve& plain, const sol_karman3d_cfg* c, size_t* bytes);
// the two launches (k3_re_partial, k3_re_final) on stream s: no synchronisation, no allocation, nothing read on the host
int sol_re3_reduce(hipStream_t s, const sol_karman3d_cfg* c, const Re3In& in);
