// Gradient with respect to the Reynolds number of an explicit-diffusion step, u = v_in + alpha L v_in with alpha = dt res^2 / re[b]:
//     g_re[b] = -(dt res^2 / re[b]^2) * sum over the faces e of every component of  g'_e (L v_in)_e
// g' = the cotangent the step's diffusion adjoint applies (I + alpha L^T) to, L = the replicate-padded (2 D + 1)-point Laplacian.  This
// header is the dimension-independent part (used by karman_re_bwd.hip for D = 2, karman3d_re_bwd.hip for D = 3): the forward Laplacian at one element, the order-fixed
// workgroup sum and the final sum.  A caller supplies g' and the component arrays.
//   Order     every sum is taken in a FIXED order -- a thread over its strided share, the 64 lanes of a wave by an xor butterfly, the
//             waves of the workgroup through LDS in wave order, the workgroups' partial sums in index order -- and the number of workgroups
//             is a function of the element count alone (re_nblk), never of the device: the bits do not depend on the machine or the run.
//             No floating-point atomics.
//   Precision the products and every sum are fp64 (g' and L v_in are fp32 values): the rounding of the sum itself is far below that of
//             its fp32 terms.
#pragma once
#include "common.hpp"

constexpr int RE_THREADS = 256;         // threads of a k_re_partial workgroup (four waves)
constexpr int RE_PER_THREAD = 8;        // elements per thread until RE_MAX_BLOCKS workgroups are reached
constexpr int RE_MAX_BLOCKS = 256;      // partial sums per simulation at most (the final sum walks them serially)

// workgroups (= partial sums) per simulation for `items` elements: a function of the grid alone
inline int re_nblk(size_t items) {
    const size_t per = (size_t)RE_THREADS * RE_PER_THREAD, n = (items + per - 1) / per;
    return (int)(n < 1 ? 1 : n > (size_t)RE_MAX_BLOCKS ? (size_t)RE_MAX_BLOCKS : n);
}

// (L v)[c] at element c = index x[] of a D-dimensional component array of extents n[] (last axis contiguous), replicate padding, fp32,
// in the forward step's summation order: axis 0 +, axis 0 -, axis 1 +, axis 1 -, ..., then - 2 D v[c] (2-D: up, down, right, left, - 4 c)
template <int D>
__device__ __forceinline__ float re_lap(const float* v, int c, const int (&x)[D], const int (&n)[D]) {
    int stride[D];
    stride[D - 1] = 1;
#pragma unroll
    for (int d = D - 2; d >= 0; --d) stride[d] = stride[d + 1] * n[d + 1];
    const float vc = v[c];
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float hi = x[d] + 1 < n[d] ? v[c + stride[d]] : vc, lo = x[d] > 0 ? v[c - stride[d]] : vc;
        acc = d == 0 ? hi + lo : acc + hi + lo;
    }
    return acc - (2.f * D) * vc;
}

// Sum of v over the RE_THREADS threads of the workgroup, valid in thread 0.  Every thread calls this ONCE per kernel (one static LDS array).
__device__ __forceinline__ double re_block_sum(double v) {
    __shared__ double red[RE_THREADS / 64];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < RE_THREADS / 64; ++w) s += red[w];
    return s;
}

// g_re[b] from simulation b's nblk partial sums, added in index order; accumulate: ONE fp32 add onto what g_re[b] holds
__device__ __forceinline__ void re_final(const double* partial_b, int nblk, float adt, float re_b, float* g_re_b, int accumulate) {
    double s = 0.0;
    for (int k = 0; k < nblk; ++k) s += partial_b[k];
    const float r = (float)(-(double)adt / ((double)re_b * (double)re_b) * s);
    *g_re_b = accumulate ? *g_re_b + r : r;
}
