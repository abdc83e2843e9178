// Order-independent scatter in 64-bit fixed point: the accumulation scheme of the advection adjoints of the 3-D step (karman3d.hip,
// k3b_*) and of the large-grid 2-D step (karman_large_bwd.hip, k_lb_*).  This comment is the one statement of the scheme.
//
// A cotangent g_a is scattered through the gathers of the semi-Lagrangian step into accumulators g_c.  Floating-point atomics would make
// the sum depend on the order of arrival; here every contribution is rounded to a fixed-point grid ON ITS OWN (__float2ll_rn(v * qs)) and
// added as a 64-bit integer.  Integer addition commutes, so the adjoint is reproducible bit for bit, and a contribution may be added to
// global memory or to an LDS window that is flushed later: both give the same bits.
//   Scale       per simulation, a power of two: qs = 2^(37 - e) with max|g_a| in [2^e, 2^(e+1)), so max|g_a| * qs lies in [2^37, 2^38);
//               qi = 1 / qs converts back.  max|g_a| is published by the kernel that writes g_a (fx_publish_max) into FX_SLOTS words per
//               simulation and read back by every later kernel (fx_scale).
//   Range       int64 leaves 2^25 above max|g_a| for a single contribution.  A FINITE contribution beyond that saturates in __float2ll_rn:
//               the back-trace term is g_a times a DIFFERENCE of the saved velocity times dt/dx, so that takes |dv| dt/dx > 3e7 -- a
//               simulation that has long blown up.  The MacCormack adjoint (karman_maccormack.hip) keeps this one scale for its second
//               accumulator too: g_h = g_a + the scattered g_b has |g_h| <= max|g_a| (1 + s/2 x fan-in), a small multiple of max|g_a| and
//               far inside the 2^25 of headroom, so the statement above holds for every contribution of both stages.
//   Resolution  2^-37 max|g_a| per contribution.
//   Poisoning   a NON-FINITE g_a publishes the bits of a NaN, the largest value the integer maximum can see; fx_scale turns that into
//               "scatter nothing (qs = 0), convert back to NaN (qi = NaN)": EVERY input gradient of that simulation is NaN -- as fp32
//               atomics would have left it -- never a finite number made of saturated integer conversions.
#pragma once
#include "common.hpp"

constexpr int FX_SLOTS = 64;            // absmax slots per simulation (one per lane of the reading wave; same-address atomics serialise in the L2)
constexpr int FX_FIXBITS = 37;          // max|g_a| * qs lies in [2^37, 2^38)

// scale of simulation b's scatter and its inverse, from the published max|g_a| (wave-uniform result)
__device__ __forceinline__ void fx_scale(const unsigned* gmax_b, float& qs, float& qi) {
    const unsigned m = amax_wave_max(gmax_b[threadIdx.x & (FX_SLOTS - 1)]);
    if (m >= 0x7f800000u) {                   // poisoned (see above)
        qs = 0.f;
        qi = __uint_as_float(0x7fc00000u);
        return;
    }
    int e = (int)(m >> 23) - 127;
    e = m == 0u ? 0 : min(max(e, -80), 120);
    qs = __uint_as_float((unsigned)(FX_FIXBITS - e + 127) << 23);
    qi = __uint_as_float((unsigned)(e - FX_FIXBITS + 127) << 23);
}

// Publishes max|g_a| of simulation b (slots_b = its FX_SLOTS words, zeroed beforehand): vmax = this thread's maximum, bad = it met an inf
// or a nan (fmaxf drops a NaN, so the caller tracks it).  Every thread of the workgroup calls this ONCE per kernel, after its loop (it holds
// a barrier and one static LDS array: a second call in the same kernel would race on it).  At most one
// atomic per workgroup: thousands of workgroups share the slots and same-address atomics serialise in the L2 (~0.3 us apiece), so a
// workgroup whose maximum does not exceed what its slot already holds publishes nothing; the maximum is order independent, the filter
// changes nothing but the number of atomics.
// (the two pieces of it: what a wave publishes -- the bits of its maximum, of a NaN when it met a non-finite value -- and the workgroup's
// filtered atomic into its slot)
__device__ __forceinline__ unsigned fx_wave_bits(float vmax, bool bad) { return amax_wave_max(bad ? 0x7fc00000u : __float_as_uint(vmax)); }
__device__ __forceinline__ void fx_slot_max(unsigned* slots_b, const unsigned* red) {
    unsigned mb = 0u;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) mb = max(mb, red[w]);
    unsigned* slot = &slots_b[blockIdx.x & (FX_SLOTS - 1)];
    if (mb > __atomic_load_n(slot, __ATOMIC_RELAXED)) atomicMax(slot, mb);
}
__device__ __forceinline__ void fx_publish_max(unsigned* slots_b, float vmax, bool bad) {
    __shared__ unsigned red[16];
    const unsigned wmax = fx_wave_bits(vmax, bad);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wmax;
    __syncthreads();
    if (threadIdx.x == 0) fx_slot_max(slots_b, red);
}
// the same for TWO cotangents of one kernel (the stage-alone MacCormack adjoint: velocity and density), one barrier: thread 0 publishes
// the first, thread 1 the second.  Once per kernel, like fx_publish_max, and not in a kernel that also calls that.
__device__ __forceinline__ void fx_publish_max2(unsigned* slots_a, float vmax_a, bool bad_a, unsigned* slots_b, float vmax_b, bool bad_b) {
    __shared__ unsigned red[2][16];
    const unsigned wa = fx_wave_bits(vmax_a, bad_a), wb = fx_wave_bits(vmax_b, bad_b);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = wa; red[1][threadIdx.x >> 6] = wb; }
    __syncthreads();
    if (threadIdx.x < 2) fx_slot_max(threadIdx.x == 0 ? slots_a : slots_b, red[threadIdx.x]);
}

// one contribution: rounded to the grid first, then an integer add -- to an accumulator in global memory, or to a cell of an LDS window
__device__ __forceinline__ void fx_add(long long* p, float v, float qs) {
    ::atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__float2ll_rn(v * qs));
}
__device__ __forceinline__ void fx_add(unsigned long long* p, float v, float qs) { ::atomicAdd(p, (unsigned long long)__float2ll_rn(v * qs)); }

// An LDS window of n cells, worked by `nthreads` threads: cleared before the scatter, flushed after it with ONE global atomic per non-zero
// cell.  global_of(e) = the accumulator of window cell e.  (Window cells outside the arrays never receive a contribution, so they are
// zero and global_of is never asked for them.)  The caller puts a __syncthreads() between clear, scatter and flush.
__device__ __forceinline__ void fx_window_clear(unsigned long long* win, int n, int nthreads) {
    for (int e = threadIdx.x; e < n; e += nthreads) win[e] = 0ull;
}
template <class GlobalOf>
__device__ __forceinline__ void fx_window_flush(const unsigned long long* win, int n, int nthreads, const GlobalOf& global_of) {
    for (int e = threadIdx.x; e < n; e += nthreads) {
        const unsigned long long v = win[e];
        if (v == 0ull) continue;
        ::atomicAdd(reinterpret_cast<unsigned long long*>(global_of(e)), v);
    }
}

// accumulator q back in fp32; fx_get_fma: the same fused with an addend, fma(convert(g[q]), qi, add) -- one rounding
__device__ __forceinline__ float fx_get(const long long* g, int q, float qi) { return __ll2float_rn(g[q]) * qi; }
__device__ __forceinline__ float fx_get_fma(const long long* g, int q, float qi, float add) { return __fmaf_rn(__ll2float_rn(g[q]), qi, add); }

// (L^T g') at element c = index x[] of a D-dimensional component array of extents n[] (last axis contiguous), g' = g . sc (sc_here at c,
// 1 - scm[] at the neighbours; scm = NULL: sc = 1): the transposed replicate-padded (2 D + 1)-point Laplacian in gather form -- a
// neighbour inside the array contributes g' there, a direction that leaves the array contributes g'[c] itself.  The neighbours are added
// in the order axis 0 +, axis 0 -, axis 1 +, ...: a reordered sum would move the bits.
// CAUTION for the callers' last step, g' + alpha * lapT: the two diffusion adjoints round it DIFFERENTLY, each as its kernel always has.
// k3b_diffuse_adj fuses the CENTRE product, fma(g[c] (* qi), sc or qi, round(alpha * lapT)); k_lb_diffuse_adj fuses alpha * lapT,
// fma(alpha, lapT, round(g')).  Both spell their fma out (the compiler's own choice depended on the surrounding code); a kernel that
// switches form moves its gradients by an ulp.
template <int D>
__device__ __forceinline__ float lapT(const long long* g, float qi, float sc_here, const float* scm, int c, const int (&x)[D], const int (&n)[D]) {
    auto at = [&](int q) { const float v = fx_get(g, q, qi); return scm ? v * (1.f - scm[q]) : v; };
    const float v = fx_get(g, c, qi) * sc_here;
    float acc = (-2.f * D) * v;
    int stride[D];
    stride[D - 1] = 1;
#pragma unroll
    for (int d = D - 2; d >= 0; --d) stride[d] = stride[d + 1] * n[d + 1];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        acc += x[d] + 1 < n[d] ? at(c + stride[d]) : v;
        acc += x[d] > 0 ? at(c - stride[d]) : v;
    }
    return acc;
}
