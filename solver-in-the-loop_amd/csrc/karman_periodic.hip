// Periodic domain boundaries of the large-grid karman-2d step: the stencil phases of karman_large.hip and the adjoint stages of
// karman_large_bwd.hip with WRAPPED indices along an axis declared periodic, templated on <PY, PX>.  The open kernels are not touched:
// sol_large_front, sol_large_project and the body of the adjoint come here only when the host header of the direct blob carries a
// periodic bit (SOL_DIRECT_HDR_PERIODIC_Y / _X, sol_periodic_bits).  The pressure solve is the same algorithm on other tables
// (precond.hartley_matrix); its products accumulate in fp64 on a periodic blob (k_p_gemm below says why).
//
// Conventions (include/sol_hip.h, "PERIODIC BOUNDARIES"):
//   - array shapes do not change; on a periodic axis the last face plane is a DUPLICATE of plane 0 (y: vy[:, Y, :], x: vx[:, :, X]);
//   - no kernel reads a duplicate plane of an input: every index the open kernels clamp (or send to the density's zero ghost ring) is
//     taken modulo n over the unique planes 0 .. n-1 -- a true modulo (wrapi), a departure point several periods away lands correctly;
//   - the forward kernels write the duplicate plane of their outputs by running plane 0's arithmetic a second time on plane 0's inputs
//     (a thread of the duplicate plane maps itself to the unique face first): equal bits;
//   - the adjoint first adds the cotangent of an output duplicate plane onto plane 0's (pb_gy / pb_gx: one fp32 add, spelled once and
//     evaluated wherever the cotangent is read), scatters into unique planes only, and writes an exact zero to the duplicate planes of
//     the input gradient;
//   - the open axis of a mixed scene keeps the open kernels' expressions: clamp, velBC blend, grad_pad.
// The advection adjoint scatters in 64-bit fixed point (fixed_scatter.hpp) with global atomics; the LDS-window form is not built for
// periodic scenes (the option k2d_adj_tile does not apply to them).
#include "fixed_scatter.hpp"
#include "large2d.hpp"

namespace {

__device__ __forceinline__ int wrapi(int i, int n) { const int r = i % n; return r < 0 ? r + n : r; }
// an index along one axis: periodic -> modulo the n unique planes; open -> clamped to [0, hi] as the open kernels do
template <bool P> __device__ __forceinline__ int axi(int i, int n, int hi) { return P ? wrapi(i, n) : clampi(i, 0, hi); }
// the successor of a unique index u (0 <= u < n on a periodic axis)
template <bool P> __device__ __forceinline__ int nxt(int u, int n) { return P ? (u + 1 == n ? 0 : u + 1) : u + 1; }

template <bool PY, bool PX> __device__ __forceinline__ float p_acc(const float* act, int Y, int X, int j, int i) {
    return act[axi<PY>(j, Y, Y - 1) * X + axi<PX>(i, X, X - 1)] != 0.f ? 1.f : 0.f;
}
template <bool PY, bool PX> __device__ __forceinline__ float p_mask_y(const float* act, int Y, int X, int j, int i) {
    return p_acc<PY, PX>(act, Y, X, j - 1, i) * p_acc<PY, PX>(act, Y, X, j, i);
}
template <bool PY, bool PX> __device__ __forceinline__ float p_mask_x(const float* act, int Y, int X, int j, int i) {
    return p_acc<PY, PX>(act, Y, X, j, i - 1) * p_acc<PY, PX>(act, Y, X, j, i);
}

struct PArgs {
    int B, Y, X;
    float dtdx, dt, adt;
    int grad_pad, inflow_before;
    const float *d_in, *vy_in, *vx_in, *re, *active, *inflow, *bcv, *bcm;
    long bc_stride;
    float *d_out, *vy_out, *vx_out, *svy, *svx, *rhs, *feat;
    const float* p;
    float fs0, fs1, fs2;
};

template <bool PY, bool PX> __global__ void __launch_bounds__(256) k_p_diffuse(PArgs a) {
    const int Y = a.Y, X = a.X, XP = X + 1, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const float alpha = a.adt / a.re[b];
    const float* vy = a.vy_in + (size_t)b * nVy;
    const float* vx = a.vx_in + (size_t)b * nVx;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nVy + nVx; k += gridDim.x * blockDim.x) {
        if (k < nVy) {
            const int j = k / X, i = k - j * X, je = (PY && j == Y) ? 0 : j, ke = je * X + i;
            const float c = vy[ke];
            const float lap = vy[axi<PY>(je + 1, Y, Y) * X + i] + vy[axi<PY>(je - 1, Y, Y) * X + i] + vy[je * X + axi<PX>(i + 1, X, X - 1)] +
                              vy[je * X + axi<PX>(i - 1, X, X - 1)] - 4.f * c;
            float v = c + alpha * lap;
            v = v * (1.f - a.bcm[(size_t)b * a.bc_stride + ke]) + a.bcv[(size_t)b * a.bc_stride + ke];
            a.svy[(size_t)b * nVy + k] = v;
        } else {
            const int q = k - nVy, j = q / XP, i = q - j * XP, ie = (PX && i == X) ? 0 : i;
            const float c = vx[j * XP + ie];
            const float lap = vx[axi<PY>(j + 1, Y, Y - 1) * XP + ie] + vx[axi<PY>(j - 1, Y, Y - 1) * XP + ie] + vx[j * XP + axi<PX>(ie + 1, X, X)] +
                              vx[j * XP + axi<PX>(ie - 1, X, X)] - 4.f * c;
            a.svx[(size_t)b * nVx + q] = c + alpha * lap;
        }
    }
}

// the four corners and the weights of a bilinear gather from component C (0: v_y [Y+1][X], 1: v_x [Y][X+1]) around (jb, ib) + (oy, ox):
// floorf and the weights as k_l_advect's bil_clamp; the corner indices wrapped on a periodic axis, clamped on an open one
struct PBil { int j0, j1, i0, i1; float wy, wx; };
template <int C, bool PY, bool PX> __device__ __forceinline__ PBil p_bil(int Y, int X, int jb, float oy, int ib, float ox) {
    PBil s;
    const float fy = floorf(oy), fx = floorf(ox);
    s.wy = oy - fy; s.wx = ox - fx;
    const int H = Y + (C == 0), W = X + (C == 1);
    const int j0 = jb + (int)fy, i0 = ib + (int)fx;
    s.j0 = axi<PY>(j0, Y, H - 1); s.j1 = PY ? nxt<true>(s.j0, Y) : clampi(j0 + 1, 0, H - 1);
    s.i0 = axi<PX>(i0, X, W - 1); s.i1 = PX ? nxt<true>(s.i0, X) : clampi(i0 + 1, 0, W - 1);
    return s;
}
__device__ __forceinline__ float p_bil_eval(const float* f, int W, const PBil& s) {
    const float f00 = f[s.j0 * W + s.i0], f01 = f[s.j0 * W + s.i1], f10 = f[s.j1 * W + s.i0], f11 = f[s.j1 * W + s.i1];
    return (1.f - s.wy) * ((1.f - s.wx) * f00 + s.wx * f01) + s.wy * ((1.f - s.wx) * f10 + s.wx * f11);
}

template <bool PY, bool PX> __global__ void __launch_bounds__(256) k_p_advect(PArgs a) {
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const float* sy = a.svy + (size_t)b * nVy;
    const float* sx = a.svx + (size_t)b * nVx;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nVy + nVx + N; k += gridDim.x * blockDim.x) {
        if (k < nVy) {
            const int j = k / X, i = k - j * X, je = (PY && j == Y) ? 0 : j;
            const float uy = sy[je * X + i];
            const int ja = PY ? wrapi(je - 1, Y) : max(je - 1, 0), jb = PY ? je : min(je, Y - 1), i1 = nxt<PX>(i, X);
            const float ux = 0.25f * (sx[ja * XP + i] + sx[ja * XP + i1] + sx[jb * XP + i] + sx[jb * XP + i1]);
            const PBil s = p_bil<0, PY, PX>(Y, X, je, -uy * a.dtdx, i, -ux * a.dtdx);
            a.vy_out[(size_t)b * nVy + k] = p_bil_eval(sy, X, s) * p_mask_y<PY, PX>(a.active, Y, X, je, i);
        } else if (k < nVy + nVx) {
            const int q = k - nVy, j = q / XP, i = q - j * XP, ie = (PX && i == X) ? 0 : i;
            const float ux = sx[j * XP + ie];
            const int ia = PX ? wrapi(ie - 1, X) : max(ie - 1, 0), ib = PX ? ie : min(ie, X - 1), j1 = nxt<PY>(j, Y);
            const float uy = 0.25f * (sy[j * X + ia] + sy[j * X + ib] + sy[j1 * X + ia] + sy[j1 * X + ib]);
            const PBil s = p_bil<1, PY, PX>(Y, X, j, -uy * a.dtdx, ie, -ux * a.dtdx);
            a.vx_out[(size_t)b * nVx + q] = p_bil_eval(sx, XP, s) * p_mask_x<PY, PX>(a.active, Y, X, j, ie);
        } else if (a.d_out) {
            const int c = k - nVy - nVx, j = c / X, i = c - j * X;
            const float* gd = a.d_in + (size_t)b * N;
            const float uy = 0.5f * (sy[c] + sy[nxt<PY>(j, Y) * X + i]);
            const float ux = 0.5f * (sx[j * XP + i] + sx[j * XP + nxt<PX>(i, X)]);
            const float oy = -uy * a.dtdx, ox = -ux * a.dtdx;
            const float fy = floorf(oy), fx = floorf(ox);
            const float wy = oy - fy, wx = ox - fx;
            const int j0 = j + (int)fy, i0 = i + (int)fx;
            float f[2][2];
            for (int dj = 0; dj < 2; ++dj)
                for (int di = 0; di < 2; ++di) {
                    // periodic axis: modulo; open axis: one ring of zero ghost cells (extrapolation 'constant')
                    const int jr = j0 + dj, ir = i0 + di;
                    const int jj = PY ? wrapi(jr, Y) : jr, ii = PX ? wrapi(ir, X) : ir;
                    float v = 0.f;
                    if (jj >= 0 && jj < Y && ii >= 0 && ii < X) {
                        v = gd[jj * X + ii];
                        if (a.inflow_before) v += a.inflow[jj * X + ii];
                    }
                    f[dj][di] = v;
                }
            float v = (1.f - wy) * ((1.f - wx) * f[0][0] + wx * f[0][1]) + wy * ((1.f - wx) * f[1][0] + wx * f[1][1]);
            if (!a.inflow_before) v += a.inflow[c] * a.dt;
            a.d_out[(size_t)b * N + c] = v;
        }
    }
}

template <bool PY, bool PX> __global__ void __launch_bounds__(256) k_p_div(PArgs a) {
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const float* vy = a.vy_out + (size_t)b * nVy;
    const float* vx = a.vx_out + (size_t)b * nVx;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < N; c += gridDim.x * blockDim.x) {
        const int j = c / X, i = c - j * X;
        const float div = (vy[nxt<PY>(j, Y) * X + i] - vy[j * X + i]) + (vx[j * XP + nxt<PX>(i, X)] - vx[j * XP + i]);
        a.rhs[(size_t)b * N + c] = -div;
    }
}

// v -= mask * grad p in place.  A face reads and writes ITS OWN element only (the duplicate plane holds plane 0's bits since k_p_advect
// and gets plane 0's arithmetic): no thread reads an element another one writes.
template <bool PY, bool PX> __global__ void __launch_bounds__(256) k_p_project(PArgs a) {
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const float* P = a.p + (size_t)b * N;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nVy + nVx; k += gridDim.x * blockDim.x) {
        if (k < nVy) {
            const int j = k / X, i = k - j * X, je = (PY && j == Y) ? 0 : j;
            float g = 0.f;
            if (PY) g = P[je * X + i] - P[wrapi(je - 1, Y) * X + i];         // no boundary face along a periodic axis: grad_pad is not read
            else if (j >= 1 && j <= Y - 1) g = P[j * X + i] - P[(j - 1) * X + i];
            else if (a.grad_pad == 1) g = (j == 0) ? P[i] : -P[(Y - 1) * X + i];
            const float v = a.vy_out[(size_t)b * nVy + k] - p_mask_y<PY, PX>(a.active, Y, X, je, i) * g;
            a.vy_out[(size_t)b * nVy + k] = v;
            if (a.feat && j < Y) a.feat[((size_t)b * N + k) * 4 + 0] = v * a.fs0;
        } else {
            const int q = k - nVy, j = q / XP, i = q - j * XP, ie = (PX && i == X) ? 0 : i;
            float g = 0.f;
            if (PX) g = P[j * X + ie] - P[j * X + wrapi(ie - 1, X)];
            else if (i >= 1 && i <= X - 1) g = P[j * X + i] - P[j * X + i - 1];
            else if (a.grad_pad == 1) g = (i == 0) ? P[j * X] : -P[j * X + X - 1];
            const float v = a.vx_out[(size_t)b * nVx + q] - p_mask_x<PY, PX>(a.active, Y, X, j, ie) * g;
            a.vx_out[(size_t)b * nVx + q] = v;
            if (a.feat && i < X) {
                float* f = a.feat + ((size_t)b * N + j * X + i) * 4;
                f[1] = v * a.fs1; f[2] = a.re[b] * a.fs2; f[3] = 0.f;
            }
        }
    }
}

PArgs p_args(const sol_karman_cfg* c, const SolLargeStep& io, float* svy, float* svx, float* rhs, const float* p) {
    PArgs a{};
    a.B = c->B; a.Y = c->Y; a.X = c->X; a.dtdx = c->dt / c->dx; a.dt = c->dt; a.adt = c->dt * c->res * c->res;
    a.grad_pad = c->grad_pad; a.inflow_before = c->inflow_before;
    a.d_in = io.d_in; a.vy_in = io.vy_in; a.vx_in = io.vx_in; a.re = io.re; a.active = io.active; a.inflow = io.inflow;
    a.bcv = io.velBCy; a.bcm = io.velBCyMask; a.bc_stride = io.bc_stride;
    a.d_out = io.d_out; a.vy_out = io.vy_out; a.vx_out = io.vx_out; a.svy = svy; a.svx = svx; a.rhs = rhs; a.feat = io.feat_out; a.p = p;
    if (io.feat_scale) { a.fs0 = io.feat_scale[0]; a.fs1 = io.feat_scale[1]; a.fs2 = io.feat_scale[2]; }
    return a;
}

// one launch of KERNEL<PY, PX> for the header's bits (at least one of them set)
#define P_LAUNCH(bits, KERNEL, grid, s, ...)                                                                                      \
    do {                                                                                                                          \
        const int pb_ = (bits) & (SOL_DIRECT_HDR_PERIODIC_Y | SOL_DIRECT_HDR_PERIODIC_X);                                         \
        if (pb_ == SOL_DIRECT_HDR_PERIODIC_Y) SOL_LAUNCH_NAMED(#KERNEL "<y>", (KERNEL<true, false>), grid, dim3(256), 0, s, __VA_ARGS__);       \
        else if (pb_ == SOL_DIRECT_HDR_PERIODIC_X) SOL_LAUNCH_NAMED(#KERNEL "<x>", (KERNEL<false, true>), grid, dim3(256), 0, s, __VA_ARGS__);  \
        else SOL_LAUNCH_NAMED(#KERNEL "<yx>", (KERNEL<true, true>), grid, dim3(256), 0, s, __VA_ARGS__);                           \
    } while (0)

}  // namespace

// ---- the products of the pressure solve with fp64 accumulators -----------------------------------------------------------------------
// A periodic axis has a constant mode that only the OPEN axis holds down: in an x-periodic channel the x-mean of the pressure is fixed by
// the far y ends alone, so |p| grows with (Y / X)^2 against the open box and reaches tens of times |v_x|.  The gradient along x then
// differences the rounding noise of that large, x-independent part: with k_l_gemm's fp32 sums (2.5e-7 of |p|, fine as a solve) v_x after
// the projection misses the float64 reference by 1.1e-5 ... 1.3e-5 at CFL 2.5; with fp64 sums and ONE rounding per stored element the
// solve is at the resolution of its fp32 intermediates (5e-8 ... 8e-8 of |p|).  Same tiling as k_l_gemm: 64 x 64 per workgroup, K in
// slabs of 16 through LDS, operands fp32.  The open scenes keep k_l_gemm and their bits.
namespace {
struct PGArgs {
    const float *A, *Bm;
    float* C;
    int M, N, K, lda, ldb, ldc;
    long sA, sB, sC;
    int accumulate;
};
__global__ void __launch_bounds__(256) k_p_gemm(PGArgs g) {
    __shared__ float As[16][65], Bs[16][65];
    const int b = blockIdx.z, m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const float* A = g.A + (size_t)b * g.sA;
    const float* Bm = g.Bm + (size_t)b * g.sB;
    float* C = g.C + (size_t)b * g.sC;
    double acc[4][4] = {};
    for (int k0 = 0; k0 < g.K; k0 += 16) {
        for (int e = threadIdx.x; e < 64 * 16; e += 256) {
            const int r = e >> 4, kk = e & 15;              // A tile: 64 rows x 16 k
            const int m = m0 + r, k = k0 + kk;
            As[kk][r] = (m < g.M && k < g.K) ? A[(size_t)m * g.lda + k] : 0.f;
            const int kr = e >> 6, c = e & 63;              // B tile: 16 k x 64 cols
            const int kb = k0 + kr, n = n0 + c;
            Bs[kr][c] = (kb < g.K && n < g.N) ? Bm[(size_t)kb * g.ldb + n] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            double av[4], bv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { av[r] = (double)As[kk][ty * 4 + r]; bv[r] = (double)Bs[kk][tx * 4 + r]; }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = fma(av[r], bv[c], acc[r][c]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int m = m0 + ty * 4 + r, n = n0 + tx * 4 + c;
            if (m < g.M && n < g.N) {
                float* dst = &C[(size_t)m * g.ldc + n];
                *dst = g.accumulate ? (float)((double)*dst + acc[r][c]) : (float)acc[r][c];
            }
        }
}
}  // namespace

int sol_periodic_gemm(hipStream_t s, int batch, const float* A, int lda, long sA, const float* Bm, int ldb, long sB, float* C, int ldc, long sC,
                      int M, int N, int K, int accumulate) {
    const PGArgs g{A, Bm, C, M, N, K, lda, ldb, ldc, sA, sB, sC, accumulate};
    SOL_LAUNCH(k_p_gemm, dim3((N + 63) / 64, (M + 63) / 64, batch), dim3(256), 0, s, g);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

int sol_periodic_front(const sol_karman_cfg* c, hipStream_t s, const SolLargeStep& io, float* svy, float* svx, float* rhs) {
    SOL_REQUIRE(io.advection == 0, "periodic boundaries: the mac_cormack advection is not built for periodic scenes; use advection = semi_lagrangian");
    SOL_REQUIRE(io.buoy_y == 0.f && io.buoy_x == 0.f, "periodic boundaries: the buoyancy force is not built for periodic scenes; use a zero force");
    const PArgs a = p_args(c, io, svy, svx, rhs, nullptr);
    const int B = c->B, N = c->Y * c->X, faces = (c->Y + 1) * c->X + c->Y * (c->X + 1);
    P_LAUNCH(io.periodic, k_p_diffuse, dim3((faces + 255) / 256, B), s, a);
    P_LAUNCH(io.periodic, k_p_advect, dim3((faces + N + 255) / 256, B), s, a);
    P_LAUNCH(io.periodic, k_p_div, dim3((N + 255) / 256, B), s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

int sol_periodic_project(const sol_karman_cfg* c, hipStream_t s, const SolLargeStep& io, const float* p) {
    const PArgs a = p_args(c, io, nullptr, nullptr, nullptr, p);
    const int faces = (c->Y + 1) * c->X + c->Y * (c->X + 1);
    P_LAUNCH(io.periodic, k_p_project, dim3((faces + 255) / 256, c->B), s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

// ---- adjoint: the five stages of karman_large_bwd.hip (k_lb_rhs, the solve, k_lb_ga, k_lb_advect_adj, k_lb_diffuse_adj) ----
namespace {

// the cotangent of the step's output at a UNIQUE face, the duplicate plane's folded onto plane 0: one fp32 add, before anything else
template <bool PY> __device__ __forceinline__ float pb_gy(const float* gy, int Y, int X, int j, int i) {
#pragma clang fp contract(off)
    return (PY && j == 0) ? gy[i] + gy[Y * X + i] : gy[j * X + i];
}
template <bool PX> __device__ __forceinline__ float pb_gx(const float* gx, int X, int j, int i) {
#pragma clang fp contract(off)
    return (PX && i == 0) ? gx[j * (X + 1)] + gx[j * (X + 1) + X] : gx[j * (X + 1) + i];
}

template <bool PY, bool PX> __global__ void __launch_bounds__(256) k_pb_rhs(SolPeriodicBwd a) {
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const float* gy = a.goy + (size_t)b * nVy;
    const float* gx = a.gox + (size_t)b * nVx;
    const bool keep = a.grad_pad == 1;           // open axis only: dirichlet0 keeps the boundary faces' gradient, replicate has none
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < N; c += gridDim.x * blockDim.x) {
        const int j = c / X, i = c - j * X;
        auto wy = [&](int jj) {         // jj: j or j + 1
            if (PY) { const int ju = jj == Y ? 0 : jj; return p_mask_y<PY, PX>(a.active, Y, X, ju, i) * pb_gy<PY>(gy, Y, X, ju, i); }
            return (keep || (jj != 0 && jj != Y)) ? p_mask_y<PY, PX>(a.active, Y, X, jj, i) * gy[jj * X + i] : 0.f;
        };
        auto wx = [&](int ii) {
            if (PX) { const int iu = ii == X ? 0 : ii; return p_mask_x<PY, PX>(a.active, Y, X, j, iu) * pb_gx<PX>(gx, X, j, iu); }
            return (keep || (ii != 0 && ii != X)) ? p_mask_x<PY, PX>(a.active, Y, X, j, ii) * gx[j * XP + ii] : 0.f;
        };
        a.rhs[(size_t)b * N + c] = (wy(j) - wy(j + 1)) + (wx(i) - wx(i + 1));
    }
    // side job, as k_lb_rhs: clear slice b of the fixed-point accumulators ([B][nVy] then [B][nVx], contiguous) and the absmax slots
    const size_t faces = (size_t)nVy + nVx;
    long long* zy = a.gcy + (size_t)b * nVy;
    long long* zx = a.gcx + (size_t)b * nVx;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < faces; e += (size_t)gridDim.x * blockDim.x) {
        if (e < (size_t)nVy) zy[e] = 0ll;
        else zx[e - nVy] = 0ll;
    }
    if (blockIdx.x == 0 && threadIdx.x < FX_SLOTS) a.gmax[b * FX_SLOTS + threadIdx.x] = 0u;
}

template <bool PY, bool PX> __global__ void __launch_bounds__(256) k_pb_ga(SolPeriodicBwd a) {
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const float* P = a.gdiv + (size_t)b * N;
    const float* gy = a.goy + (size_t)b * nVy;
    const float* gx = a.gox + (size_t)b * nVx;
    // the pressure cotangent of a cell: wrapped on a periodic axis, zero outside an open one
    auto cell = [&](int j, int i) {
        const int jj = PY ? wrapi(j, Y) : j, ii = PX ? wrapi(i, X) : i;
        return ((unsigned)jj < (unsigned)Y && (unsigned)ii < (unsigned)X) ? P[jj * X + ii] : 0.f;
    };
    float vmax = 0.f;
    bool bad = false;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nVy + nVx; k += gridDim.x * blockDim.x) {
        float v;
        if (k < nVy) {
            const int j = k / X, i = k - j * X;
            v = (PY && j == Y) ? 0.f : p_mask_y<PY, PX>(a.active, Y, X, j, i) * (pb_gy<PY>(gy, Y, X, j, i) + cell(j - 1, i) - cell(j, i));
            a.gay[(size_t)b * nVy + k] = v;
        } else {
            const int q = k - nVy, j = q / XP, i = q - j * XP;
            v = (PX && i == X) ? 0.f : p_mask_x<PY, PX>(a.active, Y, X, j, i) * (pb_gx<PX>(gx, X, j, i) + cell(j, i - 1) - cell(j, i));
            a.gax[(size_t)b * nVx + q] = v;
        }
        vmax = fmaxf(vmax, fabsf(v));
        bad |= !(fabsf(v) <= 3.402823466e38f);
    }
    fx_publish_max(a.gmax + b * FX_SLOTS, vmax, bad);
}

struct PGAdd {
    long long *gy, *gx;
    float qs;
    int X;
    __device__ __forceinline__ void operator()(int comp, int jj, int ii, float v) const {
        fx_add(comp == 0 ? gy + jj * X + ii : gx + jj * (X + 1) + ii, v, qs);
    }
};

// adjoint of one advected UNIQUE face of component C at (j, i), gs = g_a there: k_p_advect's expressions, operation for operation, so
// floorf, the modulo and the clamps decide as they did; every target is a unique face.  No fused multiply-adds (as lb_advect_adj_point).
template <int C, bool PY, bool PX>
__device__ __forceinline__ void pb_advect_adj_point(const SolPeriodicBwd& a, const float* sy, const float* sx, const PGAdd& add, int j, int i, float gs) {
#pragma clang fp contract(off)
    const int Y = a.Y, X = a.X, XP = X + 1;
    float uy, ux;
    int ja = 0, jb = 0, ia = 0, ib = 0, j1 = 0, i1 = 0;
    if (C == 0) {
        ja = PY ? wrapi(j - 1, Y) : max(j - 1, 0); jb = PY ? j : min(j, Y - 1); i1 = nxt<PX>(i, X);
        uy = sy[j * X + i];
        ux = 0.25f * (sx[ja * XP + i] + sx[ja * XP + i1] + sx[jb * XP + i] + sx[jb * XP + i1]);
    } else {
        ia = PX ? wrapi(i - 1, X) : max(i - 1, 0); ib = PX ? i : min(i, X - 1); j1 = nxt<PY>(j, Y);
        ux = sx[j * XP + i];
        uy = 0.25f * (sy[j * X + ia] + sy[j * X + ib] + sy[j1 * X + ia] + sy[j1 * X + ib]);
    }
    const int W = X + (C == 1);
    const float* f = C == 0 ? sy : sx;
    const PBil s = p_bil<C, PY, PX>(Y, X, j, -uy * a.dtdx, i, -ux * a.dtdx);
    float dy = 0.f, dx = 0.f;                    // d(sample) / d(offset) along each axis
#pragma unroll
    for (int cj = 0; cj < 2; ++cj)
#pragma unroll
        for (int ci = 0; ci < 2; ++ci) {
            const int jj = cj ? s.j1 : s.j0, ii = ci ? s.i1 : s.i0;
            const float by = cj ? s.wy : 1.f - s.wy, bx = ci ? s.wx : 1.f - s.wx;
            const float v = f[jj * W + ii];
            add(C, jj, ii, by * bx * gs);                   // field term
            dy += (cj ? 1.f : -1.f) * bx * v;
            dx += by * (ci ? 1.f : -1.f) * v;
        }
    // back-trace term: offset = -dtdx * u(x0), onto the velocity samples that formed u
    const float guy = -a.dtdx * gs * dy, gux = -a.dtdx * gs * dx;
    if (C == 0) {
        add(0, j, i, guy);
        const float qx = 0.25f * gux;
        add(1, ja, i, qx); add(1, ja, i1, qx); add(1, jb, i, qx); add(1, jb, i1, qx);
    } else {
        add(1, j, i, gux);
        const float qy = 0.25f * guy;
        add(0, j, ia, qy); add(0, j, ib, qy); add(0, j1, ia, qy); add(0, j1, ib, qy);
    }
}

template <bool PY, bool PX> __global__ void __launch_bounds__(256) k_pb_advect_adj(SolPeriodicBwd a) {
    const int Y = a.Y, X = a.X, XP = X + 1, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const float* sy = a.svy + (size_t)b * nVy;
    const float* sx = a.svx + (size_t)b * nVx;
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    const PGAdd add{a.gcy + (size_t)b * nVy, a.gcx + (size_t)b * nVx, qs, X};
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nVy + nVx; k += gridDim.x * blockDim.x) {
        if (k < nVy) {
            const int j = k / X, i = k - j * X;
            const float g = a.gay[(size_t)b * nVy + k];         // zero on a duplicate plane (k_pb_ga)
            if (g != 0.f && !(PY && j == Y)) pb_advect_adj_point<0, PY, PX>(a, sy, sx, add, j, i, g);
        } else {
            const int q = k - nVy, j = q / XP, i = q - j * XP;
            const float g = a.gax[(size_t)b * nVx + q];
            if (g != 0.f && !(PX && i == X)) pb_advect_adj_point<1, PY, PX>(a, sy, sx, add, j, i, g);
        }
    }
}

// g_in = (I + alpha L^T) g', g' = g_c . (1 - bcm) on v_y: lapT's gather (fixed_scatter.hpp) and its order of additions -- axis 0 +, axis 0 -,
// axis 1 +, axis 1 - -- with the wrapped neighbour on a periodic axis (L is symmetric there) and the replicate rule on an open one; the
// last step is k_lb_diffuse_adj's fma(alpha, lapT, round(g')).  A duplicate plane of the input gradient is exactly zero.
template <bool PY, bool PX> __global__ void __launch_bounds__(256) k_pb_diffuse_adj(SolPeriodicBwd a) {
    const int Y = a.Y, X = a.X, XP = X + 1, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const float alpha = a.adt / a.re[b];
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nVy + nVx; e += gridDim.x * blockDim.x) {
        if (e < nVy) {
            const int j = e / X, i = e - j * X;
            float out = 0.f;
            if (!(PY && j == Y)) {
                const long long* g = a.gcy + (size_t)b * nVy;
                const float* m = a.bcm + (size_t)b * a.bc_stride;
                auto at = [&](int q) { return fx_get(g, q, qi) * (1.f - m[q]); };
                const float v = fx_get(g, e, qi) * (1.f - m[e]);
                float acc = -4.f * v;
                acc += PY ? at(nxt<true>(j, Y) * X + i) : (j + 1 < Y + 1 ? at(e + X) : v);
                acc += PY ? at(wrapi(j - 1, Y) * X + i) : (j > 0 ? at(e - X) : v);
                acc += PX ? at(j * X + nxt<true>(i, X)) : (i + 1 < X ? at(e + 1) : v);
                acc += PX ? at(j * X + wrapi(i - 1, X)) : (i > 0 ? at(e - 1) : v);
                out = __fmaf_rn(alpha, acc, v);
            }
            a.giy[(size_t)b * nVy + e] = out;
        } else {
            const int q = e - nVy, j = q / XP, i = q - j * XP;
            float out = 0.f;
            if (!(PX && i == X)) {
                const long long* g = a.gcx + (size_t)b * nVx;
                auto at = [&](int t) { return fx_get(g, t, qi); };
                const float v = fx_get(g, q, qi);
                float acc = -4.f * v;
                acc += PY ? at(nxt<true>(j, Y) * XP + i) : (j + 1 < Y ? at(q + XP) : v);
                acc += PY ? at(wrapi(j - 1, Y) * XP + i) : (j > 0 ? at(q - XP) : v);
                acc += PX ? at(j * XP + nxt<true>(i, X)) : (i + 1 < XP ? at(q + 1) : v);
                acc += PX ? at(j * XP + wrapi(i - 1, X)) : (i > 0 ? at(q - 1) : v);
                out = __fmaf_rn(alpha, acc, v);
            }
            a.gix[(size_t)b * nVx + q] = out;
        }
    }
}

// ---- the seam of a field the step did not write (the trainer's correction launch leaves the duplicate plane stale) ----
// sync: duplicate plane = plane 0.  fold (its adjoint): g[plane 0] += g[duplicate], then g[duplicate] = 0.  One thread per seam face.
template <bool FOLD> __global__ void __launch_bounds__(256) k_p_seam(float* __restrict__ vy, float* __restrict__ vx, int B, int Y, int X, int bits) {
    const int nY = (bits & SOL_DIRECT_HDR_PERIODIC_Y) ? X : 0, nX = (bits & SOL_DIRECT_HDR_PERIODIC_X) ? Y : 0, per = nY + nX;
    const size_t n = (size_t)B * per;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const size_t b = e / per;
        const int t = (int)(e - b * per);
        float *lo, *hi;
        if (t < nY) { lo = vy + b * (size_t)(Y + 1) * X + t; hi = lo + (size_t)Y * X; }
        else { lo = vx + b * (size_t)Y * (X + 1) + (size_t)(t - nY) * (X + 1); hi = lo + X; }
        if (FOLD) {
#pragma clang fp contract(off)
            *lo = *lo + *hi;
            *hi = 0.f;
        } else {
            *hi = *lo;
        }
    }
}

int seam(const char* who, bool fold, void* stream, float* vy, float* vx, int32_t B, int32_t Y, int32_t X, int32_t bits) {
    SOL_REQUIRE(vy && vx, "%s: NULL pointer argument", who);
    SOL_REQUIRE(B >= 1 && Y >= 1 && X >= 1, "%s: B, Y, X >= 1 (got %d, %d, %d)", who, B, Y, X);
    SOL_REQUIRE((bits & ~(SOL_DIRECT_HDR_PERIODIC_Y | SOL_DIRECT_HDR_PERIODIC_X)) == 0, "%s: periodic_bits must be a combination of 2 (y periodic) "
                "and 4 (x periodic), got %d", who, bits);
    if (bits == 0) return SOL_OK;          // an open scene has no seam: nothing is launched
    const size_t n = (size_t)B * (((bits & SOL_DIRECT_HDR_PERIODIC_Y) ? X : 0) + ((bits & SOL_DIRECT_HDR_PERIODIC_X) ? Y : 0)), nb = (n + 255) / 256;
    const dim3 grid((unsigned)(nb < 1024 ? nb : 1024));
    if (fold) SOL_LAUNCH_NAMED("k_p_seam<fold>", (k_p_seam<true>), grid, dim3(256), 0, (hipStream_t)stream, vy, vx, B, Y, X, bits);
    else SOL_LAUNCH_NAMED("k_p_seam<sync>", (k_p_seam<false>), grid, dim3(256), 0, (hipStream_t)stream, vy, vx, B, Y, X, bits);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

}  // namespace

int sol_periodic_bwd_rhs(hipStream_t s, const SolPeriodicBwd& a) {
    P_LAUNCH(a.periodic, k_pb_rhs, dim3((unsigned)((a.Y * a.X + 255) / 256), a.B), s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

int sol_periodic_bwd_tail(hipStream_t s, const SolPeriodicBwd& a) {
    const unsigned gF = (unsigned)(((a.Y + 1) * a.X + a.Y * (a.X + 1) + 255) / 256);
    P_LAUNCH(a.periodic, k_pb_ga, dim3(gF, a.B), s, a);
    P_LAUNCH(a.periodic, k_pb_advect_adj, dim3(gF, a.B), s, a);
    P_LAUNCH(a.periodic, k_pb_diffuse_adj, dim3(gF, a.B), s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

extern "C" int sol_karman_seam_sync(void* stream, float* vy, float* vx, int32_t B, int32_t Y, int32_t X, int32_t periodic_bits) {
    return seam("sol_karman_seam_sync", false, stream, vy, vx, B, Y, X, periodic_bits);
}

extern "C" int sol_karman_seam_fold(void* stream, float* g_vy, float* g_vx, int32_t B, int32_t Y, int32_t X, int32_t periodic_bits) {
    return seam("sol_karman_seam_fold", true, stream, g_vy, g_vx, B, Y, X, periodic_bits);
}
