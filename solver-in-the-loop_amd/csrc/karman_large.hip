// Forward solver step for grids that do not fit one workgroup's LDS (the reference's data generation runs
// KarmanFlow.step at 256 x 128: /root/reference/karman-2d/karman.py:98-159, Makefile:19-28 `-r 128`).
//
// Same arithmetic as k_karman_fwd (csrc/karman_step.hip), decomposed into chip-wide launches on global memory
// (the whole state of a batch is a few MB, L2 resident):
//   k_l_diffuse   explicit diffusion (replicate padding, dx = 1) + velocity BC              -> sv_y, sv_x
//   k_l_advect    semi-Lagrangian advection of v_y, v_x (clamped) and density (zero ghost ring) + inflow,
//                 hard-BC face masks                                                           -> v_out (pre-projection), d_out
//   k_l_div       rhs = -div
//   pressure      DIRECT solve: x = G (b - U_S E_SS x_S) with the sine-transform diagonalisation of the rectangle and
//                 the capacitance correction of the obstacle (precond.direct_solver_blob, window 16/32/64): eight small
//                 fp32 GEMMs (k_l_gemm) + gather / K' / scatter kernels; or, for obstacles beyond one window, the SCATTERED form of the
//                 same correction on the support set's row and column lists (precond.scattered_solver_blob, magic "FDS1": scattered_solve,
//                 k_l_capacitance_sc) -- sol_large_direct_check / _solve dispatch on the blob's magic word
//   k_l_project   v -= mask * grad p  (+ fused to_feature)
// and, for a roll-out with the trained corrector (trainer.LargeGridRollout), the correction launch after the network:
//   k_l_correct   v_y, v_x += out_std * to_staggered(network output)  (+ the applied correction as a field of its own)
// The adjoint of this path lives in karman_large_bwd.hip; it reads the post-diffusion velocity (sv_y, sv_x) that
// sol_karman_step_fwd_large_saved hands out and runs the same pressure solve (pressure_solve_any2d, pcg.hip).
// The host side of the step -- its six entry points, their checks and their workspace -- is large_fwd in pcg.hip.
#include "large2d.hpp"

namespace {

constexpr int FDL_HEADER = 16;

struct LArgs {
    int B, Y, X;
    float dtdx, dt, adt;
    int grad_pad, inflow_before;
    const float *d_in, *vy_in, *vx_in, *re, *active, *inflow, *bcv, *bcm;
    long bc_stride;
    float *d_out, *vy_out, *vx_out, *svy, *svx, *rhs, *feat;
    const float* p;
    float fs0, fs1, fs2;
};

__global__ void k_l_diffuse(LArgs a) {
    const int Y = a.Y, X = a.X, XP = X + 1, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const float alpha = a.adt / a.re[b];
    const float* vy = a.vy_in + (size_t)b * nVy;
    const float* vx = a.vx_in + (size_t)b * nVx;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nVy + nVx; k += gridDim.x * blockDim.x) {
        if (k < nVy) {
            const int j = k / X, i = k - j * X;
            const float c = vy[k];
            const float lap = vy[min(j + 1, Y) * X + i] + vy[max(j - 1, 0) * X + i] + vy[j * X + min(i + 1, X - 1)] + vy[j * X + max(i - 1, 0)] - 4.f * c;
            float v = c + alpha * lap;
            v = v * (1.f - a.bcm[(size_t)b * a.bc_stride + k]) + a.bcv[(size_t)b * a.bc_stride + k];
            a.svy[(size_t)b * nVy + k] = v;
        } else {
            const int q = k - nVy, j = q / XP, i = q - j * XP;
            const float c = vx[q];
            const float lap = vx[min(j + 1, Y - 1) * XP + i] + vx[max(j - 1, 0) * XP + i] + vx[j * XP + min(i + 1, X)] + vx[j * XP + max(i - 1, 0)] - 4.f * c;
            a.svx[(size_t)b * nVx + q] = c + alpha * lap;
        }
    }
}

struct Bil { int j0, j1, i0, i1; float wy, wx; };
__device__ __forceinline__ Bil bil_clamp(int H, int W, int jb, float oy, int ib, float ox) {
    Bil s;
    const float fy = floorf(oy), fx = floorf(ox);
    s.wy = oy - fy; s.wx = ox - fx;
    const int j0 = jb + (int)fy, i0 = ib + (int)fx;
    s.j0 = clampi(j0, 0, H - 1); s.j1 = clampi(j0 + 1, 0, H - 1);
    s.i0 = clampi(i0, 0, W - 1); s.i1 = clampi(i0 + 1, 0, W - 1);
    return s;
}
__device__ __forceinline__ float bil_eval(const float* f, int W, const Bil& s) {
    const float f00 = f[s.j0 * W + s.i0], f01 = f[s.j0 * W + s.i1], f10 = f[s.j1 * W + s.i0], f11 = f[s.j1 * W + s.i1];
    return (1.f - s.wy) * ((1.f - s.wx) * f00 + s.wx * f01) + s.wy * ((1.f - s.wx) * f10 + s.wx * f11);
}

__global__ void k_l_advect(LArgs a) {
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const float* sy = a.svy + (size_t)b * nVy;
    const float* sx = a.svx + (size_t)b * nVx;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nVy + nVx + N; k += gridDim.x * blockDim.x) {
        if (k < nVy) {
            const int j = k / X, i = k - j * X;
            const float uy = sy[k];
            const int ja = max(j - 1, 0), jb = min(j, Y - 1);
            const float ux = 0.25f * (sx[ja * XP + i] + sx[ja * XP + i + 1] + sx[jb * XP + i] + sx[jb * XP + i + 1]);
            const Bil s = bil_clamp(Y + 1, X, j, -uy * a.dtdx, i, -ux * a.dtdx);
            a.vy_out[(size_t)b * nVy + k] = bil_eval(sy, X, s) * mask_y(a.active, Y, X, j, i);
        } else if (k < nVy + nVx) {
            const int q = k - nVy, j = q / XP, i = q - j * XP;
            const float ux = sx[q];
            const int ia = max(i - 1, 0), ib = min(i, X - 1);
            const float uy = 0.25f * (sy[j * X + ia] + sy[j * X + ib] + sy[(j + 1) * X + ia] + sy[(j + 1) * X + ib]);
            const Bil s = bil_clamp(Y, XP, j, -uy * a.dtdx, i, -ux * a.dtdx);
            a.vx_out[(size_t)b * nVx + q] = bil_eval(sx, XP, s) * mask_x(a.active, Y, X, j, i);
        } else if (a.d_out) {
            const int c = k - nVy - nVx, j = c / X, i = c - j * X;
            const float* gd = a.d_in + (size_t)b * N;
            const float uy = 0.5f * (sy[c] + sy[c + X]);
            const float ux = 0.5f * (sx[j * XP + i] + sx[j * XP + i + 1]);
            const float oy = -uy * a.dtdx, ox = -ux * a.dtdx;
            const float fy = floorf(oy), fx = floorf(ox);
            const float wy = oy - fy, wx = ox - fx;
            const int j0 = j + (int)fy, i0 = i + (int)fx;
            float f[2][2];
            for (int dj = 0; dj < 2; ++dj)
                for (int di = 0; di < 2; ++di) {
                    const int jj = j0 + dj, ii = i0 + di;
                    float v = 0.f;   // extrapolation 'constant': one ring of zero ghost cells
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

__global__ void k_l_div(LArgs a) {
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const float* vy = a.vy_out + (size_t)b * nVy;
    const float* vx = a.vx_out + (size_t)b * nVx;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < N; c += gridDim.x * blockDim.x) {
        const int j = c / X, i = c - j * X;
        const float div = (vy[(j + 1) * X + i] - vy[j * X + i]) + (vx[j * XP + i + 1] - vx[j * XP + i]);
        a.rhs[(size_t)b * N + c] = -div;        // M p = -div  <=>  A p = div
    }
}

__global__ void k_l_project(LArgs a) {
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const float* P = a.p + (size_t)b * N;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nVy + nVx; k += gridDim.x * blockDim.x) {
        if (k < nVy) {
            const int j = k / X, i = k - j * X;
            float g = 0.f;
            if (j >= 1 && j <= Y - 1) g = P[j * X + i] - P[(j - 1) * X + i];
            else if (a.grad_pad == 1) g = (j == 0) ? P[i] : -P[(Y - 1) * X + i];
            const float v = a.vy_out[(size_t)b * nVy + k] - mask_y(a.active, Y, X, j, i) * g;
            a.vy_out[(size_t)b * nVy + k] = v;
            if (a.feat && j < Y) a.feat[((size_t)b * N + k) * 4 + 0] = v * a.fs0;
        } else {
            const int q = k - nVy, j = q / XP, i = q - j * XP;
            float g = 0.f;
            if (i >= 1 && i <= X - 1) g = P[j * X + i] - P[j * X + i - 1];
            else if (a.grad_pad == 1) g = (i == 0) ? P[j * X] : -P[j * X + X - 1];
            const float v = a.vx_out[(size_t)b * nVx + q] - mask_x(a.active, Y, X, j, i) * g;
            a.vx_out[(size_t)b * nVx + q] = v;
            if (a.feat && i < X) {
                float* f = a.feat + ((size_t)b * N + j * X + i) * 4;
                f[1] = v * a.fs1; f[2] = a.re[b] * a.fs2; f[3] = 0.f;
            }
        }
    }
}

// velocity += s * to_staggered(out) (karman_train.py:88-90, 424-426), both components in one launch: a thread takes one pixel, reads its
// two channels as one 8-byte load and adds them to the pixel's low y face and low x face -- consecutive lanes store consecutive
// addresses in both components; the high row of v_y and the high column of v_x have no pixel and stay as they are.  cor_y / cor_x
// (both or neither): the applied correction [B,Y+1,X] / [B,Y,X+1], zero on that row and column.  The result is fl(v + fl(s * o)).
__global__ void __launch_bounds__(256) k_l_correct(const float2* __restrict__ out, float* __restrict__ vy, float* __restrict__ vx,
                                                   float* __restrict__ cor_y, float* __restrict__ cor_x, size_t n, int Y, int X, float s0, float s1) {
    const size_t N = (size_t)Y * X;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const float2 o = out[e];
        const size_t b = e / N;
        const int c = (int)(e - b * N), j = c / X, i = c - j * X;
        const size_t ky = b * (N + X) + c, kx = b * (N + Y) + (size_t)j * (X + 1) + i;
        float cy, cx, ny, nx;
        {
#pragma clang fp contract(off)
            cy = s0 * o.x; cx = s1 * o.y;
            ny = vy[ky] + cy; nx = vx[kx] + cx;
        }
        vy[ky] = ny;
        vx[kx] = nx;
        if (cor_y) {
            cor_y[ky] = cy;
            cor_x[kx] = cx;
            if (j == Y - 1) cor_y[ky + X] = 0.f;
            if (i == X - 1) cor_x[kx + 1] = 0.f;
        }
    }
}

// ---- small fp32 GEMM: C[b] (M x N) = (accumulate ? C[b] : 0) + scale (.) (A[b] (M x K) * B[b] (K x N)) ----------
// row-major with leading dimensions; batch strides may be 0 (shared operand); `scale` (M x N, ld = lds) optional.
// 64 x 64 tile per workgroup, 16 x 16 threads x (4 x 4) outputs, K in slabs of 16 through LDS.
struct GArgs {
    const float *A, *Bm, *scale;
    float* C;
    int M, N, K, lda, ldb, ldc, lds;
    long sA, sB, sC;
    int accumulate;
    const int* skip;        // per-simulation done words [batch] (the CG solve's preconditioner) or NULL
};
__global__ void __launch_bounds__(256) k_l_gemm(GArgs g) {
    __shared__ float As[16][65], Bs[16][65];
    const int b = blockIdx.z, m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    if (g.skip && g.skip[b]) return;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const float* A = g.A + (size_t)b * g.sA;
    const float* Bm = g.Bm + (size_t)b * g.sB;
    float* C = g.C + (size_t)b * g.sC;
    float acc[4][4] = {};
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
            float av[4], bv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { av[r] = As[kk][ty * 4 + r]; bv[r] = Bs[kk][tx * 4 + r]; }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] += av[r] * bv[c];
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int m = m0 + ty * 4 + r, n = n0 + tx * 4 + c;
            if (m < g.M && n < g.N) {
                float v = acc[r][c];
                if (g.scale) v *= g.scale[(size_t)m * g.lds + n];
                float* dst = &C[(size_t)m * g.ldc + n];
                *dst = g.accumulate ? *dst + v : v;
            }
        }
}

// T[m][c] = (add ? T[m][c] + add[m][c] * il : T[m][c] * il) with il = ilT[c][m] (1 / eigenvalue, stored transposed in the blob)
__global__ void k_l_scale(float* __restrict__ T, const float* __restrict__ add, const float* __restrict__ ilT, int Y, int X,
                          const int* __restrict__ skip) {
    const int b = blockIdx.y;
    if (skip && skip[b]) return;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < Y * X; e += gridDim.x * blockDim.x) {
        const int m = e / X, c = e - m * X;
        const float il = ilT[(size_t)c * Y + m];
        float* t = T + (size_t)b * Y * X + e;
        *t = add ? *t + add[(size_t)b * Y * X + e] * il : *t * il;
    }
}

// capacitance correction on the window values: xs = x0w[sidx], c = K' xs (KpT stored transposed), W2[sidx] = -c
__global__ void k_l_capacitance(const float* __restrict__ x0w, const float* __restrict__ KpT, const int* __restrict__ sidx,
                                float* __restrict__ W2, int SP, int win) {
    extern __shared__ float xs[];
    const int b = blockIdx.x;
    const float* xw = x0w + (size_t)b * 64 * 64;      // per-simulation stride of the window scratch (host carve)
    float* w2 = W2 + (size_t)b * 64 * 64;
    for (int t = threadIdx.x; t < SP; t += blockDim.x) { const int si = sidx[t]; xs[t] = si >= 0 ? xw[si] : 0.f; }
    for (int t = threadIdx.x; t < win * win; t += blockDim.x) w2[t] = 0.f;
    __syncthreads();
    for (int s = threadIdx.x; s < SP; s += blockDim.x) {
        const int si = sidx[s];
        if (si < 0) continue;
        float c = 0.f;
        for (int q = 0; q < SP; ++q) c += KpT[(size_t)q * SP + s] * xs[q];
        w2[si] = -c;
    }
}

// ---- scattered direct solve (precond.scattered_solver_blob): the capacitance product for support sets of a thousand cells and more ----
// c = K' xs with xs gathered from X0 [RP][CP], W2[sidx] = -c.  grid = (SP / 64, B): a workgroup owns 64 rows of K' (= 64 columns of the
// stored K'^T) and walks all SP entries of xs (staged in LDS).  Lane = (q phase 0..3, four consecutive columns): a wave reads four rows
// of K'^T per step as 16-byte loads (16 lanes x 16 B = 256 contiguous bytes per row), wave w takes the fixed q range [w, w + 1) * SP / 4.
// The sixteen partials per column (4 waves x 4 phases) are added in a fixed order through LDS: no atomics, the same bits on every call.
// A matrix-vector product has one right-hand side per simulation: nothing for the matrix cores to tile, the kernel is a streaming read
// of K' (5.9 MB at SP = 1216) spread over SP / 64 x B compute units.
constexpr int SC_TILE = 64;          // columns of K'^T per workgroup
constexpr int SC_MAXSP = 4096;       // precond.FDS_MAX_SUPPORT
__global__ void __launch_bounds__(256) k_l_capacitance_sc(const float* __restrict__ X0, const float* __restrict__ KpT, const int* __restrict__ sidx,
                                                          float* __restrict__ W2, int SP, int nW) {
    __shared__ float xs[SC_MAXSP];
    __shared__ float part[16][SC_TILE];
    const int b = blockIdx.y, s0 = blockIdx.x * SC_TILE;
    const float* x0 = X0 + (size_t)b * nW;
    for (int t = threadIdx.x; t < SP; t += 256) {
        const int si = sidx[t];
        xs[t] = (si >= 0 && si < nW) ? x0[si] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = (lane & 15) * 4, ph = lane >> 4;
    const int q0 = wave * (SP >> 2), q1 = q0 + (SP >> 2);            // SP % 64 == 0: a multiple of 16 rows per wave
    const float* k = KpT + (size_t)s0 + col;
    float4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int q = q0 + ph; q < q1; q += 4) {
        const float4 kv = *reinterpret_cast<const float4*>(k + (size_t)q * SP);
        const float x = xs[q];
        acc.x += kv.x * x; acc.y += kv.y * x; acc.z += kv.z * x; acc.w += kv.w * x;
    }
    *reinterpret_cast<float4*>(&part[wave * 4 + ph][col]) = acc;
    __syncthreads();
    if (threadIdx.x < SC_TILE) {
        const int si = sidx[s0 + threadIdx.x];
        if (si >= 0 && si < nW) {
            float c = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) c += part[r][threadIdx.x];
            W2[(size_t)b * nW + si] = -c;
        }
    }
}

__global__ void __launch_bounds__(256) k_l_copy(float* __restrict__ dst, const float* __restrict__ src, size_t n) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) dst[e] = src[e];
}
__global__ void __launch_bounds__(256) k_l_zero(float* __restrict__ p, size_t n) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) p[e] = 0.f;
}

constexpr int FDL_MAGIC = 0x46443032;      // "FD02": precond.direct_solver_blob (one window)
constexpr int FDS_MAGIC = 0x46445331;      // "FDS1": precond.scattered_solver_blob (row list x column list)
struct HeaderSc { int Y, X, nR, nC, nS, SP, RP, CP; };
inline HeaderSc header_sc(const int32_t* hdr) { return HeaderSc{hdr[1], hdr[2], hdr[3], hdr[4], hdr[5], hdr[6], hdr[7], hdr[8]}; }

struct Header { int Y, X, wy0, wx0, nS, SP, win; };

int gemm(hipStream_t s, int batch, const float* A, int lda, long sA, const float* Bm, int ldb, long sB, float* C, int ldc, long sC,
         int M, int N, int K, int accumulate, const int* skip = nullptr, bool wide = false) {
    // periodic scenes: the same product with fp64 accumulators (karman_periodic.hip says why); never with a CG solve's done words
    if (wide) return sol_periodic_gemm(s, batch, A, lda, sA, Bm, ldb, sB, C, ldc, sC, M, N, K, accumulate);
    GArgs g{A, Bm, nullptr, C, M, N, K, lda, ldb, ldc, 0, sA, sB, sC, accumulate, skip};
    SOL_LAUNCH(k_l_gemm, dim3((N + 63) / 64, (M + 63) / 64, batch), dim3(256), 0, s, g);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

LArgs large_args(const sol_karman_cfg* c, const SolLargeStep& io, float* svy, float* svx, float* rhs, const float* p) {
    LArgs a{};
    a.B = c->B; a.Y = c->Y; a.X = c->X; a.dtdx = c->dt / c->dx; a.dt = c->dt; a.adt = c->dt * c->res * c->res;
    a.grad_pad = c->grad_pad; a.inflow_before = c->inflow_before;
    a.d_in = io.d_in; a.vy_in = io.vy_in; a.vx_in = io.vx_in; a.re = io.re; a.active = io.active; a.inflow = io.inflow;
    a.bcv = io.velBCy; a.bcm = io.velBCyMask; a.bc_stride = io.bc_stride;
    a.d_out = io.d_out; a.vy_out = io.vy_out; a.vx_out = io.vx_out; a.svy = svy; a.svx = svx; a.rhs = rhs; a.feat = io.feat_out; a.p = p;
    if (io.feat_scale) { a.fs0 = io.feat_scale[0]; a.fs1 = io.feat_scale[1]; a.fs2 = io.feat_scale[2]; }
    return a;
}

}  // namespace

// shared with karman3d.hip (the sine transforms of the 3-D direct solve are batched products of this kind)
int sol_gemm_f32(hipStream_t s, int batch, const float* A, int lda, long sA, const float* Bm, int ldb, long sB, float* C, int ldc, long sC,
                 int M, int N, int K, int accumulate) {
    return gemm(s, batch, A, lda, sA, Bm, ldb, sB, C, ldc, sC, M, N, K, accumulate);
}

// ---- the stencil phases around the pressure solve (shared with pcg.hip) ----
int sol_large_front(const sol_karman_cfg* c, hipStream_t s, const SolLargeStep& io, float* svy, float* svx, float* rhs) {
    if (io.periodic) return sol_periodic_front(c, s, io, svy, svx, rhs);      // wrapped indices: karman_periodic.hip
    const LArgs a = large_args(c, io, svy, svx, rhs, nullptr);
    const int B = c->B, N = c->Y * c->X, faces = (c->Y + 1) * c->X + c->Y * (c->X + 1);
    SOL_LAUNCH(k_l_diffuse, dim3((faces + 255) / 256, B), dim3(256), 0, s, a);
    if (io.advection == 0) SOL_LAUNCH(k_l_advect, dim3((faces + N + 255) / 256, B), dim3(256), 0, s, a);
    else if (int e = sol_mc_advect(c, s, io.mc_strength, io.d_in, svy, svx, io.active, io.inflow, io.d_out, io.vy_out, io.vx_out, io.mc_ws)) return e;
    // buoyancy (optional; io.buoy = dt F): the step's output density pushes the advected velocity (karman_buoyancy.hip)
    SOL_REQUIRE((io.buoy_y == 0.f && io.buoy_x == 0.f) || (io.d_in && io.inflow && io.d_out), "a buoyancy force needs the density: d_in, inflow and d_out");
    if (int e = sol_buoyancy_add(s, B, c->Y, c->X, io.active, io.d_out, io.buoy_y, io.buoy_x, io.vy_out, io.vx_out)) return e;
    SOL_LAUNCH(k_l_div, dim3((N + 255) / 256, B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

// k_l_advect alone on a given post-diffusion velocity (sol_karman_advect with advection = 0, karman_maccormack.hip)
int sol_large_advect(const sol_karman_cfg* c, hipStream_t s, const float* d_in, const float* svy, const float* svx, const float* active,
                     const float* inflow, float* d_out, float* vy_out, float* vx_out) {
    SolLargeStep io{};
    io.d_in = d_in; io.active = active; io.inflow = inflow; io.d_out = d_out; io.vy_out = vy_out; io.vx_out = vx_out;
    const LArgs a = large_args(c, io, const_cast<float*>(svy), const_cast<float*>(svx), nullptr, nullptr);
    const int items = (c->Y + 1) * c->X + c->Y * (c->X + 1) + c->Y * c->X;
    SOL_LAUNCH(k_l_advect, dim3((items + 255) / 256, c->B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

int sol_large_project(const sol_karman_cfg* c, hipStream_t s, const SolLargeStep& io, const float* p) {
    if (io.periodic) return sol_periodic_project(c, s, io, p);
    const LArgs a = large_args(c, io, nullptr, nullptr, nullptr, p);
    const int faces = (c->Y + 1) * c->X + c->Y * (c->X + 1);
    SOL_LAUNCH(k_l_project, dim3((faces + 255) / 256, c->B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

// ---- the empty-box solve G = M_r^-1 (sine-transform diagonalisation of the rectangle), in two halves: the direct solve adds its
// capacitance correction to the spectral coefficients T2 in between, the CG solve applies both halves back to back.  All matrices
// row-major [Y][X] per simulation; Qy, Qx symmetric.  blob: the sections after the header (Qy, Qx, 1/lam transposed)
int sol_large_box_forward(hipStream_t s, int B, int Y, int X, const float* blob, const float* src, float* T1, float* T2, const int* skip, bool wide) {
    const float* Qy = blob + FDL_HEADER;
    const float* Qx = Qy + (size_t)Y * Y;
    const float* ilT = Qx + (size_t)X * X;             // [X][Y]
    const long sN = (long)Y * X;
    // T1 = Qy src ;  T2 = (T1 Qx) / lam
    if (int e = gemm(s, B, Qy, Y, 0, src, X, sN, T1, X, sN, Y, X, Y, 0, skip, wide)) return e;
    if (int e = gemm(s, B, T1, X, sN, Qx, X, 0, T2, X, sN, Y, X, X, 0, skip, wide)) return e;
    SOL_LAUNCH(k_l_scale, dim3((Y * X + 255) / 256, B), dim3(256), 0, s, T2, (const float*)nullptr, ilT, Y, X, skip);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

int sol_large_box_back(hipStream_t s, int B, int Y, int X, const float* blob, const float* T2, float* T1, float* dst, const int* skip, bool wide) {
    const float* Qy = blob + FDL_HEADER;
    const float* Qx = Qy + (size_t)Y * Y;
    const long sN = (long)Y * X;
    // dst = Qy (T2 Qx)
    if (int e = gemm(s, B, T2, X, sN, Qx, X, 0, T1, X, sN, Y, X, X, 0, skip, wide)) return e;
    return gemm(s, B, Qy, Y, 0, T1, X, sN, dst, X, sN, Y, X, Y, 0, skip, wide);
}

// ---- the direct pressure solve on its own buffers (shared by the forward step and the adjoint, karman_large_bwd.hip) ----
namespace {

// float-dense from `base`: T0 (rhs in, pressure out), T1, T2 (spectral coefficients, stored TRANSPOSED [X][Y] as ilT), then the scratch
// of the capacitance correction: U, V [Y][64] and X0, W2 [64][64] per simulation in the one-window form whatever the window (hdr NULL or
// FD02), [Y][CP] and [RP][CP] in the scattered form (hdr FDS1)
struct DirectLayout { float *T0, *T1, *T2, *U, *V, *X0, *W2; size_t bytes; };
DirectLayout direct_layout(const sol_karman_cfg* c, const int32_t* hdr, void* base) {
    const size_t B = c->B, Y = c->Y, X = c->X;
    size_t uv = Y * 64, xw = 64 * 64;
    if (hdr && hdr[0] == FDS_MAGIC) {
        const HeaderSc h = header_sc(hdr);
        const size_t RP = h.RP > 0 ? h.RP : 0, CP = h.CP > 0 ? h.CP : 0;
        uv = Y * CP; xw = RP * CP;
    }
    Carve w = Carve::packed(base);
    DirectLayout l{w.take<float>(B * Y * X), w.take<float>(B * Y * X), w.take<float>(B * Y * X), w.take<float>(B * uv), w.take<float>(B * uv),
                   w.take<float>(B * xw), w.take<float>(B * xw)};
    l.bytes = w.bytes();
    return l;
}


inline size_t pad4(size_t n) { return (n + 3) / 4 * 4; }
// words of a scattered blob with this header (precond.scattered_solver_blob's layout)
size_t scattered_words(const HeaderSc& h) {
    const size_t Y = h.Y, X = h.X, SP = h.SP, RP = h.RP, CP = h.CP;
    return FDL_HEADER + pad4(Y * Y + X * X + X * Y) + SP * SP + RP + CP + SP + 2 * RP * Y + 2 * X * CP;
}

int scattered_check(const sol_karman_cfg* c, const char* who, const int32_t* hdr) {
    const HeaderSc h = header_sc(hdr);
    SOL_REQUIRE(h.Y == c->Y && h.X == c->X, "%s: the scattered direct-solver blob is for a %dx%d grid, cfg is %dx%d", who, h.Y, h.X, c->Y, c->X);
    SOL_REQUIRE(h.nS >= 1 && h.SP >= h.nS && h.SP <= SC_MAXSP && h.SP % SC_TILE == 0 && h.nR >= 1 && h.nR <= h.Y && h.nC >= 1 && h.nC <= h.X &&
                    h.RP >= h.nR && h.RP % 4 == 0 && h.RP < h.nR + 4 && h.CP >= h.nC && h.CP % 4 == 0 && h.CP < h.nC + 4 &&
                    (long)h.nR * h.nC >= h.nS,
                "%s: scattered direct-solver blob header is inconsistent", who);
    SOL_REQUIRE((size_t)c->direct_n >= scattered_words(h), "%s: cfg.direct_n = %d words, the scattered direct-solver blob of this header has %zu",
                who, c->direct_n, scattered_words(h));
    SOL_REQUIRE(c->B <= 65535, "%s: B <= 65535 with the scattered direct solve (got %d)", who, c->B);
    return SOL_OK;
}

// M p = T0 as sol_large_direct_solve, the window replaced by the row list R and the column list C of the support set:
//   box forward;  U = T2 Qx[:,C];  X0 = Qy[R,:] U;  W2 = 0, W2[S] = -K' X0[S];  V = Qy[:,R] W2;  T1 = V Qx[C,:];  T2 += T1 / lam;  box back
int scattered_solve(hipStream_t s, const sol_karman_cfg* c, const int32_t* hdr, float* base) {
    const HeaderSc h = header_sc(hdr);
    const int B = c->B, Y = c->Y, X = c->X, N = Y * X, SP = h.SP, RP = h.RP, CP = h.CP;
    const float* Qy = c->direct + FDL_HEADER;
    const float* Qx = Qy + (size_t)Y * Y;
    const float* ilT = Qx + (size_t)X * X;             // [X][Y]
    const float* KpT = c->direct + FDL_HEADER + pad4((size_t)Y * Y + (size_t)X * X + (size_t)X * Y);      // 16-byte aligned rows
    const int* sidx = reinterpret_cast<const int*>(KpT + (size_t)SP * SP) + RP + CP;                      // behind the row and column lists
    const float* QyR = reinterpret_cast<const float*>(sidx + SP);     // [RP][Y]
    const float* QxC = QyR + (size_t)RP * Y;                          // [X][CP]
    const float* QyRt = QxC + (size_t)X * CP;                         // [Y][RP]
    const float* QxCr = QyRt + (size_t)Y * RP;                        // [CP][X]
    const DirectLayout l = direct_layout(c, hdr, base);
    float *T0 = l.T0, *T1 = l.T1, *T2 = l.T2, *U = l.U, *V = l.V, *X0 = l.X0, *W2 = l.W2;
    const long sN = N, sU = (long)Y * CP, sW = (long)RP * CP;
    const bool wide = sol_periodic_bits(hdr) != 0;      // periodic scenes: fp64 accumulators in every product of the solve
    if (int e = sol_large_box_forward(s, B, Y, X, c->direct, T0, T1, T2, nullptr, wide)) return e;
    if (int e = gemm(s, B, T2, X, sN, QxC, CP, 0, U, CP, sU, Y, CP, X, 0, nullptr, wide)) return e;
    if (int e = gemm(s, B, QyR, Y, 0, U, CP, sU, X0, CP, sW, RP, CP, Y, 0, nullptr, wide)) return e;
    // the workspace is the caller's: every call clears W2 before the support entries are written
    const size_t nw = (size_t)B * sW, nb = (nw + 255) / 256;
    SOL_LAUNCH(k_l_zero, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), 0, s, W2, nw);
    SOL_LAUNCH(k_l_capacitance_sc, dim3(SP / SC_TILE, B), dim3(256), 0, s, (const float*)X0, KpT, sidx, W2, SP, (int)sW);
    SOL_LAUNCH_CHECK();
    if (int e = gemm(s, B, QyRt, RP, 0, W2, CP, sW, V, CP, sU, Y, CP, RP, 0, nullptr, wide)) return e;
    if (int e = gemm(s, B, V, CP, sU, QxCr, X, 0, T1, X, sN, Y, X, CP, 0, nullptr, wide)) return e;
    SOL_LAUNCH(k_l_scale, dim3((N + 255) / 256, B), dim3(256), 0, s, T2, (const float*)T1, ilT, Y, X, (const int*)nullptr);
    return sol_large_box_back(s, B, Y, X, c->direct, T2, T1, T0, nullptr, wide);
}

}  // namespace

size_t sol_large_direct_bytes(const sol_karman_cfg* c, const int32_t* hdr) { return direct_layout(c, hdr, nullptr).bytes; }

int sol_large_direct_check(const sol_karman_cfg* c, const char* who, const int32_t* hdr) {
    SOL_REQUIRE(c->direct && c->direct_n > 0, "%s needs the direct-solver blob (cfg.direct)", who);
    if (hdr && hdr[0] == FDS_MAGIC) return scattered_check(c, who, hdr);
    SOL_REQUIRE(hdr && hdr[0] == 0x46443032, "%s: direct_header_host must be the first 16 words of the blob (host copy)", who);
    const Header h{hdr[1], hdr[2], hdr[3], hdr[4], hdr[5], hdr[6], hdr[7]};
    if (h.nS == 0 && sol_periodic_bits(hdr)) {      // an empty periodic scene: the box blob as its direct blob (box forward, box back)
        SOL_REQUIRE(h.Y == c->Y && h.X == c->X, "direct-solver blob is for a %dx%d grid, cfg is %dx%d", h.Y, h.X, c->Y, c->X);
        SOL_REQUIRE(h.SP == 0 && h.win == 0, "direct-solver blob header is inconsistent");
        SOL_REQUIRE((size_t)c->direct_n >= FDL_HEADER + (size_t)h.Y * h.Y + (size_t)h.X * h.X + (size_t)h.X * h.Y,
                    "%s: cfg.direct_n = %d words is less than the box blob of this header", who, c->direct_n);
        return SOL_OK;
    }
    SOL_REQUIRE(h.SP >= h.nS && h.SP <= 4096 && h.wy0 >= 0 && h.wx0 >= 0 && h.wy0 + h.win <= c->Y && h.wx0 + h.win <= c->X,
                "direct-solver blob header is inconsistent");
    SOL_REQUIRE(h.Y == c->Y && h.X == c->X, "direct-solver blob is for a %dx%d grid, cfg is %dx%d", h.Y, h.X, c->Y, c->X);
    SOL_REQUIRE(h.win == 16 || h.win == 32 || h.win == 64, "direct-solver blob: unsupported window %d", h.win);
    return SOL_OK;
}

// M p = T0 by the empty-box solve of the rhs with the capacitance correction on its spectral coefficients; p overwrites T0 (= base)
int sol_large_direct_solve(hipStream_t s, const sol_karman_cfg* c, const int32_t* hdr, float* base) {
    if (hdr[0] == FDS_MAGIC) return scattered_solve(s, c, hdr, base);
    const Header h{hdr[1], hdr[2], hdr[3], hdr[4], hdr[5], hdr[6], hdr[7]};
    const int B = c->B, Y = c->Y, X = c->X, N = Y * X, win = h.win, SP = h.SP;
    if (h.nS == 0) {            // the empty periodic box (sol_large_direct_check): no capacitance part
        const DirectLayout l = direct_layout(c, hdr, base);
        if (int e = sol_large_box_forward(s, B, Y, X, c->direct, l.T0, l.T1, l.T2, nullptr, true)) return e;
        return sol_large_box_back(s, B, Y, X, c->direct, l.T2, l.T1, l.T0, nullptr, true);
    }
    // a scene built with multi_launch on a grid one workgroup holds: the whole solve as one launch (karman_solve_small.hip)
    if ((hdr[SOL_DIRECT_HDR_FLAGS] & SOL_DIRECT_HDR_ONE_WG) && sol_opt().k2d_solve_one_wg && sol_solve_one_wg_supported(Y, X, win))
        return sol_solve_one_wg(s, c, hdr, base);
    // blob sections
    const float* Qy = c->direct + FDL_HEADER;
    const float* Qx = Qy + (size_t)Y * Y;
    const float* ilT = Qx + (size_t)X * X;             // [X][Y]
    const float* KpT = ilT + (size_t)X * Y;
    const int* sidx = reinterpret_cast<const int*>(KpT + (size_t)SP * SP);
    const float* QxW = reinterpret_cast<const float*>(sidx + SP);     // [X][win]
    const DirectLayout l = direct_layout(c, hdr, base);
    float *T0 = l.T0, *T1 = l.T1, *T2 = l.T2, *U = l.U, *V = l.V, *X0 = l.X0, *W2 = l.W2;      // U, V: [Y][win], X0, W2: [win][win]
    const long sN = N, sU = (long)Y * 64, sW = 64 * 64;
    const bool wide = sol_periodic_bits(hdr) != 0;      // periodic scenes: fp64 accumulators in every product of the solve
    if (int e = sol_large_box_forward(s, B, Y, X, c->direct, T0, T1, T2, nullptr, wide)) return e;
    // window values of G b: U = T2 Qx[:, win] ; X0 = Qy[win, :] U
    if (int e = gemm(s, B, T2, X, sN, QxW, win, 0, U, win, sU, Y, win, X, 0, nullptr, wide)) return e;
    if (int e = gemm(s, B, Qy + (size_t)h.wy0 * Y, Y, 0, U, win, sU, X0, win, sW, win, win, Y, 0, nullptr, wide)) return e;
    // W2 = -scatter(K' gather(X0))
    SOL_LAUNCH(k_l_capacitance, dim3(B), dim3(256), SP * sizeof(float), s, X0, KpT, sidx, W2, SP, win);
    SOL_LAUNCH_CHECK();
    // spectral coefficients of the correction: V = Qy[:, win] W2 ; T2 += ((V Qx[win, :])) / lam
    if (int e = gemm(s, B, Qy + h.wy0, Y, 0, W2, win, sW, V, win, sU, Y, win, win, 0, nullptr, wide)) return e;
    if (int e = gemm(s, B, V, win, sU, Qx + (size_t)h.wx0 * X, X, 0, T1, X, sN, Y, X, win, 0, nullptr, wide)) return e;
    SOL_LAUNCH(k_l_scale, dim3((N + 255) / 256, B), dim3(256), 0, s, T2, (const float*)T1, ilT, Y, X, (const int*)nullptr);
    // p = Qy (T2 Qx)
    return sol_large_box_back(s, B, Y, X, c->direct, T2, T1, T0, nullptr, wide);
}

extern "C" int sol_karman_correct(void* stream, const float* out, float* vy, float* vx, float* cor_y, float* cor_x,
                                  int32_t B, int32_t Y, int32_t X, float s0, float s1) {
    SOL_REQUIRE(out && vy && vx, "sol_karman_correct: NULL pointer argument");
    SOL_REQUIRE((cor_y != nullptr) == (cor_x != nullptr), "sol_karman_correct: cor_y and cor_x go together (both or neither NULL)");
    SOL_REQUIRE(B >= 1 && Y >= 1 && X >= 1, "sol_karman_correct: B, Y, X >= 1 (got %d, %d, %d)", B, Y, X);
    const size_t n = (size_t)B * Y * X, nb = (n + 255) / 256;
    SOL_LAUNCH(k_l_correct, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float2*>(out), vy, vx,
               cor_y, cor_x, n, Y, X, s0, s1);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

extern "C" int sol_karman_pressure_solve_large_direct(const sol_karman_cfg* c, void* stream, const float* rhs, float* p,
                                                      const int32_t* direct_header_host, void* workspace, size_t workspace_bytes) {
    const char* who = "sol_karman_pressure_solve_large_direct";
    SOL_REQUIRE(c != nullptr, "cfg is NULL");
    SOL_REQUIRE(c->B >= 1 && c->Y >= 16 && c->X >= 16, "%s: B >= 1, Y, X >= 16 (got %d, %d, %d)", who, c->B, c->Y, c->X);
    SOL_REQUIRE(rhs && p && workspace, "%s: NULL pointer argument", who);
    SOL_REQUIRE(p != rhs, "%s: outputs must not alias the inputs", who);
    if (int e = sol_large_direct_check(c, who, direct_header_host)) return e;
    const size_t need = sol_large_direct_bytes(c, direct_header_host);
    SOL_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    float* base = static_cast<float*>(workspace);
    const size_t n = (size_t)c->B * c->Y * c->X, nb = (n + 255) / 256;
    const unsigned g = (unsigned)(nb < 4096 ? nb : 4096);
    SOL_LAUNCH(k_l_copy, dim3(g), dim3(256), 0, s, base, rhs, n);
    if (int e = sol_large_direct_solve(s, c, direct_header_host, base)) return e;
    SOL_LAUNCH(k_l_copy, dim3(g), dim3(256), 0, s, p, (const float*)base, n);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}
