// karman-3d with a PERIODIC spanwise (z) axis, for gfx950: the forward step's stencil launches with every z index taken modulo the Z
// unique planes (include/sol_hip.h, "PERIODIC SPANWISE BOUNDARIES on the karman-3d step"), and the seam sync / fold entries.
//
// Array shapes are the open step's.  v_z [B,Y,X,Z+1] carries a DUPLICATE plane: plane Z is never read (a NaN there changes nothing) and
// is written equal to plane 0 bit for bit -- the thread of plane Z runs plane 0's arithmetic on plane 0's inputs.  y and x keep the open
// step's clamp, velBC blend, grad_pad and zero ghost ring; floorf and the weights are the open kernels'.
//   k3p_diffuse       k3_diffuse with the z neighbours wrapped
//   k3p_advect_tile   k3_advect_tile: the LDS tile holds full z columns, so the wrap is an index into the column the workgroup already
//                     holds -- no global read at the seam (samples that leave the (y, x) halo fall back to global reads as before)
//   k3p_advect        the same arithmetic straight from global memory (option k3d_tile = 0, and any Z > 82)
//   k3p_div           rhs = -div, the high z face of cell Z - 1 is face 0
//   k3p_project       v -= mask * grad p: along z there is no boundary face, grad_pad is not read
// The pressure solve between k3p_div and k3p_project is the open step's launches on the blob's tables (karman3d.hip: they assume a
// symmetric orthogonal Q_z only, and a periodic blob carries the Hartley table).
#include "karman3d_advect.hpp"

namespace {

// true modulo: a departure point several periods away lands on its plane
__device__ __forceinline__ int wrapz(int k, int Z) {
    k %= Z;
    return k < 0 ? k + Z : k;
}
__device__ __forceinline__ int nextz(int k, int Z) { return k + 1 == Z ? 0 : k + 1; }      // k in [0, Z)
__device__ __forceinline__ int prevz(int k, int Z) { return k == 0 ? Z - 1 : k - 1; }

// lap7 of karman3d.hip on an array [n0][n1][zs] whose unique z planes are 0 .. Z - 1 (zs = Z, or Z + 1 with the duplicate plane), k in [0, Z)
__device__ __forceinline__ float lap7_pz(const float* f, int n0, int n1, int Z, int zs, int j, int i, int k) {
    const size_t s0 = (size_t)n1 * zs, s1 = zs;
    const size_t c0 = (size_t)j * s0 + (size_t)i * s1, c = c0 + k;
    const float v = f[c];
    return f[j + 1 < n0 ? c + s0 : c] + f[j > 0 ? c - s0 : c] + f[i + 1 < n1 ? c + s1 : c] + f[i > 0 ? c - s1 : c] +
           f[c0 + nextz(k, Z)] + f[c0 + prevz(k, Z)] - 6.f * v;
}

__global__ void __launch_bounds__(256) k3p_diffuse(K3Args a) {
    const int Y = a.Y, X = a.X, Z = a.Z;
    const int nVy = (Y + 1) * X * Z, nVx = Y * (X + 1) * Z, nVz = Y * X * (Z + 1);
    const int b = blockIdx.y;
    const float alpha = a.adt / a.re[b];
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nVy + nVx + nVz; e += gridDim.x * blockDim.x) {
        if (e < nVy) {
            const int k = e % Z, i = (e / Z) % X, j = e / (Z * X);
            const float* f = a.vy_in + (size_t)b * nVy;
            float v = f[e] + alpha * lap7_pz(f, Y + 1, X, Z, Z, j, i, k);
            const size_t m = (size_t)b * a.bc_stride + e;
            v = v * (1.f - a.bcm[m]) + a.bcv[m];
            a.svy[(size_t)b * nVy + e] = v;
        } else if (e < nVy + nVx) {
            const int q = e - nVy, k = q % Z, i = (q / Z) % (X + 1), j = q / (Z * (X + 1));
            const float* f = a.vx_in + (size_t)b * nVx;
            a.svx[(size_t)b * nVx + q] = f[q] + alpha * lap7_pz(f, Y, X + 1, Z, Z, j, i, k);
        } else {
            const int q = e - nVy - nVx, k = q % (Z + 1), i = (q / (Z + 1)) % X, j = q / ((Z + 1) * X);
            const int ku = k == Z ? 0 : k;                 // the duplicate plane: plane 0's arithmetic
            const float* f = a.vz_in + (size_t)b * nVz;
            a.svz[(size_t)b * nVz + q] = f[q - k + ku] + alpha * lap7_pz(f, Y, X, Z, Z + 1, j, i, ku);
        }
    }
}

// tri_clamp of karman3d.hip with the z index wrapped: y and x clamped ('boundary' extrapolation), z modulo the Z unique planes of every
// component (the z faces' duplicate plane is never addressed)
template <int C, class R>
__device__ __forceinline__ float tri_pz(const R& r, int j, float oy, int i, float ox, int k, float oz) {
    // no fused multiply-adds in the advection arithmetic (here and in advect_point_pz): which products the compiler contracts depends on the
    // kernel this is inlined into, and the tile and the global kernel are held to the same advected values; the adjoint's adv3_u_pz forms
    // the departure points the same way
#pragma clang fp contract(off)
    const int n0 = r.g_Y() + (C == 0), n1 = r.g_X() + (C == 1), Z = r.g_Z();
    const float fy = floorf(oy), fx = floorf(ox), fz = floorf(oz);
    const float wy = oy - fy, wx = ox - fx, wz = oz - fz;
    const int ja = j + (int)fy, ia = i + (int)fx;
    const int j0 = clampi(ja, 0, n0 - 1), j1 = clampi(ja + 1, 0, n0 - 1);
    const int i0 = clampi(ia, 0, n1 - 1), i1 = clampi(ia + 1, 0, n1 - 1);
    const int k0 = wrapz(k + (int)fz, Z), k1 = nextz(k0, Z);
    auto rd = [&](int jj, int ii, int kk) { return C == 0 ? r.y(jj, ii, kk) : (C == 1 ? r.x(jj, ii, kk) : r.z(jj, ii, kk)); };
    const float c00 = (1.f - wz) * rd(j0, i0, k0) + wz * rd(j0, i0, k1);
    const float c01 = (1.f - wz) * rd(j0, i1, k0) + wz * rd(j0, i1, k1);
    const float c10 = (1.f - wz) * rd(j1, i0, k0) + wz * rd(j1, i0, k1);
    const float c11 = (1.f - wz) * rd(j1, i1, k0) + wz * rd(j1, i1, k1);
    return (1.f - wy) * ((1.f - wx) * c00 + wx * c01) + wy * ((1.f - wx) * c10 + wx * c11);
}

// advect_point of karman3d.hip with z wrapped.  kind 2 is called for k = 0 .. Z: plane Z runs plane 0's arithmetic and stores to plane Z.
template <class R>
__device__ __forceinline__ void advect_point_pz(const K3Args& a, const R& r, int b, int kind, int j, int i, int k) {
#pragma clang fp contract(off)
    const int Y = a.Y, X = a.X, Z = a.Z;
    if (kind == 0) {
        const int kp = nextz(k, Z);
        const float uy = r.y(j, i, k);
        const int ja = max(j - 1, 0), jb = min(j, Y - 1);
        const float ux = 0.25f * (r.x(ja, i, k) + r.x(ja, i + 1, k) + r.x(jb, i, k) + r.x(jb, i + 1, k));
        const float uz = 0.25f * (r.z(ja, i, k) + r.z(ja, i, kp) + r.z(jb, i, k) + r.z(jb, i, kp));
        const float v = tri_pz<0>(r, j, -uy * a.dtdx, i, -ux * a.dtdx, k, -uz * a.dtdx);
        a.vy_out[(size_t)b * (Y + 1) * X * Z + ((size_t)j * X + i) * Z + k] = v * (r.acc(j - 1, i, k) * r.acc(j, i, k));
    } else if (kind == 1) {
        const int kp = nextz(k, Z);
        const float ux = r.x(j, i, k);
        const int ia = max(i - 1, 0), ib = min(i, X - 1);
        const float uy = 0.25f * (r.y(j, ia, k) + r.y(j, ib, k) + r.y(j + 1, ia, k) + r.y(j + 1, ib, k));
        const float uz = 0.25f * (r.z(j, ia, k) + r.z(j, ia, kp) + r.z(j, ib, k) + r.z(j, ib, kp));
        const float v = tri_pz<1>(r, j, -uy * a.dtdx, i, -ux * a.dtdx, k, -uz * a.dtdx);
        a.vx_out[(size_t)b * Y * (X + 1) * Z + ((size_t)j * (X + 1) + i) * Z + k] = v * (r.acc(j, i - 1, k) * r.acc(j, i, k));
    } else if (kind == 2) {
        const int kb = k == Z ? 0 : k, ka = prevz(kb, Z);          // the cells on either side of the face
        const float uz = r.z(j, i, kb);
        const float uy = 0.25f * (r.y(j, i, ka) + r.y(j, i, kb) + r.y(j + 1, i, ka) + r.y(j + 1, i, kb));
        const float ux = 0.25f * (r.x(j, i, ka) + r.x(j, i, kb) + r.x(j, i + 1, ka) + r.x(j, i + 1, kb));
        const float v = tri_pz<2>(r, j, -uy * a.dtdx, i, -ux * a.dtdx, kb, -uz * a.dtdx);
        a.vz_out[(size_t)b * Y * X * (Z + 1) + ((size_t)j * X + i) * (Z + 1) + k] = v * (r.acc(j, i, ka) * r.acc(j, i, kb));
    } else {
        const size_t N = (size_t)Y * X * Z, c = ((size_t)j * X + i) * Z + k;
        const float uy = 0.5f * (r.y(j, i, k) + r.y(j + 1, i, k));
        const float ux = 0.5f * (r.x(j, i, k) + r.x(j, i + 1, k));
        const float uz = 0.5f * (r.z(j, i, k) + r.z(j, i, nextz(k, Z)));
        const float oy = -uy * a.dtdx, ox = -ux * a.dtdx, oz = -uz * a.dtdx;
        const float fy = floorf(oy), fx = floorf(ox), fz = floorf(oz);
        const float wy = oy - fy, wx = ox - fx, wz = oz - fz;
        const int j0 = j + (int)fy, i0 = i + (int)fx, k0 = wrapz(k + (int)fz, Z);
        const float* gd = a.d_in + (size_t)b * N;
        float acc = 0.f;
#pragma unroll
        for (int dj = 0; dj < 2; ++dj)
#pragma unroll
            for (int di = 0; di < 2; ++di)
#pragma unroll
                for (int dk = 0; dk < 2; ++dk) {
                    const int jj = j0 + dj, ii = i0 + di, kk = dk ? nextz(k0, Z) : k0;
                    float v = 0.f;                    // y and x: one ring of zero ghost cells; z wraps
                    if ((unsigned)jj < (unsigned)Y && (unsigned)ii < (unsigned)X) {
                        const size_t q = ((size_t)jj * X + ii) * Z + kk;
                        v = gd[q];
                        if (a.inflow_before) v += a.inflow[q];
                    }
                    acc += (dj ? wy : 1.f - wy) * (di ? wx : 1.f - wx) * (dk ? wz : 1.f - wz) * v;
                }
        if (!a.inflow_before) acc += a.inflow[c] * a.dt;
        a.d_out[(size_t)b * N + c] = acc;
    }
}

template <class R>
__device__ __forceinline__ void advect_column_pz(const K3Args& a, const R& r, int b, int kind, int j, int i, int lane) {
    const int nk = a.Z + (kind == 2 ? 1 : 0);
    for (int k = lane; k < nk; k += 64) advect_point_pz(a, r, b, kind, j, i, k);
}

// k3_advect's work split: one z column (fixed kind, j, i) per wave, lanes along z
__global__ void __launch_bounds__(256) k3p_advect(K3Args a) {
    const int Y = a.Y, X = a.X, Z = a.Z;
    const int nVy = (Y + 1) * X * Z, nVx = Y * (X + 1) * Z, nVz = Y * X * (Z + 1);
    const int b = blockIdx.y;
    GR r;
    r.sy = a.svy + (size_t)b * nVy; r.sx = a.svx + (size_t)b * nVx; r.sz = a.svz + (size_t)b * nVz; r.act = a.active; r.Y = Y; r.X = X; r.Z = Z;
    const int cY = (Y + 1) * X, cX = Y * (X + 1), cC = Y * X;
    const int total = cY + cX + cC + (a.d_out ? cC : 0);
    const int lane = threadIdx.x & 63;
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const int nwaves = gridDim.x * (blockDim.x >> 6);
    for (int c = wave0; c < total; c += nwaves) {
        if (c < cY) advect_column_pz(a, r, b, 0, c / X, c % X, lane);
        else if (c < cY + cX) { const int q = c - cY; advect_column_pz(a, r, b, 1, q / (X + 1), q % (X + 1), lane); }
        else if (c < cY + cX + cC) { const int q = c - cY - cX; advect_column_pz(a, r, b, 2, q / X, q % X, lane); }
        else { const int q = c - cY - cX - cC; advect_column_pz(a, r, b, 3, q / X, q % X, lane); }
    }
}

// k3_advect_tile's tile, staging and ownership; the wrapped z index addresses the LDS column.  The staged plane Z of the z faces is the
// duplicate k3p_diffuse wrote; no index reaches it.
__global__ void __launch_bounds__(ADV_T) k3p_advect_tile(K3Args a, int tiles_x) {
    extern __shared__ __align__(16) float lds3p[];
    const int Y = a.Y, X = a.X, Z = a.Z;
    const int nVy = (Y + 1) * X * Z, nVx = Y * (X + 1) * Z, nVz = Y * X * (Z + 1);
    const int b = blockIdx.y, ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
    const int jt = ty * T3, it = tx * T3;             // first owned cell
    TRd r;
    r.g.sy = a.svy + (size_t)b * nVy; r.g.sx = a.svx + (size_t)b * nVx; r.g.sz = a.svz + (size_t)b * nVz;
    r.g.Y = Y; r.g.X = X; r.g.Z = Z;
    r.j0 = jt - HL3; r.i0 = it - HL3;
    float* ly = lds3p;
    float* lx = ly + (TR + 1) * TR * Z;
    float* lz = lx + TR * (TR + 1) * Z;
    unsigned char* la = reinterpret_cast<unsigned char*>(lz + TR * TR * (Z + 1));
    r.ly = ly; r.lx = lx; r.lz = lz; r.la = la; r.g.act = a.active;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    constexpr int NW = ADV_T / 64;
    // unconditional loads with clamped indices, four columns in flight per wave (k3_advect_tile)
    auto stage = [&](float* dst, int ncol_r, int ncol_i, int nj, int ni, int nz, auto&& rd) {
        const int ncol = ncol_r * ncol_i;
        for (int c0 = wave; c0 < ncol; c0 += 4 * NW) {
            float v[4][2];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = min(c0 + u * NW, ncol - 1), j = clampi(r.j0 + c / ncol_i, 0, nj - 1), i = clampi(r.i0 + c % ncol_i, 0, ni - 1);
                v[u][0] = rd(j, i, min(lane, nz - 1));
                v[u][1] = rd(j, i, min(lane + 64, nz - 1));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * NW;
                if (c < ncol) {
                    if (lane < nz) dst[c * nz + lane] = v[u][0];
                    if (lane + 64 < nz) dst[c * nz + lane + 64] = v[u][1];
                }
            }
        }
    };
    stage(ly, TR + 1, TR, Y + 1, X, Z, [&](int j, int i, int k) { return r.g.y(j, i, k); });
    stage(lx, TR, TR + 1, Y, X + 1, Z, [&](int j, int i, int k) { return r.g.x(j, i, k); });
    stage(lz, TR, TR, Y, X, Z + 1, [&](int j, int i, int k) { return r.g.z(j, i, k); });
    for (int c = wave; c < TR * TR; c += NW) {            // accessible mask of the region's cells: y and x clamped
        const int j = r.j0 + c / TR, i = r.i0 + c % TR;
        for (int k = lane; k < Z; k += 64) la[c * Z + k] = acc_at(a.active, Y, X, Z, j, i, k) != 0.f ? 1 : 0;
    }
    __syncthreads();
    const int ny = min(T3, Y - jt) + (jt + T3 >= Y ? 1 : 0);      // y-face rows owned
    const int nx = min(T3, X - it) + (it + T3 >= X ? 1 : 0);      // x-face columns owned
    const int cy = min(T3, Y - jt), cx = min(T3, X - it);         // cells owned
    const int cY = ny * cx, cX = cy * nx, cC = cy * cx;
    const int total = cY + cX + cC + (a.d_out ? cC : 0);
    for (int c = wave; c < total; c += NW) {
        if (c < cY) advect_column_pz(a, r, b, 0, jt + c / cx, it + c % cx, lane);
        else if (c < cY + cX) { const int q = c - cY; advect_column_pz(a, r, b, 1, jt + q / nx, it + q % nx, lane); }
        else if (c < cY + cX + cC) { const int q = c - cY - cX; advect_column_pz(a, r, b, 2, jt + q / cx, it + q % cx, lane); }
        else { const int q = c - cY - cX - cC; advect_column_pz(a, r, b, 3, jt + q / cx, it + q % cx, lane); }
    }
}

__global__ void __launch_bounds__(256) k3p_div(K3Args a) {
    const int Y = a.Y, X = a.X, Z = a.Z, N = Y * X * Z;
    const int b = blockIdx.y;
    const float* vy = a.vy_out + (size_t)b * (Y + 1) * X * Z;
    const float* vx = a.vx_out + (size_t)b * Y * (X + 1) * Z;
    const float* vz = a.vz_out + (size_t)b * Y * X * (Z + 1);
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < N; c += gridDim.x * blockDim.x) {
        const int k = c % Z, i = (c / Z) % X, j = c / (Z * X);
        const float div = (vy[((size_t)(j + 1) * X + i) * Z + k] - vy[((size_t)j * X + i) * Z + k]) +
                          (vx[((size_t)j * (X + 1) + i + 1) * Z + k] - vx[((size_t)j * (X + 1) + i) * Z + k]) +
                          (vz[((size_t)j * X + i) * (Z + 1) + nextz(k, Z)] - vz[((size_t)j * X + i) * (Z + 1) + k]);
        a.rhs[(size_t)b * N + c] = -div;
    }
}

__global__ void __launch_bounds__(256) k3p_project(K3Args a) {
    const int Y = a.Y, X = a.X, Z = a.Z, N = Y * X * Z;
    const int nVy = (Y + 1) * X * Z, nVx = Y * (X + 1) * Z, nVz = Y * X * (Z + 1);
    const int b = blockIdx.y;
    const float* P = a.p + (size_t)b * N;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nVy + nVx + nVz; e += gridDim.x * blockDim.x) {
        if (e < nVy) {
            const int k = e % Z, i = (e / Z) % X, j = e / (Z * X);
            float g = 0.f;
            if (j >= 1 && j <= Y - 1) g = P[((size_t)j * X + i) * Z + k] - P[((size_t)(j - 1) * X + i) * Z + k];
            else if (a.grad_pad == 1) g = j == 0 ? P[((size_t)i) * Z + k] : -P[((size_t)(Y - 1) * X + i) * Z + k];
            float* dst = a.vy_out + (size_t)b * nVy + e;
            const float v = *dst - face_mask<0>(a.active, Y, X, Z, j, i, k) * g;
            *dst = v;
            if (a.feat && j < Y) a.feat[((size_t)b * N + e) * 4 + 0] = v * a.fs0;
        } else if (e < nVy + nVx) {
            const int q = e - nVy, k = q % Z, i = (q / Z) % (X + 1), j = q / (Z * (X + 1));
            float g = 0.f;
            if (i >= 1 && i <= X - 1) g = P[((size_t)j * X + i) * Z + k] - P[((size_t)j * X + i - 1) * Z + k];
            else if (a.grad_pad == 1) g = i == 0 ? P[((size_t)j * X) * Z + k] : -P[((size_t)j * X + X - 1) * Z + k];
            float* dst = a.vx_out + (size_t)b * nVx + q;
            const float v = *dst - face_mask<1>(a.active, Y, X, Z, j, i, k) * g;
            *dst = v;
            if (a.feat && i < X) a.feat[((size_t)b * N + ((size_t)j * X + i) * Z + k) * 4 + 1] = v * a.fs1;
        } else {
            // every z face lies between two cells: plane Z reads its own pre-projection value (the advection wrote it equal to plane 0's)
            // and runs plane 0's arithmetic
            const int q = e - nVy - nVx, k = q % (Z + 1), i = (q / (Z + 1)) % X, j = q / ((Z + 1) * X);
            const int kb = k == Z ? 0 : k, ka = prevz(kb, Z);
            const size_t col = ((size_t)j * X + i) * Z;
            const float g = P[col + kb] - P[col + ka];
            float* dst = a.vz_out + (size_t)b * nVz + q;
            const float v = *dst - acc_at(a.active, Y, X, Z, j, i, ka) * acc_at(a.active, Y, X, Z, j, i, kb) * g;
            *dst = v;
            if (a.feat && k < Z) {
                float* f = a.feat + ((size_t)b * N + col + k) * 4;
                f[2] = v * a.fs2;
                f[3] = a.re[b] * a.fs3;
            }
        }
    }
}

// seam sync: plane 0 of v_z onto the duplicate plane.  seam fold, its adjoint: g[0] += g[dup] (one fp32 add), g[dup] = 0
__global__ void __launch_bounds__(256) k3p_seam(float* __restrict__ vz, size_t cols, int Z, int fold) {
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < cols; c += (size_t)gridDim.x * blockDim.x) {
        float* p = vz + c * (Z + 1);
        if (fold) { p[0] += p[Z]; p[Z] = 0.f; }
        else p[Z] = p[0];
    }
}

// ========================================================================================================================
// Adjoint (the stages of karman3d.hip's k3b_* kernels, z wrapped).  The cotangent of the output duplicate plane is first added onto plane
// 0's with one fp32 add (goz_u); no stage reads or scatters to plane Z afterwards, and g_vz_in[..., Z] is written 0.
// ========================================================================================================================
__device__ __forceinline__ float goz_u(const float* gz_col, int k, int Z) { return k == 0 ? gz_col[0] + gz_col[Z] : gz_col[k]; }      // k in [0, Z)
__device__ __forceinline__ float mask_z(const float* act, int Y, int X, int Z, int j, int i, int k) {                                // face k in [0, Z)
    return acc_at(act, Y, X, Z, j, i, prevz(k, Z)) * acc_at(act, Y, X, Z, j, i, k);
}

__global__ void __launch_bounds__(256) k3pb_rhs(K3BArgs a) {
    const int Y = a.Y, X = a.X, Z = a.Z, N = Y * X * Z;
    const int b = blockIdx.y;
    const float* gy = a.goy + (size_t)b * (Y + 1) * X * Z;
    const float* gx = a.gox + (size_t)b * Y * (X + 1) * Z;
    const float* gz = a.goz + (size_t)b * Y * X * (Z + 1);
    const bool keep = a.grad_pad == 1;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < N; c += gridDim.x * blockDim.x) {
        const int k = c % Z, i = (c / Z) % X, j = c / (Z * X);
        auto wy = [&](int jj) { return (keep || (jj != 0 && jj != Y)) ? face_mask<0>(a.active, Y, X, Z, jj, i, k) * gy[((size_t)jj * X + i) * Z + k] : 0.f; };
        auto wx = [&](int ii) { return (keep || (ii != 0 && ii != X)) ? face_mask<1>(a.active, Y, X, Z, j, ii, k) * gx[((size_t)j * (X + 1) + ii) * Z + k] : 0.f; };
        auto wz = [&](int kk) { return mask_z(a.active, Y, X, Z, j, i, kk) * goz_u(gz + ((size_t)j * X + i) * (Z + 1), kk, Z); };
        a.rhs[(size_t)b * N + c] = (wy(j) - wy(j + 1)) + (wx(i) - wx(i + 1)) + (wz(k) - wz(nextz(k, Z)));
    }
    // side job (k3b_rhs): clear this simulation's fixed-point accumulators and its absmax slots
    const size_t faces = (size_t)(Y + 1) * X * Z + (size_t)Y * (X + 1) * Z + (size_t)Y * X * (Z + 1);
    uint4* zc = reinterpret_cast<uint4*>(a.gcy) + (size_t)b * (faces / 2);
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < faces / 2; e += (size_t)gridDim.x * blockDim.x) zc[e] = make_uint4(0u, 0u, 0u, 0u);
    if (blockIdx.x == 0 && threadIdx.x < FX_SLOTS) a.gmax[b * FX_SLOTS + threadIdx.x] = 0u;
}

__global__ void __launch_bounds__(256) k3pb_gva(K3BArgs a) {
    const int Y = a.Y, X = a.X, Z = a.Z, N = Y * X * Z;
    const int nVy = (Y + 1) * X * Z, nVx = Y * (X + 1) * Z, nVz = Y * X * (Z + 1);
    const int b = blockIdx.y;
    const float* P = a.gdiv + (size_t)b * N;
    auto cell = [&](int j, int i, int k) { return ((unsigned)j < (unsigned)Y && (unsigned)i < (unsigned)X) ? P[((size_t)j * X + i) * Z + k] : 0.f; };     // k in [0, Z)
    float vmax = 0.f;
    bool bad = false;
    const int cY = (Y + 1) * X, cX = Y * (X + 1), cC = Y * X;
    const int lane = threadIdx.x & 63;
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const int nwaves = gridDim.x * (blockDim.x >> 6);
    for (int c = wave0; c < cY + cX + cC; c += nwaves) {
        if (c < cY) {
            const int j = c / X, i = c % X;
            for (int k = lane; k < Z; k += 64) {
                const size_t e = (size_t)b * nVy + ((size_t)j * X + i) * Z + k;
                const float v = face_mask<0>(a.active, Y, X, Z, j, i, k) * (a.goy[e] + cell(j - 1, i, k) - cell(j, i, k));
                a.gay[e] = v; vmax = fmaxf(vmax, fabsf(v)); bad |= !(fabsf(v) <= 3.402823466e38f);
            }
        } else if (c < cY + cX) {
            const int q = c - cY, j = q / (X + 1), i = q % (X + 1);
            for (int k = lane; k < Z; k += 64) {
                const size_t e = (size_t)b * nVx + ((size_t)j * (X + 1) + i) * Z + k;
                const float v = face_mask<1>(a.active, Y, X, Z, j, i, k) * (a.gox[e] + cell(j, i - 1, k) - cell(j, i, k));
                a.gax[e] = v; vmax = fmaxf(vmax, fabsf(v)); bad |= !(fabsf(v) <= 3.402823466e38f);
            }
        } else {
            const int q = c - cY - cX, j = q / X, i = q % X;
            const size_t col = (size_t)b * nVz + ((size_t)j * X + i) * (Z + 1);
            for (int k = lane; k <= Z; k += 64) {
                float v = 0.f;                  // plane Z: its cotangent went onto plane 0's; nothing is scattered from it
                if (k < Z) v = mask_z(a.active, Y, X, Z, j, i, k) * (goz_u(a.goz + col, k, Z) + cell(j, i, prevz(k, Z)) - cell(j, i, k));
                a.gaz[col + k] = v; vmax = fmaxf(vmax, fabsf(v)); bad |= !(fabsf(v) <= 3.402823466e38f);
            }
        }
    }
    fx_publish_max(a.gmax + b * FX_SLOTS, vmax, bad);
}

// adv3_u / adv3_u_scatter of karman3d_advect.hpp with z wrapped; k in [0, Z).  na / nb: the two indices along C's own axis (clamped for y
// and x, the wrapped neighbours for z)
template <int C>
__device__ __forceinline__ AdvU adv3_u_pz(const GR& r, int j, int i, int k) {
#pragma clang fp contract(off)
    const int Y = r.Y, X = r.X, Z = r.Z;
    AdvU u;
    if (C == 0) {
        const int ja = max(j - 1, 0), jb = min(j, Y - 1), kp = nextz(k, Z);
        u.na = ja; u.nb = jb;
        u.uy = r.y(j, i, k);
        u.ux = 0.25f * (r.x(ja, i, k) + r.x(ja, i + 1, k) + r.x(jb, i, k) + r.x(jb, i + 1, k));
        u.uz = 0.25f * (r.z(ja, i, k) + r.z(ja, i, kp) + r.z(jb, i, k) + r.z(jb, i, kp));
    } else if (C == 1) {
        const int ia = max(i - 1, 0), ib = min(i, X - 1), kp = nextz(k, Z);
        u.na = ia; u.nb = ib;
        u.ux = r.x(j, i, k);
        u.uy = 0.25f * (r.y(j, ia, k) + r.y(j, ib, k) + r.y(j + 1, ia, k) + r.y(j + 1, ib, k));
        u.uz = 0.25f * (r.z(j, ia, k) + r.z(j, ia, kp) + r.z(j, ib, k) + r.z(j, ib, kp));
    } else {
        const int ka = prevz(k, Z), kb = k;
        u.na = ka; u.nb = kb;
        u.uz = r.z(j, i, k);
        u.uy = 0.25f * (r.y(j, i, ka) + r.y(j, i, kb) + r.y(j + 1, i, ka) + r.y(j + 1, i, kb));
        u.ux = 0.25f * (r.x(j, i, ka) + r.x(j, i, kb) + r.x(j, i + 1, ka) + r.x(j, i + 1, kb));
    }
    return u;
}
template <int C, class Add>
__device__ __forceinline__ void adv3_u_scatter_pz(const Add& add, const AdvU& u, int Z, int j, int i, int k, float guy, float gux, float guz) {
#pragma clang fp contract(off)
    if (C == 0) {
        const int ja = u.na, jb = u.nb, kp = nextz(k, Z);
        add(0, j, i, k, guy);
        const float qx = 0.25f * gux, qz = 0.25f * guz;
        add(1, ja, i, k, qx); add(1, ja, i + 1, k, qx); add(1, jb, i, k, qx); add(1, jb, i + 1, k, qx);
        add(2, ja, i, k, qz); add(2, ja, i, kp, qz); add(2, jb, i, k, qz); add(2, jb, i, kp, qz);
    } else if (C == 1) {
        const int ia = u.na, ib = u.nb, kp = nextz(k, Z);
        add(1, j, i, k, gux);
        const float qy = 0.25f * guy, qz = 0.25f * guz;
        add(0, j, ia, k, qy); add(0, j, ib, k, qy); add(0, j + 1, ia, k, qy); add(0, j + 1, ib, k, qy);
        add(2, j, ia, k, qz); add(2, j, ia, kp, qz); add(2, j, ib, k, qz); add(2, j, ib, kp, qz);
    } else {
        const int ka = u.na, kb = u.nb;
        add(2, j, i, k, guz);
        const float qy = 0.25f * guy, qx = 0.25f * gux;
        add(0, j, i, ka, qy); add(0, j, i, kb, qy); add(0, j + 1, i, ka, qy); add(0, j + 1, i, kb, qy);
        add(1, j, i, ka, qx); add(1, j, i, kb, qx); add(1, j, i + 1, ka, qx); add(1, j, i + 1, kb, qx);
    }
}

// advect_adj_point of karman3d_advect.hpp with z wrapped: every target index is in [0, Z) BEFORE the adder sees it, so the LDS window and
// the global path take the same contributions
template <int C, class Add>
__device__ __forceinline__ void advect_adj_point_pz(const K3BArgs& a, const GR& r, const Add& add, int j, int i, int k, float gs) {
#pragma clang fp contract(off)
    const int Y = a.Y, X = a.X, Z = a.Z;
    const AdvU u = adv3_u_pz<C>(r, j, i, k);
    const float oy = -u.uy * a.dtdx, ox = -u.ux * a.dtdx, oz = -u.uz * a.dtdx;
    const int n0 = Y + (C == 0), n1 = X + (C == 1);
    const float fy = floorf(oy), fx = floorf(ox), fz = floorf(oz);
    const float wy = oy - fy, wx = ox - fx, wz = oz - fz;
    const int j0 = clampi(j + (int)fy, 0, n0 - 1), j1 = clampi(j + (int)fy + 1, 0, n0 - 1);
    const int i0 = clampi(i + (int)fx, 0, n1 - 1), i1 = clampi(i + (int)fx + 1, 0, n1 - 1);
    const int k0 = wrapz(k + (int)fz, Z), k1 = nextz(k0, Z);
    auto val = [&](int jj, int ii, int kk) { return C == 0 ? r.y(jj, ii, kk) : (C == 1 ? r.x(jj, ii, kk) : r.z(jj, ii, kk)); };
    float dy = 0.f, dx = 0.f, dz = 0.f;
#pragma unroll
    for (int cj = 0; cj < 2; ++cj)
#pragma unroll
        for (int ci = 0; ci < 2; ++ci)
#pragma unroll
            for (int ck = 0; ck < 2; ++ck) {
                const int jj = cj ? j1 : j0, ii = ci ? i1 : i0, kk = ck ? k1 : k0;
                const float by = cj ? wy : 1.f - wy, bx = ci ? wx : 1.f - wx, bz = ck ? wz : 1.f - wz;
                const float v = val(jj, ii, kk);
                add(C, jj, ii, kk, by * bx * bz * gs);          // field term
                dy += (cj ? 1.f : -1.f) * bx * bz * v;
                dx += by * (ci ? 1.f : -1.f) * bz * v;
                dz += by * bx * (ck ? 1.f : -1.f) * v;
            }
    adv3_u_scatter_pz<C>(add, u, Z, j, i, k, -a.dtdx * gs * dy, -a.dtdx * gs * dx, -a.dtdx * gs * dz);
}

// k3b_advect_adj: wave per z column, global int64 atomics.  Every component has Z unique planes.
__global__ void __launch_bounds__(256) k3pb_advect_adj(K3BArgs a) {
    const int Y = a.Y, X = a.X, Z = a.Z;
    const int nVy = (Y + 1) * X * Z, nVx = Y * (X + 1) * Z, nVz = Y * X * (Z + 1);
    const int b = blockIdx.y;
    GR r;
    r.sy = a.svy + (size_t)b * nVy; r.sx = a.svx + (size_t)b * nVx; r.sz = a.svz + (size_t)b * nVz; r.Y = Y; r.X = X; r.Z = Z;
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    const GAdd add{a.gcy + (size_t)b * nVy, a.gcx + (size_t)b * nVx, a.gcz + (size_t)b * nVz, qs, X, Z};
    const int cY = (Y + 1) * X, cX = Y * (X + 1), cC = Y * X;
    const int lane = threadIdx.x & 63;
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const int nwaves = gridDim.x * (blockDim.x >> 6);
    for (int c = wave0; c < cY + cX + cC; c += nwaves) {
        if (c < cY) {
            const int j = c / X, i = c % X;
            for (int k = lane; k < Z; k += 64) { const float g = a.gay[(size_t)b * nVy + ((size_t)j * X + i) * Z + k]; if (g != 0.f) advect_adj_point_pz<0>(a, r, add, j, i, k, g); }
        } else if (c < cY + cX) {
            const int q = c - cY, j = q / (X + 1), i = q % (X + 1);
            for (int k = lane; k < Z; k += 64) { const float g = a.gax[(size_t)b * nVx + ((size_t)j * (X + 1) + i) * Z + k]; if (g != 0.f) advect_adj_point_pz<1>(a, r, add, j, i, k, g); }
        } else {
            const int q = c - cY - cX, j = q / X, i = q % X;
            for (int k = lane; k < Z; k += 64) { const float g = a.gaz[(size_t)b * nVz + ((size_t)j * X + i) * (Z + 1) + k]; if (g != 0.f) advect_adj_point_pz<2>(a, r, add, j, i, k, g); }
        }
    }
}

// k3b_advect_adj_tile: the int64 LDS window of 8 x 8 columns x (Z + 1) planes per component; the wrapped targets fall in planes 0 .. Z - 1
// of the window the workgroup already holds.  Integer adds commute: the result equals k3pb_advect_adj's bit for bit.
__global__ void __launch_bounds__(256) k3pb_advect_adj_tile(K3BArgs a, int nti) {
    extern __shared__ __align__(16) unsigned long long smem_adj_pz[];
    const int Y = a.Y, X = a.X, Z = a.Z, ZP = Z + 1;
    const int nVy = (Y + 1) * X * Z, nVx = Y * (X + 1) * Z, nVz = Y * X * (Z + 1);
    const int b = blockIdx.y;
    const int tj = (int)blockIdx.x / nti, ti = (int)blockIdx.x % nti, j0 = tj * K3B_TJ, i0 = ti * K3B_TJ;
    GR r;
    r.sy = a.svy + (size_t)b * nVy; r.sx = a.svx + (size_t)b * nVx; r.sz = a.svz + (size_t)b * nVz; r.Y = Y; r.X = X; r.Z = Z;
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    const GAdd gadd{a.gcy + (size_t)b * nVy, a.gcx + (size_t)b * nVx, a.gcz + (size_t)b * nVz, qs, X, Z};
    const TAdd add{gadd, smem_adj_pz, j0 - K3B_TH, i0 - K3B_TH, ZP};
    const int ncell = 3 * K3B_TW * K3B_TW * ZP;
    fx_window_clear(smem_adj_pz, ncell, 256);
    __syncthreads();
    const int j1 = min(j0 + K3B_TJ, Y), i1 = min(i0 + K3B_TJ, X);
    const int j1y = j0 + K3B_TJ >= Y ? Y + 1 : j1, i1x = i0 + K3B_TJ >= X ? X + 1 : i1;
    const int nJ = j1 - j0, nI = i1 - i0, nY = (j1y - j0) * nI, nX = nJ * (i1x - i0), nC = nJ * nI;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int t = wave; t < nY + nX + nC; t += 4) {
        if (t < nY) {
            const int j = j0 + t / nI, i = i0 + t % nI;
            for (int k = lane; k < Z; k += 64) { const float g = a.gay[(size_t)b * nVy + ((size_t)j * X + i) * Z + k]; if (g != 0.f) advect_adj_point_pz<0>(a, r, add, j, i, k, g); }
        } else if (t < nY + nX) {
            const int q = t - nY, w = i1x - i0, j = j0 + q / w, i = i0 + q % w;
            for (int k = lane; k < Z; k += 64) { const float g = a.gax[(size_t)b * nVx + ((size_t)j * (X + 1) + i) * Z + k]; if (g != 0.f) advect_adj_point_pz<1>(a, r, add, j, i, k, g); }
        } else {
            const int q = t - nY - nX, j = j0 + q / nI, i = i0 + q % nI;
            for (int k = lane; k < Z; k += 64) { const float g = a.gaz[(size_t)b * nVz + ((size_t)j * X + i) * (Z + 1) + k]; if (g != 0.f) advect_adj_point_pz<2>(a, r, add, j, i, k, g); }
        }
    }
    __syncthreads();
    fx_window_flush(smem_adj_pz, ncell, 256, [&](int e) {
        const int kk = e % ZP, li = (e / ZP) % K3B_TW, lj = (e / (ZP * K3B_TW)) % K3B_TW, comp = e / (ZP * K3B_TW * K3B_TW);
        return gadd.at(comp, j0 - K3B_TH + lj, i0 - K3B_TH + li, kk);
    });
}

// lapT of fixed_scatter.hpp on a component array [n0][n1][zs] whose unique z planes are 0 .. Z - 1: y and x replicate padded (a direction
// that leaves the array contributes g'[c] itself), z wrapped (the circulant second difference is its own transpose).  Order: y +, y -, x +,
// x -, z +, z -.
__device__ __forceinline__ float lapT_pz(const long long* g, float qi, float sc_here, const float* scm, int n0, int n1, int Z, int zs, int j, int i, int k) {
    auto at = [&](int q) { const float v = fx_get(g, q, qi); return scm ? v * (1.f - scm[q]) : v; };
    const int s1 = zs, s0 = n1 * zs, c0 = j * s0 + i * s1, c = c0 + k;
    const float v = fx_get(g, c, qi) * sc_here;
    float acc = -6.f * v;
    acc += j + 1 < n0 ? at(c + s0) : v;
    acc += j > 0 ? at(c - s0) : v;
    acc += i + 1 < n1 ? at(c + s1) : v;
    acc += i > 0 ? at(c - s1) : v;
    acc += at(c0 + nextz(k, Z));
    acc += at(c0 + prevz(k, Z));
    return acc;
}

__global__ void __launch_bounds__(256) k3pb_diffuse_adj(K3BArgs a) {
    const int Y = a.Y, X = a.X, Z = a.Z;
    const int nVy = (Y + 1) * X * Z, nVx = Y * (X + 1) * Z, nVz = Y * X * (Z + 1);
    const int b = blockIdx.y;
    const float alpha = a.adt / a.re[b];
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nVy + nVx + nVz; e += gridDim.x * blockDim.x) {
        if (e < nVy) {
            const int k = e % Z, i = (e / Z) % X, j = e / (Z * X);
            const long long* g = a.gcy + (size_t)b * nVy;
            const float* m = a.bcm + (size_t)b * a.bc_stride;
            const float sc = 1.f - m[e];
            a.giy[(size_t)b * nVy + e] = __fmaf_rn(fx_get(g, e, qi), sc, alpha * lapT_pz(g, qi, sc, m, Y + 1, X, Z, Z, j, i, k));
        } else if (e < nVy + nVx) {
            const int q = e - nVy, k = q % Z, i = (q / Z) % (X + 1), j = q / (Z * (X + 1));
            const long long* g = a.gcx + (size_t)b * nVx;
            a.gix[(size_t)b * nVx + q] = fx_get_fma(g, q, qi, alpha * lapT_pz(g, qi, 1.f, nullptr, Y, X + 1, Z, Z, j, i, k));
        } else {
            const int q = e - nVy - nVx, k = q % (Z + 1), i = (q / (Z + 1)) % X, j = q / ((Z + 1) * X);
            const long long* g = a.gcz + (size_t)b * nVz;
            a.giz[(size_t)b * nVz + q] = k == Z ? 0.f : fx_get_fma(g, q, qi, alpha * lapT_pz(g, qi, 1.f, nullptr, Y, X, Z, Z + 1, j, i, k));
        }
    }
}

int grid_pz(size_t n) { const size_t g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 65535 ? 65535 : g)); }

int seam3d(const char* who, void* stream, float* vz, int32_t B, int32_t Y, int32_t X, int32_t Z, int32_t periodic_bits, int fold) {
    SOL_REQUIRE(vz && B >= 1 && Y >= 1 && X >= 1 && Z >= 1, "%s: bad arguments", who);
    SOL_REQUIRE(periodic_bits == 0 || periodic_bits == SOL_K3_PERIODIC_Z, "%s: periodic_bits = %d: only the z axis (8) is built; a periodic y (2) or x (4) is not",
                who, periodic_bits);
    if (!periodic_bits) return SOL_OK;
    const size_t cols = (size_t)B * Y * X;
    SOL_LAUNCH(k3p_seam, dim3(grid_pz(cols)), dim3(256), 0, (hipStream_t)stream, vz, cols, Z, fold);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

}  // namespace

// the launches of the z-periodic forward step before the pressure solve: diffusion, advection (the LDS-tile kernel where the option asks
// for it and the tile fits, k3_advect_tile's rule), divergence
int sol_k3p_front(hipStream_t s, const K3Args& a) {
    const int B = a.B, Y = a.Y, X = a.X, Z = a.Z;
    const size_t faces = (size_t)(Y + 1) * X * Z + (size_t)Y * (X + 1) * Z + (size_t)Y * X * (Z + 1);
    SOL_LAUNCH(k3p_diffuse, dim3(grid_pz(faces), B), dim3(256), 0, s, a);
    const size_t tile_lds = ((size_t)(TR + 1) * TR * Z + (size_t)TR * (TR + 1) * Z + (size_t)TR * TR * (Z + 1)) * sizeof(float) + (size_t)TR * TR * Z;
    if (sol_opt().k3d_tile && tile_lds <= 160 * 1024) {
        static std::atomic<unsigned long long> optin{0};
        if (int e = sol_lds_optin(optin, {SOL_K(k3p_advect_tile)}, "k3p_advect_tile")) return e;
        const int tiles_y = (Y + T3 - 1) / T3, tiles_x = (X + T3 - 1) / T3;
        SOL_LAUNCH(k3p_advect_tile, dim3(tiles_y * tiles_x, B), dim3(ADV_T), tile_lds, s, a, tiles_x);
    } else {
        SOL_LAUNCH(k3p_advect, dim3(grid_pz((size_t)((Y + 1) * X + Y * (X + 1) + 2 * Y * X) * 64), B), dim3(256), 0, s, a);
    }
    SOL_LAUNCH(k3p_div, dim3(grid_pz((size_t)Y * X * Z), B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

int sol_k3p_project(hipStream_t s, const K3Args& a) {
    const size_t faces = (size_t)(a.Y + 1) * a.X * a.Z + (size_t)a.Y * (a.X + 1) * a.Z + (size_t)a.Y * a.X * (a.Z + 1);
    SOL_LAUNCH(k3p_project, dim3(grid_pz(faces), a.B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

int sol_k3pb_rhs(hipStream_t s, const K3BArgs& a) {
    SOL_LAUNCH(k3pb_rhs, dim3(grid_pz((size_t)a.Y * a.X * a.Z), a.B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

// g_a (k3b_gva's grid: 1 024 workgroups at most publish into the 64 absmax slots), the scatter (the LDS window where Z <= 64 and `tile`
// -- or, tile < 0, the option k3d_adj_tile -- asks for it: launch_advect_adj3d's rule), the diffusion adjoint
int sol_k3pb_back(hipStream_t s, const K3BArgs& a, int tile) {
    const int B = a.B, Y = a.Y, X = a.X, Z = a.Z;
    const size_t cols = (size_t)(Y + 1) * X + (size_t)Y * (X + 1) + (size_t)Y * X;
    const size_t faces = (size_t)(Y + 1) * X * Z + (size_t)Y * (X + 1) * Z + (size_t)Y * X * (Z + 1);
    SOL_LAUNCH(k3pb_gva, dim3((unsigned)std::min<size_t>(1024, (cols + 3) / 4), B), dim3(256), 0, s, a);
    if ((tile < 0 ? sol_opt().k3d_adj_tile != 0 : tile != 0) && Z <= 64) {
        static std::atomic<unsigned long long> optin_adj{0};
        if (int e = sol_lds_optin(optin_adj, {SOL_K(k3pb_advect_adj_tile)}, "k3pb_advect_adj_tile")) return e;
        const int ntj = (Y + K3B_TJ - 1) / K3B_TJ, nti = (X + K3B_TJ - 1) / K3B_TJ;
        SOL_LAUNCH(k3pb_advect_adj_tile, dim3(ntj * nti, B), dim3(256), (size_t)3 * K3B_TW * K3B_TW * (Z + 1) * 8, s, a, nti);
    } else {
        SOL_LAUNCH(k3pb_advect_adj, dim3(grid_pz(cols * 64), B), dim3(256), 0, s, a);
    }
    SOL_LAUNCH(k3pb_diffuse_adj, dim3(grid_pz(faces), B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

extern "C" int sol_karman3d_seam_sync(void* stream, float* vz, int32_t B, int32_t Y, int32_t X, int32_t Z, int32_t periodic_bits) {
    return seam3d("sol_karman3d_seam_sync", stream, vz, B, Y, X, Z, periodic_bits, 0);
}

extern "C" int sol_karman3d_seam_fold(void* stream, float* g_vz, int32_t B, int32_t Y, int32_t X, int32_t Z, int32_t periodic_bits) {
    return seam3d("sol_karman3d_seam_fold", stream, g_vz, B, Y, X, Z, periodic_bits, 1);
}
