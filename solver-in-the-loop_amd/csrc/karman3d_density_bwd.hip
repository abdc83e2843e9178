// Adjoint of the karman-3d step's marker density: the gradient of a loss on d_out with respect to d_in and -- through the departure points
// of the density's semi-Lagrangian advection -- to the step's input velocity.  The 3-D twin of karman_density_bwd.hip.  The density path is
// linear in the cotangents and meets the velocity path only at the post-diffusion velocity c = saved_v*, so it is a set of launches of its
// own, chip wide on global memory; it runs no pressure solve:
//   k3d_clear          clears the int64 accumulators of g_d_in and publishes max|g_d_out| per simulation (the scale of the scatter): one
//                      workgroup per absmax slot, no atomics, nothing to clear beforehand
//   k3d_advect_adj*    per cell: the departure point recomputed from c with the forward step's expressions (advect_point kind 3 of
//                      karman3d.hip), the field term scattered into g_d_in in 64-bit fixed point (fixed_scatter.hpp: order independent, bit
//                      reproducible; what a non-finite cotangent does), the back-trace term gU = -dt/dx g slope written per cell.  One z
//                      column per wave, lanes along k, as k3b_advect_adj.  The default form accumulates in an int64 LDS window per tile of
//                      4 x 4 columns (halo 2 columns, all k: 8 x 8 x Z x 8 B = 32 KB at Z = 64; targets beyond it go to global memory, so
//                      any CFL number is handled); option k3d_dens_adj_tile = 0, or a Z whose window exceeds 64 KB: every contribution a
//                      global atomic.  Same bits.
//   k3d_diffuse_adj    g_c = the cell-to-face transpose of gU (a centre velocity is the mean of its two faces), gathered on the fly, then
//                      the diffusion / boundary-condition adjoint: g_vy_in = (I + alpha L^T)((1 - bcm) g_cy), g_vx_in = (I + alpha L^T) g_cx,
//                      g_vz_in likewise, written or added onto the velocity adjoint's result; converts g_d_in back to fp32
// sol_karman3d_density_bwd_re: the same launches, then the reduction of that g' against L v_in to the density path's part of the gradient
// with respect to the Reynolds number (karman3d_re_bwd.hip).
#include "carve.hpp"
#include "karman3d_advect.hpp"
#include "karman3d_re.hpp"

namespace {

constexpr int K3D_TJ = 4, K3D_TH = 2, K3D_TW = K3D_TJ + 2 * K3D_TH;      // tile of 4 x 4 columns, window of 8 x 8 columns (the velocity adjoint's)
constexpr size_t K3D_LDS_MAX = 64 * 1024;                                 // the window stays below what needs an LDS opt-in

struct K3DArgs {
    int B, Y, X, Z;
    float dtdx, adt;
    int inflow_before, accumulate;
    const float *d_in, *inflow, *svy, *svx, *svz, *re, *bcm;
    long bc_stride;
    const float* gdo;                   // gradient w.r.t. the step's output density
    long long* gD;                      // int64 fixed-point accumulators of g_d_in [B][Y][X][Z]
    float *gUy, *gUx, *gUz;             // back-trace term per cell [B][Y][X][Z]: gradient w.r.t. the centre velocity the cell was traced with
    unsigned* gmax;                     // [B][FX_SLOTS] bits of max|g_d_out| per simulation: slot k is WRITTEN by workgroup k of k3d_clear
    float *gdi, *giy, *gix, *giz;       // results
};

// gridDim.x == FX_SLOTS: every workgroup owns one absmax slot of its simulation and stores it (no atomics, nothing to clear beforehand).
// Sixteen waves per workgroup: 64 workgroups are all the parallelism a 3-D field of half a million cells gets here.
constexpr int K3D_CLEAR_T = 1024;
__global__ void __launch_bounds__(K3D_CLEAR_T) k3d_clear(K3DArgs a) {
    __shared__ unsigned red[K3D_CLEAR_T / 64];
    const int N = a.Y * a.X * a.Z, b = blockIdx.y;
    const float* g = a.gdo + (size_t)b * N;
    long long* z = a.gD + (size_t)b * N;
    float vmax = 0.f;
    bool bad = false;
    for (int c = blockIdx.x * K3D_CLEAR_T + threadIdx.x; c < N; c += FX_SLOTS * K3D_CLEAR_T) {
        z[c] = 0ll;
        const float v = fabsf(g[c]);
        vmax = fmaxf(vmax, v);
        bad |= !(v <= 3.402823466e38f);          // inf or nan (fmaxf drops a NaN)
    }
    const unsigned wmax = amax_wave_max(bad ? 0x7fc00000u : __float_as_uint(vmax));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wmax;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned m = 0u;
        for (int w = 0; w < K3D_CLEAR_T / 64; ++w) m = max(m, red[w]);
        a.gmax[b * FX_SLOTS + blockIdx.x] = m;
    }
}

// Where a field-term contribution goes (fx_add).  DGAdd: straight into the accumulators in global memory.  DTAdd: into the workgroup's LDS
// window when the target cell's column lies inside it, else into global memory.  The callers pass cells INSIDE the grid only.
struct DGAdd {
    long long* g;
    float qs;
    int X, Z;
    __device__ __forceinline__ long long* at(int jj, int ii, int kk) const { return g + ((size_t)jj * X + ii) * Z + kk; }
    __device__ __forceinline__ void operator()(int jj, int ii, int kk, float v) const { fx_add(at(jj, ii, kk), v, qs); }
};
struct DTAdd {
    DGAdd g;
    unsigned long long* L;         // [K3D_TW][K3D_TW][Z]
    int jw0, iw0;
    __device__ __forceinline__ void operator()(int jj, int ii, int kk, float v) const {
        const int lj = jj - jw0, li = ii - iw0;
        if ((unsigned)lj < (unsigned)K3D_TW && (unsigned)li < (unsigned)K3D_TW) fx_add(&L[(lj * K3D_TW + li) * g.Z + kk], v, g.qs);
        else g(jj, ii, kk, v);
    }
};

// adjoint of the advected density of cell (j, i, k) of simulation b.  The departure point is recomputed from the saved field with the
// forward step's expressions, operation for operation, so floorf decides as it did.  No fused multiply-adds: the two scatter kernels are
// held to the same bits by the test suite.
// ACC (stage B of the MacCormack adjoint): the back-trace term is added onto what gU holds (stage A's part) instead of written.
template <bool ACC, class Add>
__device__ __forceinline__ void k3d_point(const K3DArgs& a, int b, const float* sy, const float* sx, const float* sz, const Add& add, int j, int i, int k) {
#pragma clang fp contract(off)
    const int Y = a.Y, X = a.X, Z = a.Z;
    const size_t N = (size_t)Y * X * Z, c = ((size_t)j * X + i) * Z + k;
    const float g = a.gdo[(size_t)b * N + c];
    float guy = 0.f, gux = 0.f, guz = 0.f;
    if (g != 0.f) {
        const float* gd = a.d_in + (size_t)b * N;
        const float uy = 0.5f * (sy[c] + sy[c + (size_t)X * Z]);
        const float ux = 0.5f * (sx[((size_t)j * (X + 1) + i) * Z + k] + sx[((size_t)j * (X + 1) + i + 1) * Z + k]);
        const float uz = 0.5f * (sz[((size_t)j * X + i) * (Z + 1) + k] + sz[((size_t)j * X + i) * (Z + 1) + k + 1]);
        const float oy = -uy * a.dtdx, ox = -ux * a.dtdx, oz = -uz * a.dtdx;
        const float fy = floorf(oy), fx = floorf(ox), fz = floorf(oz);
        const float wy = oy - fy, wx = ox - fx, wz = oz - fz;
        const int j0 = j + (int)fy, i0 = i + (int)fx, k0 = k + (int)fz;
        float dy = 0.f, dx = 0.f, dz = 0.f;          // d(sample) / d(offset) along each axis
#pragma unroll
        for (int dj = 0; dj < 2; ++dj)
#pragma unroll
            for (int di = 0; di < 2; ++di)
#pragma unroll
                for (int dk = 0; dk < 2; ++dk) {
                    const int jj = j0 + dj, ii = i0 + di, kk = k0 + dk;
                    const float by = dj ? wy : 1.f - wy, bx = di ? wx : 1.f - wx, bz = dk ? wz : 1.f - wz;
                    float v = 0.f;   // one ring of zero ghost cells: it takes no gradient
                    if ((unsigned)jj < (unsigned)Y && (unsigned)ii < (unsigned)X && (unsigned)kk < (unsigned)Z) {
                        const size_t q = ((size_t)jj * X + ii) * Z + kk;
                        v = gd[q];
                        if (a.inflow_before) v += a.inflow[q];
                        add(jj, ii, kk, by * bx * bz * g);      // field term
                    }
                    dy += (dj ? 1.f : -1.f) * bx * bz * v;
                    dx += by * (di ? 1.f : -1.f) * bz * v;
                    dz += by * bx * (dk ? 1.f : -1.f) * v;
                }
        // back-trace term: offset_a = -dtdx * u_a(cell)
        guy = -a.dtdx * g * dy;
        gux = -a.dtdx * g * dx;
        guz = -a.dtdx * g * dz;
    }
    float *oy = a.gUy + (size_t)b * N + c, *ox = a.gUx + (size_t)b * N + c, *oz = a.gUz + (size_t)b * N + c;
    *oy = ACC ? *oy + guy : guy;
    *ox = ACC ? *ox + gux : gux;
    *oz = ACC ? *oz + guz : guz;
}

// every contribution a global int64 atomic (option k3d_dens_adj_tile = 0; the reference form of the tile kernel): one z column per wave
template <bool ACC>
__global__ void __launch_bounds__(256) k3d_advect_adj(K3DArgs a) {
    const int Y = a.Y, X = a.X, Z = a.Z;
    const size_t N = (size_t)Y * X * Z;
    const int b = blockIdx.y;
    const float* sy = a.svy + (size_t)b * (Y + 1) * X * Z;
    const float* sx = a.svx + (size_t)b * Y * (X + 1) * Z;
    const float* sz = a.svz + (size_t)b * Y * X * (Z + 1);
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    const DGAdd add{a.gD + (size_t)b * N, qs, X, Z};
    const int lane = threadIdx.x & 63;
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const int nwaves = gridDim.x * (blockDim.x >> 6);
    for (int c = wave0; c < Y * X; c += nwaves) {
        const int j = c / X, i = c % X;
        for (int k = lane; k < Z; k += 64) k3d_point<ACC>(a, b, sy, sx, sz, add, j, i, k);
    }
}

// The same scatter with an LDS window per workgroup: a workgroup owns 4 x 4 columns (all k), four columns per wave, and accumulates into an
// 8 x 8-column int64 window: the eight corners of a cell's gather lie within |u| dt/dx + 1 cells of it.  Integer adds commute: the result
// equals k3d_advect_adj's bit for bit.
template <bool ACC>
__global__ void __launch_bounds__(256) k3d_advect_adj_tile(K3DArgs a, int nti) {
    extern __shared__ __align__(16) unsigned long long smem_dens[];
    const int Y = a.Y, X = a.X, Z = a.Z;
    const size_t N = (size_t)Y * X * Z;
    const int b = blockIdx.y;
    const int tj = (int)blockIdx.x / nti, ti = (int)blockIdx.x % nti, j0 = tj * K3D_TJ, i0 = ti * K3D_TJ;
    const float* sy = a.svy + (size_t)b * (Y + 1) * X * Z;
    const float* sx = a.svx + (size_t)b * Y * (X + 1) * Z;
    const float* sz = a.svz + (size_t)b * Y * X * (Z + 1);
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    const DGAdd gadd{a.gD + (size_t)b * N, qs, X, Z};
    const DTAdd add{gadd, smem_dens, j0 - K3D_TH, i0 - K3D_TH};
    const int ncell = K3D_TW * K3D_TW * Z;
    fx_window_clear(smem_dens, ncell, 256);
    __syncthreads();
    const int j1 = min(j0 + K3D_TJ, Y), i1 = min(i0 + K3D_TJ, X);
    const int nI = i1 - i0, nC = (j1 - j0) * nI;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int t = wave; t < nC; t += 4) {
        const int j = j0 + t / nI, i = i0 + t % nI;
        for (int k = lane; k < Z; k += 64) k3d_point<ACC>(a, b, sy, sx, sz, add, j, i, k);
    }
    __syncthreads();
    // (window cells outside the grid never received a contribution: they are zero and their address is never formed)
    fx_window_flush(smem_dens, ncell, 256, [&](int e) {
        const int kk = e % Z, li = (e / Z) % K3D_TW, lj = e / (Z * K3D_TW);
        return gadd.at(j0 - K3D_TH + lj, i0 - K3D_TH + li, kk);
    });
}

__global__ void __launch_bounds__(256) k3d_diffuse_adj(K3DArgs a) {
#pragma clang fp contract(off)
    const int Y = a.Y, X = a.X, Z = a.Z, XP = X + 1, ZP = Z + 1, N = Y * X * Z;
    const int nVy = (Y + 1) * X * Z, nVx = Y * XP * Z, nVz = Y * X * ZP;
    const int b = blockIdx.y;
    const float alpha = a.adt / a.re[b];
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    const bool poisoned = qi != qi;                        // a non-finite g_d_out: every gradient of the simulation is NaN
    const float nan = __uint_as_float(0x7fc00000u);
    const float* uy = a.gUy + (size_t)b * N;
    const float* ux = a.gUx + (size_t)b * N;
    const float* uz = a.gUz + (size_t)b * N;
    const float* m = a.bcm + (size_t)b * a.bc_stride;
    // g' at a face of each component (karman3d_re.hpp: shared with the Reynolds-number reduction)
    auto gy = [&](int jf, int i, int k) { return k3d_face_y(uy, m, Y, X, Z, jf, i, k); };
    auto gx = [&](int j, int iF, int k) { return k3d_face_x(ux, X, Z, j, iF, k); };
    auto gz = [&](int j, int i, int kF) { return k3d_face_z(uz, X, Z, j, i, kF); };
    // g' + alpha L^T g': the transposed replicate-padded 7-point Laplacian in gather form (a direction that leaves the array contributes g'
    // of the face itself; neighbours in the order y +, y -, x +, x -, z +, z -), ONE fused multiply-add, spelled out
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nVy + nVx + nVz + N; e += gridDim.x * blockDim.x) {
        if (e < nVy) {
            const int k = e % Z, i = (e / Z) % X, j = e / (Z * X);
            const float v = gy(j, i, k);
            float acc = -6.f * v;
            acc += j + 1 < Y + 1 ? gy(j + 1, i, k) : v;
            acc += j > 0 ? gy(j - 1, i, k) : v;
            acc += i + 1 < X ? gy(j, i + 1, k) : v;
            acc += i > 0 ? gy(j, i - 1, k) : v;
            acc += k + 1 < Z ? gy(j, i, k + 1) : v;
            acc += k > 0 ? gy(j, i, k - 1) : v;
            const float r = poisoned ? nan : __fmaf_rn(alpha, acc, v);
            float* o = a.giy + (size_t)b * nVy + e;
            *o = a.accumulate ? *o + r : r;
        } else if (e < nVy + nVx) {
            const int q = e - nVy, k = q % Z, i = (q / Z) % XP, j = q / (Z * XP);
            const float v = gx(j, i, k);
            float acc = -6.f * v;
            acc += j + 1 < Y ? gx(j + 1, i, k) : v;
            acc += j > 0 ? gx(j - 1, i, k) : v;
            acc += i + 1 < XP ? gx(j, i + 1, k) : v;
            acc += i > 0 ? gx(j, i - 1, k) : v;
            acc += k + 1 < Z ? gx(j, i, k + 1) : v;
            acc += k > 0 ? gx(j, i, k - 1) : v;
            const float r = poisoned ? nan : __fmaf_rn(alpha, acc, v);
            float* o = a.gix + (size_t)b * nVx + q;
            *o = a.accumulate ? *o + r : r;
        } else if (e < nVy + nVx + nVz) {
            const int q = e - nVy - nVx, k = q % ZP, i = (q / ZP) % X, j = q / (ZP * X);
            const float v = gz(j, i, k);
            float acc = -6.f * v;
            acc += j + 1 < Y ? gz(j + 1, i, k) : v;
            acc += j > 0 ? gz(j - 1, i, k) : v;
            acc += i + 1 < X ? gz(j, i + 1, k) : v;
            acc += i > 0 ? gz(j, i - 1, k) : v;
            acc += k + 1 < ZP ? gz(j, i, k + 1) : v;
            acc += k > 0 ? gz(j, i, k - 1) : v;
            const float r = poisoned ? nan : __fmaf_rn(alpha, acc, v);
            float* o = a.giz + (size_t)b * nVz + q;
            *o = a.accumulate ? *o + r : r;
        } else {
            const int c = e - nVy - nVx - nVz;
            a.gdi[(size_t)b * N + c] = fx_get(a.gD + (size_t)b * N, c, qi);
        }
    }
}

// the workspace: g_d_in accumulators (int64), gU_y, gU_x, gU_z (fp32), the absmax slots; 256-byte granules; with re, the partial sums of
// the Reynolds-number reduction behind them
struct K3DLayout {
    long long* gD;
    float *gUy, *gUx, *gUz;
    unsigned* gmax;
    double* partial;
    size_t bytes;
    void* mc;                           // the _adv forms with the MacCormack advection: what sol_mc3_adj_den takes, behind everything else
};
K3DLayout k3d_layout(const sol_karman3d_cfg* c, bool re, void* ws, bool mc = false) {
    const size_t B = c->B, N = (size_t)c->Y * c->X * c->Z;
    Carve w(ws);
    K3DLayout l{w.take<long long>(B * N), w.take<float>(B * N), w.take<float>(B * N), w.take<float>(B * N), w.take<unsigned>(B * FX_SLOTS)};
    l.bytes = w.bytes();
    if (re) l.partial = sol_re3_partial_behind(w, c, &l.bytes);
    l.mc = mc ? k3_behind(ws, &l.bytes, sol_mc3_adj_den_bytes(c)) : nullptr;
    return l;
}

int grid_of(size_t n) { const size_t g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 65535 ? 65535 : g)); }

// the semi-Lagrangian advection adjoint of the density.  acc: the back-trace term is added onto gU (stage B of the MacCormack adjoint);
// tile: 1 the LDS-window kernel where the window fits, 0 global atomics, -1 as option k3d_dens_adj_tile says.  Same bits.
int launch_advect_adj(hipStream_t s, const K3DArgs& a, bool acc, int tile) {
    const int B = a.B, Y = a.Y, X = a.X, Z = a.Z;
    const size_t win = (size_t)K3D_TW * K3D_TW * Z * sizeof(unsigned long long);
    if ((tile < 0 ? sol_opt().k3d_dens_adj_tile != 0 : tile != 0) && win <= K3D_LDS_MAX) {
        const int ntj = (Y + K3D_TJ - 1) / K3D_TJ, nti = (X + K3D_TJ - 1) / K3D_TJ;
        if (acc) SOL_LAUNCH_NAMED("k3d_advect_adj_tile", k3d_advect_adj_tile<true>, dim3(ntj * nti, B), dim3(256), win, s, a, nti);
        else SOL_LAUNCH_NAMED("k3d_advect_adj_tile", k3d_advect_adj_tile<false>, dim3(ntj * nti, B), dim3(256), win, s, a, nti);
    } else {
        if (acc) SOL_LAUNCH_NAMED("k3d_advect_adj", k3d_advect_adj<true>, dim3(grid_of((size_t)Y * X * 64), B), dim3(256), 0, s, a);
        else SOL_LAUNCH_NAMED("k3d_advect_adj", k3d_advect_adj<false>, dim3(grid_of((size_t)Y * X * 64), B), dim3(256), 0, s, a);
    }
    return SOL_OK;
}

bool shape_ok(const sol_karman3d_cfg* c) { return c && c->B >= 1 && c->B <= 65535 && c->Y >= 8 && c->X >= 8 && c->Z >= 8; }

// the launches of sol_karman3d_density_bwd; with rx, followed by the Reynolds-number reduction over the gU they leave in the workspace
// (sol_karman3d_density_bwd_re): g_d_in / g_v*_in are the same launches' results either way
int density_bwd3d(const char* who, const sol_karman3d_cfg* c, void* stream,
                  const float* d_in, const float* inflow, const float* saved_vy, const float* saved_vx, const float* saved_vz,
                  const float* re, const float* velBCyMask, int64_t bc_batch_stride,
                  const float* g_d_out, float* g_d_in, float* g_vy_in, float* g_vx_in, float* g_vz_in, int accumulate,
                  void* workspace, size_t workspace_bytes, const Re3Extra* rx, const Adv3Extra* ax = nullptr) {
    SOL_REQUIRE(c != nullptr, "%s: cfg is NULL", who);
    if (ax)
        if (int e = sol_mc3_check(who, ax->advection, ax->strength)) return e;
    SOL_REQUIRE(shape_ok(c), "%s: B in [1, 65535], Y, X, Z >= 8 (got %d, %d, %d, %d)", who, c->B, c->Y, c->X, c->Z);
    SOL_REQUIRE((size_t)(c->Y + 1) * (c->X + 1) * (c->Z + 1) < ((size_t)1 << 28), "%s: grid too large for 32-bit face indices", who);
    SOL_REQUIRE(d_in && saved_vy && saved_vx && saved_vz && re && velBCyMask && g_d_out && g_d_in && g_vy_in && g_vx_in && g_vz_in && workspace,
                "%s: NULL pointer argument", who);
    SOL_REQUIRE(inflow || !c->inflow_before, "%s: cfg.inflow_before needs the inflow mask (the advected field is d_in + inflow)", who);
    SOL_REQUIRE(!rx || (rx->vy_in && rx->vx_in && rx->vz_in && rx->g_re), "%s: NULL pointer argument", who);
    const int B = c->B, Y = c->Y, X = c->X, Z = c->Z;
    const size_t N = (size_t)Y * X * Z, faces = (size_t)(Y + 1) * X * Z + (size_t)Y * (X + 1) * Z + (size_t)Y * X * (Z + 1);
    SOL_REQUIRE(faces % 2 == 0, "%s: odd face count (%zu): even X, Z expected", who, faces);
    SOL_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    const K3DLayout l = k3d_layout(c, rx != nullptr, workspace, ax && ax->advection == 1);
    SOL_REQUIRE(workspace_bytes >= l.bytes, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, l.bytes);
    const void* outs[] = {g_d_in, g_vy_in, g_vx_in, g_vz_in, rx ? rx->g_re : nullptr};
    const void* ins[] = {d_in, inflow, saved_vy, saved_vx, saved_vz, re, velBCyMask, g_d_out,
                         rx ? rx->vy_in : nullptr, rx ? rx->vx_in : nullptr, rx ? rx->vz_in : nullptr};
    for (const void* o : outs)
        for (const void* i : ins) SOL_REQUIRE(!o || o != i, "%s: outputs must not alias the inputs", who);
    for (int p = 0; p < 5; ++p)
        for (int q = p + 1; q < 5; ++q) SOL_REQUIRE(!outs[q] || outs[p] != outs[q], "%s: g_d_in, g_v*_in and g_re must be buffers of their own", who);
    hipStream_t s = (hipStream_t)stream;
    K3DArgs a{};
    a.B = B; a.Y = Y; a.X = X; a.Z = Z; a.dtdx = c->dt / c->dx; a.adt = c->dt * c->res * c->res;
    a.inflow_before = c->inflow_before; a.accumulate = accumulate != 0;
    a.d_in = d_in; a.inflow = inflow; a.svy = saved_vy; a.svx = saved_vx; a.svz = saved_vz; a.re = re; a.bcm = velBCyMask; a.bc_stride = bc_batch_stride;
    a.gdo = g_d_out;
    a.gD = l.gD; a.gUy = l.gUy; a.gUx = l.gUx; a.gUz = l.gUz; a.gmax = l.gmax;
    a.gdi = g_d_in; a.giy = g_vy_in; a.gix = g_vx_in; a.giz = g_vz_in;
    SOL_LAUNCH(k3d_clear, dim3(FX_SLOTS, B), dim3(K3D_CLEAR_T), 0, s, a);
    if (ax && ax->advection == 1) {
        if (int e = sol_mc3_adj_den(c, s, ax->strength, d_in, inflow, saved_vy, saved_vx, saved_vz, g_d_out, l.gmax, l.gD, l.gUy, l.gUx, l.gUz, l.mc, -1)) return e;
    } else if (int e = launch_advect_adj(s, a, false, -1)) return e;
    SOL_LAUNCH(k3d_diffuse_adj, dim3(grid_of(faces + N), B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    if (!rx) return SOL_OK;
    // g' of the Reynolds-number gradient = the face values k3d_diffuse_adj has just formed from gU
    Re3In in{};
    in.src = RE3_GU;
    in.gUy = l.gUy; in.gUx = l.gUx; in.gUz = l.gUz; in.gmax = l.gmax; in.bcm = velBCyMask; in.bc_stride = bc_batch_stride;
    in.vy_in = rx->vy_in; in.vx_in = rx->vx_in; in.vz_in = rx->vz_in; in.re = re;
    in.partial = l.partial;
    in.g_re = rx->g_re; in.accumulate = rx->accumulate;
    return sol_re3_reduce(s, c, in);
}

}  // namespace

extern "C" size_t sol_karman3d_density_bwd_workspace_bytes(const sol_karman3d_cfg* c) {
    if (!shape_ok(c)) return 0;
    return k3d_layout(c, false, nullptr).bytes;
}

extern "C" int sol_karman3d_density_bwd(const sol_karman3d_cfg* c, void* stream,
                                        const float* d_in, const float* inflow, const float* saved_vy, const float* saved_vx, const float* saved_vz,
                                        const float* re, const float* velBCyMask, int64_t bc_batch_stride,
                                        const float* g_d_out, float* g_d_in, float* g_vy_in, float* g_vx_in, float* g_vz_in, int accumulate,
                                        void* workspace, size_t workspace_bytes) {
    return density_bwd3d("sol_karman3d_density_bwd", c, stream, d_in, inflow, saved_vy, saved_vx, saved_vz, re, velBCyMask, bc_batch_stride,
                         g_d_out, g_d_in, g_vy_in, g_vx_in, g_vz_in, accumulate, workspace, workspace_bytes, nullptr);
}

extern "C" size_t sol_karman3d_density_bwd_re_workspace_bytes(const sol_karman3d_cfg* c) {
    if (!shape_ok(c)) return 0;
    return k3d_layout(c, true, nullptr).bytes;
}

extern "C" int sol_karman3d_density_bwd_re(const sol_karman3d_cfg* c, void* stream,
                                           const float* d_in, const float* inflow, const float* saved_vy, const float* saved_vx, const float* saved_vz,
                                           const float* re, const float* velBCyMask, int64_t bc_batch_stride,
                                           const float* g_d_out, float* g_d_in, float* g_vy_in, float* g_vx_in, float* g_vz_in, int accumulate,
                                           void* workspace, size_t workspace_bytes,
                                           const float* vy_in, const float* vx_in, const float* vz_in, float* g_re, int accumulate_re) {
    const Re3Extra rx{vy_in, vx_in, vz_in, g_re, accumulate_re};
    return density_bwd3d("sol_karman3d_density_bwd_re", c, stream, d_in, inflow, saved_vy, saved_vx, saved_vz, re, velBCyMask, bc_batch_stride,
                         g_d_out, g_d_in, g_vy_in, g_vx_in, g_vz_in, accumulate, workspace, workspace_bytes, &rx);
}

// The _adv forms: every argument of the plain / _re form, then the advection the forward step ran (0: semi-Lagrangian -- that form's
// launches, bits and workspace size; 1: MacCormack -- sol_mc3_adj_den in place of k3d_advect_adj*) and its correction strength.
extern "C" size_t sol_karman3d_density_bwd_adv_workspace_bytes(const sol_karman3d_cfg* c, int32_t with_re, int32_t advection) {
    if (!shape_ok(c)) return 0;
    return k3d_layout(c, with_re != 0, nullptr, advection == 1).bytes;
}

extern "C" int sol_karman3d_density_bwd_adv(const sol_karman3d_cfg* c, void* stream,
                                            const float* d_in, const float* inflow, const float* saved_vy, const float* saved_vx, const float* saved_vz,
                                            const float* re, const float* velBCyMask, int64_t bc_batch_stride,
                                            const float* g_d_out, float* g_d_in, float* g_vy_in, float* g_vx_in, float* g_vz_in, int accumulate,
                                            void* workspace, size_t workspace_bytes, int32_t advection, float correction_strength) {
    const Adv3Extra ax{advection, correction_strength};
    return density_bwd3d("sol_karman3d_density_bwd_adv", c, stream, d_in, inflow, saved_vy, saved_vx, saved_vz, re, velBCyMask, bc_batch_stride,
                         g_d_out, g_d_in, g_vy_in, g_vx_in, g_vz_in, accumulate, workspace, workspace_bytes, nullptr, &ax);
}

extern "C" int sol_karman3d_density_bwd_adv_re(const sol_karman3d_cfg* c, void* stream,
                                               const float* d_in, const float* inflow, const float* saved_vy, const float* saved_vx, const float* saved_vz,
                                               const float* re, const float* velBCyMask, int64_t bc_batch_stride,
                                               const float* g_d_out, float* g_d_in, float* g_vy_in, float* g_vx_in, float* g_vz_in, int accumulate,
                                               void* workspace, size_t workspace_bytes,
                                               const float* vy_in, const float* vx_in, const float* vz_in, float* g_re, int accumulate_re,
                                               int32_t advection, float correction_strength) {
    const Re3Extra rx{vy_in, vx_in, vz_in, g_re, accumulate_re};
    const Adv3Extra ax{advection, correction_strength};
    return density_bwd3d("sol_karman3d_density_bwd_adv_re", c, stream, d_in, inflow, saved_vy, saved_vx, saved_vz, re, velBCyMask, bc_batch_stride,
                         g_d_out, g_d_in, g_vy_in, g_vx_in, g_vz_in, accumulate, workspace, workspace_bytes, &rx, &ax);
}

// the semi-Lagrangian adjoint of the density alone (stage B of the MacCormack adjoint; sol_karman3d_advect_bwd with advection = 0)
int sol_k3d_advect_adj(const sol_karman3d_cfg* c, hipStream_t s, const float* d_in, const float* inflow, const float* svy, const float* svx, const float* svz,
                       const float* g, const unsigned* gmax, long long* gD, float* gUy, float* gUx, float* gUz, bool add_gU, int tile) {
    K3DArgs a{};
    a.B = c->B; a.Y = c->Y; a.X = c->X; a.Z = c->Z; a.dtdx = c->dt / c->dx; a.inflow_before = c->inflow_before;
    a.d_in = d_in; a.inflow = inflow; a.svy = svy; a.svx = svx; a.svz = svz;
    a.gdo = g; a.gD = gD; a.gUy = gUy; a.gUx = gUx; a.gUz = gUz; a.gmax = const_cast<unsigned*>(gmax);
    if (int e = launch_advect_adj(s, a, add_gU, tile)) return e;
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}
