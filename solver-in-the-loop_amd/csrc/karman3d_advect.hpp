// karman-3d: what the advection adjoint of the step (karman3d.hip, k3b_advect_adj*) shares with the MacCormack advection
// (karman3d_maccormack.hip): the reader of the post-diffusion velocity, the velocity at an array's sample point and the transpose of
// forming it, the fixed-point adders, and the semi-Lagrangian adjoint of one face value.  ONE spelling of each: the MacCormack kernels
// must take every decision (floor, clamp, limiter) as the forward step took it.  Below them, the launchers the three files call across.
#pragma once
#include "fixed_scatter.hpp"
#include "karman3d_mask.hpp"

// the arguments of the forward step's kernels (karman3d.hip; the z-periodic forms of karman3d_periodic.hip take the same value)
struct K3Args {
    int B, Y, X, Z;
    float dtdx, dt, adt;
    int grad_pad, inflow_before;
    const float *d_in, *vy_in, *vx_in, *vz_in, *re, *active, *inflow, *bcv, *bcm;
    long bc_stride;
    float *d_out, *vy_out, *vx_out, *vz_out, *svy, *svx, *svz, *rhs, *feat;
    const float* p;
    float fs0, fs1, fs2, fs3;
};

namespace {

// ---- reader of the diffused components straight from global memory -------------------------------------------------------------------
struct GlobalReader {
    const float *sy, *sx, *sz;
    const float* act;                 // the scene's `active` cell mask [Y][X][Z]
    int Y, X, Z;
    // accessible mask at a cell index that may lie one cell outside the domain ('boundary' extrapolation: edge value)
    __device__ __forceinline__ float acc(int j, int i, int k) const { return acc_at(act, Y, X, Z, j, i, k); }
    __device__ __forceinline__ float y(int j, int i, int k) const { return sy[((size_t)j * X + i) * Z + k]; }
    __device__ __forceinline__ float x(int j, int i, int k) const { return sx[((size_t)j * (X + 1) + i) * Z + k]; }
    __device__ __forceinline__ float z(int j, int i, int k) const { return sz[((size_t)j * X + i) * (Z + 1) + k]; }
};
struct GR : GlobalReader {
    __device__ __forceinline__ int g_Y() const { return Y; }
    __device__ __forceinline__ int g_X() const { return X; }
    __device__ __forceinline__ int g_Z() const { return Z; }
};

// ---- reader of the diffused components from the workgroup's LDS tile (k3_advect_tile, k3p_advect_tile) ----------------------------------
constexpr int T3 = 8;         // tile edge (cells) in y and x
constexpr int HL3 = 2;         // halo cells
constexpr int TR = T3 + 2 * HL3;      // cell rows / columns of the tile region (12); face arrays have one more along their axis
constexpr int ADV_T = 1024;      // 16 waves per workgroup: the tile kernel owns a CU (117 KB of LDS), its gathers are latency bound
struct TileReader {
    GlobalReader g;
    const float *ly, *lx, *lz;        // LDS: [TR+1][TR][Z], [TR][TR+1][Z], [TR][TR][Z+1]
    const unsigned char* la;          // LDS: accessible mask of the region's cells [TR][TR][Z] (bytes; rows / columns beyond the domain hold the edge value)
    int j0, i0;                       // first cell row / column of the region (may be negative: clipped rows are never read)
    __device__ __forceinline__ float acc(int j, int i, int k) const {
        const int rj = j - j0, ri = i - i0, kk = clampi(k, 0, g.Z - 1);
        return ((unsigned)rj < (unsigned)TR && (unsigned)ri < (unsigned)TR) ? (float)la[(rj * TR + ri) * g.Z + kk] : g.acc(j, i, k);
    }
    __device__ __forceinline__ float y(int j, int i, int k) const {
        const int rj = j - j0, ri = i - i0;
        return ((unsigned)rj <= (unsigned)TR && (unsigned)ri < (unsigned)TR) ? ly[(rj * TR + ri) * g.Z + k] : g.y(j, i, k);
    }
    __device__ __forceinline__ float x(int j, int i, int k) const {
        const int rj = j - j0, ri = i - i0;
        return ((unsigned)rj < (unsigned)TR && (unsigned)ri <= (unsigned)TR) ? lx[(rj * (TR + 1) + ri) * g.Z + k] : g.x(j, i, k);
    }
    __device__ __forceinline__ float z(int j, int i, int k) const {
        const int rj = j - j0, ri = i - i0;
        return ((unsigned)rj < (unsigned)TR && (unsigned)ri < (unsigned)TR) ? lz[(rj * TR + ri) * (g.Z + 1) + k] : g.z(j, i, k);
    }
};
struct TRd : TileReader {
    __device__ __forceinline__ int g_Y() const { return g.Y; }
    __device__ __forceinline__ int g_X() const { return g.X; }
    __device__ __forceinline__ int g_Z() const { return g.Z; }
};

}  // namespace

// the arguments of the adjoint's kernels (karman3d.hip; the z-periodic forms of karman3d_periodic.hip take the same value)
struct K3BArgs {
    int B, Y, X, Z;
    float dtdx, adt;
    int grad_pad;
    const float *re, *active, *bcm;
    long bc_stride;
    const float *svy, *svx, *svz;           // saved post-diffusion velocity
    const float *goy, *gox, *goz;           // gradient w.r.t. the step's output velocity
    float *gay, *gax, *gaz;                 // g_a
    long long *gcy, *gcx, *gcz;             // g_c: int64 fixed-point accumulators (zeroed by k3b_rhs before the scatter)
    unsigned* gmax;                         // [B][FX_SLOTS] bits of max|g_a| per simulation (zeroed by k3b_rhs, published by k3b_gva)
    float *giy, *gix, *giz;                 // result: gradient w.r.t. the step's input velocity
    float* rhs;
    const float* gdiv;
};

namespace {

// Where a contribution goes (fx_add).  GAdd: straight into the int64 accumulators in global memory.  TAdd (k3b_advect_adj_tile): into the
// workgroup's int64 LDS window when the target face lies inside it, else into global memory.
struct GAdd {
    long long *gy, *gx, *gz;
    float qs;
    int X, Z;
    __device__ __forceinline__ long long* at(int comp, int jj, int ii, int kk) const {
        return comp == 0 ? gy + ((size_t)jj * X + ii) * Z + kk : (comp == 1 ? gx + ((size_t)jj * (X + 1) + ii) * Z + kk : gz + ((size_t)jj * X + ii) * (Z + 1) + kk);
    }
    __device__ __forceinline__ void operator()(int comp, int jj, int ii, int kk, float v) const { fx_add(at(comp, jj, ii, kk), v, qs); }
};
constexpr int K3B_TJ = 4, K3B_TH = 2, K3B_TW = K3B_TJ + 2 * K3B_TH;      // tile of 4 x 4 columns, window of 8 x 8 columns (halo 2: CFL < 2)
struct TAdd {
    GAdd g;
    unsigned long long* L;         // [3][K3B_TW][K3B_TW][ZP]
    int jw0, iw0, ZP;
    __device__ __forceinline__ void operator()(int comp, int jj, int ii, int kk, float v) const {
        const int lj = jj - jw0, li = ii - iw0;
        if ((unsigned)lj < (unsigned)K3B_TW && (unsigned)li < (unsigned)K3B_TW) fx_add(&L[((comp * K3B_TW + lj) * K3B_TW + li) * ZP + kk], v, g.qs);
        else g(comp, jj, ii, kk, v);
    }
};

// The velocity at the sample point of face (j, i, k) of component C, exactly as the forward pass forms it: the own component is the stored
// value, the others the averages of their four surrounding faces with clamped indices; na / nb = the two clamped indices along C's own axis
struct AdvU {
    float uy, ux, uz;
    int na, nb;
};
template <int C>
__device__ __forceinline__ AdvU adv3_u(const GR& r, int j, int i, int k) {
#pragma clang fp contract(off)
    const int Y = r.Y, X = r.X, Z = r.Z;
    AdvU u;
    if (C == 0) {
        const int ja = max(j - 1, 0), jb = min(j, Y - 1);
        u.na = ja; u.nb = jb;
        u.uy = r.y(j, i, k);
        u.ux = 0.25f * (r.x(ja, i, k) + r.x(ja, i + 1, k) + r.x(jb, i, k) + r.x(jb, i + 1, k));
        u.uz = 0.25f * (r.z(ja, i, k) + r.z(ja, i, k + 1) + r.z(jb, i, k) + r.z(jb, i, k + 1));
    } else if (C == 1) {
        const int ia = max(i - 1, 0), ib = min(i, X - 1);
        u.na = ia; u.nb = ib;
        u.ux = r.x(j, i, k);
        u.uy = 0.25f * (r.y(j, ia, k) + r.y(j, ib, k) + r.y(j + 1, ia, k) + r.y(j + 1, ib, k));
        u.uz = 0.25f * (r.z(j, ia, k) + r.z(j, ia, k + 1) + r.z(j, ib, k) + r.z(j, ib, k + 1));
    } else {
        const int ka = max(k - 1, 0), kb = min(k, Z - 1);
        u.na = ka; u.nb = kb;
        u.uz = r.z(j, i, k);
        u.uy = 0.25f * (r.y(j, i, ka) + r.y(j, i, kb) + r.y(j + 1, i, ka) + r.y(j + 1, i, kb));
        u.ux = 0.25f * (r.x(j, i, ka) + r.x(j, i, kb) + r.x(j, i + 1, ka) + r.x(j, i + 1, kb));
    }
    return u;
}
// the transpose of adv3_u: (guy, gux, guz), the gradient with respect to the velocity at the sample point, onto the nine samples that formed it
template <int C, class Add>
__device__ __forceinline__ void adv3_u_scatter(const Add& add, const AdvU& u, int j, int i, int k, float guy, float gux, float guz) {
#pragma clang fp contract(off)
    if (C == 0) {
        const int ja = u.na, jb = u.nb;
        add(0, j, i, k, guy);
        const float qx = 0.25f * gux, qz = 0.25f * guz;
        add(1, ja, i, k, qx); add(1, ja, i + 1, k, qx); add(1, jb, i, k, qx); add(1, jb, i + 1, k, qx);
        add(2, ja, i, k, qz); add(2, ja, i, k + 1, qz); add(2, jb, i, k, qz); add(2, jb, i, k + 1, qz);
    } else if (C == 1) {
        const int ia = u.na, ib = u.nb;
        add(1, j, i, k, gux);
        const float qy = 0.25f * guy, qz = 0.25f * guz;
        add(0, j, ia, k, qy); add(0, j, ib, k, qy); add(0, j + 1, ia, k, qy); add(0, j + 1, ib, k, qy);
        add(2, j, ia, k, qz); add(2, j, ia, k + 1, qz); add(2, j, ib, k, qz); add(2, j, ib, k + 1, qz);
    } else {
        const int ka = u.na, kb = u.nb;
        add(2, j, i, k, guz);
        const float qy = 0.25f * guy, qx = 0.25f * gux;
        add(0, j, i, ka, qy); add(0, j, i, kb, qy); add(0, j + 1, i, ka, qy); add(0, j + 1, i, kb, qy);
        add(1, j, i, ka, qx); add(1, j, i, kb, qx); add(1, j, i + 1, ka, qx); add(1, j, i + 1, kb, qx);
    }
}

// adjoint of one advected face value of component C at (j, i, k): gs = g_a there
template <int C, class Add>
__device__ __forceinline__ void advect_adj_point(const K3BArgs& a, const GR& r, const Add& add, int j, int i, int k, float gs) {
    // no fused multiply-adds here: which products the compiler contracts depends on the kernel this is inlined into, and the two scatter
    // kernels (global atomics / LDS window) are held to the SAME BITS by the test suite (the integer accumulation is exact, so the only
    // freedom is in the fp32 contributions themselves)
#pragma clang fp contract(off)
    const int Y = a.Y, X = a.X, Z = a.Z;
    // velocity at the sample point, exactly as the forward pass forms it
    const AdvU u = adv3_u<C>(r, j, i, k);
    const float oy = -u.uy * a.dtdx, ox = -u.ux * a.dtdx, oz = -u.uz * a.dtdx;
    const int n0 = Y + (C == 0), n1 = X + (C == 1), n2 = Z + (C == 2);
    const float fy = floorf(oy), fx = floorf(ox), fz = floorf(oz);
    const float wy = oy - fy, wx = ox - fx, wz = oz - fz;
    const int j0 = clampi(j + (int)fy, 0, n0 - 1), j1 = clampi(j + (int)fy + 1, 0, n0 - 1);
    const int i0 = clampi(i + (int)fx, 0, n1 - 1), i1 = clampi(i + (int)fx + 1, 0, n1 - 1);
    const int k0 = clampi(k + (int)fz, 0, n2 - 1), k1 = clampi(k + (int)fz + 1, 0, n2 - 1);
    auto val = [&](int jj, int ii, int kk) { return C == 0 ? r.y(jj, ii, kk) : (C == 1 ? r.x(jj, ii, kk) : r.z(jj, ii, kk)); };
    float dy = 0.f, dx = 0.f, dz = 0.f;          // d(sample) / d(offset) along each axis
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
    // back-trace term: offset_a = -dtdx * u_a(x0)
    adv3_u_scatter<C>(add, u, j, i, k, -a.dtdx * gs * dy, -a.dtdx * gs * dx, -a.dtdx * gs * dz);
}

// the _adv forms' extra: which advection the forward step ran (1: MacCormack, karman3d_maccormack.hip) and its correction strength
struct Adv3Extra {
    int32_t advection;
    float strength;
};

// a part of n bytes behind a layout that ends *bytes past the caller's pointer (the part aligns itself: Carve(ws)); ws NULL: sizes only
inline void* k3_behind(void* ws, size_t* bytes, size_t n) {
    void* p = ws ? static_cast<char*>(ws) + *bytes : nullptr;
    *bytes += n;
    return p;
}

}  // namespace

// ---- launchers across the three files (no synchronisation, no allocation, kernel nodes only) -------------------------------------------
// tile: 1 = the LDS-window kernel where the grid admits it, 0 = global atomics only, -1 = as the option (k3d_adj_tile / k3d_dens_adj_tile) says
// karman3d.hip: the plain advection launch on a given post-diffusion velocity (d_out NULL: the velocity alone), and the semi-Lagrangian
// adjoint of the velocity: g_a (its max in gmax) scattered onto the int64 g_c
int sol_k3_advect(const sol_karman3d_cfg* c, hipStream_t s, const float* d_in, const float* svy, const float* svx, const float* svz, const float* active,
                  const float* inflow, float* d_out, float* vy_out, float* vx_out, float* vz_out);
int sol_k3b_advect_adj(const sol_karman3d_cfg* c, hipStream_t s, const float* svy, const float* svx, const float* svz, const float* gay, const float* gax,
                       const float* gaz, const unsigned* gmax, long long* gcy, long long* gcx, long long* gcz, int tile);
// karman3d_periodic.hip: the stencil launches of the forward step on a z-periodic blob (header word 6 = SOL_K3_PERIODIC_Z): diffusion,
// advection and divergence before the pressure solve, the projection after it
int sol_k3p_front(hipStream_t s, const K3Args& a);
int sol_k3p_project(hipStream_t s, const K3Args& a);
// ... and of its adjoint: the right-hand side of the second solve (it also clears the fixed-point accumulators), then, with a.gdiv set,
// g_a, the fixed-point scatter (tile as above) and the diffusion adjoint
int sol_k3pb_rhs(hipStream_t s, const K3BArgs& a);
int sol_k3pb_back(hipStream_t s, const K3BArgs& a, int tile);
// karman3d_density_bwd.hip: the semi-Lagrangian adjoint of the density: g (its max in gmax) scattered onto the int64 gD, the back-trace
// term written to gU (add_gU: added onto what gU holds)
int sol_k3d_advect_adj(const sol_karman3d_cfg* c, hipStream_t s, const float* d_in, const float* inflow, const float* svy, const float* svx, const float* svz,
                       const float* g, const unsigned* gmax, long long* gD, float* gUy, float* gUx, float* gUz, bool add_gU, int tile);
// karman3d_maccormack.hip: the MacCormack advection in place of the plain launch (ws: sol_mc3_bytes), its velocity adjoint in place of
// k3b_advect_adj* (ws: sol_mc3_adj_vel_bytes) and its density adjoint in place of k3d_advect_adj* (gU written; ws: sol_mc3_adj_den_bytes);
// sol_mc3_check: the two arguments of the _adv entry points
int sol_mc3_check(const char* who, int32_t advection, float strength);
size_t sol_mc3_bytes(const sol_karman3d_cfg* c);
int sol_mc3_advect(const sol_karman3d_cfg* c, hipStream_t s, float strength, const float* d_in, const float* svy, const float* svx, const float* svz,
                   const float* active, const float* inflow, float* d_out, float* vy_out, float* vx_out, float* vz_out, void* ws);
size_t sol_mc3_adj_vel_bytes(const sol_karman3d_cfg* c);
int sol_mc3_adj_vel(const sol_karman3d_cfg* c, hipStream_t s, float strength, const float* svy, const float* svx, const float* svz, const float* gay,
                    const float* gax, const float* gaz, const unsigned* gmax, long long* gcy, long long* gcx, long long* gcz, void* ws, int tile);
size_t sol_mc3_adj_den_bytes(const sol_karman3d_cfg* c);
int sol_mc3_adj_den(const sol_karman3d_cfg* c, hipStream_t s, float strength, const float* d_in, const float* inflow, const float* svy, const float* svx,
                    const float* svz, const float* g_d_out, const unsigned* gmax, long long* gD, float* gUy, float* gUx, float* gUz, void* ws, int tile);
