// MacCormack advection of the karman-3d step (advection = 1 on the _adv entry points; include/sol_hip.h, "MACCORMACK ADVECTION on the
// karman-3d step"), forward and adjoint: the 3-D twin of karman_maccormack.hip.  c = (sv_y, sv_x, sv_z) is the post-diffusion velocity, f
// one advected array of kind K -- 0 / 1 / 2: c_y / c_x / c_z on its own faces, 3: the density on cells (+ inflow first when
// cfg.inflow_before) -- u the velocity at the array's sample point by advect_point's expressions (adv3_u, karman3d_advect.hpp; cells: the
// two-face means), S_g the trilinear sample of g in the array's own mode (index clamp for the velocity, one ring of zero ghost cells for
// the density):
//   h(x)   = S_f(x - u dt)                 the semi-Lagrangian value              (mc3_hat)
//   b(x)   = S_h(x + u dt)                 h carried back with the same u
//   cor(x) = h(x) + (s / 2) (f(x) - b(x))
//   out(x) = cor(x) if lo <= cor(x) <= hi else h(x),   lo, hi = min, max of the EIGHT values the first gather read (after clamping; ghost
//            zeros count); the compare is inclusive and a NaN reverts to h
// then as k3_advect: velocity x hard-BC face mask, density + inflow dt when the inflow comes after.
//
// FORWARD, two launches: k3m_hat writes h of the four arrays to the workspace, k3m_out gathers b from it, forms lo / hi / cor, applies
// the limiter, mask and inflow.  h at a point is ONE spelled-out expression (contraction off) wherever it is evaluated.
//
// ADJOINT: the derivative with every decision frozen as the forward step took it (the floorf's, the clamps, the limiter), recomputed from
// the saved c -- the forward step saves nothing new.  For a cotangent g of out (the velocity's is g_a, masked already) and kept = 1 where
// cor was kept:
//   stage A (k3m_vel_adj, k3m_den_adj)   g_b = -(s/2) kept g:  g_f += (s/2) kept g;  g_b scattered through the eight corners of the gather
//                                         at x + u dt into the accumulators G_h;  g_u += +(dt/dx) g_b dS_h/d(offset)
//   stage B                               the EXISTING semi-Lagrangian adjoint (k3b_advect_adj*, k3d_advect_adj*) of g_h = g + G_h
//                                         (k3m_gh converts): field term into g_f, back-trace term -(dt/dx) g_h dS_f/d(offset) into g_u
// g_u of a velocity face goes onto the nine velocity samples that formed u (adv3_u_scatter), g_u of a density cell is the per-cell gU that
// k3d_diffuse_adj takes (stage A writes it, stage B adds onto it).  Where a point reverted, its adjoint is the plain semi-Lagrangian one.
// g_f of the velocity is g_c, of the density g_d_in.  Every scattered sum -- g_c, g_d_in and G_h -- is 64-bit fixed point with the ONE
// scale of its cotangent (fixed_scatter.hpp), so the adjoint is reproducible bit for bit; stage A adds with global atomics, stage B as its
// options (k3d_adj_tile, k3d_dens_adj_tile) say.  A non-finite cotangent poisons its simulation as it does in the semi-Lagrangian adjoints.
// The accumulators G_h are cleared by a kernel: no host synchronisation, no allocation, kernel nodes only under capture.
// Work unit of every kernel: one z column (fixed kind, j, i) per wave, lanes along z; j, i and what derives from them are wave uniform.
// Every index that reaches memory is clamped to its array or range-checked (the zero ghost ring), whatever the velocity holds.
#include "carve.hpp"
#include "fixed_scatter.hpp"
#include "karman3d_advect.hpp"

namespace {

struct Mc3Args {
    int Y, X, Z, inflow_before, with_v, with_d;
    float dtdx, dt, hs;                     // hs = correction_strength / 2
    const float *d_in, *svy, *svx, *svz, *active, *inflow;
    float *d_out, *vy_out, *vx_out, *vz_out;
    float* h[4];                            // h of the four arrays [B][...]
};

template <int K> __device__ __forceinline__ int mc3_n0(const Mc3Args& a) { return a.Y + (K == 0); }
template <int K> __device__ __forceinline__ int mc3_n1(const Mc3Args& a) { return a.X + (K == 1); }
template <int K> __device__ __forceinline__ int mc3_n2(const Mc3Args& a) { return a.Z + (K == 2); }
template <int K> __device__ __forceinline__ size_t mc3_count(const Mc3Args& a) { return (size_t)mc3_n0<K>(a) * mc3_n1<K>(a) * mc3_n2<K>(a); }

// the arrays of simulation b
struct Mc3Sim {
    GR r;
    const float* d;
};
__device__ __forceinline__ Mc3Sim mc3_sim(const Mc3Args& a, int b) {
    const size_t Y = a.Y, X = a.X, Z = a.Z;
    Mc3Sim m;
    m.r.sy = a.svy + b * (Y + 1) * X * Z; m.r.sx = a.svx + b * Y * (X + 1) * Z; m.r.sz = a.svz + b * Y * X * (Z + 1);
    m.r.act = a.active; m.r.Y = a.Y; m.r.X = a.X; m.r.Z = a.Z;
    m.d = a.with_d ? a.d_in + b * Y * X * Z : nullptr;
    return m;
}

// u at the sample point (j, i, k) of an array of kind K
template <int K>
__device__ __forceinline__ void mc3_u(const Mc3Sim& m, int j, int i, int k, float& uy, float& ux, float& uz) {
#pragma clang fp contract(off)
    if (K < 3) {
        const AdvU u = adv3_u<(K < 3 ? K : 0)>(m.r, j, i, k);
        uy = u.uy; ux = u.ux; uz = u.uz;
    } else {
        uy = 0.5f * (m.r.y(j, i, k) + m.r.y(j + 1, i, k));
        ux = 0.5f * (m.r.x(j, i, k) + m.r.x(j, i + 1, k));
        uz = 0.5f * (m.r.z(j, i, k) + m.r.z(j, i, k + 1));
    }
}

// f at an index INSIDE its array
template <int K>
__device__ __forceinline__ float mc3_f(const Mc3Args& a, const Mc3Sim& m, int jj, int ii, int kk) {
#pragma clang fp contract(off)
    if (K == 0) return m.r.y(jj, ii, kk);
    if (K == 1) return m.r.x(jj, ii, kk);
    if (K == 2) return m.r.z(jj, ii, kk);
    const size_t q = ((size_t)jj * a.X + ii) * a.Z + kk;
    float v = m.d[q];
    if (a.inflow_before) v += a.inflow[q];
    return v;
}

// the eight corners of the trilinear gather at (j + oy, i + ox, k + oz) in an array of kind K: indices per axis, their weights, and whether
// an index lies inside the array (velocity: always, the indices are clamped; density: outside = the zero ghost ring)
struct Mc3C {
    int jj[2], ii[2], kk[2];
    bool jin[2], iin[2], kin[2];
    float wy, wx, wz;
};
template <int K>
__device__ __forceinline__ Mc3C mc3_corners(const Mc3Args& a, int j, int i, int k, float oy, float ox, float oz) {
#pragma clang fp contract(off)
    const int n0 = mc3_n0<K>(a), n1 = mc3_n1<K>(a), n2 = mc3_n2<K>(a);
    const float fy = floorf(oy), fx = floorf(ox), fz = floorf(oz), big = 268435456.f;      // 2^28: beyond any grid, and j + 2^28 stays an int
    Mc3C s;
    s.wy = oy - fy; s.wx = ox - fx; s.wz = oz - fz;
    const int jf = j + (int)fminf(fmaxf(fy, -big), big), iF = i + (int)fminf(fmaxf(fx, -big), big), kf = k + (int)fminf(fmaxf(fz, -big), big);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (K < 3) {
            s.jj[c] = clampi(jf + c, 0, n0 - 1); s.ii[c] = clampi(iF + c, 0, n1 - 1); s.kk[c] = clampi(kf + c, 0, n2 - 1);
            s.jin[c] = s.iin[c] = s.kin[c] = true;
        } else {
            s.jj[c] = jf + c; s.ii[c] = iF + c; s.kk[c] = kf + c;
            s.jin[c] = (unsigned)s.jj[c] < (unsigned)n0; s.iin[c] = (unsigned)s.ii[c] < (unsigned)n1; s.kin[c] = (unsigned)s.kk[c] < (unsigned)n2;
        }
    }
    return s;
}
// the eight values at the corners (at(jj, ii, kk) = the value at an inside index)
template <class At>
__device__ __forceinline__ void mc3_values(const Mc3C& s, const At& at, float (&f)[2][2][2]) {
#pragma unroll
    for (int cj = 0; cj < 2; ++cj)
#pragma unroll
        for (int ci = 0; ci < 2; ++ci)
#pragma unroll
            for (int ck = 0; ck < 2; ++ck) f[cj][ci][ck] = s.jin[cj] && s.iin[ci] && s.kin[ck] ? at(s.jj[cj], s.ii[ci], s.kk[ck]) : 0.f;
}
__device__ __forceinline__ float mc3_trilinear(const Mc3C& s, const float (&f)[2][2][2]) {
#pragma clang fp contract(off)
    const float c00 = (1.f - s.wz) * f[0][0][0] + s.wz * f[0][0][1];
    const float c01 = (1.f - s.wz) * f[0][1][0] + s.wz * f[0][1][1];
    const float c10 = (1.f - s.wz) * f[1][0][0] + s.wz * f[1][0][1];
    const float c11 = (1.f - s.wz) * f[1][1][0] + s.wz * f[1][1][1];
    return (1.f - s.wy) * ((1.f - s.wx) * c00 + s.wx * c01) + s.wy * ((1.f - s.wx) * c10 + s.wx * c11);
}

// h at (j, i, k): the semi-Lagrangian value, unmasked, no inflow added -- the ONE expression of it; lo / hi: min / max of the eight values read
template <int K>
__device__ __forceinline__ float mc3_hat(const Mc3Args& a, const Mc3Sim& m, int j, int i, int k, float& lo, float& hi) {
#pragma clang fp contract(off)
    float uy, ux, uz, f[2][2][2];
    mc3_u<K>(m, j, i, k, uy, ux, uz);
    const Mc3C s = mc3_corners<K>(a, j, i, k, -uy * a.dtdx, -ux * a.dtdx, -uz * a.dtdx);
    mc3_values(s, [&](int jj, int ii, int kk) { return mc3_f<K>(a, m, jj, ii, kk); }, f);
    lo = fminf(fminf(fminf(f[0][0][0], f[0][0][1]), fminf(f[0][1][0], f[0][1][1])), fminf(fminf(f[1][0][0], f[1][0][1]), fminf(f[1][1][0], f[1][1][1])));
    hi = fmaxf(fmaxf(fmaxf(f[0][0][0], f[0][0][1]), fmaxf(f[0][1][0], f[0][1][1])), fmaxf(fmaxf(f[1][0][0], f[1][0][1]), fmaxf(f[1][1][0], f[1][1][1])));
    return mc3_trilinear(s, f);
}

// the limiter's decision with h, lo, hi of mc3_hat and back = the value carried back: cor, and whether it is kept
__device__ __forceinline__ bool mc3_limit(const Mc3Args& a, float h, float lo, float hi, float fv, float back, float& cor) {
#pragma clang fp contract(off)
    cor = h + a.hs * (fv - back);
    return lo <= cor && cor <= hi;
}

// everything the forward step decides at (j, i, k) of an array of kind K, recomputed: h, the corners of the gather at x + u dt with the
// values of h there (hb = the simulation's h array of kind K), cor and whether it is kept
template <int K>
struct Mc3Dec {
    float h, cor;
    bool kept;
    Mc3C s;
    float hv[2][2][2];
};
template <int K>
__device__ __forceinline__ void mc3_decide(const Mc3Args& a, const Mc3Sim& m, const float* hb, int j, int i, int k, Mc3Dec<K>& d) {
#pragma clang fp contract(off)
    const int n1 = mc3_n1<K>(a), n2 = mc3_n2<K>(a);
    float lo, hi, uy, ux, uz;
    d.h = mc3_hat<K>(a, m, j, i, k, lo, hi);
    mc3_u<K>(m, j, i, k, uy, ux, uz);
    d.s = mc3_corners<K>(a, j, i, k, uy * a.dtdx, ux * a.dtdx, uz * a.dtdx);
    mc3_values(d.s, [&](int jj, int ii, int kk) { return hb[((size_t)jj * n1 + ii) * n2 + kk]; }, d.hv);
    d.kept = mc3_limit(a, d.h, lo, hi, mc3_f<K>(a, m, j, i, k), mc3_trilinear(d.s, d.hv), d.cor);
}

// one z column of kind K.  PASS 0: h into the workspace; 1: the step's advected values
template <int K, int PASS>
__device__ __forceinline__ void mc3_column(const Mc3Args& a, const Mc3Sim& m, int b, int j, int i, int lane) {
#pragma clang fp contract(off)
    const int n1 = mc3_n1<K>(a), n2 = mc3_n2<K>(a);
    const size_t n = mc3_count<K>(a);
    float* hb = a.h[K] + (size_t)b * n;
    for (int k = lane; k < n2; k += 64) {
        const size_t q = ((size_t)j * n1 + i) * n2 + k;
        if (PASS == 0) {
            float lo, hi;
            hb[q] = mc3_hat<K>(a, m, j, i, k, lo, hi);
            continue;
        }
        Mc3Dec<K> d;
        mc3_decide<K>(a, m, hb, j, i, k, d);
        float v = d.kept ? d.cor : d.h;
        if (K == 0) a.vy_out[(size_t)b * n + q] = v * (m.r.acc(j - 1, i, k) * m.r.acc(j, i, k));
        else if (K == 1) a.vx_out[(size_t)b * n + q] = v * (m.r.acc(j, i - 1, k) * m.r.acc(j, i, k));
        else if (K == 2) a.vz_out[(size_t)b * n + q] = v * (m.r.acc(j, i, k - 1) * m.r.acc(j, i, k));
        else {
            if (!a.inflow_before) v += a.inflow[q] * a.dt;
            a.d_out[(size_t)b * n + q] = v;
        }
    }
}

// the columns of a launch: y faces, x faces, z faces, cells; a wave's column index c -> (kind, j, i), wave uniform
struct Mc3Col {
    int kind, j, i;
};
__device__ __forceinline__ Mc3Col mc3_col(int Y, int X, int c) {
    const int cY = (Y + 1) * X, cX = Y * (X + 1), cC = Y * X;
    if (c < cY) return Mc3Col{0, c / X, c % X};
    if (c < cY + cX) { const int q = c - cY; return Mc3Col{1, q / (X + 1), q % (X + 1)}; }
    if (c < cY + cX + cC) { const int q = c - cY - cX; return Mc3Col{2, q / X, q % X}; }
    const int q = c - cY - cX - cC;
    return Mc3Col{3, q / X, q % X};
}
// first and one-past-last column of the arrays a launch works on
__device__ __forceinline__ void mc3_range(const Mc3Args& a, int& c0, int& c1) {
    const int cV = (a.Y + 1) * a.X + a.Y * (a.X + 1) + a.Y * a.X;
    c0 = a.with_v ? 0 : cV;
    c1 = a.with_d ? cV + a.Y * a.X : cV;
}

template <int PASS>
__global__ void __launch_bounds__(256) k3m_fwd(Mc3Args a) {
    const int b = blockIdx.y;
    const Mc3Sim m = mc3_sim(a, b);
    int c0, c1;
    mc3_range(a, c0, c1);
    const int lane = threadIdx.x & 63;
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const int nwaves = gridDim.x * (blockDim.x >> 6);
    for (int c = c0 + wave0; c < c1; c += nwaves) {
        const Mc3Col t = mc3_col(a.Y, a.X, c);
        if (t.kind == 0) mc3_column<0, PASS>(a, m, b, t.j, t.i, lane);
        else if (t.kind == 1) mc3_column<1, PASS>(a, m, b, t.j, t.i, lane);
        else if (t.kind == 2) mc3_column<2, PASS>(a, m, b, t.j, t.i, lane);
        else mc3_column<3, PASS>(a, m, b, t.j, t.i, lane);
    }
}

int grid_cols(size_t cols) { const size_t g = (cols * 64 + 255) / 256; return (int)(g < 1 ? 1 : (g > 65535 ? 65535 : g)); }
int grid_elems(size_t n) { const size_t g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g)); }

// the workspace of the forward launches: h of the four arrays
struct Mc3Layout {
    float* h[4];
    size_t bytes;
};
Mc3Layout mc3_layout(const sol_karman3d_cfg* c, void* ws) {
    const size_t B = c->B, Y = c->Y, X = c->X, Z = c->Z;
    Carve w(ws);
    Mc3Layout l{{w.take<float>(B * (Y + 1) * X * Z), w.take<float>(B * Y * (X + 1) * Z), w.take<float>(B * Y * X * (Z + 1)), w.take<float>(B * Y * X * Z)}, 0};
    l.bytes = w.bytes();
    return l;
}

Mc3Args mc3_args(const sol_karman3d_cfg* c, float strength, const float* d_in, const float* svy, const float* svx, const float* svz, const float* active,
                 const float* inflow) {
    Mc3Args a{};
    a.Y = c->Y; a.X = c->X; a.Z = c->Z; a.inflow_before = c->inflow_before; a.with_v = 1; a.with_d = d_in != nullptr;
    a.dtdx = c->dt / c->dx; a.dt = c->dt; a.hs = 0.5f * strength;
    a.d_in = d_in; a.svy = svy; a.svx = svx; a.svz = svz; a.active = active; a.inflow = inflow;
    return a;
}
size_t mc3_cols(const sol_karman3d_cfg* c, bool with_v, bool with_d) {
    const size_t Y = c->Y, X = c->X;
    return (with_v ? (Y + 1) * X + Y * (X + 1) + Y * X : 0) + (with_d ? Y * X : 0);
}

// ================================================================ adjoint ================================================================
struct Ma3Args {
    Mc3Args f;                              // the forward step's arguments (h arrays filled by k3m_hat)
    const float* g[4];                      // cotangents: g_a of the three components (masked), g_d_out
    const unsigned* gmax;                   // [B][FX_SLOTS]: the scale of this kernel's cotangent
    long long *gc[3], *Gh[3];               // velocity: g_c and G_h per component [B][...]
    long long *gD, *Ghd;                    // density: g_d_in and G_h [B][YXZ]
    float *gUy, *gUx, *gUz;                 // density: back-trace term per cell [B][YXZ]
    float* gh[4];                           // stage B's cotangent g_h = g + G_h
};

// transpose of one trilinear gather with corners s and corner values f: gs times the weights through add (inside corners only; the ghost
// ring takes no gradient), and the slopes d(sample)/d(offset) along y, x and z
template <class Add>
__device__ __forceinline__ void ma3_gather_adj(const Mc3C& s, const float (&f)[2][2][2], const Add& add, float gs, float& dy, float& dx, float& dz) {
#pragma clang fp contract(off)
    dy = 0.f; dx = 0.f; dz = 0.f;
#pragma unroll
    for (int cj = 0; cj < 2; ++cj)
#pragma unroll
        for (int ci = 0; ci < 2; ++ci)
#pragma unroll
            for (int ck = 0; ck < 2; ++ck) {
                const float by = cj ? s.wy : 1.f - s.wy, bx = ci ? s.wx : 1.f - s.wx, bz = ck ? s.wz : 1.f - s.wz;
                const float v = f[cj][ci][ck];
                if (s.jin[cj] && s.iin[ci] && s.kin[ck]) add(s.jj[cj], s.ii[ci], s.kk[ck], by * bx * bz * gs);
                dy += (cj ? 1.f : -1.f) * bx * bz * v;
                dx += by * (ci ? 1.f : -1.f) * bz * v;
                dz += by * bx * (ck ? 1.f : -1.f) * v;
            }
}

// stage A at face (j, i, k) of component K with cotangent g
template <int K>
__device__ __forceinline__ void ma3_vel_point(const Ma3Args& a, const Mc3Sim& m, const float* hb, const GAdd& addc, const GAdd& addh, int j, int i, int k, float g) {
#pragma clang fp contract(off)
    Mc3Dec<K> d;
    mc3_decide<K>(a.f, m, hb, j, i, k, d);
    if (!d.kept) return;
    const float gf = a.f.hs * g, gb = -gf;
    addc(K, j, i, k, gf);
    float dy, dx, dz;
    ma3_gather_adj(d.s, d.hv, [&](int jj, int ii, int kk, float v) { addh(K, jj, ii, kk, v); }, gb, dy, dx, dz);
    const AdvU u = adv3_u<K>(m.r, j, i, k);
    adv3_u_scatter<K>(addc, u, j, i, k, a.f.dtdx * gb * dy, a.f.dtdx * gb * dx, a.f.dtdx * gb * dz);
}
template <int K>
__device__ __forceinline__ void ma3_vel_column(const Ma3Args& a, const Mc3Sim& m, int b, const GAdd& addc, const GAdd& addh, int j, int i, int lane) {
    const int n1 = mc3_n1<K>(a.f), n2 = mc3_n2<K>(a.f);
    const size_t n = mc3_count<K>(a.f);
    const float* hb = a.f.h[K] + (size_t)b * n;
    const float* gk = a.g[K] + (size_t)b * n;
    for (int k = lane; k < n2; k += 64) {
        const float g = gk[((size_t)j * n1 + i) * n2 + k];
        if (g != 0.f) ma3_vel_point<K>(a, m, hb, addc, addh, j, i, k, g);
    }
}

__global__ void __launch_bounds__(256) k3m_vel_adj(Ma3Args a) {
    const int Y = a.f.Y, X = a.f.X, Z = a.f.Z;
    const size_t nVy = (size_t)(Y + 1) * X * Z, nVx = (size_t)Y * (X + 1) * Z, nVz = (size_t)Y * X * (Z + 1);
    const int b = blockIdx.y;
    const Mc3Sim m = mc3_sim(a.f, b);
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    const GAdd addc{a.gc[0] + b * nVy, a.gc[1] + b * nVx, a.gc[2] + b * nVz, qs, X, Z};
    const GAdd addh{a.Gh[0] + b * nVy, a.Gh[1] + b * nVx, a.Gh[2] + b * nVz, qs, X, Z};
    const int cV = (Y + 1) * X + Y * (X + 1) + Y * X;
    const int lane = threadIdx.x & 63;
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const int nwaves = gridDim.x * (blockDim.x >> 6);
    for (int c = wave0; c < cV; c += nwaves) {
        const Mc3Col t = mc3_col(Y, X, c);
        if (t.kind == 0) ma3_vel_column<0>(a, m, b, addc, addh, t.j, t.i, lane);
        else if (t.kind == 1) ma3_vel_column<1>(a, m, b, addc, addh, t.j, t.i, lane);
        else ma3_vel_column<2>(a, m, b, addc, addh, t.j, t.i, lane);
    }
}

// stage A of the density: g_d_in += (s/2) kept g, G_h scattered, its part of gU WRITTEN (zero where the point reverted or g is zero)
__global__ void __launch_bounds__(256) k3m_den_adj(Ma3Args a) {
#pragma clang fp contract(off)
    const int Y = a.f.Y, X = a.f.X, Z = a.f.Z;
    const size_t N = (size_t)Y * X * Z;
    const int b = blockIdx.y;
    const Mc3Sim m = mc3_sim(a.f, b);
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    long long *gD = a.gD + b * N, *Gh = a.Ghd + b * N;
    const float *hb = a.f.h[3] + b * N, *gd = a.g[3] + b * N;
    const int lane = threadIdx.x & 63;
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const int nwaves = gridDim.x * (blockDim.x >> 6);
    for (int c = wave0; c < Y * X; c += nwaves) {
        const int j = c / X, i = c % X;
        for (int k = lane; k < Z; k += 64) {
            const size_t q = ((size_t)j * X + i) * Z + k;
            const float g = gd[q];
            float guy = 0.f, gux = 0.f, guz = 0.f;
            if (g != 0.f) {
                Mc3Dec<3> d;
                mc3_decide<3>(a.f, m, hb, j, i, k, d);
                if (d.kept) {
                    const float gf = a.f.hs * g, gb = -gf;
                    fx_add(gD + q, gf, qs);
                    float dy, dx, dz;
                    ma3_gather_adj(d.s, d.hv, [&](int jj, int ii, int kk, float v) { fx_add(Gh + ((size_t)jj * X + ii) * Z + kk, v, qs); }, gb, dy, dx, dz);
                    guy = a.f.dtdx * gb * dy; gux = a.f.dtdx * gb * dx; guz = a.f.dtdx * gb * dz;
                }
            }
            a.gUy[b * N + q] = guy; a.gUx[b * N + q] = gux; a.gUz[b * N + q] = guz;
        }
    }
}

// stage B's cotangent g_h = g + G_h of up to three arrays of n[t] elements per simulation, back in fp32 (a poisoned simulation: NaN)
struct GhArgs {
    const float* g[3];
    const long long* G[3];
    float* out[3];
    int n[3];
    const unsigned* gmax;
};
__global__ void __launch_bounds__(256) k3m_gh(GhArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.y, total = a.n[0] + a.n[1] + a.n[2];
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const int t = e < a.n[0] ? 0 : (e < a.n[0] + a.n[1] ? 1 : 2);
        const int q = e - (t > 0 ? a.n[0] : 0) - (t > 1 ? a.n[1] : 0);
        const size_t o = (size_t)b * a.n[t] + q;
        a.out[t][o] = a.g[t][o] + fx_get(a.G[t] + (size_t)b * a.n[t], q, qi);
    }
}

// clears n words from p: a kernel, so that a captured schedule holds kernel nodes only
__global__ void __launch_bounds__(256) k3m_clear(unsigned* __restrict__ p, size_t n) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) p[e] = 0u;
}
int mc3_clear(hipStream_t s, void* p, size_t bytes) {
    SOL_LAUNCH(k3m_clear, dim3(grid_elems(bytes / 4)), dim3(256), 0, s, static_cast<unsigned*>(p), bytes / 4);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

// the adjoints' workspaces: h of the arrays, the accumulators G_h, stage B's cotangent g_h
struct Ma3VLayout {
    float *hy, *hx, *hz;
    long long* Gh;                      // [B][y faces] [B][x faces] [B][z faces], one block: one clear
    float *ghy, *ghx, *ghz;
    size_t bytes;
};
Ma3VLayout ma3v_layout(const sol_karman3d_cfg* c, void* ws) {
    const size_t B = c->B, Y = c->Y, X = c->X, Z = c->Z, nVy = (Y + 1) * X * Z, nVx = Y * (X + 1) * Z, nVz = Y * X * (Z + 1);
    Carve w(ws);
    Ma3VLayout l{w.take<float>(B * nVy), w.take<float>(B * nVx), w.take<float>(B * nVz), w.take<long long>(B * (nVy + nVx + nVz)),
                 w.take<float>(B * nVy), w.take<float>(B * nVx), w.take<float>(B * nVz), 0};
    l.bytes = w.bytes();
    return l;
}
struct Ma3DLayout {
    float* hd;
    long long* Ghd;
    float* ghd;
    size_t bytes;
};
Ma3DLayout ma3d_layout(const sol_karman3d_cfg* c, void* ws) {
    const size_t BN = (size_t)c->B * c->Y * c->X * c->Z;
    Carve w(ws);
    Ma3DLayout l{w.take<float>(BN), w.take<long long>(BN), w.take<float>(BN), 0};
    l.bytes = w.bytes();
    return l;
}

// ---- the stage alone: what surrounds the two adjoints when no solver step does ----
struct St3Args {
    int Y, X, Z;
    const float *active, *g_a[3], *g_d_out;
    float* ga[3];                       // the masked velocity cotangent
    unsigned *gmax_v, *gmax_d;          // zeroed beforehand
    const long long *gc[3], *gD;
    const float *gUy, *gUx, *gUz;
    float *g_d_in, *g_sv[3];
};
// g_a = mask . g and max|g_a| (columns of the three components), max|g_d_out| (cell columns)
__global__ void __launch_bounds__(256) k3m_prep(St3Args a) {
    const int Y = a.Y, X = a.X, Z = a.Z;
    const size_t nVy = (size_t)(Y + 1) * X * Z, nVx = (size_t)Y * (X + 1) * Z, nVz = (size_t)Y * X * (Z + 1), N = (size_t)Y * X * Z;
    const int b = blockIdx.y, cV = (Y + 1) * X + Y * (X + 1) + Y * X;
    float vmax = 0.f, dmax = 0.f;
    bool bad = false, dbad = false;
    const int lane = threadIdx.x & 63;
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const int nwaves = gridDim.x * (blockDim.x >> 6);
    for (int c = wave0; c < cV + Y * X; c += nwaves) {
        const Mc3Col t = mc3_col(Y, X, c);
        const int j = t.j, i = t.i;
        if (t.kind == 0) {
            for (int k = lane; k < Z; k += 64) {
                const size_t e = b * nVy + ((size_t)j * X + i) * Z + k;
                const float v = face_mask<0>(a.active, Y, X, Z, j, i, k) * a.g_a[0][e];
                a.ga[0][e] = v; vmax = fmaxf(vmax, fabsf(v)); bad |= !(fabsf(v) <= 3.402823466e38f);
            }
        } else if (t.kind == 1) {
            for (int k = lane; k < Z; k += 64) {
                const size_t e = b * nVx + ((size_t)j * (X + 1) + i) * Z + k;
                const float v = face_mask<1>(a.active, Y, X, Z, j, i, k) * a.g_a[1][e];
                a.ga[1][e] = v; vmax = fmaxf(vmax, fabsf(v)); bad |= !(fabsf(v) <= 3.402823466e38f);
            }
        } else if (t.kind == 2) {
            for (int k = lane; k <= Z; k += 64) {
                const size_t e = b * nVz + ((size_t)j * X + i) * (Z + 1) + k;
                const float v = face_mask<2>(a.active, Y, X, Z, j, i, k) * a.g_a[2][e];
                a.ga[2][e] = v; vmax = fmaxf(vmax, fabsf(v)); bad |= !(fabsf(v) <= 3.402823466e38f);
            }
        } else {
            for (int k = lane; k < Z; k += 64) {
                const float v = fabsf(a.g_d_out[b * N + ((size_t)j * X + i) * Z + k]);
                dmax = fmaxf(dmax, v); dbad |= !(v <= 3.402823466e38f);
            }
        }
    }
    fx_publish_max2(a.gmax_v + b * FX_SLOTS, vmax, bad, a.gmax_d + b * FX_SLOTS, dmax, dbad);
}
// g_sv = g_c + the cell-to-face transpose of gU (a centre velocity is the mean of its two faces), g_d_in: back in fp32
__global__ void __launch_bounds__(256) k3m_finish(St3Args a) {
#pragma clang fp contract(off)
    const int Y = a.Y, X = a.X, Z = a.Z;
    const size_t nVy = (size_t)(Y + 1) * X * Z, nVx = (size_t)Y * (X + 1) * Z, nVz = (size_t)Y * X * (Z + 1), N = (size_t)Y * X * Z;
    const int b = blockIdx.y, cV = (Y + 1) * X + Y * (X + 1) + Y * X;
    float qs, qv, qd;
    fx_scale(a.gmax_v + b * FX_SLOTS, qs, qv);
    fx_scale(a.gmax_d + b * FX_SLOTS, qs, qd);
    const bool poisoned = qv != qv || qd != qd;        // a non-finite cotangent of either kind: every gradient of the simulation is NaN
    const float nan = __uint_as_float(0x7fc00000u);
    const float *uy = a.gUy + b * N, *ux = a.gUx + b * N, *uz = a.gUz + b * N;
    const int lane = threadIdx.x & 63;
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const int nwaves = gridDim.x * (blockDim.x >> 6);
    for (int c = wave0; c < cV + Y * X; c += nwaves) {
        const Mc3Col t = mc3_col(Y, X, c);
        const int j = t.j, i = t.i;
        if (t.kind == 0) {
            for (int k = lane; k < Z; k += 64) {
                const size_t q = ((size_t)j * X + i) * Z + k;
                const float lo = j > 0 ? uy[q - (size_t)X * Z] : 0.f, hi = j < Y ? uy[q] : 0.f;
                a.g_sv[0][b * nVy + q] = poisoned ? nan : fx_get(a.gc[0] + b * nVy, (int)q, qv) + 0.5f * (lo + hi);
            }
        } else if (t.kind == 1) {
            for (int k = lane; k < Z; k += 64) {
                const size_t q = ((size_t)j * (X + 1) + i) * Z + k, cq = ((size_t)j * X + i) * Z + k;
                const float lo = i > 0 ? ux[cq - Z] : 0.f, hi = i < X ? ux[cq] : 0.f;
                a.g_sv[1][b * nVx + q] = poisoned ? nan : fx_get(a.gc[1] + b * nVx, (int)q, qv) + 0.5f * (lo + hi);
            }
        } else if (t.kind == 2) {
            for (int k = lane; k <= Z; k += 64) {
                const size_t q = ((size_t)j * X + i) * (Z + 1) + k, cq = ((size_t)j * X + i) * Z + k;
                const float lo = k > 0 ? uz[cq - 1] : 0.f, hi = k < Z ? uz[cq] : 0.f;
                a.g_sv[2][b * nVz + q] = poisoned ? nan : fx_get(a.gc[2] + b * nVz, (int)q, qv) + 0.5f * (lo + hi);
            }
        } else {
            for (int k = lane; k < Z; k += 64) {
                const size_t q = ((size_t)j * X + i) * Z + k;
                a.g_d_in[b * N + q] = poisoned ? nan : fx_get(a.gD + b * N, (int)q, qd);
            }
        }
    }
}

struct St3Layout {
    long long *gc, *gD;                 // g_c [B][y faces] [B][x faces] [B][z faces], g_d_in [B][N]
    unsigned* gmax;                     // [2][B][FX_SLOTS]: velocity, density
    float *gay, *gax, *gaz, *gUy, *gUx, *gUz;
    void *mav, *mad;
    size_t bytes;
};
St3Layout st3_layout(const sol_karman3d_cfg* c, void* ws) {
    const size_t B = c->B, Y = c->Y, X = c->X, Z = c->Z, nVy = (Y + 1) * X * Z, nVx = Y * (X + 1) * Z, nVz = Y * X * (Z + 1), N = Y * X * Z;
    Carve w(ws);
    St3Layout l{w.take<long long>(B * (nVy + nVx + nVz)), w.take<long long>(B * N), w.take<unsigned>(2 * B * FX_SLOTS),
                w.take<float>(B * nVy), w.take<float>(B * nVx), w.take<float>(B * nVz), w.take<float>(B * N), w.take<float>(B * N), w.take<float>(B * N),
                w.take<char>(ma3v_layout(c, nullptr).bytes), w.take<char>(ma3d_layout(c, nullptr).bytes), 0};
    l.bytes = w.bytes();
    return l;
}

bool mc3_shape_ok(const sol_karman3d_cfg* c) {
    return c && c->B >= 1 && c->B <= 65535 && c->Y >= 8 && c->X >= 8 && c->Z >= 8 && (size_t)(c->Y + 1) * (c->X + 1) * (c->Z + 1) * 3 < ((size_t)1 << 31);
}

}  // namespace

size_t sol_mc3_bytes(const sol_karman3d_cfg* c) { return mc3_layout(c, nullptr).bytes; }
size_t sol_mc3_adj_vel_bytes(const sol_karman3d_cfg* c) { return ma3v_layout(c, nullptr).bytes; }
size_t sol_mc3_adj_den_bytes(const sol_karman3d_cfg* c) { return ma3d_layout(c, nullptr).bytes; }

int sol_mc3_check(const char* who, int32_t advection, float strength) {
    SOL_REQUIRE(advection == 0 || advection == 1, "%s: advection must be 0 (semi-Lagrangian) or 1 (MacCormack), got %d", who, advection);
    SOL_REQUIRE(strength >= 0.f && strength <= 1.f, "%s: correction_strength must lie in [0, 1] (got %g)", who, (double)strength);
    return SOL_OK;
}

// the launches of the MacCormack advection in place of k3_advect's (d_out NULL: the velocity alone)
int sol_mc3_advect(const sol_karman3d_cfg* c, hipStream_t s, float strength, const float* d_in, const float* svy, const float* svx, const float* svz,
                   const float* active, const float* inflow, float* d_out, float* vy_out, float* vx_out, float* vz_out, void* ws) {
    const Mc3Layout l = mc3_layout(c, ws);
    Mc3Args a = mc3_args(c, strength, d_out ? d_in : nullptr, svy, svx, svz, active, inflow);
    a.d_out = d_out; a.vy_out = vy_out; a.vx_out = vx_out; a.vz_out = vz_out;
    for (int k = 0; k < 4; ++k) a.h[k] = l.h[k];
    const int grid = grid_cols(mc3_cols(c, true, a.with_d != 0));
    SOL_LAUNCH_NAMED("k3m_hat", k3m_fwd<0>, dim3(grid, c->B), dim3(256), 0, s, a);
    SOL_LAUNCH_NAMED("k3m_out", k3m_fwd<1>, dim3(grid, c->B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

// The advection adjoint of the VELOCITY in place of k3b_advect_adj*: g_a (masked, its max published in gmax) -> added onto the cleared
// int64 g_c.  tile: stage B's form (karman3d_advect.hpp)
int sol_mc3_adj_vel(const sol_karman3d_cfg* c, hipStream_t s, float strength, const float* svy, const float* svx, const float* svz, const float* gay,
                    const float* gax, const float* gaz, const unsigned* gmax, long long* gcy, long long* gcx, long long* gcz, void* ws, int tile) {
    const Ma3VLayout l = ma3v_layout(c, ws);
    const size_t B = c->B, Y = c->Y, X = c->X, Z = c->Z, nVy = (Y + 1) * X * Z, nVx = Y * (X + 1) * Z, nVz = Y * X * (Z + 1);
    Ma3Args a{};
    a.f = mc3_args(c, strength, nullptr, svy, svx, svz, nullptr, nullptr);
    a.f.h[0] = l.hy; a.f.h[1] = l.hx; a.f.h[2] = l.hz;
    a.g[0] = gay; a.g[1] = gax; a.g[2] = gaz; a.gmax = gmax;
    a.gc[0] = gcy; a.gc[1] = gcx; a.gc[2] = gcz;
    a.Gh[0] = l.Gh; a.Gh[1] = l.Gh + B * nVy; a.Gh[2] = a.Gh[1] + B * nVx;
    if (int e = mc3_clear(s, l.Gh, B * (nVy + nVx + nVz) * sizeof(long long))) return e;
    const int grid = grid_cols(mc3_cols(c, true, false));
    SOL_LAUNCH_NAMED("k3m_hat", k3m_fwd<0>, dim3(grid, c->B), dim3(256), 0, s, a.f);
    SOL_LAUNCH(k3m_vel_adj, dim3(grid, c->B), dim3(256), 0, s, a);
    GhArgs h{};
    h.g[0] = gay; h.g[1] = gax; h.g[2] = gaz;
    for (int k = 0; k < 3; ++k) h.G[k] = a.Gh[k];
    h.out[0] = l.ghy; h.out[1] = l.ghx; h.out[2] = l.ghz;
    h.n[0] = (int)nVy; h.n[1] = (int)nVx; h.n[2] = (int)nVz;
    h.gmax = gmax;
    SOL_LAUNCH(k3m_gh, dim3(grid_elems(nVy + nVx + nVz), c->B), dim3(256), 0, s, h);
    SOL_LAUNCH_CHECK();
    return sol_k3b_advect_adj(c, s, svy, svx, svz, l.ghy, l.ghx, l.ghz, gmax, gcy, gcx, gcz, tile);
}

// The advection adjoint of the DENSITY in place of k3d_advect_adj*: g_d_out (its max in gmax) -> added onto the cleared int64 gD, gU written
int sol_mc3_adj_den(const sol_karman3d_cfg* c, hipStream_t s, float strength, const float* d_in, const float* inflow, const float* svy, const float* svx,
                    const float* svz, const float* g_d_out, const unsigned* gmax, long long* gD, float* gUy, float* gUx, float* gUz, void* ws, int tile) {
    const Ma3DLayout l = ma3d_layout(c, ws);
    const size_t BN = (size_t)c->B * c->Y * c->X * c->Z;
    Ma3Args a{};
    a.f = mc3_args(c, strength, d_in, svy, svx, svz, nullptr, inflow);
    a.f.with_v = 0;
    a.f.h[3] = l.hd;
    a.g[3] = g_d_out; a.gmax = gmax;
    a.gD = gD; a.Ghd = l.Ghd;
    a.gUy = gUy; a.gUx = gUx; a.gUz = gUz;
    if (int e = mc3_clear(s, l.Ghd, BN * sizeof(long long))) return e;
    const int grid = grid_cols(mc3_cols(c, false, true));
    SOL_LAUNCH_NAMED("k3m_hat", k3m_fwd<0>, dim3(grid, c->B), dim3(256), 0, s, a.f);
    SOL_LAUNCH(k3m_den_adj, dim3(grid, c->B), dim3(256), 0, s, a);
    GhArgs h{};
    h.g[0] = g_d_out; h.G[0] = l.Ghd; h.out[0] = l.ghd; h.n[0] = (int)(BN / c->B);
    h.gmax = gmax;
    SOL_LAUNCH(k3m_gh, dim3(grid_elems(BN / c->B), c->B), dim3(256), 0, s, h);
    SOL_LAUNCH_CHECK();
    return sol_k3d_advect_adj(c, s, d_in, inflow, svy, svx, svz, l.ghd, gmax, gD, gUy, gUx, gUz, true, tile);
}

extern "C" size_t sol_karman3d_advect_workspace_bytes(const sol_karman3d_cfg* c, int32_t advection) {
    if (!mc3_shape_ok(c) || advection != 1) return 0;
    return sol_mc3_bytes(c);
}

// The advection stage alone: (d_in, sv_y, sv_x, sv_z) -> (d_out, a_y, a_x, a_z), the velocity masked, the inflow added as cfg.inflow_before
// says.  advection = 0: the plain launch (sol_k3_advect); 1: the kernels above.
extern "C" int sol_karman3d_advect(const sol_karman3d_cfg* c, void* stream, const float* d_in, const float* svy, const float* svx, const float* svz,
                                   const float* active, const float* inflow, int32_t advection, float correction_strength,
                                   float* d_out, float* ay, float* ax, float* az, void* workspace, size_t workspace_bytes) {
    const char* who = "sol_karman3d_advect";
    SOL_REQUIRE(c != nullptr, "%s: cfg is NULL", who);
    SOL_REQUIRE(c->B >= 1 && c->B <= 65535 && c->Y >= 8 && c->X >= 8 && c->Z >= 8, "%s: B in [1, 65535], Y, X, Z >= 8 (got %d, %d, %d, %d)", who, c->B, c->Y, c->X, c->Z);
    SOL_REQUIRE(mc3_shape_ok(c), "%s: grid too large for 32-bit face indices", who);
    if (int e = sol_mc3_check(who, advection, correction_strength)) return e;
    SOL_REQUIRE(d_in && svy && svx && svz && active && inflow && d_out && ay && ax && az, "%s: NULL pointer argument", who);
    const void* outs[] = {d_out, ay, ax, az};
    const void* ins[] = {d_in, svy, svx, svz, active, inflow};
    for (const void* o : outs)
        for (const void* i : ins) SOL_REQUIRE(o != i, "%s: outputs must not alias the inputs", who);
    for (int p = 0; p < 4; ++p)
        for (int q = p + 1; q < 4; ++q) SOL_REQUIRE(outs[p] != outs[q], "%s: d_out, ay, ax and az must be buffers of their own", who);
    const size_t need = sol_karman3d_advect_workspace_bytes(c, advection);
    SOL_REQUIRE(need == 0 || workspace != nullptr, "%s: the MacCormack advection needs a workspace (%zu bytes)", who, need);
    SOL_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    if (advection == 0) return sol_k3_advect(c, s, d_in, svy, svx, svz, active, inflow, d_out, ay, ax, az);
    return sol_mc3_advect(c, s, correction_strength, d_in, svy, svx, svz, active, inflow, d_out, ay, ax, az, workspace);
}

extern "C" size_t sol_karman3d_advect_bwd_workspace_bytes(const sol_karman3d_cfg* c) {
    if (!mc3_shape_ok(c)) return 0;
    return st3_layout(c, nullptr).bytes;
}

// The transpose of sol_karman3d_advect: cotangents of (d_out, a_y, a_x, a_z) -> (g_d_in, g_sv_y, g_sv_x, g_sv_z).  tile_window: 1 = the
// semi-Lagrangian scatters (stage B; all of advection = 0) through their LDS windows where the grid admits them, 0 = global atomics only
// (equal bits).
extern "C" int sol_karman3d_advect_bwd(const sol_karman3d_cfg* c, void* stream, const float* d_in, const float* svy, const float* svx, const float* svz,
                                       const float* active, const float* inflow, int32_t advection, float correction_strength,
                                       const float* g_d_out, const float* g_ay, const float* g_ax, const float* g_az,
                                       float* g_d_in, float* g_svy, float* g_svx, float* g_svz, int32_t tile_window, void* workspace, size_t workspace_bytes) {
    const char* who = "sol_karman3d_advect_bwd";
    SOL_REQUIRE(c != nullptr, "%s: cfg is NULL", who);
    SOL_REQUIRE(c->B >= 1 && c->B <= 65535 && c->Y >= 8 && c->X >= 8 && c->Z >= 8, "%s: B in [1, 65535], Y, X, Z >= 8 (got %d, %d, %d, %d)", who, c->B, c->Y, c->X, c->Z);
    SOL_REQUIRE(mc3_shape_ok(c), "%s: grid too large for 32-bit face indices", who);
    if (int e = sol_mc3_check(who, advection, correction_strength)) return e;
    SOL_REQUIRE(tile_window == 0 || tile_window == 1, "%s: tile_window must be 0 or 1 (got %d)", who, tile_window);
    SOL_REQUIRE(d_in && svy && svx && svz && active && inflow && g_d_out && g_ay && g_ax && g_az && g_d_in && g_svy && g_svx && g_svz && workspace,
                "%s: NULL pointer argument", who);
    const void* outs[] = {g_d_in, g_svy, g_svx, g_svz};
    const void* ins[] = {d_in, svy, svx, svz, active, inflow, g_d_out, g_ay, g_ax, g_az};
    for (const void* o : outs)
        for (const void* i : ins) SOL_REQUIRE(o != i, "%s: outputs must not alias the inputs", who);
    for (int p = 0; p < 4; ++p)
        for (int q = p + 1; q < 4; ++q) SOL_REQUIRE(outs[p] != outs[q], "%s: g_d_in, g_svy, g_svx and g_svz must be buffers of their own", who);
    const St3Layout l = st3_layout(c, workspace);
    SOL_REQUIRE(workspace_bytes >= l.bytes, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, l.bytes);
    const size_t B = c->B, Y = c->Y, X = c->X, Z = c->Z, nVy = (Y + 1) * X * Z, nVx = Y * (X + 1) * Z;
    hipStream_t s = (hipStream_t)stream;
    St3Args a{};
    a.Y = c->Y; a.X = c->X; a.Z = c->Z; a.active = active; a.g_a[0] = g_ay; a.g_a[1] = g_ax; a.g_a[2] = g_az; a.g_d_out = g_d_out;
    a.ga[0] = l.gay; a.ga[1] = l.gax; a.ga[2] = l.gaz;
    a.gmax_v = l.gmax; a.gmax_d = l.gmax + B * FX_SLOTS;
    long long *gcy = l.gc, *gcx = l.gc + B * nVy, *gcz = gcx + B * nVx;
    a.gc[0] = gcy; a.gc[1] = gcx; a.gc[2] = gcz; a.gD = l.gD; a.gUy = l.gUy; a.gUx = l.gUx; a.gUz = l.gUz;
    a.g_d_in = g_d_in; a.g_sv[0] = g_svy; a.g_sv[1] = g_svx; a.g_sv[2] = g_svz;
    // g_c, g_d_in and the absmax slots are neighbours in the layout: one clear
    if (int e = mc3_clear(s, l.gc, (size_t)(reinterpret_cast<char*>(l.gay) - reinterpret_cast<char*>(l.gc)))) return e;
    const int grid = grid_cols(mc3_cols(c, true, true));
    SOL_LAUNCH(k3m_prep, dim3(grid > 1024 ? 1024 : grid, c->B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    if (advection == 1) {
        if (int e = sol_mc3_adj_vel(c, s, correction_strength, svy, svx, svz, l.gay, l.gax, l.gaz, a.gmax_v, gcy, gcx, gcz, l.mav, tile_window)) return e;
        if (int e = sol_mc3_adj_den(c, s, correction_strength, d_in, inflow, svy, svx, svz, g_d_out, a.gmax_d, l.gD, l.gUy, l.gUx, l.gUz, l.mad, tile_window)) return e;
    } else {
        if (int e = sol_k3b_advect_adj(c, s, svy, svx, svz, l.gay, l.gax, l.gaz, a.gmax_v, gcy, gcx, gcz, tile_window)) return e;
        if (int e = sol_k3d_advect_adj(c, s, d_in, inflow, svy, svx, svz, g_d_out, a.gmax_d, l.gD, l.gUy, l.gUx, l.gUz, false, tile_window)) return e;
    }
    SOL_LAUNCH(k3m_finish, dim3(grid, c->B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}
