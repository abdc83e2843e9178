// MacCormack advection of the large-grid karman-2d step (advection = 1 on the _adv entry points; include/sol_hip.h, "MACCORMACK ADVECTION
// on the large-grid step"), forward and adjoint.  c = (sv_y, sv_x) is the post-diffusion velocity, f one advected array of kind K -- 0: c_y
// on its faces [Y+1][X], 1: c_x on its faces [Y][X+1], 2: the density on cells [Y][X] (+ inflow first when cfg.inflow_before) -- u the
// velocity at the array's sample point by k_l_advect's expressions, S_g the bilinear sample of g in the array's own extrapolation mode
// (index clamp for the velocity, one ring of zero ghost cells for the density):
//   h(x)   = S_f(x - u dt)                 the semi-Lagrangian value              (mc_hat)
//   b(x)   = S_h(x + u dt)                 h carried back with the same u
//   cor(x) = h(x) + (s / 2) (f(x) - b(x))
//   out(x) = cor(x) if lo <= cor(x) <= hi else h(x),   lo, hi = min, max of the four values the FIRST gather read (after clamping; ghost
//            zeros count); the compare is inclusive and a NaN reverts to h
// then as k_l_advect: velocity x hard-BC face mask, density + inflow dt when the inflow comes after.
//
// FORWARD.  h must be complete before b is gathered.  Two forms (option k2d_mc_tile), equal bit for bit because h at a point is ONE
// spelled-out expression (contraction off) wherever it is evaluated:
//   k_mc_tile           (1, default) one launch.  A workgroup takes a 16 x 32 tile of one array, evaluates h on the tile and a halo of 2
//                       (clipped to the array) into LDS, then gathers b from LDS; a corner beyond the halo (|u| dt/dx >= 2) is evaluated on
//                       the fly from c, so any CFL number is handled.
//   k_mc_hat, k_mc_out  (0, the reference form) h of the three arrays into the workspace, then gather / limiter / mask / inflow.
//
// ADJOINT: the derivative with every decision frozen as the forward step took it (the floorf's, the clamps, the limiter), recomputed from
// the saved c -- the forward step saves nothing new.  For a cotangent g of out (the velocity's is g_a, masked already) and kept = 1 where
// cor was kept:
//   stage 2 (k_ma_vel<2>, k_ma_den<2>)   g_b = -(s/2) kept g:  g_f += (s/2) kept g;  g_b scattered through the four corners of the gather at
//                                         x + u dt into the accumulators G_h;  g_u += +(dt/dx) g_b dS_h/d(offset)
//   stage 1 (k_ma_vel<1>, k_ma_den<1>)   the semi-Lagrangian adjoint of g_h = g + G_h: field term into g_f, back-trace term
//                                         -(dt/dx) g_h dS_f/d(offset) into g_u
// g_u of a velocity face goes onto the five velocity samples that formed u (as lb_advect_adj_point), g_u of a density cell is the per-cell
// gU that k_kd_diffuse_adj takes.  Where a point reverted, its adjoint is the plain semi-Lagrangian one (stage 2 adds nothing).  g_f of the
// velocity is g_c, of the density g_d_in.  Every scattered sum -- g_c, g_d_in and G_h -- is 64-bit fixed point with the ONE scale of its
// cotangent (fixed_scatter.hpp), so the adjoint is reproducible bit for bit; `tile` selects an int64 LDS window per 16 x 16-cell tile (halo
// 4; targets beyond it go to global memory) or global atomics only, equal bit for bit.  A non-finite cotangent poisons its simulation as
// it does in the semi-Lagrangian adjoints.  k_mc_hat provides h; the accumulators G_h are cleared by a kernel (k_mc_clear): no host
// synchronisation, no allocation, kernel nodes only under capture.
// Every index that reaches memory is clamped to its array or range-checked (the zero ghost ring), whatever the velocity holds.
#include "carve.hpp"
#include "fixed_scatter.hpp"
#include "large2d.hpp"

namespace {

constexpr int MC_TY = 16, MC_TX = 32, MC_HL = 2;                  // the forward tile and its halo
constexpr int MC_PY = MC_TY + 2 * MC_HL, MC_PX = MC_TX + 2 * MC_HL;    // the LDS plane: 20 x 36 floats
constexpr int MC_THREADS = 256;

struct McArgs {
    int Y, X, inflow_before, with_v, with_d;
    float dtdx, dt, hs;                     // hs = correction_strength / 2
    const float *d_in, *svy, *svx, *active, *inflow;
    float *d_out, *vy_out, *vx_out;
    float *hy, *hx, *hd;                    // h of the three arrays (two-launch form, adjoint)
    int ntx[3], nt[3];                      // tiled form: tile columns and tile count of each array
};

template <int K> __device__ __forceinline__ int mc_h(const McArgs& a) { return a.Y + (K == 0); }
template <int K> __device__ __forceinline__ int mc_w(const McArgs& a) { return a.X + (K == 1); }

// the arrays of simulation b
struct McSim {
    const float *sy, *sx, *d;
};
__device__ __forceinline__ McSim mc_sim(const McArgs& a, int b) {
    const size_t Y = a.Y, X = a.X;
    return McSim{a.svy + b * (Y + 1) * X, a.svx + b * Y * (X + 1), a.with_d ? a.d_in + b * Y * X : nullptr};
}

// u at the sample point (j, i) of an array of kind K: k_l_advect's expressions
template <int K>
__device__ __forceinline__ void mc_u(const McArgs& a, const McSim& m, int j, int i, float& uy, float& ux) {
#pragma clang fp contract(off)
    const int Y = a.Y, X = a.X, XP = X + 1;
    if (K == 0) {
        const int ja = max(j - 1, 0), jb = min(j, Y - 1);
        uy = m.sy[j * X + i];
        ux = 0.25f * (m.sx[ja * XP + i] + m.sx[ja * XP + i + 1] + m.sx[jb * XP + i] + m.sx[jb * XP + i + 1]);
    } else if (K == 1) {
        const int ia = max(i - 1, 0), ib = min(i, X - 1);
        ux = m.sx[j * XP + i];
        uy = 0.25f * (m.sy[j * X + ia] + m.sy[j * X + ib] + m.sy[(j + 1) * X + ia] + m.sy[(j + 1) * X + ib]);
    } else {
        uy = 0.5f * (m.sy[j * X + i] + m.sy[(j + 1) * X + i]);
        ux = 0.5f * (m.sx[j * XP + i] + m.sx[j * XP + i + 1]);
    }
}

// f at an index INSIDE its array
template <int K>
__device__ __forceinline__ float mc_f(const McArgs& a, const McSim& m, int jj, int ii) {
#pragma clang fp contract(off)
    if (K == 0) return m.sy[jj * a.X + ii];
    if (K == 1) return m.sx[jj * (a.X + 1) + ii];
    float v = m.d[jj * a.X + ii];
    if (a.inflow_before) v += a.inflow[jj * a.X + ii];
    return v;
}

// the four corners of the bilinear gather at (j + oy, i + ox) in an array of kind K: rows jj[0..1], columns ii[0..1], their weights, and
// whether a row / column lies inside the array (velocity: always, the indices are clamped; density: outside = the zero ghost ring)
struct McC {
    int jj[2], ii[2];
    bool rin[2], cin[2];
    float wy, wx;
};
template <int K>
__device__ __forceinline__ McC mc_corners(const McArgs& a, int j, int i, float oy, float ox) {
#pragma clang fp contract(off)
    const int H = mc_h<K>(a), W = mc_w<K>(a);
    const float fy = floorf(oy), fx = floorf(ox), big = 268435456.f;      // 2^28: beyond any grid, and j + 2^28 stays an int
    McC s;
    s.wy = oy - fy; s.wx = ox - fx;
    const int jf = j + (int)fminf(fmaxf(fy, -big), big), iF = i + (int)fminf(fmaxf(fx, -big), big);
    if (K < 2) {
        s.jj[0] = clampi(jf, 0, H - 1); s.jj[1] = clampi(jf + 1, 0, H - 1);
        s.ii[0] = clampi(iF, 0, W - 1); s.ii[1] = clampi(iF + 1, 0, W - 1);
        s.rin[0] = s.rin[1] = s.cin[0] = s.cin[1] = true;
    } else {
        s.jj[0] = jf; s.jj[1] = jf + 1; s.ii[0] = iF; s.ii[1] = iF + 1;
        for (int k = 0; k < 2; ++k) { s.rin[k] = s.jj[k] >= 0 && s.jj[k] < H; s.cin[k] = s.ii[k] >= 0 && s.ii[k] < W; }
    }
    return s;
}
// the four values at the corners (at(jj, ii) = the value at an inside index)
template <class At>
__device__ __forceinline__ void mc_values(const McC& s, const At& at, float (&f)[2][2]) {
#pragma unroll
    for (int cj = 0; cj < 2; ++cj)
#pragma unroll
        for (int ci = 0; ci < 2; ++ci) f[cj][ci] = s.rin[cj] && s.cin[ci] ? at(s.jj[cj], s.ii[ci]) : 0.f;
}
__device__ __forceinline__ float mc_bilinear(const McC& s, const float (&f)[2][2]) {
#pragma clang fp contract(off)
    return (1.f - s.wy) * ((1.f - s.wx) * f[0][0] + s.wx * f[0][1]) + s.wy * ((1.f - s.wx) * f[1][0] + s.wx * f[1][1]);
}

// h at (j, i): the semi-Lagrangian value, unmasked, no inflow added -- the ONE expression of it; lo / hi: min / max of the four values read
template <int K>
__device__ __forceinline__ float mc_hat(const McArgs& a, const McSim& m, int j, int i, float& lo, float& hi) {
#pragma clang fp contract(off)
    float uy, ux, f[2][2];
    mc_u<K>(a, m, j, i, uy, ux);
    const McC s = mc_corners<K>(a, j, i, -uy * a.dtdx, -ux * a.dtdx);
    mc_values(s, [&](int jj, int ii) { return mc_f<K>(a, m, jj, ii); }, f);
    lo = fminf(fminf(f[0][0], f[0][1]), fminf(f[1][0], f[1][1]));
    hi = fmaxf(fmaxf(f[0][0], f[0][1]), fmaxf(f[1][0], f[1][1]));
    return mc_bilinear(s, f);
}

// the limiter's decision at (j, i) with h, lo, hi of mc_hat and b = the value carried back: cor, and whether it is kept
__device__ __forceinline__ bool mc_limit(const McArgs& a, float h, float lo, float hi, float fv, float back, float& cor) {
#pragma clang fp contract(off)
    cor = h + a.hs * (fv - back);
    return lo <= cor && cor <= hi;
}

// the step's advected value at (j, i) of simulation b; hat_at(jj, ii) = h at an inside index
template <int K, class HatAt>
__device__ __forceinline__ void mc_point(const McArgs& a, const McSim& m, int b, int j, int i, const HatAt& hat_at) {
#pragma clang fp contract(off)
    float lo, hi, uy, ux, cor, hb[2][2];
    const float h = mc_hat<K>(a, m, j, i, lo, hi);
    mc_u<K>(a, m, j, i, uy, ux);
    const McC s = mc_corners<K>(a, j, i, uy * a.dtdx, ux * a.dtdx);
    mc_values(s, hat_at, hb);
    float v = mc_limit(a, h, lo, hi, mc_f<K>(a, m, j, i), mc_bilinear(s, hb), cor) ? cor : h;
    const int Y = a.Y, X = a.X;
    if (K == 0) a.vy_out[(size_t)b * (Y + 1) * X + j * X + i] = v * mask_y(a.active, Y, X, j, i);
    else if (K == 1) a.vx_out[(size_t)b * Y * (X + 1) + j * (X + 1) + i] = v * mask_x(a.active, Y, X, j, i);
    else {
        if (!a.inflow_before) v += a.inflow[j * X + i] * a.dt;
        a.d_out[(size_t)b * Y * X + j * X + i] = v;
    }
}

// ---- the two-launch form ----
__global__ void __launch_bounds__(256) k_mc_hat(McArgs a) {
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y, k0 = a.with_v ? 0 : nVy + nVx, k1 = nVy + nVx + (a.with_d ? N : 0);
    const McSim m = mc_sim(a, b);
    float lo, hi;
    for (int k = k0 + blockIdx.x * blockDim.x + threadIdx.x; k < k1; k += gridDim.x * blockDim.x) {
        if (k < nVy) a.hy[(size_t)b * nVy + k] = mc_hat<0>(a, m, k / X, k % X, lo, hi);
        else if (k < nVy + nVx) { const int q = k - nVy; a.hx[(size_t)b * nVx + q] = mc_hat<1>(a, m, q / XP, q % XP, lo, hi); }
        else { const int c = k - nVy - nVx; a.hd[(size_t)b * N + c] = mc_hat<2>(a, m, c / X, c % X, lo, hi); }
    }
}

__global__ void __launch_bounds__(256) k_mc_out(McArgs a) {
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y, items = nVy + nVx + (a.with_d ? N : 0);
    const McSim m = mc_sim(a, b);
    const float *hy = a.hy + (size_t)b * nVy, *hx = a.hx + (size_t)b * nVx, *hd = a.hd + (size_t)b * N;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < items; k += gridDim.x * blockDim.x) {
        if (k < nVy) mc_point<0>(a, m, b, k / X, k % X, [&](int jj, int ii) { return hy[jj * X + ii]; });
        else if (k < nVy + nVx) { const int q = k - nVy; mc_point<1>(a, m, b, q / XP, q % XP, [&](int jj, int ii) { return hx[jj * XP + ii]; }); }
        else { const int c = k - nVy - nVx; mc_point<2>(a, m, b, c / X, c % X, [&](int jj, int ii) { return hd[jj * X + ii]; }); }
    }
}

// ---- the tiled form ----
template <int K>
__device__ __forceinline__ void mc_tile(const McArgs& a, int b, int t, float* plane) {
    const int H = mc_h<K>(a), W = mc_w<K>(a);
    const McSim m = mc_sim(a, b);
    const int j0 = (t / a.ntx[K]) * MC_TY, i0 = (t % a.ntx[K]) * MC_TX;       // the tile's first point
    const int oj = j0 - MC_HL, oi = i0 - MC_HL;                                // plane row r holds array row oj + r, column c array column oi + c
    float lo, hi;
    for (int k = threadIdx.x; k < MC_PY * MC_PX; k += MC_THREADS) {
        const int jj = oj + k / MC_PX, ii = oi + k % MC_PX;
        if (jj >= 0 && jj < H && ii >= 0 && ii < W) plane[k] = mc_hat<K>(a, m, jj, ii, lo, hi);
    }
    __syncthreads();
    // h at an inside index: from the plane where it holds it (every inside index within the plane was written above), else on the fly
    auto hat_at = [&](int jj, int ii) {
        const int r = jj - oj, c = ii - oi;
        if ((unsigned)r < (unsigned)MC_PY && (unsigned)c < (unsigned)MC_PX) return plane[r * MC_PX + c];
        float l, h;
        return mc_hat<K>(a, m, jj, ii, l, h);
    };
    for (int k = threadIdx.x; k < MC_TY * MC_TX; k += MC_THREADS) {
        const int j = j0 + k / MC_TX, i = i0 + k % MC_TX;
        if (j < H && i < W) mc_point<K>(a, m, b, j, i, hat_at);
    }
}

__global__ void __launch_bounds__(MC_THREADS) k_mc_tile(McArgs a) {
    __shared__ float plane[MC_PY * MC_PX];
    const int b = blockIdx.y;
    int t = blockIdx.x;
    if (t < a.nt[0]) { mc_tile<0>(a, b, t, plane); return; }
    t -= a.nt[0];
    if (t < a.nt[1]) { mc_tile<1>(a, b, t, plane); return; }
    mc_tile<2>(a, b, t - a.nt[1], plane);
}

// the workspace: h of the three arrays (the two-launch form reads it; sized whatever the option says, the option may change between calls)
struct McLayout {
    float *hy, *hx, *hd;
    size_t bytes;
};
McLayout mc_layout(const sol_karman_cfg* c, void* ws) {
    const size_t B = c->B, Y = c->Y, X = c->X;
    Carve w(ws);
    McLayout l{w.take<float>(B * (Y + 1) * X), w.take<float>(B * Y * (X + 1)), w.take<float>(B * Y * X)};
    l.bytes = w.bytes();
    return l;
}

McArgs mc_args(const sol_karman_cfg* c, float strength, const float* d_in, const float* svy, const float* svx, const float* active, const float* inflow) {
    McArgs a{};
    a.Y = c->Y; a.X = c->X; a.inflow_before = c->inflow_before; a.with_v = 1; a.with_d = d_in != nullptr;
    a.dtdx = c->dt / c->dx; a.dt = c->dt; a.hs = 0.5f * strength;
    a.d_in = d_in; a.svy = svy; a.svx = svx; a.active = active; a.inflow = inflow;
    return a;
}

// ================================================================ adjoint ================================================================
constexpr int MA_T = 16, MA_H = 4, MA_W = MA_T + 2 * MA_H + 1;      // tile of 16 x 16 cells; window of 25 x 25 entries per accumulator array

// the accumulator arrays a kernel scatters into: velocity kernels g_c y, g_c x, G_h y, G_h x; density kernels g_d_in, G_h
enum { MA_CY = 0, MA_CX = 1, MA_HY = 2, MA_HX = 3, MA_D = 0, MA_HD = 1 };

struct MaArgs {
    McArgs f;                           // the forward step's arguments (h arrays filled by k_mc_hat)
    const float *gy, *gx, *gd;          // cotangents: g_a [B][(Y+1)X], [B][Y(X+1)] (masked); g_d_out [B][YX]
    const unsigned* gmax;               // [B][FX_SLOTS]: the scale of this kernel's cotangent
    long long* acc[4];                  // the accumulator arrays (above), [B][...] each
    float *gUy, *gUx;                   // density: back-trace term per cell [B][YX]
};

// where a contribution goes.  MaG: the int64 accumulators in global memory (w[t] = row length of array t).  MaT: the workgroup's LDS window
// of array t when the target lies inside it, else global memory
struct MaG {
    long long* p[4];
    int w[4];
    float qs;
    __device__ __forceinline__ long long* at(int t, int jj, int ii) const { return p[t] + jj * w[t] + ii; }
    __device__ __forceinline__ void operator()(int t, int jj, int ii, float v) const { fx_add(at(t, jj, ii), v, qs); }
};
struct MaT {
    MaG g;
    unsigned long long* L;         // [arrays][MA_W][MA_W]
    int jw0, iw0;
    __device__ __forceinline__ void operator()(int t, int jj, int ii, float v) const {
        const int lj = jj - jw0, li = ii - iw0;
        if ((unsigned)lj < (unsigned)MA_W && (unsigned)li < (unsigned)MA_W) fx_add(&L[(t * MA_W + lj) * MA_W + li], v, g.qs);
        else g(t, jj, ii, v);
    }
};

// g_u of a velocity face (K = 0, 1) onto the five velocity samples that formed u
template <int K, class Add>
__device__ __forceinline__ void ma_u_scatter(const McArgs& a, const Add& add, int j, int i, float guy, float gux) {
#pragma clang fp contract(off)
    const int Y = a.Y, X = a.X;
    if (K == 0) {
        const int ja = max(j - 1, 0), jb = min(j, Y - 1);
        add(MA_CY, j, i, guy);
        const float qx = 0.25f * gux;
        add(MA_CX, ja, i, qx); add(MA_CX, ja, i + 1, qx); add(MA_CX, jb, i, qx); add(MA_CX, jb, i + 1, qx);
    } else {
        const int ia = max(i - 1, 0), ib = min(i, X - 1);
        add(MA_CX, j, i, gux);
        const float qy = 0.25f * guy;
        add(MA_CY, j, ia, qy); add(MA_CY, j, ib, qy); add(MA_CY, j + 1, ia, qy); add(MA_CY, j + 1, ib, qy);
    }
}

// transpose of one bilinear gather with corners s and corner values f: gs times the weights onto array t (inside corners only; the ghost
// ring takes no gradient), and the slopes d(sample)/d(offset) along y and x
template <class Add>
__device__ __forceinline__ void ma_gather_adj(const McC& s, const float (&f)[2][2], const Add& add, int t, float gs, float& dy, float& dx) {
#pragma clang fp contract(off)
    dy = 0.f; dx = 0.f;
#pragma unroll
    for (int cj = 0; cj < 2; ++cj)
#pragma unroll
        for (int ci = 0; ci < 2; ++ci) {
            const float by = cj ? s.wy : 1.f - s.wy, bx = ci ? s.wx : 1.f - s.wx;
            if (s.rin[cj] && s.cin[ci]) add(t, s.jj[cj], s.ii[ci], by * bx * gs);
            dy += (cj ? 1.f : -1.f) * bx * f[cj][ci];
            dx += by * (ci ? 1.f : -1.f) * f[cj][ci];
        }
}

// one point of kind K, stage ST, with cotangent g (stage 2) or g_h (stage 1); hb = the simulation's h array of kind K.  -> g_u
template <int K, int ST, class Add>
__device__ __forceinline__ void ma_point(const McArgs& a, const McSim& m, const float* hb, const Add& add, int j, int i, float g, float& guy, float& gux) {
#pragma clang fp contract(off)
    const int W = mc_w<K>(a);
    const int tf = K == 0 ? MA_CY : (K == 1 ? MA_CX : MA_D), th = K == 0 ? MA_HY : (K == 1 ? MA_HX : MA_HD);
    float uy, ux, dy, dx, f[2][2];
    guy = 0.f; gux = 0.f;
    mc_u<K>(a, m, j, i, uy, ux);
    if (ST == 1) {          // h = S_f(x - u dt)
        const McC s = mc_corners<K>(a, j, i, -uy * a.dtdx, -ux * a.dtdx);
        mc_values(s, [&](int jj, int ii) { return mc_f<K>(a, m, jj, ii); }, f);
        ma_gather_adj(s, f, add, tf, g, dy, dx);
        guy = -a.dtdx * g * dy; gux = -a.dtdx * g * dx;
        return;
    }
    // stage 2: the forward step's decision, operation for operation
    float lo, hi, cor;
    const float h = mc_hat<K>(a, m, j, i, lo, hi);
    const McC s = mc_corners<K>(a, j, i, uy * a.dtdx, ux * a.dtdx);
    mc_values(s, [&](int jj, int ii) { return hb[jj * W + ii]; }, f);
    if (!mc_limit(a, h, lo, hi, mc_f<K>(a, m, j, i), mc_bilinear(s, f), cor)) return;
    const float gf = a.hs * g, gb = -gf;
    add(tf, j, i, gf);
    ma_gather_adj(s, f, add, th, gb, dy, dx);
    guy = a.dtdx * gb * dy; gux = a.dtdx * gb * dx;
}

// the cotangent a stage works on: stage 2 g itself, stage 1 g_h = g + G_h
template <int ST>
__device__ __forceinline__ float ma_cot(float g, const long long* Gh, int q, float qi) {
#pragma clang fp contract(off)
    return ST == 2 ? g : g + fx_get(Gh, q, qi);
}

template <int K, int ST, class Add>
__device__ __forceinline__ void ma_vel_point(const MaArgs& a, const McSim& m, int b, const Add& add, int j, int i, float qi) {
    const int Y = a.f.Y, X = a.f.X, W = mc_w<K>(a.f);
    const size_t n = K == 0 ? (size_t)(Y + 1) * X : (size_t)Y * (X + 1);
    const int q = j * W + i;
    const float g = ma_cot<ST>((K == 0 ? a.gy : a.gx)[b * n + q], a.acc[K == 0 ? MA_HY : MA_HX] + b * n, q, qi);
    if (!(g != 0.f)) return;
    float guy, gux;
    ma_point<K, ST>(a.f, m, (K == 0 ? a.f.hy : a.f.hx) + b * n, add, j, i, g, guy, gux);
    ma_u_scatter<K>(a.f, add, j, i, guy, gux);
}

__device__ __forceinline__ MaG ma_globals_vel(const MaArgs& a, int b, float qs) {
    const size_t Y = a.f.Y, X = a.f.X, nVy = (Y + 1) * X, nVx = Y * (X + 1);
    return MaG{{a.acc[MA_CY] + b * nVy, a.acc[MA_CX] + b * nVx, a.acc[MA_HY] + b * nVy, a.acc[MA_HX] + b * nVx}, {(int)X, (int)X + 1, (int)X, (int)X + 1}, qs};
}

// velocity, every contribution a global int64 atomic (the reference form of the tile kernel)
template <int ST>
__global__ void __launch_bounds__(256) k_ma_vel(MaArgs a) {
    const int Y = a.f.Y, X = a.f.X, XP = X + 1, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const McSim m = mc_sim(a.f, b);
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    const MaG add = ma_globals_vel(a, b, qs);
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nVy + nVx; k += gridDim.x * blockDim.x) {
        if (k < nVy) ma_vel_point<0, ST>(a, m, b, add, k / X, k % X, qi);
        else ma_vel_point<1, ST>(a, m, b, add, (k - nVy) / XP, (k - nVy) % XP, qi);
    }
}

// the same with an LDS window per workgroup (k_lb_advect_adj_tile's shape: a workgroup owns the faces of 16 x 16 cells, the last tile row
// also face row Y, the last tile column face column X); the windows of the arrays this stage does not touch stay zero and flush nothing
template <int ST>
__global__ void __launch_bounds__(256) k_ma_vel_tile(MaArgs a, int nti) {
    __shared__ unsigned long long win[4 * MA_W * MA_W];
    const int Y = a.f.Y, X = a.f.X;
    const int b = blockIdx.y;
    const int j0 = ((int)blockIdx.x / nti) * MA_T, i0 = ((int)blockIdx.x % nti) * MA_T;
    const McSim m = mc_sim(a.f, b);
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    const MaG gadd = ma_globals_vel(a, b, qs);
    const MaT add{gadd, win, j0 - MA_H, i0 - MA_H};
    fx_window_clear(win, 4 * MA_W * MA_W, 256);
    __syncthreads();
    const int j1 = min(j0 + MA_T, Y), i1 = min(i0 + MA_T, X);
    const int j1y = j0 + MA_T >= Y ? Y + 1 : j1, i1x = i0 + MA_T >= X ? X + 1 : i1;
    const int nI = i1 - i0, wX = i1x - i0, nY = (j1y - j0) * nI, nX = (j1 - j0) * wX;
    for (int t = threadIdx.x; t < nY + nX; t += 256) {
        if (t < nY) ma_vel_point<0, ST>(a, m, b, add, j0 + t / nI, i0 + t % nI, qi);
        else ma_vel_point<1, ST>(a, m, b, add, j0 + (t - nY) / wX, i0 + (t - nY) % wX, qi);
    }
    __syncthreads();
    fx_window_flush(win, 4 * MA_W * MA_W, 256, [&](int e) {
        return gadd.at(e / (MA_W * MA_W), j0 - MA_H + (e / MA_W) % MA_W, i0 - MA_H + e % MA_W);
    });
}

// density cell (j, i): stage 2 WRITES its part of gU, stage 1 adds its own
template <int ST, class Add>
__device__ __forceinline__ void ma_den_point(const MaArgs& a, const McSim& m, int b, const Add& add, int j, int i, float qi) {
#pragma clang fp contract(off)
    const size_t N = (size_t)a.f.Y * a.f.X;
    const int c = j * a.f.X + i;
    const float g = ma_cot<ST>(a.gd[b * N + c], a.acc[MA_HD] + b * N, c, qi);
    float guy = 0.f, gux = 0.f;
    if (g != 0.f) ma_point<2, ST>(a.f, m, a.f.hd + b * N, add, j, i, g, guy, gux);
    float *uy = a.gUy + b * N + c, *ux = a.gUx + b * N + c;
    if (ST == 2) { *uy = guy; *ux = gux; }
    else { *uy = *uy + guy; *ux = *ux + gux; }
}

template <int ST>
__global__ void __launch_bounds__(256) k_ma_den(MaArgs a) {
    const int X = a.f.X, N = a.f.Y * X;
    const int b = blockIdx.y;
    const McSim m = mc_sim(a.f, b);
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    const MaG add{{a.acc[MA_D] + (size_t)b * N, a.acc[MA_HD] + (size_t)b * N, nullptr, nullptr}, {X, X, 0, 0}, qs};
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < N; c += gridDim.x * blockDim.x) ma_den_point<ST>(a, m, b, add, c / X, c % X, qi);
}

template <int ST>
__global__ void __launch_bounds__(256) k_ma_den_tile(MaArgs a, int nti) {
    __shared__ unsigned long long win[2 * MA_W * MA_W];
    const int Y = a.f.Y, X = a.f.X, N = Y * X;
    const int b = blockIdx.y;
    const int j0 = ((int)blockIdx.x / nti) * MA_T, i0 = ((int)blockIdx.x % nti) * MA_T;
    const McSim m = mc_sim(a.f, b);
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    const MaG gadd{{a.acc[MA_D] + (size_t)b * N, a.acc[MA_HD] + (size_t)b * N, nullptr, nullptr}, {X, X, 0, 0}, qs};
    const MaT add{gadd, win, j0 - MA_H, i0 - MA_H};
    fx_window_clear(win, 2 * MA_W * MA_W, 256);
    __syncthreads();
    const int j = j0 + (int)threadIdx.x / MA_T, i = i0 + (int)threadIdx.x % MA_T;
    if (j < Y && i < X) ma_den_point<ST>(a, m, b, add, j, i, qi);
    __syncthreads();
    fx_window_flush(win, 2 * MA_W * MA_W, 256, [&](int e) {
        return gadd.at(e / (MA_W * MA_W), j0 - MA_H + (e / MA_W) % MA_W, i0 - MA_H + e % MA_W);
    });
}

// clears `bytes` (a multiple of 4) from p: a kernel, so that a captured schedule holds kernel nodes only
__global__ void __launch_bounds__(256) k_mc_clear(unsigned* __restrict__ p, size_t n) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) p[e] = 0u;
}
int mc_clear(hipStream_t s, void* p, size_t bytes) {
    const size_t n = bytes / 4, nb = (n + 255) / 256;
    SOL_LAUNCH(k_mc_clear, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, s, static_cast<unsigned*>(p), n);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

// the adjoint's workspace: h of the arrays, then the accumulators G_h (velocity: y and x; density: one)
struct MaLayout {
    McLayout h;
    long long *Ghy, *Ghx, *Ghd;
    size_t bytes;
};
MaLayout ma_layout(const sol_karman_cfg* c, void* ws) {
    const size_t B = c->B, Y = c->Y, X = c->X;
    Carve w(ws);
    MaLayout l{};
    l.h = McLayout{w.take<float>(B * (Y + 1) * X), w.take<float>(B * Y * (X + 1)), w.take<float>(B * Y * X), 0};
    l.Ghy = w.take<long long>(B * (Y + 1) * X);
    l.Ghx = w.take<long long>(B * Y * (X + 1));
    l.Ghd = w.take<long long>(B * Y * X);
    l.bytes = w.bytes();
    return l;
}

// ---- the stage alone: what surrounds the two adjoints when no solver step does ----
struct StArgs {
    int Y, X;
    const float *active, *g_ay, *g_ax, *g_d_out;
    float *gay, *gax;                   // the masked velocity cotangent
    unsigned *gmax_v, *gmax_d;          // zeroed beforehand
    const long long *gcy, *gcx, *gD;
    const float *gUy, *gUx;
    float *g_d_in, *g_svy, *g_svx;
};
// PART 0: g_a = mask . g and max|g_a|; 1: max|g_d_out|
template <int PART>
__global__ void __launch_bounds__(256) k_ma_prep(StArgs a) {
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y, items = PART == 0 ? nVy + nVx : N;
    float vmax = 0.f;
    bool bad = false;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < items; k += gridDim.x * blockDim.x) {
        float v;
        if (PART == 1) v = a.g_d_out[(size_t)b * N + k];
        else if (k < nVy) { v = mask_y(a.active, Y, X, k / X, k % X) * a.g_ay[(size_t)b * nVy + k]; a.gay[(size_t)b * nVy + k] = v; }
        else { const int q = k - nVy; v = mask_x(a.active, Y, X, q / XP, q % XP) * a.g_ax[(size_t)b * nVx + q]; a.gax[(size_t)b * nVx + q] = v; }
        vmax = fmaxf(vmax, fabsf(v));
        bad |= !(fabsf(v) <= 3.402823466e38f);
    }
    fx_publish_max((PART == 0 ? a.gmax_v : a.gmax_d) + b * FX_SLOTS, vmax, bad);
}
// g_sv = g_c + the cell-to-face transpose of gU (a centre velocity is the mean of its two faces), g_d_in: back in fp32
__global__ void __launch_bounds__(256) k_ma_finish(StArgs a) {
#pragma clang fp contract(off)
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    float qs, qv, qd;
    fx_scale(a.gmax_v + b * FX_SLOTS, qs, qv);
    fx_scale(a.gmax_d + b * FX_SLOTS, qs, qd);
    // a non-finite cotangent of either kind: every gradient of the simulation is NaN
    const bool poisoned = qv != qv || qd != qd;
    const float nan = __uint_as_float(0x7fc00000u);
    const float *uy = a.gUy + (size_t)b * N, *ux = a.gUx + (size_t)b * N;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nVy + nVx + N; e += gridDim.x * blockDim.x) {
        if (e < nVy) {
            const int j = e / X, i = e - j * X;
            const float lo = j > 0 ? uy[(j - 1) * X + i] : 0.f, hi = j < Y ? uy[j * X + i] : 0.f;
            a.g_svy[(size_t)b * nVy + e] = poisoned ? nan : fx_get(a.gcy + (size_t)b * nVy, e, qv) + 0.5f * (lo + hi);
        } else if (e < nVy + nVx) {
            const int q = e - nVy, j = q / XP, i = q - j * XP;
            const float lo = i > 0 ? ux[j * X + i - 1] : 0.f, hi = i < X ? ux[j * X + i] : 0.f;
            a.g_svx[(size_t)b * nVx + q] = poisoned ? nan : fx_get(a.gcx + (size_t)b * nVx, q, qv) + 0.5f * (lo + hi);
        } else {
            const int c = e - nVy - nVx;
            a.g_d_in[(size_t)b * N + c] = poisoned ? nan : fx_get(a.gD + (size_t)b * N, c, qd);
        }
    }
}

struct StLayout {
    long long *gc, *gD;                 // g_c [B][faces], g_d_in [B][N]
    unsigned* gmax;                     // [2][B][FX_SLOTS]: velocity, density
    float *ga, *gUy, *gUx;
    void* ma;
    size_t bytes;
};
StLayout st_layout(const sol_karman_cfg* c, void* ws) {
    const size_t B = c->B, Y = c->Y, X = c->X, faces = (Y + 1) * X + Y * (X + 1), N = Y * X;
    Carve w(ws);
    StLayout l{w.take<long long>(B * faces), w.take<long long>(B * N), w.take<unsigned>(2 * B * FX_SLOTS), w.take<float>(B * faces), w.take<float>(B * N),
               w.take<float>(B * N), w.take<char>(ma_layout(c, nullptr).bytes)};
    l.bytes = w.bytes();
    return l;
}

bool mc_shape_ok(const sol_karman_cfg* c) { return c && c->B >= 1 && c->B <= 65535 && c->Y >= 16 && c->X >= 16 && (size_t)c->Y * c->X < ((size_t)1 << 28); }

}  // namespace

size_t sol_mc_bytes(const sol_karman_cfg* c) { return mc_layout(c, nullptr).bytes; }
size_t sol_mc_adj_bytes(const sol_karman_cfg* c) { return ma_layout(c, nullptr).bytes; }

// the launches of the MacCormack advection in place of k_l_advect's (d_out NULL: the velocity alone)
int sol_mc_advect(const sol_karman_cfg* c, hipStream_t s, float strength, const float* d_in, const float* svy, const float* svx, const float* active,
                  const float* inflow, float* d_out, float* vy_out, float* vx_out, void* ws) {
    const McLayout l = mc_layout(c, ws);
    McArgs a = mc_args(c, strength, d_out ? d_in : nullptr, svy, svx, active, inflow);
    a.d_out = d_out; a.vy_out = vy_out; a.vx_out = vx_out;
    a.hy = l.hy; a.hx = l.hx; a.hd = l.hd;
    const int Y = c->Y, X = c->X, B = c->B;
    if (sol_opt().k2d_mc_tile) {
        const int hs[3] = {Y + 1, Y, Y}, wd[3] = {X, X + 1, X};
        for (int k = 0; k < 3; ++k) {
            a.ntx[k] = (wd[k] + MC_TX - 1) / MC_TX;
            a.nt[k] = ((hs[k] + MC_TY - 1) / MC_TY) * a.ntx[k];
        }
        if (!a.with_d) a.nt[2] = 0;
        SOL_LAUNCH(k_mc_tile, dim3(a.nt[0] + a.nt[1] + a.nt[2], B), dim3(MC_THREADS), 0, s, a);
    } else {
        const int items = (Y + 1) * X + Y * (X + 1) + (a.with_d ? Y * X : 0);
        SOL_LAUNCH(k_mc_hat, dim3((items + 255) / 256, B), dim3(256), 0, s, a);
        SOL_LAUNCH(k_mc_out, dim3((items + 255) / 256, B), dim3(256), 0, s, a);
    }
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

// The advection adjoint of the VELOCITY in place of k_lb_advect_adj*: g_a (masked, its max published in gmax) -> added onto the cleared
// int64 g_c.  mc = false: stage 1 alone on g_a, the semi-Lagrangian adjoint (sol_karman_advect_bwd with advection = 0).
int sol_mc_adj_vel(const sol_karman_cfg* c, hipStream_t s, bool mc, float strength, const float* svy, const float* svx, const float* gay, const float* gax,
                   const unsigned* gmax, long long* gcy, long long* gcx, void* ws, bool tile) {
    const MaLayout l = ma_layout(c, ws);
    const int Y = c->Y, X = c->X, B = c->B;
    const size_t faces = (size_t)(Y + 1) * X + (size_t)Y * (X + 1);
    MaArgs a{};
    a.f = mc_args(c, strength, nullptr, svy, svx, nullptr, nullptr);
    a.f.hy = l.h.hy; a.f.hx = l.h.hx;
    a.gy = gay; a.gx = gax; a.gmax = gmax;
    a.acc[MA_CY] = gcy; a.acc[MA_CX] = gcx; a.acc[MA_HY] = l.Ghy; a.acc[MA_HX] = l.Ghx;
    const unsigned gF = (unsigned)((faces + 255) / 256);
    const int nti = (X + MA_T - 1) / MA_T, ntiles = ((Y + MA_T - 1) / MA_T) * nti;
    // G_h y and G_h x are neighbours in the layout: one clear (the granule padding between them included)
    if (int e = mc_clear(s, l.Ghy, (size_t)(reinterpret_cast<char*>(l.Ghd) - reinterpret_cast<char*>(l.Ghy)))) return e;
    if (mc) {
        SOL_LAUNCH(k_mc_hat, dim3(gF, B), dim3(256), 0, s, a.f);
        if (tile) SOL_LAUNCH(k_ma_vel_tile<2>, dim3(ntiles, B), dim3(256), 0, s, a, nti);
        else SOL_LAUNCH(k_ma_vel<2>, dim3(gF, B), dim3(256), 0, s, a);
    }
    if (tile) SOL_LAUNCH(k_ma_vel_tile<1>, dim3(ntiles, B), dim3(256), 0, s, a, nti);
    else SOL_LAUNCH(k_ma_vel<1>, dim3(gF, B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

// The advection adjoint of the DENSITY in place of k_kd_advect_adj*: g_d_out (its max in gmax) -> added onto the cleared int64 gD, gU written
int sol_mc_adj_den(const sol_karman_cfg* c, hipStream_t s, bool mc, float strength, const float* d_in, const float* inflow, const float* svy, const float* svx,
                   const float* g_d_out, const unsigned* gmax, long long* gD, float* gUy, float* gUx, void* ws, bool tile) {
    const MaLayout l = ma_layout(c, ws);
    const int Y = c->Y, X = c->X, B = c->B, N = Y * X;
    MaArgs a{};
    a.f = mc_args(c, strength, d_in, svy, svx, nullptr, inflow);
    a.f.with_v = 0;
    a.f.hd = l.h.hd;
    a.gd = g_d_out; a.gmax = gmax;
    a.acc[MA_D] = gD; a.acc[MA_HD] = l.Ghd;
    a.gUy = gUy; a.gUx = gUx;
    const unsigned gN = (unsigned)((N + 255) / 256);
    const int nti = (X + MA_T - 1) / MA_T, ntiles = ((Y + MA_T - 1) / MA_T) * nti;
    if (int e = mc_clear(s, l.Ghd, (size_t)B * N * sizeof(long long))) return e;
    if (mc) {
        SOL_LAUNCH(k_mc_hat, dim3(gN, B), dim3(256), 0, s, a.f);
        if (tile) SOL_LAUNCH(k_ma_den_tile<2>, dim3(ntiles, B), dim3(256), 0, s, a, nti);
        else SOL_LAUNCH(k_ma_den<2>, dim3(gN, B), dim3(256), 0, s, a);
    } else {
        if (int e = mc_clear(s, gUy, (size_t)B * N * sizeof(float))) return e;
        if (int e = mc_clear(s, gUx, (size_t)B * N * sizeof(float))) return e;
    }
    if (tile) SOL_LAUNCH(k_ma_den_tile<1>, dim3(ntiles, B), dim3(256), 0, s, a, nti);
    else SOL_LAUNCH(k_ma_den<1>, dim3(gN, B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

int sol_mc_check(const char* who, int32_t advection, float strength) {
    SOL_REQUIRE(advection == 0 || advection == 1, "%s: advection must be 0 (semi-Lagrangian) or 1 (MacCormack), got %d", who, advection);
    SOL_REQUIRE(strength >= 0.f && strength <= 1.f, "%s: correction_strength must lie in [0, 1] (got %g)", who, (double)strength);
    return SOL_OK;
}

extern "C" size_t sol_karman_advect_workspace_bytes(const sol_karman_cfg* c, int32_t advection) {
    if (!mc_shape_ok(c) || advection != 1) return 0;
    return sol_mc_bytes(c);
}

// The advection stage alone (any Y, X >= 16): (d_in, sv_y, sv_x) -> (d_out, a_y, a_x), the velocity masked, the inflow added as
// cfg.inflow_before says.  advection = 0: k_l_advect (sol_large_advect); 1: the kernels above.
extern "C" int sol_karman_advect(const sol_karman_cfg* c, void* stream, const float* d_in, const float* svy, const float* svx,
                                 const float* active, const float* inflow, int32_t advection, float correction_strength,
                                 float* d_out, float* ay, float* ax, void* workspace, size_t workspace_bytes) {
    const char* who = "sol_karman_advect";
    SOL_REQUIRE(c != nullptr, "%s: cfg is NULL", who);
    SOL_REQUIRE(c->B >= 1 && c->B <= 65535 && c->Y >= 16 && c->X >= 16, "%s: B in [1, 65535], Y, X >= 16 (got %d, %d, %d)", who, c->B, c->Y, c->X);
    SOL_REQUIRE((size_t)c->Y * c->X < ((size_t)1 << 28), "%s: grid too large for 32-bit face indices", who);
    if (int e = sol_mc_check(who, advection, correction_strength)) return e;
    SOL_REQUIRE(d_in && svy && svx && active && inflow && d_out && ay && ax, "%s: NULL pointer argument", who);
    const void* outs[] = {d_out, ay, ax};
    const void* ins[] = {d_in, svy, svx, active, inflow};
    for (const void* o : outs)
        for (const void* i : ins) SOL_REQUIRE(o != i, "%s: outputs must not alias the inputs", who);
    SOL_REQUIRE(d_out != ay && d_out != ax && ay != ax, "%s: d_out, ay and ax must be buffers of their own", who);
    const size_t need = sol_karman_advect_workspace_bytes(c, advection);
    SOL_REQUIRE(need == 0 || workspace != nullptr, "%s: the MacCormack advection needs a workspace (%zu bytes)", who, need);
    SOL_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    if (advection == 0) return sol_large_advect(c, s, d_in, svy, svx, active, inflow, d_out, ay, ax);
    return sol_mc_advect(c, s, correction_strength, d_in, svy, svx, active, inflow, d_out, ay, ax, workspace);
}

extern "C" size_t sol_karman_advect_bwd_workspace_bytes(const sol_karman_cfg* c) {
    if (!mc_shape_ok(c)) return 0;
    return st_layout(c, nullptr).bytes;
}

// The transpose of sol_karman_advect: cotangents of (d_out, a_y, a_x) -> (g_d_in, g_sv_y, g_sv_x).  tile_window: 1 = the LDS windows, 0 =
// global atomics only (equal bits).  Both advections run the kernels of this file (advection = 0: stage 1 alone).
extern "C" int sol_karman_advect_bwd(const sol_karman_cfg* c, void* stream, const float* d_in, const float* svy, const float* svx,
                                     const float* active, const float* inflow, int32_t advection, float correction_strength,
                                     const float* g_d_out, const float* g_ay, const float* g_ax,
                                     float* g_d_in, float* g_svy, float* g_svx, int32_t tile_window, void* workspace, size_t workspace_bytes) {
    const char* who = "sol_karman_advect_bwd";
    SOL_REQUIRE(c != nullptr, "%s: cfg is NULL", who);
    SOL_REQUIRE(c->B >= 1 && c->B <= 65535 && c->Y >= 16 && c->X >= 16, "%s: B in [1, 65535], Y, X >= 16 (got %d, %d, %d)", who, c->B, c->Y, c->X);
    SOL_REQUIRE((size_t)c->Y * c->X < ((size_t)1 << 28), "%s: grid too large for 32-bit face indices", who);
    if (int e = sol_mc_check(who, advection, correction_strength)) return e;
    SOL_REQUIRE(tile_window == 0 || tile_window == 1, "%s: tile_window must be 0 or 1 (got %d)", who, tile_window);
    SOL_REQUIRE(d_in && svy && svx && active && inflow && g_d_out && g_ay && g_ax && g_d_in && g_svy && g_svx && workspace, "%s: NULL pointer argument", who);
    const void* outs[] = {g_d_in, g_svy, g_svx};
    const void* ins[] = {d_in, svy, svx, active, inflow, g_d_out, g_ay, g_ax};
    for (const void* o : outs)
        for (const void* i : ins) SOL_REQUIRE(o != i, "%s: outputs must not alias the inputs", who);
    SOL_REQUIRE(g_d_in != g_svy && g_d_in != g_svx && g_svy != g_svx, "%s: g_d_in, g_svy and g_svx must be buffers of their own", who);
    const StLayout l = st_layout(c, workspace);
    SOL_REQUIRE(workspace_bytes >= l.bytes, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, l.bytes);
    const int B = c->B, Y = c->Y, X = c->X, N = Y * X;
    const size_t nVy = (size_t)(Y + 1) * X, nVx = (size_t)Y * (X + 1), faces = nVy + nVx;
    hipStream_t s = (hipStream_t)stream;
    StArgs a{};
    a.Y = Y; a.X = X; a.active = active; a.g_ay = g_ay; a.g_ax = g_ax; a.g_d_out = g_d_out;
    a.gay = l.ga; a.gax = l.ga + B * nVy;
    a.gmax_v = l.gmax; a.gmax_d = l.gmax + (size_t)B * FX_SLOTS;
    a.gcy = l.gc; a.gcx = l.gc + B * nVy; a.gD = l.gD; a.gUy = l.gUy; a.gUx = l.gUx;
    a.g_d_in = g_d_in; a.g_svy = g_svy; a.g_svx = g_svx;
    // g_c, g_d_in and the absmax slots are neighbours in the layout: one clear
    if (int e = mc_clear(s, l.gc, (size_t)(reinterpret_cast<char*>(l.ga) - reinterpret_cast<char*>(l.gc)))) return e;
    const unsigned gF = (unsigned)((faces + 255) / 256), gN = (unsigned)((N + 255) / 256);
    SOL_LAUNCH(k_ma_prep<0>, dim3(gF, B), dim3(256), 0, s, a);
    SOL_LAUNCH(k_ma_prep<1>, dim3(gN, B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    const bool mc = advection == 1;
    if (int e = sol_mc_adj_vel(c, s, mc, correction_strength, svy, svx, a.gay, a.gax, a.gmax_v, l.gc, l.gc + B * nVy, l.ma, tile_window != 0)) return e;
    if (int e = sol_mc_adj_den(c, s, mc, correction_strength, d_in, inflow, svy, svx, g_d_out, a.gmax_d, l.gD, l.gUy, l.gUx, l.ma, tile_window != 0)) return e;
    SOL_LAUNCH(k_ma_finish, dim3((unsigned)((faces + N + 255) / 256), B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}
