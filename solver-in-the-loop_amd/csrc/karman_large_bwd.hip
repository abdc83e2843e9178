// Adjoint of the large-grid karman-2d step (karman_large.hip) with respect to its input velocity, for both pressure solvers.
// The density is a passive tracer here: its own adjoint is karman_density_bwd.hip, and the buoyant step's coupling (the density pushes the
// velocity) is the one extra launch of sol_karman_step_bwd_large_buoy (karman_buoyancy.hip).  The chain is the 2-D projection of the 3-D adjoint
// (karman3d.hip, "Adjoint of the 3-D step"); stages in reverse order of the forward step:
//   k_lb_rhs          q = G^T (mask . g_out)                  adjoint of  out = v~ - mask . G p.  Boundary faces: with replicate padding
//                                                              their pressure gradient is zero (they do not depend on p), with dirichlet0
//                                                              it is +-p of the adjacent cell.  Side job: clears the scatter accumulators
//                                                              and the absmax slots.
//   pressure          g_div = M^-1 q                           the forward step's solve with the same symmetric matrix
//                                                              (pressure_solve_any2d: direct launches or PCG)
//   k_lb_ga           g_a = mask . (g_out + D^T g_div)         adjoint of rhs = -div and of the hard-BC face masks; publishes max|g_a|
//   k_lb_advect_adj*  scatter of g_a through the bilinear gathers of the semi-Lagrangian step, for the field term AND the back-trace
//                     (velocity) term, into g_c: int64 fixed point, order independent, so the adjoint is reproducible bit for bit
//                     (fixed_scatter.hpp states the scheme, its range, its resolution and what a non-finite g_a does).  The default
//                     form accumulates in an int64 LDS window per 16 x 16-cell tile (halo 4 faces; targets beyond the window go to
//                     global memory) and flushes one vector atomic per non-zero window cell.
//   k_lb_diffuse_adj  g_in = (I + alpha L^T)(g_c . (1 - bcm)) for v_y, (I + alpha L^T) g_c for v_x: gather form of the transposed
//                     replicate-padded Laplacian; converts the fixed-point g_c back to fp32 as it reads it
// sol_karman_step_bwd_large_re: the same launches (bwd_large), then the reduction of g' = g_c . (1 - bcm) against L v_in to the gradient
// with respect to the Reynolds number (karman_re_bwd.hip); it serves the one-workgroup grids too (any Y, X >= 16).
#include "fixed_scatter.hpp"
#include "karman_re.hpp"
#include "large2d.hpp"

namespace {

constexpr int LB_T = 16, LB_H = 4, LB_W = LB_T + 2 * LB_H + 1;      // tile of 16 x 16 cells; window of 25 x 25 faces per component

struct LBArgs {
    int B, Y, X;
    float dtdx, adt;
    int grad_pad;
    const float *re, *active, *bcm;
    long bc_stride;
    const float *svy, *svx;             // saved post-diffusion velocity
    const float *goy, *gox;             // gradient w.r.t. the step's output velocity
    float *gay, *gax;                   // g_a
    long long *gcy, *gcx;               // g_c: int64 fixed-point accumulators [B][faces] (cleared by k_lb_rhs)
    unsigned* gmax;                     // [B][FX_SLOTS] bits of max|g_a| per simulation (cleared by k_lb_rhs, published by k_lb_ga)
    float *giy, *gix;                   // result: gradient w.r.t. the step's input velocity
    float* rhs;
    const float* gdiv;
};

__global__ void __launch_bounds__(256) k_lb_rhs(LBArgs a) {
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const float* gy = a.goy + (size_t)b * nVy;
    const float* gx = a.gox + (size_t)b * nVx;
    const bool keep = a.grad_pad == 1;           // dirichlet0: the boundary faces' gradient depends on p; replicate: it is zero
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < N; c += gridDim.x * blockDim.x) {
        const int j = c / X, i = c - j * X;
        auto wy = [&](int jj) { return (keep || (jj != 0 && jj != Y)) ? mask_y(a.active, Y, X, jj, i) * gy[jj * X + i] : 0.f; };
        auto wx = [&](int ii) { return (keep || (ii != 0 && ii != X)) ? mask_x(a.active, Y, X, j, ii) * gx[j * XP + ii] : 0.f; };
        a.rhs[(size_t)b * N + c] = (wy(j) - wy(j + 1)) + (wx(i) - wx(i + 1));
    }
    // side job: clear slice b of the fixed-point accumulators (y and x components are contiguous: [B][nVy] then [B][nVx]) and the absmax slots
    const size_t faces = (size_t)nVy + nVx;
    long long* zc = a.gcy + (size_t)b * faces;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < faces; e += (size_t)gridDim.x * blockDim.x) zc[e] = 0ll;
    if (blockIdx.x == 0 && threadIdx.x < FX_SLOTS) a.gmax[b * FX_SLOTS + threadIdx.x] = 0u;
}

__global__ void __launch_bounds__(256) k_lb_ga(LBArgs a) {
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const float* P = a.gdiv + (size_t)b * N;
    auto cell = [&](int j, int i) { return ((unsigned)j < (unsigned)Y && (unsigned)i < (unsigned)X) ? P[j * X + i] : 0.f; };
    float vmax = 0.f;
    bool bad = false;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nVy + nVx; k += gridDim.x * blockDim.x) {
        float v;
        if (k < nVy) {
            const int j = k / X, i = k - j * X;
            v = mask_y(a.active, Y, X, j, i) * (a.goy[(size_t)b * nVy + k] + cell(j - 1, i) - cell(j, i));
            a.gay[(size_t)b * nVy + k] = v;
        } else {
            const int q = k - nVy, j = q / XP, i = q - j * XP;
            v = mask_x(a.active, Y, X, j, i) * (a.gox[(size_t)b * nVx + q] + cell(j, i - 1) - cell(j, i));
            a.gax[(size_t)b * nVx + q] = v;
        }
        vmax = fmaxf(vmax, fabsf(v));
        bad |= !(fabsf(v) <= 3.402823466e38f);      // inf or nan (fmaxf drops a NaN)
    }
    fx_publish_max(a.gmax + b * FX_SLOTS, vmax, bad);      // max|g_a| of this simulation -> the scale of the fixed-point scatter
}

// Where a contribution goes (fx_add).  GAdd: straight into the int64 accumulators in global memory.  TAdd: into the workgroup's int64 LDS
// window when the target face lies inside it, else into global memory.
struct GAdd {
    long long *gy, *gx;
    float qs;
    int X;
    __device__ __forceinline__ long long* at(int comp, int jj, int ii) const { return comp == 0 ? gy + jj * X + ii : gx + jj * (X + 1) + ii; }
    __device__ __forceinline__ void operator()(int comp, int jj, int ii, float v) const { fx_add(at(comp, jj, ii), v, qs); }
};
struct TAdd {
    GAdd g;
    unsigned long long* L;         // [2][LB_W][LB_W]
    int jw0, iw0;
    __device__ __forceinline__ void operator()(int comp, int jj, int ii, float v) const {
        const int lj = jj - jw0, li = ii - iw0;
        if ((unsigned)lj < (unsigned)LB_W && (unsigned)li < (unsigned)LB_W) fx_add(&L[(comp * LB_W + lj) * LB_W + li], v, g.qs);
        else g(comp, jj, ii, v);
    }
};

// adjoint of one advected face value of component C (0: v_y [Y+1][X], 1: v_x [Y][X+1]) at (j, i): gs = g_a there.  The departure point
// is recomputed from the saved field with the forward step's expressions (k_l_advect, bil_clamp), operation for operation, so floorf and
// the clamps decide as they did.  No fused multiply-adds: the two scatter kernels are held to the same bits by the test suite.
template <int C, class Add>
__device__ __forceinline__ void lb_advect_adj_point(const LBArgs& a, const float* sy, const float* sx, const Add& add, int j, int i, float gs) {
#pragma clang fp contract(off)
    const int Y = a.Y, X = a.X, XP = X + 1;
    float uy, ux;
    int ja = 0, jb = 0, ia = 0, ib = 0;
    if (C == 0) {
        ja = max(j - 1, 0); jb = min(j, Y - 1);
        uy = sy[j * X + i];
        ux = 0.25f * (sx[ja * XP + i] + sx[ja * XP + i + 1] + sx[jb * XP + i] + sx[jb * XP + i + 1]);
    } else {
        ia = max(i - 1, 0); ib = min(i, X - 1);
        ux = sx[j * XP + i];
        uy = 0.25f * (sy[j * X + ia] + sy[j * X + ib] + sy[(j + 1) * X + ia] + sy[(j + 1) * X + ib]);
    }
    const int H = Y + (C == 0), W = X + (C == 1);
    const float* f = C == 0 ? sy : sx;
    const float oy = -uy * a.dtdx, ox = -ux * a.dtdx;
    const float fy = floorf(oy), fx = floorf(ox);
    const float wy = oy - fy, wx = ox - fx;
    const int jf = j + (int)fy, iF = i + (int)fx;
    const int j0 = clampi(jf, 0, H - 1), j1 = clampi(jf + 1, 0, H - 1);
    const int i0 = clampi(iF, 0, W - 1), i1 = clampi(iF + 1, 0, W - 1);
    float dy = 0.f, dx = 0.f;                    // d(sample) / d(offset) along each axis
#pragma unroll
    for (int cj = 0; cj < 2; ++cj)
#pragma unroll
        for (int ci = 0; ci < 2; ++ci) {
            const int jj = cj ? j1 : j0, ii = ci ? i1 : i0;
            const float by = cj ? wy : 1.f - wy, bx = ci ? wx : 1.f - wx;
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
        add(1, ja, i, qx); add(1, ja, i + 1, qx); add(1, jb, i, qx); add(1, jb, i + 1, qx);
    } else {
        add(1, j, i, gux);
        const float qy = 0.25f * guy;
        add(0, j, ia, qy); add(0, j, ib, qy); add(0, j + 1, ia, qy); add(0, j + 1, ib, qy);
    }
}

// every contribution a global int64 atomic (option k2d_adj_tile = 0; the reference form of the tile kernel)
__global__ void __launch_bounds__(256) k_lb_advect_adj(LBArgs a) {
    const int Y = a.Y, X = a.X, XP = X + 1, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const float* sy = a.svy + (size_t)b * nVy;
    const float* sx = a.svx + (size_t)b * nVx;
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    const GAdd add{a.gcy + (size_t)b * nVy, a.gcx + (size_t)b * nVx, qs, X};
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nVy + nVx; k += gridDim.x * blockDim.x) {
        if (k < nVy) {
            const float g = a.gay[(size_t)b * nVy + k];
            if (g != 0.f) lb_advect_adj_point<0>(a, sy, sx, add, k / X, k % X, g);
        } else {
            const int q = k - nVy;
            const float g = a.gax[(size_t)b * nVx + q];
            if (g != 0.f) lb_advect_adj_point<1>(a, sy, sx, add, q / XP, q % XP, g);
        }
    }
}

// The same scatter with an LDS window per workgroup: a workgroup owns the faces of 16 x 16 cells (the last tile row also face row Y, the
// last tile column face column X) and accumulates into a 25 x 25 int64 window per component (10 KB); the nine contributions of a face --
// four corners of its bilinear gather, five back-trace terms -- land within |u| dt/dx + 1 faces of it.  Targets beyond the halo of 4 go
// to global memory directly, so any CFL number is handled.  Integer adds commute: the result equals k_lb_advect_adj's bit for bit.
__global__ void __launch_bounds__(256) k_lb_advect_adj_tile(LBArgs a, int nti) {
    __shared__ unsigned long long win[2 * LB_W * LB_W];
    const int Y = a.Y, X = a.X, XP = X + 1, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const int tj = (int)blockIdx.x / nti, ti = (int)blockIdx.x % nti, j0 = tj * LB_T, i0 = ti * LB_T;
    const float* sy = a.svy + (size_t)b * nVy;
    const float* sx = a.svx + (size_t)b * nVx;
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    const GAdd gadd{a.gcy + (size_t)b * nVy, a.gcx + (size_t)b * nVx, qs, X};
    const TAdd add{gadd, win, j0 - LB_H, i0 - LB_H};
    fx_window_clear(win, 2 * LB_W * LB_W, 256);
    __syncthreads();
    const int j1 = min(j0 + LB_T, Y), i1 = min(i0 + LB_T, X);
    const int j1y = j0 + LB_T >= Y ? Y + 1 : j1, i1x = i0 + LB_T >= X ? X + 1 : i1;
    const int nI = i1 - i0, wX = i1x - i0, nY = (j1y - j0) * nI, nX = (j1 - j0) * wX;
    for (int t = threadIdx.x; t < nY + nX; t += 256) {
        if (t < nY) {
            const int j = j0 + t / nI, i = i0 + t % nI;
            const float g = a.gay[(size_t)b * nVy + j * X + i];
            if (g != 0.f) lb_advect_adj_point<0>(a, sy, sx, add, j, i, g);
        } else {
            const int q = t - nY, j = j0 + q / wX, i = i0 + q % wX;
            const float g = a.gax[(size_t)b * nVx + j * XP + i];
            if (g != 0.f) lb_advect_adj_point<1>(a, sy, sx, add, j, i, g);
        }
    }
    __syncthreads();
    fx_window_flush(win, 2 * LB_W * LB_W, 256, [&](int e) {
        const int li = e % LB_W, lj = (e / LB_W) % LB_W, comp = e / (LB_W * LB_W);
        return gadd.at(comp, j0 - LB_H + lj, i0 - LB_H + li);
    });
}

__global__ void __launch_bounds__(256) k_lb_diffuse_adj(LBArgs a) {
    const int Y = a.Y, X = a.X, XP = X + 1, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const float alpha = a.adt / a.re[b];
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    // g' + alpha L^T g' with the rounded g' as the addend of ONE fused multiply-add, spelled out: left to the compiler, which product is
    // fused depends on the surrounding code, and the bits move with it
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nVy + nVx; e += gridDim.x * blockDim.x) {
        if (e < nVy) {
            const int j = e / X, i = e - j * X;
            const long long* g = a.gcy + (size_t)b * nVy;
            const float* m = a.bcm + (size_t)b * a.bc_stride;          // g' = g . (1 - bcm): the BC blend's adjoint
            const float sc = 1.f - m[e];
            a.giy[(size_t)b * nVy + e] = __fmaf_rn(alpha, lapT<2>(g, qi, sc, m, e, {j, i}, {Y + 1, X}), fx_get(g, e, qi) * sc);
        } else {
            const int q = e - nVy, j = q / XP, i = q - j * XP;
            const long long* g = a.gcx + (size_t)b * nVx;
            a.gix[(size_t)b * nVx + q] = __fmaf_rn(alpha, lapT<2>(g, qi, 1.f, nullptr, q, {j, i}, {Y, XP}), fx_get(g, q, qi));
        }
    }
}

// the adjoint's own buffers in front of the solver's part: g_c (int64), g_a (fp32), the absmax slots; with re, the partial sums of the
// Reynolds-number reduction behind it; 256-byte granules
struct BwdLayout {
    long long* gc;
    float* ga;
    unsigned* gmax;
    void* solver;
    double* partial;
    void* mc;                           // the _adv forms with the MacCormack advection: what sol_mc_adj_vel takes, behind everything else
    size_t bytes;
};
BwdLayout bwd_layout(const sol_karman_cfg* c, bool direct, bool re, void* ws, const int32_t* hdr = nullptr, bool mc = false) {
    const size_t B = c->B, Y = c->Y, X = c->X, faces = (Y + 1) * X + Y * (X + 1);
    Carve w(ws);
    BwdLayout l{w.take<long long>(B * faces), w.take<float>(B * faces), w.take<unsigned>(B * FX_SLOTS), w.take<char>(sol_large_solver_bytes(c, direct, hdr))};
    if (re) l.partial = sol_re_partial_take(w, c);
    if (mc) l.mc = w.take<char>(sol_mc_adj_bytes(c));
    l.bytes = w.bytes();
    return l;
}

int common_check(const sol_karman_cfg* c, const char* who) {
    SOL_REQUIRE(c != nullptr, "%s: cfg is NULL", who);
    SOL_REQUIRE(c->B >= 1 && c->B <= 65535 && c->Y >= 16 && c->X >= 16, "%s: B in [1, 65535], Y, X >= 16 (got %d, %d, %d)", who, c->B, c->Y, c->X);
    SOL_REQUIRE((size_t)c->Y * c->X < ((size_t)1 << 28), "%s: grid too large for 32-bit face indices", who);
    return SOL_OK;
}

}  // namespace

extern "C" size_t sol_karman_step_bwd_large_workspace_bytes(const sol_karman_cfg* c) {
    if (!c || c->B < 1 || c->Y < 1 || c->X < 1) return 0;
    return bwd_layout(c, c->direct != nullptr, false, nullptr).bytes;
}

extern "C" size_t sol_karman_step_bwd_large_workspace_bytes_for(const sol_karman_cfg* c, const int32_t* direct_header_host) {
    if (!c || c->B < 1 || c->Y < 1 || c->X < 1) return 0;
    return bwd_layout(c, c->direct != nullptr, false, nullptr, direct_header_host).bytes;
}

namespace {

// the buoyant step's extra (sol_karman_step_bwd_large_buoy): the force, the cotangent of the step's output density (NULL = zero) and where
// g_dsum [B,Y,X] goes -- what the caller hands to the density adjoint as ITS g_d_out
struct BuoyExtra {
    float fy, fx;
    const float* g_d_out;
    float* g_dsum;
};

// the _adv forms' extra: which advection the forward step ran (1: MacCormack, karman_maccormack.hip) and its correction strength
struct AdvExtra {
    int32_t advection;
    float strength;
};

// the launches of sol_karman_step_bwd_large; with bx, followed by the transpose of the buoyancy term over the g_a they leave in the
// workspace (k_lb_buoyancy_adj, karman_buoyancy.hip); with rx, followed by the Reynolds-number reduction over the g_c they leave in the workspace
// (sol_karman_step_bwd_large_re): g_vy_in / g_vx_in are the same launches' results either way
int bwd_large(const char* who, const sol_karman_cfg* c, void* stream,
              const float* saved_vy, const float* saved_vx, const float* re, const float* active,
              const float* velBCyMask, int64_t bc_batch_stride,
              const float* g_vy_out, const float* g_vx_out, float* g_vy_in, float* g_vx_in,
              const int32_t* direct_header_host,
              const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
              void* workspace, size_t workspace_bytes, const ReExtra* rx, const BuoyExtra* bx = nullptr, const AdvExtra* ax = nullptr) {
    if (int e = common_check(c, who)) return e;
    if (ax)
        if (int e = sol_mc_check(who, ax->advection, ax->strength)) return e;
    const bool mc = ax && ax->advection == 1;
    SOL_REQUIRE(!rx || (rx->vy_in && rx->vx_in && rx->g_re), "%s: NULL pointer argument", who);
    SOL_REQUIRE(!bx || bx->g_dsum, "%s: NULL pointer argument (g_dsum)", who);
    SOL_REQUIRE(!bx || (bx->fy - bx->fy == 0.f && bx->fx - bx->fx == 0.f), "%s: the force must be finite", who);
    const bool direct = c->direct != nullptr;
    SOL_REQUIRE(saved_vy && saved_vx && re && active && velBCyMask && g_vy_out && g_vx_out && g_vy_in && g_vx_in && workspace,
                "%s: NULL pointer argument", who);
    if (direct) { if (int e = sol_large_direct_check(c, who, direct_header_host)) return e; }
    else if (int e = sol_large_cg_check(c, who, box_blob, box_header_host, cg_info, workspace)) return e;
    const BwdLayout l = bwd_layout(c, direct, rx != nullptr, workspace, direct ? direct_header_host : nullptr, mc);
    SOL_REQUIRE(workspace_bytes >= l.bytes, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, l.bytes);
    const void* outs[] = {g_vy_in, g_vx_in, cg_info, rx ? rx->g_re : nullptr, bx ? bx->g_dsum : nullptr};
    const void* ins[] = {saved_vy, saved_vx, re, active, velBCyMask, g_vy_out, g_vx_out, box_blob, rx ? rx->vy_in : nullptr, rx ? rx->vx_in : nullptr,
                         bx ? bx->g_d_out : nullptr};
    for (const void* o : outs)
        for (const void* i : ins) SOL_REQUIRE(!o || o != i, "%s: outputs must not alias the inputs", who);
    SOL_REQUIRE(g_vy_in != g_vx_in, "%s: g_vy_in and g_vx_in must be buffers of their own", who);
    SOL_REQUIRE(!rx || (rx->g_re != g_vy_in && rx->g_re != g_vx_in && (void*)rx->g_re != (void*)cg_info), "%s: g_re must be a buffer of its own", who);
    SOL_REQUIRE(!bx || (bx->g_dsum != g_vy_in && bx->g_dsum != g_vx_in && (void*)bx->g_dsum != (void*)cg_info && (!rx || bx->g_dsum != rx->g_re)),
                "%s: g_dsum must be a buffer of its own", who);
    const int B = c->B, Y = c->Y, X = c->X, N = Y * X;
    const size_t nVy = (size_t)(Y + 1) * X, nVx = (size_t)Y * (X + 1), faces = nVy + nVx;
    hipStream_t s = (hipStream_t)stream;
    LBArgs a{};
    a.B = B; a.Y = Y; a.X = X; a.dtdx = c->dt / c->dx; a.adt = c->dt * c->res * c->res; a.grad_pad = c->grad_pad;
    a.re = re; a.active = active; a.bcm = velBCyMask; a.bc_stride = bc_batch_stride;
    a.svy = saved_vy; a.svx = saved_vx; a.goy = g_vy_out; a.gox = g_vx_out;
    a.gcy = l.gc; a.gcx = l.gc + B * nVy;
    a.gay = l.ga; a.gax = l.ga + B * nVy;
    a.gmax = l.gmax;
    a.giy = g_vy_in; a.gix = g_vx_in;
    a.rhs = sol_large_solver_rhs(c, direct, l.solver);
    const unsigned gN = (unsigned)((N + 255) / 256), gF = (unsigned)((faces + 255) / 256);
    // periodic axes (the direct blob's header bits): the same five stages with wrapped indices, karman_periodic.hip
    const int periodic = direct ? sol_periodic_bits(direct_header_host) : 0;
    SOL_REQUIRE(direct || !sol_periodic_bits(box_header_host), "%s: the CG pressure solve is not built for periodic scenes; use the direct solve", who);
    if (periodic) {
        SOL_REQUIRE(!rx && !bx && !mc, "%s: periodic scenes run the plain velocity adjoint only: the gradient in re, the buoyancy force and the "
                    "mac_cormack advection are not built for them (use sol_karman_step_bwd_large)", who);
        SolPeriodicBwd pa{B, Y, X, periodic, a.dtdx, a.adt, a.grad_pad, re, active, velBCyMask, (long)bc_batch_stride, saved_vy, saved_vx, g_vy_out, g_vx_out,
                          a.gay, a.gax, a.gcy, a.gcx, a.gmax, g_vy_in, g_vx_in, a.rhs, nullptr};
        if (int e = sol_periodic_bwd_rhs(s, pa)) return e;
        float* pq = nullptr;
        if (int e = pressure_solve_any2d(s, c, direct, direct_header_host, box_blob, active, cg_info, l.solver, &pq)) return e;
        pa.gdiv = pq;
        return sol_periodic_bwd_tail(s, pa);
    }
    SOL_LAUNCH(k_lb_rhs, dim3(gN, B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    float* q = nullptr;
    if (int e = pressure_solve_any2d(s, c, direct, direct_header_host, box_blob, active, cg_info, l.solver, &q)) return e;
    a.gdiv = q;
    SOL_LAUNCH(k_lb_ga, dim3(gF, B), dim3(256), 0, s, a);
    if (mc) {
        if (int e = sol_mc_adj_vel(c, s, true, ax->strength, saved_vy, saved_vx, a.gay, a.gax, a.gmax, a.gcy, a.gcx, l.mc, sol_opt().k2d_adj_tile != 0)) return e;
    } else if (sol_opt().k2d_adj_tile) {
        const int ntj = (Y + LB_T - 1) / LB_T, nti = (X + LB_T - 1) / LB_T;
        SOL_LAUNCH(k_lb_advect_adj_tile, dim3(ntj * nti, B), dim3(256), 0, s, a, nti);
    } else {
        SOL_LAUNCH(k_lb_advect_adj, dim3(gF, B), dim3(256), 0, s, a);
    }
    SOL_LAUNCH(k_lb_diffuse_adj, dim3(gF, B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    // g_dsum = g_d_out + dt F . (face-to-cell transpose of g_a); a poisoned simulation (gmax) gets NaN throughout
    if (bx)
        if (int e = sol_buoyancy_adj(s, B, Y, X, active, a.gay, a.gax, a.gmax, c->dt * bx->fy, c->dt * bx->fx, bx->g_d_out, bx->g_dsum)) return e;
    if (!rx) return SOL_OK;
    // g' of the Reynolds-number gradient = the fixed-point g_c that k_lb_diffuse_adj has just read (. (1 - bcm) on v_y)
    ReIn in{};
    in.src = RE_FIXED;
    in.gcy = a.gcy; in.gcx = a.gcx; in.gmax = a.gmax; in.bcm = velBCyMask; in.bc_stride = bc_batch_stride;
    in.vy_in = rx->vy_in; in.vx_in = rx->vx_in; in.re = re;
    in.partial = l.partial;
    in.g_re = rx->g_re; in.accumulate = rx->accumulate;
    return sol_re_reduce(s, c, in);
}

}  // namespace

extern "C" int sol_karman_step_bwd_large(const sol_karman_cfg* c, void* stream,
                                         const float* saved_vy, const float* saved_vx, const float* re, const float* active,
                                         const float* velBCyMask, int64_t bc_batch_stride,
                                         const float* g_vy_out, const float* g_vx_out, float* g_vy_in, float* g_vx_in,
                                         const int32_t* direct_header_host,
                                         const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                         void* workspace, size_t workspace_bytes) {
    return bwd_large("sol_karman_step_bwd_large", c, stream, saved_vy, saved_vx, re, active, velBCyMask, bc_batch_stride, g_vy_out, g_vx_out,
                     g_vy_in, g_vx_in, direct_header_host, box_blob, box_header_host, cg_info, workspace, workspace_bytes, nullptr);
}

extern "C" size_t sol_karman_step_bwd_large_re_workspace_bytes_for(const sol_karman_cfg* c, const int32_t* direct_header_host) {
    if (!c || c->B < 1 || c->Y < 1 || c->X < 1) return 0;
    return bwd_layout(c, c->direct != nullptr, true, nullptr, direct_header_host).bytes;
}

extern "C" int sol_karman_step_bwd_large_re(const sol_karman_cfg* c, void* stream,
                                            const float* saved_vy, const float* saved_vx, const float* re, const float* active,
                                            const float* velBCyMask, int64_t bc_batch_stride,
                                            const float* g_vy_out, const float* g_vx_out, float* g_vy_in, float* g_vx_in,
                                            const int32_t* direct_header_host,
                                            const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                            void* workspace, size_t workspace_bytes,
                                            const float* vy_in, const float* vx_in, float* g_re, int accumulate_re) {
    const ReExtra rx{vy_in, vx_in, g_re, accumulate_re};
    return bwd_large("sol_karman_step_bwd_large_re", c, stream, saved_vy, saved_vx, re, active, velBCyMask, bc_batch_stride, g_vy_out, g_vx_out,
                     g_vy_in, g_vx_in, direct_header_host, box_blob, box_header_host, cg_info, workspace, workspace_bytes, &rx);
}

// The adjoint of the BUOYANT large-grid step (sol_karman_step_fwd_large_saved_buoy): sol_karman_step_bwd_large's launches, then
// k_lb_buoyancy_adj.  The caller runs sol_karman_density_bwd (accumulate = 1) on g_dsum next.
extern "C" int sol_karman_step_bwd_large_buoy(const sol_karman_cfg* c, void* stream,
                                              const float* saved_vy, const float* saved_vx, const float* re, const float* active,
                                              const float* velBCyMask, int64_t bc_batch_stride,
                                              const float* g_vy_out, const float* g_vx_out, float* g_vy_in, float* g_vx_in,
                                              const int32_t* direct_header_host,
                                              const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                              void* workspace, size_t workspace_bytes,
                                              float fy, float fx, const float* g_d_out, float* g_dsum) {
    const BuoyExtra bx{fy, fx, g_d_out, g_dsum};
    return bwd_large("sol_karman_step_bwd_large_buoy", c, stream, saved_vy, saved_vx, re, active, velBCyMask, bc_batch_stride, g_vy_out, g_vx_out,
                     g_vy_in, g_vx_in, direct_header_host, box_blob, box_header_host, cg_info, workspace, workspace_bytes, nullptr, &bx);
}

extern "C" int sol_karman_step_bwd_large_buoy_re(const sol_karman_cfg* c, void* stream,
                                                 const float* saved_vy, const float* saved_vx, const float* re, const float* active,
                                                 const float* velBCyMask, int64_t bc_batch_stride,
                                                 const float* g_vy_out, const float* g_vx_out, float* g_vy_in, float* g_vx_in,
                                                 const int32_t* direct_header_host,
                                                 const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                                 void* workspace, size_t workspace_bytes,
                                                 const float* vy_in, const float* vx_in, float* g_re, int accumulate_re,
                                                 float fy, float fx, const float* g_d_out, float* g_dsum) {
    const ReExtra rx{vy_in, vx_in, g_re, accumulate_re};
    const BuoyExtra bx{fy, fx, g_d_out, g_dsum};
    return bwd_large("sol_karman_step_bwd_large_buoy_re", c, stream, saved_vy, saved_vx, re, active, velBCyMask, bc_batch_stride, g_vy_out, g_vx_out,
                     g_vy_in, g_vx_in, direct_header_host, box_blob, box_header_host, cg_info, workspace, workspace_bytes, &rx, &bx);
}

// The _adv forms: every argument of the _buoy / _buoy_re form, then the advection the forward step ran (0: semi-Lagrangian -- that form's
// launches and bits; 1: MacCormack -- sol_mc_adj_vel in place of k_lb_advect_adj*) and its correction strength.  A zero force with
// g_d_out = NULL is the unbuoyant adjoint plus one launch that writes g_dsum = 0.
extern "C" size_t sol_karman_step_bwd_large_adv_workspace_bytes_for(const sol_karman_cfg* c, const int32_t* direct_header_host, int32_t with_re, int32_t advection) {
    if (!c || c->B < 1 || c->Y < 1 || c->X < 1) return 0;
    return bwd_layout(c, c->direct != nullptr, with_re != 0, nullptr, direct_header_host, advection == 1).bytes;
}

extern "C" int sol_karman_step_bwd_large_adv(const sol_karman_cfg* c, void* stream,
                                             const float* saved_vy, const float* saved_vx, const float* re, const float* active,
                                             const float* velBCyMask, int64_t bc_batch_stride,
                                             const float* g_vy_out, const float* g_vx_out, float* g_vy_in, float* g_vx_in,
                                             const int32_t* direct_header_host,
                                             const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                             void* workspace, size_t workspace_bytes,
                                             float fy, float fx, const float* g_d_out, float* g_dsum,
                                             int32_t advection, float correction_strength) {
    const BuoyExtra bx{fy, fx, g_d_out, g_dsum};
    const AdvExtra ax{advection, correction_strength};
    return bwd_large("sol_karman_step_bwd_large_adv", c, stream, saved_vy, saved_vx, re, active, velBCyMask, bc_batch_stride, g_vy_out, g_vx_out,
                     g_vy_in, g_vx_in, direct_header_host, box_blob, box_header_host, cg_info, workspace, workspace_bytes, nullptr, &bx, &ax);
}

extern "C" int sol_karman_step_bwd_large_adv_re(const sol_karman_cfg* c, void* stream,
                                                const float* saved_vy, const float* saved_vx, const float* re, const float* active,
                                                const float* velBCyMask, int64_t bc_batch_stride,
                                                const float* g_vy_out, const float* g_vx_out, float* g_vy_in, float* g_vx_in,
                                                const int32_t* direct_header_host,
                                                const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                                void* workspace, size_t workspace_bytes,
                                                const float* vy_in, const float* vx_in, float* g_re, int accumulate_re,
                                                float fy, float fx, const float* g_d_out, float* g_dsum,
                                                int32_t advection, float correction_strength) {
    const ReExtra rx{vy_in, vx_in, g_re, accumulate_re};
    const BuoyExtra bx{fy, fx, g_d_out, g_dsum};
    const AdvExtra ax{advection, correction_strength};
    return bwd_large("sol_karman_step_bwd_large_adv_re", c, stream, saved_vy, saved_vx, re, active, velBCyMask, bc_batch_stride, g_vy_out, g_vx_out,
                     g_vy_in, g_vx_in, direct_header_host, box_blob, box_header_host, cg_info, workspace, workspace_bytes, &rx, &bx, &ax);
}
