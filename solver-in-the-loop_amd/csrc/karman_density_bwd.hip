// Adjoint of the karman-2d step's marker density: the gradient of a loss on d_out with respect to d_in and -- through the departure points
// of the density's semi-Lagrangian advection -- to the step's input velocity.  The density path is linear in the cotangents and meets the
// velocity path only at the post-diffusion velocity c = saved_vy / saved_vx, so it is a set of launches of its own, chip wide on global
// memory, for the one-workgroup grids and the large grids alike (the solver kernels and their adjoints are not involved):
//   k_kd_clear         clears the int64 accumulators of g_d_in and publishes max|g_d_out| per simulation (the scale of the scatter)
//   k_kd_advect_adj*   per cell: the departure point recomputed from c with the forward step's expressions (k_l_advect's density branch =
//                      karman_step.hip's), the field term scattered into g_d_in in 64-bit fixed point (fixed_scatter.hpp: order independent,
//                      bit reproducible; what a non-finite cotangent does), the back-trace term gU = -dt/dx g slope written per cell.
//                      The default form accumulates in an int64 LDS window per 16 x 16-cell tile (halo 4 cells; targets beyond it go to
//                      global memory, so any CFL number is handled); option k2d_dens_adj_tile = 0: every contribution a global atomic
//   k_kd_diffuse_adj   g_c = the cell-to-face transpose of gU (a centre velocity is the mean of its two faces), gathered on the fly, then
//                      the diffusion / boundary-condition adjoint of k_lb_diffuse_adj: g_vy_in = (I + alpha L^T)((1 - bcm) g_cy),
//                      g_vx_in = (I + alpha L^T) g_cx, written or added onto the velocity adjoint's result; converts g_d_in back to fp32
// sol_karman_density_bwd_re: the same launches (density_bwd), then the reduction of that g' against L v_in to the density path's part of
// the gradient with respect to the Reynolds number (karman_re_bwd.hip).
#include "fixed_scatter.hpp"
#include "karman_re.hpp"

namespace {

constexpr int KD_T = 16, KD_H = 4, KD_W = KD_T + 2 * KD_H + 1;      // tile of 16 x 16 cells; window of 25 x 25 cells

struct KDArgs {
    int B, Y, X;
    float dtdx, adt;
    int inflow_before, accumulate;
    const float *d_in, *inflow, *svy, *svx, *re, *bcm;
    long bc_stride;
    const float* gdo;                   // gradient w.r.t. the step's output density
    long long* gD;                      // int64 fixed-point accumulators of g_d_in [B][Y][X]
    float *gUy, *gUx;                   // back-trace term per cell [B][Y][X]: gradient w.r.t. the centre velocity the cell was traced with
    unsigned* gmax;                     // [B][FX_SLOTS] bits of max|g_d_out| per simulation: slot k is WRITTEN by workgroup k of k_kd_clear
    float *gdi, *giy, *gix;             // results
};

// gridDim.x == FX_SLOTS: every workgroup owns one absmax slot of its simulation and stores it (no atomics, nothing to clear beforehand)
__global__ void __launch_bounds__(256) k_kd_clear(KDArgs a) {
    __shared__ unsigned red[4];
    const int N = a.Y * a.X, b = blockIdx.y;
    const float* g = a.gdo + (size_t)b * N;
    long long* z = a.gD + (size_t)b * N;
    float vmax = 0.f;
    bool bad = false;
    for (int c = blockIdx.x * 256 + threadIdx.x; c < N; c += FX_SLOTS * 256) {
        z[c] = 0ll;
        const float v = fabsf(g[c]);
        vmax = fmaxf(vmax, v);
        bad |= !(v <= 3.402823466e38f);          // inf or nan (fmaxf drops a NaN)
    }
    const unsigned wmax = amax_wave_max(bad ? 0x7fc00000u : __float_as_uint(vmax));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wmax;
    __syncthreads();
    if (threadIdx.x == 0) a.gmax[b * FX_SLOTS + blockIdx.x] = max(max(red[0], red[1]), max(red[2], red[3]));
}

// Where a field-term contribution goes (fx_add).  KGAdd: straight into the accumulators in global memory.  KTAdd: into the workgroup's LDS
// window when the target cell lies inside it, else into global memory.
struct KGAdd {
    long long* g;
    float qs;
    int X;
    __device__ __forceinline__ void operator()(int jj, int ii, float v) const { fx_add(g + jj * X + ii, v, qs); }
};
struct KTAdd {
    KGAdd g;
    unsigned long long* L;         // [KD_W][KD_W]
    int jw0, iw0;
    __device__ __forceinline__ void operator()(int jj, int ii, float v) const {
        const int lj = jj - jw0, li = ii - iw0;
        if ((unsigned)lj < (unsigned)KD_W && (unsigned)li < (unsigned)KD_W) fx_add(&L[lj * KD_W + li], v, g.qs);
        else g(jj, ii, v);
    }
};

// adjoint of the advected density of cell (j, i) of simulation b.  The departure point is recomputed from the saved field with the forward
// step's expressions, operation for operation, so floorf decides as it did.  No fused multiply-adds: the two scatter kernels are held to
// the same bits by the test suite.
template <class Add>
__device__ __forceinline__ void kd_point(const KDArgs& a, int b, const float* sy, const float* sx, const Add& add, int j, int i) {
#pragma clang fp contract(off)
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, c = j * X + i;
    const float g = a.gdo[(size_t)b * N + c];
    float guy = 0.f, gux = 0.f;
    if (g != 0.f) {
        const float* gd = a.d_in + (size_t)b * N;
        const float uy = 0.5f * (sy[c] + sy[c + X]);
        const float ux = 0.5f * (sx[j * XP + i] + sx[j * XP + i + 1]);
        const float oy = -uy * a.dtdx, ox = -ux * a.dtdx;
        const float fy = floorf(oy), fx = floorf(ox);
        const float wy = oy - fy, wx = ox - fx;
        const int j0 = j + (int)fy, i0 = i + (int)fx;
        float f[2][2];
#pragma unroll
        for (int dj = 0; dj < 2; ++dj)
#pragma unroll
            for (int di = 0; di < 2; ++di) {
                const int jj = j0 + dj, ii = i0 + di;
                float v = 0.f;   // one ring of zero ghost cells: it takes no gradient
                if (jj >= 0 && jj < Y && ii >= 0 && ii < X) {
                    v = gd[jj * X + ii];
                    if (a.inflow_before) v += a.inflow[jj * X + ii];
                    add(jj, ii, (dj ? wy : 1.f - wy) * (di ? wx : 1.f - wx) * g);      // field term
                }
                f[dj][di] = v;
            }
        // back-trace term: offset = -dtdx * u(cell), d(sample) / d(offset) = the bilinear slopes
        const float s_y = (1.f - wx) * (f[1][0] - f[0][0]) + wx * (f[1][1] - f[0][1]);
        const float s_x = (1.f - wy) * (f[0][1] - f[0][0]) + wy * (f[1][1] - f[1][0]);
        guy = -a.dtdx * g * s_y;
        gux = -a.dtdx * g * s_x;
    }
    a.gUy[(size_t)b * N + c] = guy;
    a.gUx[(size_t)b * N + c] = gux;
}

// every contribution a global int64 atomic (option k2d_dens_adj_tile = 0; the reference form of the tile kernel)
__global__ void __launch_bounds__(256) k_kd_advect_adj(KDArgs a) {
    const int Y = a.Y, X = a.X, N = Y * X;
    const int b = blockIdx.y;
    const float* sy = a.svy + (size_t)b * (Y + 1) * X;
    const float* sx = a.svx + (size_t)b * Y * (X + 1);
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    const KGAdd add{a.gD + (size_t)b * N, qs, X};
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < N; c += gridDim.x * blockDim.x) kd_point(a, b, sy, sx, add, c / X, c % X);
}

// The same scatter with an LDS window per workgroup: a workgroup owns 16 x 16 cells, one per thread, and accumulates into a 25 x 25 int64
// window (5 KB): the four corners of a cell's gather lie within |u| dt/dx + 1 cells of it.  Integer adds commute: the result equals
// k_kd_advect_adj's bit for bit.
__global__ void __launch_bounds__(256) k_kd_advect_adj_tile(KDArgs a, int nti) {
    __shared__ unsigned long long win[KD_W * KD_W];
    const int Y = a.Y, X = a.X, N = Y * X;
    const int b = blockIdx.y;
    const int tj = (int)blockIdx.x / nti, ti = (int)blockIdx.x % nti, j0 = tj * KD_T, i0 = ti * KD_T;
    const float* sy = a.svy + (size_t)b * (Y + 1) * X;
    const float* sx = a.svx + (size_t)b * Y * (X + 1);
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    const KGAdd gadd{a.gD + (size_t)b * N, qs, X};
    const KTAdd add{gadd, win, j0 - KD_H, i0 - KD_H};
    fx_window_clear(win, KD_W * KD_W, 256);
    __syncthreads();
    const int j = j0 + (int)threadIdx.x / KD_T, i = i0 + (int)threadIdx.x % KD_T;
    if (j < Y && i < X) kd_point(a, b, sy, sx, add, j, i);
    __syncthreads();
    fx_window_flush(win, KD_W * KD_W, 256, [&](int e) { return gadd.g + (j0 - KD_H + e / KD_W) * X + (i0 - KD_H + e % KD_W); });
}

__global__ void __launch_bounds__(256) k_kd_diffuse_adj(KDArgs a) {
#pragma clang fp contract(off)
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const float alpha = a.adt / a.re[b];
    float qs, qi;
    fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
    const bool poisoned = qi != qi;                        // a non-finite g_d_out: every gradient of the simulation is NaN
    const float nan = __uint_as_float(0x7fc00000u);
    const float* uy = a.gUy + (size_t)b * N;
    const float* ux = a.gUx + (size_t)b * N;
    const float* m = a.bcm + (size_t)b * a.bc_stride;
    // g' = g_c . (1 - bcm) at face (jf, i) of v_y, g_c at face (j, iF) of v_x: out-of-range cells count as zero (karman_re.hpp: shared with
    // the Reynolds-number reduction)
    auto gy = [&](int jf, int i) { return kd_face_y(uy, m, Y, X, jf, i); };
    auto gx = [&](int j, int iF) { return kd_face_x(ux, X, j, iF); };
    // g' + alpha L^T g' as k_lb_diffuse_adj forms it: the transposed replicate-padded Laplacian in gather form (a direction that leaves the
    // array contributes g' of the face itself; neighbours in the order y +, y -, x +, x -), ONE fused multiply-add, spelled out
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nVy + nVx + N; e += gridDim.x * blockDim.x) {
        if (e < nVy) {
            const int j = e / X, i = e - j * X;
            const float v = gy(j, i);
            float acc = -4.f * v;
            acc += j + 1 < Y + 1 ? gy(j + 1, i) : v;
            acc += j > 0 ? gy(j - 1, i) : v;
            acc += i + 1 < X ? gy(j, i + 1) : v;
            acc += i > 0 ? gy(j, i - 1) : v;
            const float r = poisoned ? nan : __fmaf_rn(alpha, acc, v);
            float* o = a.giy + (size_t)b * nVy + e;
            *o = a.accumulate ? *o + r : r;
        } else if (e < nVy + nVx) {
            const int q = e - nVy, j = q / XP, i = q - j * XP;
            const float v = gx(j, i);
            float acc = -4.f * v;
            acc += j + 1 < Y ? gx(j + 1, i) : v;
            acc += j > 0 ? gx(j - 1, i) : v;
            acc += i + 1 < XP ? gx(j, i + 1) : v;
            acc += i > 0 ? gx(j, i - 1) : v;
            const float r = poisoned ? nan : __fmaf_rn(alpha, acc, v);
            float* o = a.gix + (size_t)b * nVx + q;
            *o = a.accumulate ? *o + r : r;
        } else {
            const int c = e - nVy - nVx;
            a.gdi[(size_t)b * N + c] = fx_get(a.gD + (size_t)b * N, c, qi);
        }
    }
}

// the workspace: g_d_in accumulators (int64), gU_y, gU_x (fp32), the absmax slots, with re the partial sums of the Reynolds-number
// reduction; 256-byte granules
struct KDLayout {
    long long* gD;
    float *gUy, *gUx;
    unsigned* gmax;
    double* partial;
    void* mc;                           // the _adv forms with the MacCormack advection: what sol_mc_adj_den takes, behind everything else
    size_t bytes;
};
KDLayout kd_layout(const sol_karman_cfg* c, bool re, void* ws, bool mc = false) {
    const size_t B = c->B, N = (size_t)c->Y * c->X;
    Carve w(ws);
    KDLayout l{w.take<long long>(B * N), w.take<float>(B * N), w.take<float>(B * N), w.take<unsigned>(B * FX_SLOTS)};
    if (re) l.partial = sol_re_partial_take(w, c);
    if (mc) l.mc = w.take<char>(sol_mc_adj_bytes(c));
    l.bytes = w.bytes();
    return l;
}

}  // namespace

extern "C" size_t sol_karman_density_bwd_workspace_bytes(const sol_karman_cfg* c) {
    if (!c || c->B < 1 || c->Y < 1 || c->X < 1) return 0;
    return kd_layout(c, false, nullptr).bytes;
}

namespace {

// the _adv forms' extra: which advection the forward step ran (1: MacCormack, karman_maccormack.hip) and its correction strength
struct AdvExtra {
    int32_t advection;
    float strength;
};

// the launches of sol_karman_density_bwd; with rx, followed by the Reynolds-number reduction over the gU they leave in the workspace
// (sol_karman_density_bwd_re): g_d_in / g_vy_in / g_vx_in are the same launches' results either way
int density_bwd(const char* who, const sol_karman_cfg* c, void* stream,
                const float* d_in, const float* inflow, const float* saved_vy, const float* saved_vx,
                const float* re, const float* velBCyMask, int64_t bc_batch_stride,
                const float* g_d_out, float* g_d_in, float* g_vy_in, float* g_vx_in, int accumulate,
                void* workspace, size_t workspace_bytes, const ReExtra* rx, const AdvExtra* ax = nullptr) {
    SOL_REQUIRE(c != nullptr, "%s: cfg is NULL", who);
    if (ax)
        if (int e = sol_mc_check(who, ax->advection, ax->strength)) return e;
    const bool mc = ax && ax->advection == 1;
    SOL_REQUIRE(!mc || (c->Y >= 16 && c->X >= 16), "%s: the MacCormack advection is built on grids with Y, X >= 16 (got %d, %d)", who, c ? c->Y : 0, c ? c->X : 0);
    SOL_REQUIRE(c->B >= 1 && c->B <= 65535 && c->Y >= 2 && c->X >= 2, "%s: B in [1, 65535], Y, X >= 2 (got %d, %d, %d)", who, c->B, c->Y, c->X);
    SOL_REQUIRE((size_t)c->Y * c->X < ((size_t)1 << 28), "%s: grid too large for 32-bit face indices", who);
    SOL_REQUIRE(d_in && saved_vy && saved_vx && re && velBCyMask && g_d_out && g_d_in && g_vy_in && g_vx_in && workspace,
                "%s: NULL pointer argument", who);
    SOL_REQUIRE(inflow || !c->inflow_before, "%s: cfg.inflow_before needs the inflow mask (the advected field is d_in + inflow)", who);
    SOL_REQUIRE(!rx || (rx->vy_in && rx->vx_in && rx->g_re), "%s: NULL pointer argument", who);
    const KDLayout l = kd_layout(c, rx != nullptr, workspace, mc);
    SOL_REQUIRE(workspace_bytes >= l.bytes, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, l.bytes);
    const void* outs[] = {g_d_in, g_vy_in, g_vx_in, rx ? rx->g_re : nullptr};
    const void* ins[] = {d_in, inflow, saved_vy, saved_vx, re, velBCyMask, g_d_out, rx ? rx->vy_in : nullptr, rx ? rx->vx_in : nullptr};
    for (const void* o : outs)
        for (const void* i : ins) SOL_REQUIRE(!o || o != i, "%s: outputs must not alias the inputs", who);
    SOL_REQUIRE(g_d_in != g_vy_in && g_d_in != g_vx_in && g_vy_in != g_vx_in, "%s: g_d_in, g_vy_in and g_vx_in must be buffers of their own", who);
    SOL_REQUIRE(!rx || (rx->g_re != g_d_in && rx->g_re != g_vy_in && rx->g_re != g_vx_in), "%s: g_re must be a buffer of its own", who);
    const int B = c->B, Y = c->Y, X = c->X, N = Y * X;
    const size_t items = (size_t)(Y + 1) * X + (size_t)Y * (X + 1) + N;
    hipStream_t s = (hipStream_t)stream;
    KDArgs a{};
    a.B = B; a.Y = Y; a.X = X; a.dtdx = c->dt / c->dx; a.adt = c->dt * c->res * c->res;
    a.inflow_before = c->inflow_before; a.accumulate = accumulate != 0;
    a.d_in = d_in; a.inflow = inflow; a.svy = saved_vy; a.svx = saved_vx; a.re = re; a.bcm = velBCyMask; a.bc_stride = bc_batch_stride;
    a.gdo = g_d_out;
    a.gD = l.gD; a.gUy = l.gUy; a.gUx = l.gUx; a.gmax = l.gmax;
    a.gdi = g_d_in; a.giy = g_vy_in; a.gix = g_vx_in;
    SOL_LAUNCH(k_kd_clear, dim3(FX_SLOTS, B), dim3(256), 0, s, a);
    if (mc) {
        if (int e = sol_mc_adj_den(c, s, true, ax->strength, d_in, inflow, saved_vy, saved_vx, g_d_out, l.gmax, l.gD, l.gUy, l.gUx, l.mc,
                                   sol_opt().k2d_dens_adj_tile != 0)) return e;
    } else if (sol_opt().k2d_dens_adj_tile) {
        const int ntj = (Y + KD_T - 1) / KD_T, nti = (X + KD_T - 1) / KD_T;
        SOL_LAUNCH(k_kd_advect_adj_tile, dim3(ntj * nti, B), dim3(256), 0, s, a, nti);
    } else {
        SOL_LAUNCH(k_kd_advect_adj, dim3((unsigned)((N + 255) / 256), B), dim3(256), 0, s, a);
    }
    SOL_LAUNCH(k_kd_diffuse_adj, dim3((unsigned)((items + 255) / 256), B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    if (!rx) return SOL_OK;
    // g' of the Reynolds-number gradient = the face values k_kd_diffuse_adj has just formed from gU (kd_face_y / kd_face_x)
    ReIn in{};
    in.src = RE_GU;
    in.gUy = l.gUy; in.gUx = l.gUx; in.gmax = l.gmax; in.bcm = velBCyMask; in.bc_stride = bc_batch_stride;
    in.vy_in = rx->vy_in; in.vx_in = rx->vx_in; in.re = re;
    in.partial = l.partial;
    in.g_re = rx->g_re; in.accumulate = rx->accumulate;
    return sol_re_reduce(s, c, in);
}

}  // namespace

extern "C" int sol_karman_density_bwd(const sol_karman_cfg* c, void* stream,
                                      const float* d_in, const float* inflow, const float* saved_vy, const float* saved_vx,
                                      const float* re, const float* velBCyMask, int64_t bc_batch_stride,
                                      const float* g_d_out, float* g_d_in, float* g_vy_in, float* g_vx_in, int accumulate,
                                      void* workspace, size_t workspace_bytes) {
    return density_bwd("sol_karman_density_bwd", c, stream, d_in, inflow, saved_vy, saved_vx, re, velBCyMask, bc_batch_stride, g_d_out,
                       g_d_in, g_vy_in, g_vx_in, accumulate, workspace, workspace_bytes, nullptr);
}

extern "C" size_t sol_karman_density_bwd_re_workspace_bytes(const sol_karman_cfg* c) {
    if (!c || c->B < 1 || c->Y < 1 || c->X < 1) return 0;
    return kd_layout(c, true, nullptr).bytes;
}

extern "C" int sol_karman_density_bwd_re(const sol_karman_cfg* c, void* stream,
                                         const float* d_in, const float* inflow, const float* saved_vy, const float* saved_vx,
                                         const float* re, const float* velBCyMask, int64_t bc_batch_stride,
                                         const float* g_d_out, float* g_d_in, float* g_vy_in, float* g_vx_in, int accumulate,
                                         void* workspace, size_t workspace_bytes,
                                         const float* vy_in, const float* vx_in, float* g_re, int accumulate_re) {
    const ReExtra rx{vy_in, vx_in, g_re, accumulate_re};
    return density_bwd("sol_karman_density_bwd_re", c, stream, d_in, inflow, saved_vy, saved_vx, re, velBCyMask, bc_batch_stride, g_d_out,
                       g_d_in, g_vy_in, g_vx_in, accumulate, workspace, workspace_bytes, &rx);
}

// The _adv forms: every argument of the plain / _re form, then the advection the forward step ran (0: semi-Lagrangian -- that form's
// launches and bits; 1: MacCormack -- sol_mc_adj_den in place of k_kd_advect_adj*, grids with Y, X >= 16) and its correction strength.
extern "C" size_t sol_karman_density_bwd_adv_workspace_bytes(const sol_karman_cfg* c, int32_t with_re, int32_t advection) {
    if (!c || c->B < 1 || c->Y < 1 || c->X < 1) return 0;
    return kd_layout(c, with_re != 0, nullptr, advection == 1).bytes;
}

extern "C" int sol_karman_density_bwd_adv(const sol_karman_cfg* c, void* stream,
                                          const float* d_in, const float* inflow, const float* saved_vy, const float* saved_vx,
                                          const float* re, const float* velBCyMask, int64_t bc_batch_stride,
                                          const float* g_d_out, float* g_d_in, float* g_vy_in, float* g_vx_in, int accumulate,
                                          void* workspace, size_t workspace_bytes, int32_t advection, float correction_strength) {
    const AdvExtra ax{advection, correction_strength};
    return density_bwd("sol_karman_density_bwd_adv", c, stream, d_in, inflow, saved_vy, saved_vx, re, velBCyMask, bc_batch_stride, g_d_out,
                       g_d_in, g_vy_in, g_vx_in, accumulate, workspace, workspace_bytes, nullptr, &ax);
}

extern "C" int sol_karman_density_bwd_adv_re(const sol_karman_cfg* c, void* stream,
                                             const float* d_in, const float* inflow, const float* saved_vy, const float* saved_vx,
                                             const float* re, const float* velBCyMask, int64_t bc_batch_stride,
                                             const float* g_d_out, float* g_d_in, float* g_vy_in, float* g_vx_in, int accumulate,
                                             void* workspace, size_t workspace_bytes,
                                             const float* vy_in, const float* vx_in, float* g_re, int accumulate_re,
                                             int32_t advection, float correction_strength) {
    const ReExtra rx{vy_in, vx_in, g_re, accumulate_re};
    const AdvExtra ax{advection, correction_strength};
    return density_bwd("sol_karman_density_bwd_adv_re", c, stream, d_in, inflow, saved_vy, saved_vx, re, velBCyMask, bc_batch_stride, g_d_out,
                       g_d_in, g_vy_in, g_vx_in, accumulate, workspace, workspace_bytes, &rx, &ax);
}
