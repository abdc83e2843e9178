// Preconditioned conjugate-gradient pressure solve for any obstacle mask: one engine, two users -- karman-3d (cfg.pressure_solver = 1,
// DESIGN 4.8) and the karman-2d large grids.
//
// The system is the one the direct solves (karman3d.hip, karman_large.hip) invert: M p = b with M = -A, PhiFlow's pressure matrix --
// diagonal = max(number of accessible neighbours, 1) with edge padding (a neighbour outside the box counts as the cell itself, p = 0
// there), -active_c active_n between neighbours, obstacle rows decoupled (precond.scene_matrix, precond3d._accessible_diag).  CG on M
// preconditioned with the empty-box solve G = M_r^-1 (the sine transforms of a blob with nS = 0: k3_apply_G in 3-D,
// sol_large_box_forward / _back in 2-D), i.e. oracle/sol_oracle3d.solve_pcg / precond.pcg_reference in fp32 with fp64 dot products.
//
// Launch structure (pcg_run):
//   pcg_init                      x = 0, r = b (in place), per-workgroup partials of |b|^2, done = 0, ndone = 0
//     (with an initial guess x0:  pcg_guess_scan, pcg_init_warm -- x = x0, r = b - M x0, partials of |b|^2 and |r|^2; a simulation
//      whose guess holds a NaN or an Inf starts from x = 0 instead.  The test below stays against |b|: a guess that already meets it
//      reports 0 iterations)
//   G, pcg_dot                    z = G r, convergence test, partials of <r, z>
//   cg_max_iter x [ pcg_stencil   p = z + beta p (into the other p buffer), q = M p, partials of <p, q>
//                   pcg_update    alpha = <r, z> / <p, q>, x += alpha p, r -= alpha q, partials of |r|^2
//                   G, pcg_dot ]  (the last iteration: pcg_dot as the convergence test only)
// Only pcg_stencil depends on the dimension: its Grid type decomposes the cell index and visits the neighbours in a fixed order
// (2-D j-, j+, i-, i+; 3-D j-, j+, i-, i+, k-, k+), which fixes the fp32 sums.  Every dot product is a slab of per-workgroup fp64
// partials [B][nwg <= 512] that the NEXT kernel sums in a fixed order in every one of its workgroups (no float atomics: the solve is
// bit-reproducible).  pcg_dot stops a simulation when the recursively updated |r|_2 <= max(cg_rtol |b|_2, cg_atol): it sets the
// simulation's done word and counts it in ndone, after which its x, r and p are frozen and every per-simulation kernel returns at once
// (so do the transforms of G that read the done words).  The iterations used and the converged flag go to cg_info at
// info[b * info_stride] and info[b * info_stride + info_conv]: [B][2] in 3-D, [2][B] in 2-D.
//
// The launch sequence is fixed and never synchronises with the host under capture (hipStreamIsCapturing): a trainer or roll-out graph
// captures the full cg_max_iter budget.  The ONE synchronising case: with poll_every > 0 (the 2-D user: 16), an EAGER call reads ndone
// back to the host every poll_every iterations and stops issuing iterations once all B simulations are done -- data generation runs
// thousands of eager steps with the PhiFlow budget of 2000.  The results do not depend on where it stops: a finished simulation's state
// is frozen either way.  The 3-D user passes 0 and always issues the full budget.
//
// Also here, next to sol_large_step: large_fwd, the one host path of the large-grid 2-D forward step for both solvers (six entry points).
#include "common.hpp"

namespace {

constexpr int PCG_T = 256;          // threads per workgroup
constexpr int PCG_MAXWG = 512;      // workgroups per simulation (= partials per slab row)
constexpr int FDL_MAGIC = 0x46443032;

int pcg_nwg(size_t N) { const size_t g = (N + PCG_T - 1) / PCG_T; return (int)(g < (size_t)PCG_MAXWG ? g : (size_t)PCG_MAXWG); }

struct PcgArgs {
    int B, N, nwg;
    int info_stride, info_conv;     // cg_info layout (see above)
    float rtol, atol;
    const float* active;
    float *x, *r, *q, *p[2];
    double *bb, *rr, *pq, *rz[2];   // slabs [B][nwg]
    int* done;                      // [B]
    int* ndone;                     // [1]: simulations finished so far
    int* info;
};

// cell(c): the index decomposition, taken before the cell's loads (that order keeps the loads' latency behind the integer
// divisions); neighbours: the visit in the fixed order
struct Grid2 {
    int Y, X;
    struct Cell { int j, i; };
    __device__ __forceinline__ Cell cell(int c) const { const int j = c / X; return {j, c - j * X}; }
    template <class F> __device__ __forceinline__ void neighbours(Cell p, int c, F&& nb) const {
        nb(p.j > 0, c - X); nb(p.j + 1 < Y, c + X);
        nb(p.i > 0, c - 1); nb(p.i + 1 < X, c + 1);
    }
};

struct Grid3 {
    int Y, X, Z;
    struct Cell { int j, i, k; };
    __device__ __forceinline__ Cell cell(int c) const { const int k = c % Z, i = (c / Z) % X, j = c / (X * Z); return {j, i, k}; }
    template <class F> __device__ __forceinline__ void neighbours(Cell p, int c, F&& nb) const {
        const int XZ = X * Z;
        nb(p.j > 0, c - XZ); nb(p.j + 1 < Y, c + XZ);
        nb(p.i > 0, c - Z);  nb(p.i + 1 < X, c + Z);
        nb(p.k > 0, c - 1);  nb(p.k + 1 < Z, c + 1);
    }
};

// sum of v over the workgroup, the same fixed order every run; the result is valid in every thread
__device__ double pcg_block_sum(double v) {
    __shared__ double red[PCG_T / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                                // (a previous call's readers are done with red)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < PCG_T / 64; ++w) t += red[w];
    return t;
}

__device__ double pcg_slab_sum(const double* row, int n) {
    double v = 0.0;
    for (int k = threadIdx.x; k < n; k += PCG_T) v += row[k];
    return pcg_block_sum(v);
}

__device__ __forceinline__ void pcg_publish(double* slab, int nwg, double part) {
    const double t = pcg_block_sum(part);
    if (threadIdx.x == 0) slab[(size_t)blockIdx.y * nwg + blockIdx.x] = t;
}

__global__ void __launch_bounds__(PCG_T) pcg_init(PcgArgs a) {
    const int b = blockIdx.y;
    const size_t o = (size_t)b * a.N;
    double acc = 0.0;
    for (int c = blockIdx.x * PCG_T + threadIdx.x; c < a.N; c += a.nwg * PCG_T) {
        const float v = a.r[o + c];
        a.x[o + c] = 0.f;
        acc += (double)v * v;
    }
    const double t = pcg_block_sum(acc);
    if (threadIdx.x == 0) {
        a.bb[(size_t)b * a.nwg + blockIdx.x] = t;
        a.rr[(size_t)b * a.nwg + blockIdx.x] = t;
        if (blockIdx.x == 0) a.done[b] = 0;
        if (blockIdx.x == 0 && b == 0) *a.ndone = 0;
    }
}

// ---- warm start: the caller's guess x0 [B][N] ----
// per-workgroup counts of the non-finite values of x0 into the <p, q> slab (free until the first pcg_stencil): pcg_init_warm sums a
// simulation's row and drops a guess that holds a NaN or an Inf
__global__ void __launch_bounds__(PCG_T) pcg_guess_scan(PcgArgs a, const float* __restrict__ x0) {
    const size_t o = (size_t)blockIdx.y * a.N;
    double bad = 0.0;
    for (int c = blockIdx.x * PCG_T + threadIdx.x; c < a.N; c += a.nwg * PCG_T) bad += fabsf(x0[o + c]) < INFINITY ? 0.0 : 1.0;
    pcg_publish(a.pq, a.nwg, bad);
}

// x = x0, r = b - M x0 with (M x)_c = fma(max(n, 1), x_c, -(active_c s)), n and s summed over the neighbours in pcg_stencil's order (the
// masks are 0 / 1, so the products inside s are exact); a simulation with a non-finite guess gets pcg_init's x = 0, r = b, and an
// all-zero guess gives the same bits.  Partials of |b|^2 and |r|^2, done = 0, ndone = 0
template <class Grid>
__global__ void __launch_bounds__(PCG_T) pcg_init_warm(PcgArgs a, Grid g, const float* __restrict__ x0) {
    const int b = blockIdx.y;
    const size_t o = (size_t)b * a.N;
    const bool use = pcg_slab_sum(a.pq + (size_t)b * a.nwg, a.nwg) == 0.0;
    const float* xb = x0 + o;
    double accb = 0.0, accr = 0.0;
    for (int c = blockIdx.x * PCG_T + threadIdx.x; c < a.N; c += a.nwg * PCG_T) {
        const float v = a.r[o + c];
        float pc = 0.f, r = v;
        if (use) {
            const typename Grid::Cell at = g.cell(c);
            const float ac = a.active[c] != 0.f ? 1.f : 0.f;
            pc = xb[c];
            float n = 0.f, s = 0.f;
            g.neighbours(at, c, [&](bool inside, int e) {
                float an = ac, pv = 0.f;            // outside the box: accessible iff the cell is, p = 0 there (as pcg_stencil)
                if (inside) { an = a.active[e] != 0.f ? 1.f : 0.f; pv = an * xb[e]; }
                n += an; s += pv;
            });
            const float qv = fmaf(fmaxf(n, 1.f), pc, -(ac * s));
            r = v - qv;
        }
        a.x[o + c] = pc;
        a.r[o + c] = r;
        accb += (double)v * v;
        accr += (double)r * r;
    }
    const double tb = pcg_block_sum(accb), tr = pcg_block_sum(accr);
    if (threadIdx.x == 0) {
        a.bb[(size_t)b * a.nwg + blockIdx.x] = tb;
        a.rr[(size_t)b * a.nwg + blockIdx.x] = tr;
        if (blockIdx.x == 0) a.done[b] = 0;
        if (blockIdx.x == 0 && b == 0) *a.ndone = 0;
    }
}

// p_new = z + beta p_old (beta = rz_cur / rz_prev; first: p_new = z), q = M p_new, partials of <p_new, q>
template <class Grid>
__global__ void __launch_bounds__(PCG_T) pcg_stencil(PcgArgs a, Grid g, const float* __restrict__ z, const float* __restrict__ pold,
                                                      float* __restrict__ pnew, const double* __restrict__ rzc,
                                                      const double* __restrict__ rzp, int first) {
    const int b = blockIdx.y;
    if (a.done[b]) return;
    float beta = 0.f;
    if (!first) {
        const double cur = pcg_slab_sum(rzc + (size_t)b * a.nwg, a.nwg), prev = pcg_slab_sum(rzp + (size_t)b * a.nwg, a.nwg);
        beta = (float)(cur / fmax(prev, 1e-300));
    }
    const size_t o = (size_t)b * a.N;
    const float* zb = z + o;
    const float* pb = pold + o;
    auto pn = [&](int e) { return first ? zb[e] : fmaf(beta, pb[e], zb[e]); };
    auto act = [&](int e) { return a.active[e] != 0.f ? 1.f : 0.f; };
    double acc = 0.0;
    for (int c = blockIdx.x * PCG_T + threadIdx.x; c < a.N; c += a.nwg * PCG_T) {
        const typename Grid::Cell at = g.cell(c);
        const float ac = act(c), pc = pn(c);
        float n = 0.f, s = 0.f;
        g.neighbours(at, c, [&](bool inside, int e) {
            if (inside) { const float an = act(e); n += an; s += an * pn(e); }
            else n += ac;                           // outside the box: accessible iff the cell is (edge padding), p = 0 there
        });
        const float qv = fmaxf(n, 1.f) * pc - ac * s;
        pnew[o + c] = pc;
        a.q[o + c] = qv;
        acc += (double)pc * qv;
    }
    pcg_publish(a.pq, a.nwg, acc);
}

// alpha = <r, z> / <p, q>;  x += alpha p;  r -= alpha q;  partials of |r|^2
__global__ void __launch_bounds__(PCG_T) pcg_update(PcgArgs a, const float* __restrict__ p, const double* __restrict__ rzc) {
    const int b = blockIdx.y;
    if (a.done[b]) return;
    const double rz = pcg_slab_sum(rzc + (size_t)b * a.nwg, a.nwg), pq = pcg_slab_sum(a.pq + (size_t)b * a.nwg, a.nwg);
    const float al = (float)(rz / fmax(pq, 1e-300));
    const size_t o = (size_t)b * a.N;
    double acc = 0.0;
    for (int c = blockIdx.x * PCG_T + threadIdx.x; c < a.N; c += a.nwg * PCG_T) {
        a.x[o + c] = fmaf(al, p[o + c], a.x[o + c]);
        const float r = fmaf(-al, a.q[o + c], a.r[o + c]);
        a.r[o + c] = r;
        acc += (double)r * r;
    }
    pcg_publish(a.rr, a.nwg, acc);
}

// convergence test after `iter` updates (every workgroup of the simulation takes the same decision from the same slabs; the
// first one records it and counts the simulation as finished), then the partials of <r, z> unless the simulation stopped or this
// is the last iteration (z == NULL)
__global__ void __launch_bounds__(PCG_T) pcg_dot(PcgArgs a, const float* __restrict__ z, double* __restrict__ rz, int iter) {
    const int b = blockIdx.y;
    if (a.done[b]) return;
    const double bb = pcg_slab_sum(a.bb + (size_t)b * a.nwg, a.nwg), rr = pcg_slab_sum(a.rr + (size_t)b * a.nwg, a.nwg);
    const double rt = (double)a.rtol, at = (double)a.atol;
    const bool conv = rr <= fmax(rt * rt * bb, at * at);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.info[b * a.info_stride] = iter;
        a.info[b * a.info_stride + a.info_conv] = conv ? 1 : 0;
        if (conv) { a.done[b] = 1; atomicAdd(a.ndone, 1); }
    }
    if (conv || !z) return;
    const size_t o = (size_t)b * a.N;
    double acc = 0.0;
    for (int c = blockIdx.x * PCG_T + threadIdx.x; c < a.N; c += a.nwg * PCG_T) acc += (double)a.r[o + c] * z[o + c];
    pcg_publish(rz, a.nwg, acc);
}

// the CG buffers: slabs, done words, x, the two p buffers, q (the caller sets r, active, info and the tolerances)
PcgArgs pcg_carve(Carve& w, size_t B, size_t N) {
    PcgArgs a{};
    a.B = (int)B; a.N = (int)N; a.nwg = pcg_nwg(N);
    a.bb = w.take<double>(B * a.nwg);
    a.rr = w.take<double>(B * a.nwg);
    a.pq = w.take<double>(B * a.nwg);
    a.rz[0] = w.take<double>(B * a.nwg);
    a.rz[1] = w.take<double>(B * a.nwg);
    a.done = w.take<int>(B);
    a.ndone = w.take<int>(1);
    a.x = w.take<float>(B * N);
    a.p[0] = w.take<float>(B * N);
    a.p[1] = w.take<float>(B * N);
    a.q = w.take<float>(B * N);
    return a;
}

// M x = b by PCG (b = a.r is overwritten with the residual, x = a.x); apply_G(&z) applies G to a.r and points z at the result.
// x0: NULL (start from x = 0), or the initial guess [B][N] (read by the first two launches only; not a.x)
template <class Grid, class ApplyG>
int pcg_run(hipStream_t s, const PcgArgs& a, Grid g, int K, int poll_every, ApplyG&& apply_G, const float* x0 = nullptr) {
    bool poll = false;
    if (poll_every > 0) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        SOL_HIP_CHECK(hipStreamIsCapturing(s, &cap));
        poll = cap == hipStreamCaptureStatusNone;
    }
    const dim3 grid(a.nwg, a.B), blk(PCG_T);
    float* z = nullptr;
    if (x0) {
        SOL_LAUNCH(pcg_guess_scan, grid, blk, 0, s, a, x0);
        SOL_LAUNCH(pcg_init_warm<Grid>, grid, blk, 0, s, a, g, x0);
    } else {
        SOL_LAUNCH(pcg_init, grid, blk, 0, s, a);
    }
    if (int e = apply_G(&z)) return e;
    SOL_LAUNCH(pcg_dot, grid, blk, 0, s, a, (const float*)z, a.rz[0], 0);
    for (int k = 1; k <= K; ++k) {
        SOL_LAUNCH(pcg_stencil<Grid>, grid, blk, 0, s, a, g, (const float*)z, (const float*)a.p[(k - 1) & 1], a.p[k & 1],
                   (const double*)a.rz[(k - 1) & 1], (const double*)a.rz[k & 1], k == 1 ? 1 : 0);
        SOL_LAUNCH(pcg_update, grid, blk, 0, s, a, (const float*)a.p[k & 1], (const double*)a.rz[(k - 1) & 1]);
        if (k < K) {
            if (int e = apply_G(&z)) return e;
            SOL_LAUNCH(pcg_dot, grid, blk, 0, s, a, (const float*)z, a.rz[k & 1], k);
        } else {
            SOL_LAUNCH(pcg_dot, grid, blk, 0, s, a, (const float*)nullptr, (double*)nullptr, k);
        }
        if (poll && k < K && k % poll_every == 0) {
            SOL_LAUNCH_CHECK();
            int finished = 0;
            SOL_HIP_CHECK(hipMemcpyAsync(&finished, a.ndone, sizeof(int), hipMemcpyDeviceToHost, s));
            SOL_HIP_CHECK(hipStreamSynchronize(s));
            if (finished >= a.B) break;
        }
    }
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

// ---- karman-3d: the CG buffers, then the cg_info fallback [B][2] (cfg.cg_info NULL) ----
PcgArgs k3_layout(const sol_karman3d_cfg* c, void* ws, size_t* bytes = nullptr) {
    Carve w(ws);
    PcgArgs a = pcg_carve(w, c->B, (size_t)c->Y * c->X * c->Z);
    int* info = w.take<int>(2 * (size_t)c->B);
    a.info = c->cg_info ? c->cg_info : info;
    a.info_stride = 2; a.info_conv = 1;
    a.rtol = c->cg_rtol; a.atol = c->cg_atol;
    if (bytes) *bytes = w.bytes();
    return a;
}

// ---- karman-2d large grids: the step's buffers (sv_y, sv_x, rhs / residual, two transform buffers), the CG buffers, then z ----
struct Large {
    float *svy, *svx, *T1, *T2, *z;
    PcgArgs a;
    size_t bytes;
};

// with_sv = false: the solver's part alone (the adjoint's workspace, and pressure_solve_any2d on the address of the forward layout's
// rhs buffer: every buffer starts on 256 bytes, so both carves of one workspace name the same addresses)
Large large_layout(const sol_karman_cfg* c, void* ws, bool with_sv = true) {
    const size_t B = c->B, Y = c->Y, X = c->X, N = Y * X;
    Carve w(ws);
    Large l{};
    if (with_sv) {
        l.svy = w.take<float>(B * (Y + 1) * X);
        l.svx = w.take<float>(B * Y * (X + 1));
    }
    float* R = w.take<float>(B * N);
    l.T1 = w.take<float>(B * N);
    l.T2 = w.take<float>(B * N);
    l.a = pcg_carve(w, B, N);
    l.z = w.take<float>(B * N);
    l.a.r = R;
    l.a.info_stride = 1; l.a.info_conv = c->B;
    l.a.rtol = c->cg_rtol; l.a.atol = c->cg_atol;
    l.bytes = w.bytes();
    return l;
}

}  // namespace

// checks of the CG solve's arguments (before any launch), shared with the adjoint (karman_large_bwd.hip)
int sol_large_cg_check(const sol_karman_cfg* c, const char* who, const float* box_blob, const int32_t* hdr, const int32_t* cg_info,
                       const void* workspace) {
    SOL_REQUIRE(c != nullptr, "cfg is NULL");
    SOL_REQUIRE(c->B >= 1 && c->B <= 65535 && c->Y >= 16 && c->X >= 16, "%s: B in [1, 65535], Y, X >= 16 (got %d, %d, %d)", who, c->B, c->Y, c->X);
    SOL_REQUIRE((size_t)c->Y * c->X < ((size_t)1 << 30), "%s: grid too large", who);
    SOL_REQUIRE(box_blob && hdr && cg_info && workspace, "%s: NULL pointer argument (box blob, its host header, cg_info and workspace are required)", who);
    SOL_REQUIRE(c->cg_max_iter >= 1, "%s: cfg.cg_max_iter must be >= 1, got %d", who, c->cg_max_iter);
    SOL_REQUIRE(c->cg_rtol >= 0.f && c->cg_rtol < INFINITY && c->cg_atol >= 0.f && c->cg_atol < INFINITY,
                "%s: cfg.cg_rtol and cfg.cg_atol must be >= 0 and finite, got %g, %g", who, (double)c->cg_rtol, (double)c->cg_atol);
    SOL_REQUIRE(c->cg_rtol > 0.f || c->cg_atol > 0.f, "%s: cfg.cg_rtol and cfg.cg_atol are both zero (the solve could never stop)", who);
    SOL_REQUIRE(hdr[0] == FDL_MAGIC, "%s: box_header_host must be the first 16 words of the blob (host copy)", who);
    SOL_REQUIRE(hdr[1] == c->Y && hdr[2] == c->X, "%s: the box blob is for a %dx%d grid, cfg is %dx%d", who, hdr[1], hdr[2], c->Y, c->X);
    SOL_REQUIRE(hdr[5] == 0 && hdr[6] == 0, "%s: the CG solve needs the empty-box blob (nS = 0: precond.box_solver_blob), this one has nS = %d",
                who, hdr[5]);
    return SOL_OK;
}

namespace {

// M x = b by PCG; b (= l.a.r) is overwritten with the residual
int large_solve(hipStream_t s, const sol_karman_cfg* c, const float* blob, const float* active, const Large& l, int32_t* info,
                const float* x0 = nullptr) {
    const int B = c->B, Y = c->Y, X = c->X;
    PcgArgs a = l.a;
    a.active = active;
    a.info = info;
    auto apply_G = [&](float** z) -> int {
        *z = l.z;
        if (int e = sol_large_box_forward(s, B, Y, X, blob, a.r, l.T1, l.T2, a.done)) return e;
        return sol_large_box_back(s, B, Y, X, blob, l.T2, l.T1, l.z, a.done);
    };
    return pcg_run(s, a, Grid2{Y, X}, c->cg_max_iter, 16, apply_G, x0);
}

__global__ void __launch_bounds__(PCG_T) large_copy(float* __restrict__ dst, const float* __restrict__ src, size_t n) {
    for (size_t e = (size_t)blockIdx.x * PCG_T + threadIdx.x; e < n; e += (size_t)gridDim.x * PCG_T) dst[e] = src[e];
}

}  // namespace

// ---- karman-2d large grids: the pressure solve the caller selects, M x = b, on a solver workspace of sol_large_solver_bytes ----
// direct: the capacitance solve on cfg.direct (hdr = its host header); else PCG with the empty-box solve of box_blob as preconditioner,
// reporting to cg_info [2][B].  The caller writes b into sol_large_solver_rhs(...) (overwritten); *x = the buffer that holds the solution.
size_t sol_large_solver_bytes(const sol_karman_cfg* c, bool direct, const int32_t* hdr) {
    return direct ? sol_large_direct_bytes(c, hdr) + 256 : large_layout(c, nullptr, false).bytes;
}

float* sol_large_solver_rhs(const sol_karman_cfg* c, bool direct, void* ws) {
    return direct ? static_cast<float*>(ws) : large_layout(c, ws, false).a.r;
}

int pressure_solve_any2d(hipStream_t s, const sol_karman_cfg* c, bool direct, const int32_t* hdr, const float* box_blob, const float* active,
                         int32_t* cg_info, void* ws, float** x, const float* x0) {
    if (direct) {
        *x = static_cast<float*>(ws);
        return sol_large_direct_solve(s, c, hdr, *x);
    }
    const Large l = large_layout(c, ws, false);
    *x = l.a.x;
    return large_solve(s, c, box_blob, active, l, cg_info, x0);
}

// diffuse / advect / rhs, the solve, the projection: the whole forward step (sv_y, sv_x: where the post-diffusion velocity goes)
int sol_large_step(const sol_karman_cfg* c, hipStream_t s, const SolLargeStep& io, float* svy, float* svx, bool direct, const int32_t* hdr,
                   const float* box_blob, int32_t* cg_info, void* solver_ws, const float* x0) {
    if (int e = sol_large_front(c, s, io, svy, svx, sol_large_solver_rhs(c, direct, solver_ws))) return e;
    float* p = nullptr;
    if (int e = pressure_solve_any2d(s, c, direct, hdr, box_blob, io.active, cg_info, solver_ws, &p, x0)) return e;
    return sol_large_project(c, s, io, p);
}

size_t k3_pcg_workspace_bytes(const sol_karman3d_cfg* c) {
    size_t bytes = 0;
    if (c && c->pressure_solver == 1) k3_layout(c, nullptr, &bytes);
    return bytes;
}

// the solver fields of the cfg against the blob header (shared by the forward and the adjoint entry points)
int k3_pcg_check(const sol_karman3d_cfg* c, const int32_t* hdr) {
    SOL_REQUIRE(c->pressure_solver == 0 || c->pressure_solver == 1, "cfg.pressure_solver must be 0 (direct) or 1 (preconditioned CG), got %d", c->pressure_solver);
    if (c->pressure_solver == 0) return SOL_OK;       // the direct solve takes any valid blob (nS = 0: the empty box)
    SOL_REQUIRE(hdr[4] == 0, "the preconditioned CG solve (pressure_solver = 1) needs the blob without capacitance part (nS = 0: "
                "precond3d.direct_solver_blob3d(np.ones_like(active))), this one has nS = %d", hdr[4]);
    SOL_REQUIRE(c->cg_max_iter >= 1, "cfg.cg_max_iter must be >= 1 for the CG solve, got %d", c->cg_max_iter);
    SOL_REQUIRE(c->cg_rtol > 0.f && c->cg_rtol < INFINITY, "cfg.cg_rtol must be > 0 (and finite), got %g", (double)c->cg_rtol);
    SOL_REQUIRE(c->cg_atol >= 0.f && c->cg_atol < INFINITY, "cfg.cg_atol must be >= 0 (and finite), got %g", (double)c->cg_atol);
    return SOL_OK;
}

int k3_pcg_solve(hipStream_t s, const sol_karman3d_cfg* c, const float* active, float* b, float* t1, float* t2, void* ws, float** x_out) {
    PcgArgs a = k3_layout(c, ws);
    a.active = active;
    a.r = b;
    auto apply_G = [&](float** z) { return k3_apply_G(s, c, b, t1, t2, z, a.done); };
    if (int e = pcg_run(s, a, Grid3{c->Y, c->X, c->Z}, c->cg_max_iter, 0, apply_G)) return e;
    *x_out = a.x;
    return SOL_OK;
}

// ---- karman-2d large grids: the forward step, ONE host path behind the six entry points ----
namespace {

// the step's workspace: sv_y, sv_x (with_sv; else the caller keeps them), then the solver's part
struct FwdLayout { float *svy, *svx; void* solver; size_t bytes; };
FwdLayout fwd_layout(const sol_karman_cfg* c, bool direct, const int32_t* hdr, bool with_sv, void* ws) {
    FwdLayout l{};
    if (!with_sv) {             // the solver's part alone, from the next 256 bytes
        Carve w(ws, 1, 256);
        l.solver = w.take<char>(sol_large_solver_bytes(c, direct, direct ? hdr : nullptr));
        l.bytes = w.bytes();
    } else if (direct) {        // float-dense from the caller's pointer, 256 floats of slack behind
        const size_t B = c->B, Y = c->Y, X = c->X;
        Carve w = Carve::packed(ws);
        l.svy = w.take<float>(B * (Y + 1) * X);
        l.svx = w.take<float>(B * Y * (X + 1));
        l.solver = w.take<char>(sol_large_direct_bytes(c, hdr));
        w.take<float>(256);
        l.bytes = w.bytes();
    } else {                    // 256-byte granules; the solver's part starts at the rhs buffer
        const Large g = large_layout(c, ws);
        l.svy = g.svy; l.svx = g.svx; l.solver = g.a.r; l.bytes = g.bytes;
    }
    return l;
}

// which solve, and what it reads: direct = the capacitance solve on cfg.direct with its host header, else the preconditioned CG with the
// empty-box blob, its host header and the report cg_info [2][B]; p_inout (CG only): NULL, or the initial guess in / the step's pressure out
struct LargeSolver { bool direct; const int32_t* direct_header_host; const float* box_blob; const int32_t* box_header_host; int32_t* cg_info; float* p_inout; };
// the training forms: where the post-diffusion velocity goes for the adjoint (without: into the workspace)
struct LargeSaved { float *vy, *vx; };

// the _adv forms: which advection (0: semi-Lagrangian, the plain launches; 1: MacCormack, karman_maccormack.hip) and its correction strength
struct LargeAdv { int32_t advection; float strength; };

// the workspace of an _adv step: the plain step's (fwd_layout), then -- with the MacCormack advection -- the part its launches take
// (sol_mc_bytes, carved by sol_mc_advect from the end of the step's part)
struct FwdAdvLayout { FwdLayout step; void* mc; size_t bytes; };
FwdAdvLayout fwd_adv_layout(const sol_karman_cfg* c, bool direct, const int32_t* hdr, bool with_sv, bool mc, void* ws) {
    FwdAdvLayout l{fwd_layout(c, direct, hdr, with_sv, ws), nullptr, 0};
    l.bytes = l.step.bytes;
    if (mc) {
        l.mc = ws ? static_cast<char*>(ws) + l.step.bytes : nullptr;
        l.bytes += sol_mc_bytes(c);
    }
    return l;
}

int large_fwd(const char* who, const sol_karman_cfg* c, void* stream, SolLargeStep io, const LargeSolver& sv, const LargeSaved* keep,
              void* workspace, size_t workspace_bytes, float fy = 0.f, float fx = 0.f, const LargeAdv* adv = nullptr) {
    const LargeSaved saved = keep ? *keep : LargeSaved{};
    if (adv)
        if (int e = sol_mc_check(who, adv->advection, adv->strength)) return e;
    const bool mc = adv && adv->advection == 1;
    SOL_REQUIRE(c != nullptr, "%s: cfg is NULL", who);
    SOL_REQUIRE(c->B >= 1 && c->B <= 65535 && c->Y >= 16 && c->X >= 16, "%s: B in [1, 65535], Y, X >= 16 (got %d, %d, %d)", who, c->B, c->Y, c->X);
    SOL_REQUIRE((size_t)c->Y * c->X < ((size_t)1 << 30), "%s: grid too large", who);
    SOL_REQUIRE(!saved.vy || (size_t)c->Y * c->X < ((size_t)1 << 28), "%s: grid too large for 32-bit face indices", who);
    SOL_REQUIRE(io.vy_in && io.vx_in && io.re && io.active && io.velBCy && io.velBCyMask && io.vy_out && io.vx_out && workspace &&
                    (!keep || (saved.vy && saved.vx)), "%s: NULL pointer argument", who);
    SOL_REQUIRE((io.d_in && io.inflow) || !io.d_out, "%s: density output requested without d_in / inflow", who);
    SOL_REQUIRE(!io.feat_out || io.feat_scale, "%s: feat_out requires feat_scale", who);
    SOL_REQUIRE(fy - fy == 0.f && fx - fx == 0.f, "%s: the force must be finite (got %g, %g)", who, (double)fy, (double)fx);
    SOL_REQUIRE((fy == 0.f && fx == 0.f) || (io.d_in && io.inflow && io.d_out), "%s: a non-zero force needs d_in, inflow and d_out", who);
    io.buoy_y = c->dt * fy; io.buoy_x = c->dt * fx;
    SOL_REQUIRE(!sv.direct || !sv.p_inout, "%s: p_inout warm-starts the CG solve; this cfg selects the direct solve", who);
    if (sv.direct) { if (int e = sol_large_direct_check(c, who, sv.direct_header_host)) return e; }
    else if (int e = sol_large_cg_check(c, who, sv.box_blob, sv.box_header_host, sv.cg_info, workspace)) return e;
    const FwdAdvLayout al = fwd_adv_layout(c, sv.direct, sv.direct_header_host, !saved.vy, mc, workspace);
    const FwdLayout& l = al.step;
    SOL_REQUIRE(workspace_bytes >= al.bytes, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, al.bytes);
    if (mc) { io.advection = 1; io.mc_strength = adv->strength; io.mc_ws = al.mc; }
    io.periodic = sv.direct ? sol_periodic_bits(sv.direct_header_host) : 0;      // periodic axes: the stencil phases of karman_periodic.hip
    SOL_REQUIRE(sv.direct || !sol_periodic_bits(sv.box_header_host), "%s: the CG pressure solve is not built for periodic scenes; use the direct "
                "solve (SceneMasks pressure_solver 'auto', 'direct' or 'direct_scattered')", who);
    SOL_REQUIRE(!io.periodic || (!mc && fy == 0.f && fx == 0.f), "%s: periodic scenes run the plain step only: the mac_cormack advection and the "
                "buoyancy force are not built for them (use advection = 0 and a zero force)", who);
    const void* outs[] = {io.d_out, io.vy_out, io.vx_out, io.feat_out, saved.vy, saved.vx, sv.cg_info, sv.p_inout};
    const void* ins[] = {io.d_in, io.vy_in, io.vx_in, io.re, io.active, io.inflow, io.velBCy, io.velBCyMask, sv.box_blob};
    for (const void* o : outs)
        for (const void* i : ins) SOL_REQUIRE(!o || o != i, "%s: outputs must not alias the inputs", who);
    // (kept from the direct step that carves its own sv: it never took a call without any density pointer)
    SOL_REQUIRE(!sv.direct || saved.vy || io.d_in || io.d_out, "%s: outputs must not alias the inputs (d_in and d_out are both NULL)", who);
    SOL_REQUIRE(!saved.vy || (saved.vy != io.vy_out && saved.vx != io.vx_out && saved.vy != saved.vx), "%s: saved_vy / saved_vx must be buffers of their own", who);
    hipStream_t s = (hipStream_t)stream;
    if (int e = sol_large_step(c, s, io, saved.vy ? saved.vy : l.svy, saved.vx ? saved.vx : l.svx, sv.direct, sv.direct_header_host, sv.box_blob,
                               sv.cg_info, l.solver, sv.p_inout)) return e;
    if (sv.p_inout) {
        const size_t n = (size_t)c->B * c->Y * c->X;
        const size_t nb = (n + PCG_T - 1) / PCG_T;
        SOL_LAUNCH(large_copy, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(PCG_T), 0, s, sv.p_inout, (const float*)large_layout(c, l.solver, false).a.x, n);
        SOL_LAUNCH_CHECK();
    }
    return SOL_OK;
}

}  // namespace

extern "C" size_t sol_karman_step_large_workspace_bytes_for(const sol_karman_cfg* c, const int32_t* direct_header_host) {
    if (!c) return 0;
    return fwd_layout(c, true, direct_header_host, true, nullptr).bytes;
}

extern "C" size_t sol_karman_step_large_workspace_bytes(const sol_karman_cfg* c) { return sol_karman_step_large_workspace_bytes_for(c, nullptr); }

extern "C" size_t sol_karman_step_large_cg_workspace_bytes(const sol_karman_cfg* c) {
    if (!c || c->B < 1 || c->Y < 1 || c->X < 1) return 0;
    return fwd_layout(c, false, nullptr, true, nullptr).bytes;
}

extern "C" int sol_karman_step_fwd_large(const sol_karman_cfg* c, void* stream,
                                         const float* d_in, const float* vy_in, const float* vx_in,
                                         const float* re, const float* active, const float* inflow,
                                         const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                                         float* d_out, float* vy_out, float* vx_out,
                                         float* feat_out, const float* feat_scale,
                                         const int32_t* direct_header_host,
                                         void* workspace, size_t workspace_bytes) {
    const SolLargeStep io{d_in, vy_in, vx_in, re, active, inflow, velBCy, velBCyMask, bc_batch_stride, d_out, vy_out, vx_out, feat_out, feat_scale};
    return large_fwd("sol_karman_step_fwd_large", c, stream, io, {true, direct_header_host}, nullptr, workspace, workspace_bytes);
}

extern "C" int sol_karman_step_fwd_large_cg(const sol_karman_cfg* c, void* stream,
                                            const float* d_in, const float* vy_in, const float* vx_in,
                                            const float* re, const float* active, const float* inflow,
                                            const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                                            float* d_out, float* vy_out, float* vx_out,
                                            float* feat_out, const float* feat_scale,
                                            const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                            void* workspace, size_t workspace_bytes) {
    const SolLargeStep io{d_in, vy_in, vx_in, re, active, inflow, velBCy, velBCyMask, bc_batch_stride, d_out, vy_out, vx_out, feat_out, feat_scale};
    return large_fwd("sol_karman_step_fwd_large_cg", c, stream, io, {false, nullptr, box_blob, box_header_host, cg_info}, nullptr, workspace, workspace_bytes);
}

extern "C" int sol_karman_step_fwd_large_cg_warm(const sol_karman_cfg* c, void* stream,
                                                 const float* d_in, const float* vy_in, const float* vx_in,
                                                 const float* re, const float* active, const float* inflow,
                                                 const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                                                 float* d_out, float* vy_out, float* vx_out,
                                                 float* feat_out, const float* feat_scale,
                                                 const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                                 float* p_inout, void* workspace, size_t workspace_bytes) {
    const char* who = "sol_karman_step_fwd_large_cg_warm";
    SOL_REQUIRE(p_inout != nullptr, "%s: NULL pointer argument (p_inout: the initial guess in, the step's pressure out)", who);
    const SolLargeStep io{d_in, vy_in, vx_in, re, active, inflow, velBCy, velBCyMask, bc_batch_stride, d_out, vy_out, vx_out, feat_out, feat_scale};
    return large_fwd(who, c, stream, io, {false, nullptr, box_blob, box_header_host, cg_info, p_inout}, nullptr, workspace, workspace_bytes);
}

// The no-grad step with the buoyancy force F = (fy, fx) (karman_buoyancy.hip), for either solver as the cfg selects it: cfg.direct set =
// sol_karman_step_fwd_large's launches, else sol_karman_step_fwd_large_cg's (p_inout given: _cg_warm's), with k_l_buoyancy between the
// advection and the divergence.  F = (0, 0): the plain call's launches and bits.
extern "C" int sol_karman_step_fwd_large_buoy(const sol_karman_cfg* c, void* stream,
                                              const float* d_in, const float* vy_in, const float* vx_in,
                                              const float* re, const float* active, const float* inflow,
                                              const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                                              float* d_out, float* vy_out, float* vx_out,
                                              float* feat_out, const float* feat_scale,
                                              const int32_t* direct_header_host,
                                              const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                              float* p_inout, void* workspace, size_t workspace_bytes, float fy, float fx) {
    const SolLargeStep io{d_in, vy_in, vx_in, re, active, inflow, velBCy, velBCyMask, bc_batch_stride, d_out, vy_out, vx_out, feat_out, feat_scale};
    return large_fwd("sol_karman_step_fwd_large_buoy", c, stream, io, {c && c->direct, direct_header_host, box_blob, box_header_host, cg_info, p_inout},
                     nullptr, workspace, workspace_bytes, fy, fx);
}

// The training forms (the adjoint is sol_karman_step_bwd_large*, karman_large_bwd.hip): the post-diffusion velocity goes to the caller's
// saved_vy / saved_vx, the workspace holds the solver's part alone; no features
extern "C" int sol_karman_step_fwd_large_saved(const sol_karman_cfg* c, void* stream,
                                               const float* d_in, const float* vy_in, const float* vx_in,
                                               const float* re, const float* active, const float* inflow,
                                               const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                                               float* d_out, float* vy_out, float* vx_out, float* saved_vy, float* saved_vx,
                                               const int32_t* direct_header_host,
                                               const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                               void* workspace, size_t workspace_bytes) {
    const SolLargeStep io{d_in, vy_in, vx_in, re, active, inflow, velBCy, velBCyMask, bc_batch_stride, d_out, vy_out, vx_out, nullptr, nullptr};
    const LargeSaved keep{saved_vy, saved_vx};
    return large_fwd("sol_karman_step_fwd_large_saved", c, stream, io, {c && c->direct, direct_header_host, box_blob, box_header_host, cg_info}, &keep,
                     workspace, workspace_bytes);
}

extern "C" int sol_karman_step_fwd_large_saved_buoy(const sol_karman_cfg* c, void* stream,
                                                    const float* d_in, const float* vy_in, const float* vx_in,
                                                    const float* re, const float* active, const float* inflow,
                                                    const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                                                    float* d_out, float* vy_out, float* vx_out, float* saved_vy, float* saved_vx,
                                                    const int32_t* direct_header_host,
                                                    const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                                    void* workspace, size_t workspace_bytes, float fy, float fx) {
    const SolLargeStep io{d_in, vy_in, vx_in, re, active, inflow, velBCy, velBCyMask, bc_batch_stride, d_out, vy_out, vx_out, nullptr, nullptr};
    const LargeSaved keep{saved_vy, saved_vx};
    return large_fwd("sol_karman_step_fwd_large_saved_buoy", c, stream, io, {c && c->direct, direct_header_host, box_blob, box_header_host, cg_info}, &keep,
                     workspace, workspace_bytes, fy, fx);
}

// The _adv forms of the two _buoy forward steps: every argument of theirs, then the advection (0: semi-Lagrangian -- the _buoy call's
// launches and bits; 1: MacCormack, karman_maccormack.hip) and its correction strength in [0, 1].  The workspace of advection = 1 is the
// _buoy form's plus sol_karman_advect_workspace_bytes (the *_adv_workspace_bytes_for functions).
extern "C" size_t sol_karman_step_fwd_large_adv_workspace_bytes_for(const sol_karman_cfg* c, const int32_t* direct_header_host, int32_t advection) {
    if (!c || c->B < 1 || c->Y < 1 || c->X < 1) return 0;
    return fwd_adv_layout(c, c->direct != nullptr, direct_header_host, true, advection == 1, nullptr).bytes;
}

extern "C" size_t sol_karman_step_fwd_large_saved_adv_workspace_bytes_for(const sol_karman_cfg* c, const int32_t* direct_header_host, int32_t advection) {
    if (!c || c->B < 1 || c->Y < 1 || c->X < 1) return 0;
    return fwd_adv_layout(c, c->direct != nullptr, direct_header_host, false, advection == 1, nullptr).bytes;
}

extern "C" int sol_karman_step_fwd_large_adv(const sol_karman_cfg* c, void* stream,
                                             const float* d_in, const float* vy_in, const float* vx_in,
                                             const float* re, const float* active, const float* inflow,
                                             const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                                             float* d_out, float* vy_out, float* vx_out,
                                             float* feat_out, const float* feat_scale,
                                             const int32_t* direct_header_host,
                                             const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                             float* p_inout, void* workspace, size_t workspace_bytes, float fy, float fx,
                                             int32_t advection, float correction_strength) {
    const SolLargeStep io{d_in, vy_in, vx_in, re, active, inflow, velBCy, velBCyMask, bc_batch_stride, d_out, vy_out, vx_out, feat_out, feat_scale};
    const LargeAdv adv{advection, correction_strength};
    return large_fwd("sol_karman_step_fwd_large_adv", c, stream, io, {c && c->direct, direct_header_host, box_blob, box_header_host, cg_info, p_inout},
                     nullptr, workspace, workspace_bytes, fy, fx, &adv);
}

extern "C" int sol_karman_step_fwd_large_saved_adv(const sol_karman_cfg* c, void* stream,
                                                   const float* d_in, const float* vy_in, const float* vx_in,
                                                   const float* re, const float* active, const float* inflow,
                                                   const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                                                   float* d_out, float* vy_out, float* vx_out, float* saved_vy, float* saved_vx,
                                                   const int32_t* direct_header_host,
                                                   const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                                   void* workspace, size_t workspace_bytes, float fy, float fx,
                                                   int32_t advection, float correction_strength) {
    const SolLargeStep io{d_in, vy_in, vx_in, re, active, inflow, velBCy, velBCyMask, bc_batch_stride, d_out, vy_out, vx_out, nullptr, nullptr};
    const LargeSaved keep{saved_vy, saved_vx};
    const LargeAdv adv{advection, correction_strength};
    return large_fwd("sol_karman_step_fwd_large_saved_adv", c, stream, io, {c && c->direct, direct_header_host, box_blob, box_header_host, cg_info}, &keep,
                     workspace, workspace_bytes, fy, fx, &adv);
}

extern "C" int sol_karman_pressure_solve_large(const sol_karman_cfg* c, void* stream, const float* active, const float* rhs, float* p,
                                               const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                               void* workspace, size_t workspace_bytes) {
    const char* who = "sol_karman_pressure_solve_large";
    if (int e = sol_large_cg_check(c, who, box_blob, box_header_host, cg_info, workspace)) return e;
    const Large l = large_layout(c, workspace);
    SOL_REQUIRE(workspace_bytes >= l.bytes, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, l.bytes);
    SOL_REQUIRE(active && rhs && p, "%s: NULL pointer argument", who);
    SOL_REQUIRE(p != rhs && p != active && p != box_blob && (const void*)cg_info != rhs && (const void*)cg_info != active,
                "%s: outputs must not alias the inputs", who);
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)c->B * c->Y * c->X;
    const size_t nb = (n + PCG_T - 1) / PCG_T;
    const unsigned g = (unsigned)(nb < 4096 ? nb : 4096);
    SOL_LAUNCH(large_copy, dim3(g), dim3(PCG_T), 0, s, l.a.r, rhs, n);
    if (int e = large_solve(s, c, box_blob, active, l, cg_info)) return e;
    SOL_LAUNCH(large_copy, dim3(g), dim3(PCG_T), 0, s, p, (const float*)l.a.x, n);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}
