// karman-2d large grids: preconditioned conjugate-gradient pressure solve for any obstacle mask.
//
// The system is the one the large-grid direct solve (karman_large.hip) inverts: M p = b with M = -A, precond.scene_matrix -- diagonal
// = max(number of accessible neighbours, 1) with edge padding (a neighbour outside the box counts as the cell itself, p = 0 there),
// -active_c active_n between neighbours; b = the rhs k_l_div writes.  CG on M preconditioned with the empty-box solve G = M_r^-1
// (sol_large_box_forward / _back: the sine transforms of precond.box_solver_blob, nS = 0), in fp32 with fp64 dot products.  Same
// algorithm and launch structure as the karman-3d solve (karman3d_pcg.hip):
//   klp_init                      x = 0, r = b (in place), per-workgroup partials of |b|^2, done = 0
//   G, klp_dot                    z = G r, convergence test, partials of <r, z>
//   cg_max_iter x [ klp_stencil   p = z + beta p (into the other p buffer), q = M p, partials of <p, q>
//                   klp_update    alpha = <r, z> / <p, q>, x += alpha p, r -= alpha q, partials of |r|^2
//                   G, klp_dot ]  (the last iteration: klp_dot as the convergence test only)
// Every dot product is a slab of per-workgroup fp64 partials [B][nwg <= 512] that the NEXT kernel sums in a fixed order in every one
// of its workgroups (no float atomics: the solve is bit-reproducible).  klp_dot stops a simulation when the recursively updated
// |r|_2 <= max(cg_rtol |b|_2, cg_atol): it sets the simulation's done word, after which its x, r and p are frozen and EVERY launch
// of the simulation returns at once -- the GEMM tiles and the scaling of G included (their batch index is the simulation).  The
// iterations used and the converged flag go to the caller's cg_info [2][B] (row 0 iterations, row 1 converged 0/1).
//
// The launch sequence is fixed and has no host synchronisation when the stream is being captured (hipStreamIsCapturing): a trainer
// or roll-out graph captures the full cg_max_iter budget.  The ONE synchronising case: an EAGER call (no capture) reads the count
// of finished simulations (a 4-byte device word, counted by klp_dot) back to the host every 16 iterations and stops issuing
// iterations once all B simulations are done -- data generation runs thousands of eager steps with the PhiFlow budget of 2000.
// The results do not depend on where it stops: a finished simulation's state is frozen either way.
#include "common.hpp"

namespace {

constexpr int KLP_T = 256;          // threads per workgroup
constexpr int KLP_MAXWG = 512;      // workgroups per simulation (= partials per slab row)
constexpr int KLP_POLL = 16;        // eager calls: iterations between two reads of the finished count
constexpr int FDL_MAGIC = 0x46443032;

int klp_nwg(size_t N) { const size_t g = (N + KLP_T - 1) / KLP_T; return (int)(g < (size_t)KLP_MAXWG ? g : (size_t)KLP_MAXWG); }

struct KLPArgs {
    int B, Y, X, N, nwg;
    float rtol, atol;
    const float* active;
    float *x, *r, *q;
    double *bb, *rr, *pq;           // slabs [B][nwg]
    int* done;                      // [B]
    int* ndone;                     // [1]: simulations finished so far
    int* info;                      // [2][B]
};

// sum of v over the workgroup, the same fixed order every run; the result is valid in every thread
__device__ double klp_block_sum(double v) {
    __shared__ double red[KLP_T / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                                // (a previous call's readers are done with red)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < KLP_T / 64; ++w) t += red[w];
    return t;
}

__device__ double klp_slab_sum(const double* row, int n) {
    double v = 0.0;
    for (int k = threadIdx.x; k < n; k += KLP_T) v += row[k];
    return klp_block_sum(v);
}

__device__ __forceinline__ void klp_publish(double* slab, int nwg, double part) {
    const double t = klp_block_sum(part);
    if (threadIdx.x == 0) slab[(size_t)blockIdx.y * nwg + blockIdx.x] = t;
}

__global__ void __launch_bounds__(KLP_T) klp_copy(float* __restrict__ dst, const float* __restrict__ src, size_t n) {
    for (size_t e = (size_t)blockIdx.x * KLP_T + threadIdx.x; e < n; e += (size_t)gridDim.x * KLP_T) dst[e] = src[e];
}

__global__ void __launch_bounds__(KLP_T) klp_init(KLPArgs a) {
    const int b = blockIdx.y;
    const size_t o = (size_t)b * a.N;
    double acc = 0.0;
    for (int c = blockIdx.x * KLP_T + threadIdx.x; c < a.N; c += a.nwg * KLP_T) {
        const float v = a.r[o + c];
        a.x[o + c] = 0.f;
        acc += (double)v * v;
    }
    const double t = klp_block_sum(acc);
    if (threadIdx.x == 0) {
        a.bb[(size_t)b * a.nwg + blockIdx.x] = t;
        a.rr[(size_t)b * a.nwg + blockIdx.x] = t;
        if (blockIdx.x == 0) a.done[b] = 0;
        if (blockIdx.x == 0 && b == 0) *a.ndone = 0;
    }
}

// p_new = z + beta p_old (beta = rz_cur / rz_prev; first: p_new = z), q = M p_new, partials of <p_new, q>
__global__ void __launch_bounds__(KLP_T) klp_stencil(KLPArgs a, const float* __restrict__ z, const float* __restrict__ pold,
                                                      float* __restrict__ pnew, const double* __restrict__ rzc,
                                                      const double* __restrict__ rzp, int first) {
    const int b = blockIdx.y;
    if (a.done[b]) return;
    float beta = 0.f;
    if (!first) {
        const double cur = klp_slab_sum(rzc + (size_t)b * a.nwg, a.nwg), prev = klp_slab_sum(rzp + (size_t)b * a.nwg, a.nwg);
        beta = (float)(cur / fmax(prev, 1e-300));
    }
    const int Y = a.Y, X = a.X;
    const size_t o = (size_t)b * a.N;
    const float* zb = z + o;
    const float* pb = pold + o;
    auto pn = [&](int e) { return first ? zb[e] : fmaf(beta, pb[e], zb[e]); };
    auto act = [&](int e) { return a.active[e] != 0.f ? 1.f : 0.f; };
    double acc = 0.0;
    for (int c = blockIdx.x * KLP_T + threadIdx.x; c < a.N; c += a.nwg * KLP_T) {
        const int j = c / X, i = c - j * X;
        const float ac = act(c), pc = pn(c);
        float n = 0.f, s = 0.f;
        auto nb = [&](bool inside, int e) {
            if (inside) { const float an = act(e); n += an; s += an * pn(e); }
            else n += ac;                           // outside the box: accessible iff the cell is (edge padding), p = 0 there
        };
        nb(j > 0, c - X); nb(j + 1 < Y, c + X);
        nb(i > 0, c - 1); nb(i + 1 < X, c + 1);
        const float qv = fmaxf(n, 1.f) * pc - ac * s;
        pnew[o + c] = pc;
        a.q[o + c] = qv;
        acc += (double)pc * qv;
    }
    klp_publish(a.pq, a.nwg, acc);
}

// alpha = <r, z> / <p, q>;  x += alpha p;  r -= alpha q;  partials of |r|^2
__global__ void __launch_bounds__(KLP_T) klp_update(KLPArgs a, const float* __restrict__ p, const double* __restrict__ rzc) {
    const int b = blockIdx.y;
    if (a.done[b]) return;
    const double rz = klp_slab_sum(rzc + (size_t)b * a.nwg, a.nwg), pq = klp_slab_sum(a.pq + (size_t)b * a.nwg, a.nwg);
    const float al = (float)(rz / fmax(pq, 1e-300));
    const size_t o = (size_t)b * a.N;
    double acc = 0.0;
    for (int c = blockIdx.x * KLP_T + threadIdx.x; c < a.N; c += a.nwg * KLP_T) {
        a.x[o + c] = fmaf(al, p[o + c], a.x[o + c]);
        const float r = fmaf(-al, a.q[o + c], a.r[o + c]);
        a.r[o + c] = r;
        acc += (double)r * r;
    }
    klp_publish(a.rr, a.nwg, acc);
}

// convergence test after `iter` updates (every workgroup of the simulation takes the same decision from the same slabs; the
// first one records it and counts the simulation as finished), then the partials of <r, z> unless the simulation stopped or this
// is the last iteration (z == NULL)
__global__ void __launch_bounds__(KLP_T) klp_dot(KLPArgs a, const float* __restrict__ z, double* __restrict__ rz, int iter) {
    const int b = blockIdx.y;
    if (a.done[b]) return;
    const double bb = klp_slab_sum(a.bb + (size_t)b * a.nwg, a.nwg), rr = klp_slab_sum(a.rr + (size_t)b * a.nwg, a.nwg);
    const double rt = (double)a.rtol, at = (double)a.atol;
    const bool conv = rr <= fmax(rt * rt * bb, at * at);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.info[b] = iter;
        a.info[a.B + b] = conv ? 1 : 0;
        if (conv) { a.done[b] = 1; atomicAdd(a.ndone, 1); }
    }
    if (conv || !z) return;
    const size_t o = (size_t)b * a.N;
    double acc = 0.0;
    for (int c = blockIdx.x * KLP_T + threadIdx.x; c < a.N; c += a.nwg * KLP_T) acc += (double)a.r[o + c] * z[o + c];
    klp_publish(rz, a.nwg, acc);
}

// workspace: the step's buffers (sv_y, sv_x, rhs / residual, two transform buffers), then the solve's slabs, words and vectors
struct KLPLayout {
    float *svy, *svx, *R, *T1, *T2;
    double *bb, *rr, *pq, *rz0, *rz1;
    int *done, *ndone;
    float *x, *p0, *p1, *q, *z;
    size_t bytes;
};

KLPLayout klp_layout(const sol_karman_cfg* c, void* ws) {
    const size_t B = c->B, Y = c->Y, X = c->X, N = Y * X, nwg = klp_nwg(N);
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    char* w = ws ? reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(ws) + 255) / 256 * 256) : nullptr;
    KLPLayout l{};
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = w ? w + off : nullptr; off += up(bytes); return p; };
    l.svy = reinterpret_cast<float*>(take(B * (Y + 1) * X * 4));
    l.svx = reinterpret_cast<float*>(take(B * Y * (X + 1) * 4));
    l.R = reinterpret_cast<float*>(take(B * N * 4));
    l.T1 = reinterpret_cast<float*>(take(B * N * 4));
    l.T2 = reinterpret_cast<float*>(take(B * N * 4));
    l.bb = reinterpret_cast<double*>(take(B * nwg * 8));
    l.rr = reinterpret_cast<double*>(take(B * nwg * 8));
    l.pq = reinterpret_cast<double*>(take(B * nwg * 8));
    l.rz0 = reinterpret_cast<double*>(take(B * nwg * 8));
    l.rz1 = reinterpret_cast<double*>(take(B * nwg * 8));
    l.done = reinterpret_cast<int*>(take(B * 4));
    l.ndone = reinterpret_cast<int*>(take(4));
    l.x = reinterpret_cast<float*>(take(B * N * 4));
    l.p0 = reinterpret_cast<float*>(take(B * N * 4));
    l.p1 = reinterpret_cast<float*>(take(B * N * 4));
    l.q = reinterpret_cast<float*>(take(B * N * 4));
    l.z = reinterpret_cast<float*>(take(B * N * 4));
    l.bytes = off + 256;                                // + the alignment of the caller's pointer
    return l;
}

// checks shared by the two entry points (before any launch)
int klp_check(const sol_karman_cfg* c, const char* who, const float* box_blob, const int32_t* hdr, const int32_t* cg_info,
              const void* workspace, size_t workspace_bytes) {
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
    SOL_REQUIRE(workspace_bytes >= klp_layout(c, nullptr).bytes, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes,
                klp_layout(c, nullptr).bytes);
    return SOL_OK;
}

// M x = b by PCG; b (= l.R) is overwritten with the residual
int klp_solve(hipStream_t s, const sol_karman_cfg* c, const float* blob, const float* active, const KLPLayout& l, int32_t* info) {
    const int B = c->B, Y = c->Y, X = c->X, N = Y * X, nwg = klp_nwg(N), K = c->cg_max_iter;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    SOL_HIP_CHECK(hipStreamIsCapturing(s, &cap));
    const bool eager = cap == hipStreamCaptureStatusNone;
    KLPArgs a{};
    a.B = B; a.Y = Y; a.X = X; a.N = N; a.nwg = nwg; a.rtol = c->cg_rtol; a.atol = c->cg_atol;
    a.active = active;
    a.x = l.x; a.r = l.R; a.q = l.q; a.bb = l.bb; a.rr = l.rr; a.pq = l.pq; a.done = l.done; a.ndone = l.ndone; a.info = info;
    double* rz[2] = {l.rz0, l.rz1};
    float* p[2] = {l.p0, l.p1};
    const dim3 grid(nwg, B), blk(KLP_T);
    auto apply_G = [&]() -> int {
        if (int e = sol_large_box_forward(s, B, Y, X, blob, l.R, l.T1, l.T2, l.done)) return e;
        return sol_large_box_back(s, B, Y, X, blob, l.T2, l.T1, l.z, l.done);
    };
    SOL_LAUNCH(klp_init, grid, blk, 0, s, a);
    if (int e = apply_G()) return e;
    SOL_LAUNCH(klp_dot, grid, blk, 0, s, a, (const float*)l.z, rz[0], 0);
    for (int k = 1; k <= K; ++k) {
        SOL_LAUNCH(klp_stencil, grid, blk, 0, s, a, (const float*)l.z, (const float*)p[(k - 1) & 1], p[k & 1], (const double*)rz[(k - 1) & 1],
                   (const double*)rz[k & 1], k == 1 ? 1 : 0);
        SOL_LAUNCH(klp_update, grid, blk, 0, s, a, (const float*)p[k & 1], (const double*)rz[(k - 1) & 1]);
        if (k < K) {
            if (int e = apply_G()) return e;
            SOL_LAUNCH(klp_dot, grid, blk, 0, s, a, (const float*)l.z, rz[k & 1], k);
        } else {
            SOL_LAUNCH(klp_dot, grid, blk, 0, s, a, (const float*)nullptr, (double*)nullptr, k);
        }
        SOL_LAUNCH_CHECK();
        if (eager && k < K && k % KLP_POLL == 0) {
            int finished = 0;
            SOL_HIP_CHECK(hipMemcpyAsync(&finished, l.ndone, sizeof(int), hipMemcpyDeviceToHost, s));
            SOL_HIP_CHECK(hipStreamSynchronize(s));
            if (finished >= B) break;
        }
    }
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

}  // namespace

extern "C" size_t sol_karman_step_large_cg_workspace_bytes(const sol_karman_cfg* c) {
    if (!c || c->B < 1 || c->Y < 1 || c->X < 1) return 0;
    return klp_layout(c, nullptr).bytes;
}

extern "C" int sol_karman_step_fwd_large_cg(const sol_karman_cfg* c, void* stream,
                                            const float* d_in, const float* vy_in, const float* vx_in,
                                            const float* re, const float* active, const float* inflow,
                                            const float* velBCy, const float* velBCyMask, int64_t bc_batch_stride,
                                            float* d_out, float* vy_out, float* vx_out,
                                            float* feat_out, const float* feat_scale,
                                            const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                            void* workspace, size_t workspace_bytes) {
    const char* who = "sol_karman_step_fwd_large_cg";
    if (int e = klp_check(c, who, box_blob, box_header_host, cg_info, workspace, workspace_bytes)) return e;
    SOL_REQUIRE(vy_in && vx_in && re && active && velBCy && velBCyMask && vy_out && vx_out, "%s: NULL pointer argument", who);
    SOL_REQUIRE((d_in && inflow) || !d_out, "%s: density output requested without d_in / inflow", who);
    SOL_REQUIRE(!feat_out || feat_scale, "%s: feat_out requires feat_scale", who);
    SOL_REQUIRE(vy_in != vy_out && vx_in != vx_out && (d_in != d_out || !d_out), "%s: outputs must not alias the inputs", who);
    const void* outs[] = {d_out, vy_out, vx_out, feat_out, cg_info};
    const void* ins[] = {d_in, vy_in, vx_in, re, active, inflow, velBCy, velBCyMask, box_blob};
    for (const void* o : outs)
        for (const void* i : ins) SOL_REQUIRE(!o || o != i, "%s: outputs must not alias the inputs", who);
    hipStream_t s = (hipStream_t)stream;
    const KLPLayout l = klp_layout(c, workspace);
    const SolLargeStep io{d_in, vy_in, vx_in, re, active, inflow, velBCy, velBCyMask, bc_batch_stride, d_out, vy_out, vx_out, feat_out, feat_scale};
    if (int e = sol_large_front(c, s, io, l.svy, l.svx, l.R)) return e;
    if (int e = klp_solve(s, c, box_blob, active, l, cg_info)) return e;
    return sol_large_project(c, s, io, l.x);
}

extern "C" int sol_karman_pressure_solve_large(const sol_karman_cfg* c, void* stream, const float* active, const float* rhs, float* p,
                                               const float* box_blob, const int32_t* box_header_host, int32_t* cg_info,
                                               void* workspace, size_t workspace_bytes) {
    const char* who = "sol_karman_pressure_solve_large";
    if (int e = klp_check(c, who, box_blob, box_header_host, cg_info, workspace, workspace_bytes)) return e;
    SOL_REQUIRE(active && rhs && p, "%s: NULL pointer argument", who);
    SOL_REQUIRE(p != rhs && p != active && p != box_blob && (const void*)cg_info != rhs && (const void*)cg_info != active,
                "%s: outputs must not alias the inputs", who);
    hipStream_t s = (hipStream_t)stream;
    const KLPLayout l = klp_layout(c, workspace);
    const size_t n = (size_t)c->B * c->Y * c->X;
    const size_t nb = (n + KLP_T - 1) / KLP_T;
    const unsigned g = (unsigned)(nb < 4096 ? nb : 4096);
    SOL_LAUNCH(klp_copy, dim3(g), dim3(KLP_T), 0, s, l.R, rhs, n);
    if (int e = klp_solve(s, c, box_blob, active, l, cg_info)) return e;
    SOL_LAUNCH(klp_copy, dim3(g), dim3(KLP_T), 0, s, p, (const float*)l.x, n);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}
