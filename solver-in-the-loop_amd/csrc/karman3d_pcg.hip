// karman-3d: preconditioned conjugate-gradient pressure solve for any obstacle mask (cfg.pressure_solver = 1).
//
// The system is the one the direct solve (karman3d.hip) inverts: M p = b with M = -A, PhiFlow's pressure matrix -- diagonal =
// number of accessible neighbours (precond3d._accessible_diag: a neighbour outside the box counts as the cell itself, p = 0
// there), -1 between two active cells, obstacle rows decoupled.  CG on M preconditioned with the empty-box solve G = M_r^-1
// (k3_apply_G: the sine transforms of the blob with nS = 0), i.e. oracle/sol_oracle3d.solve_pcg in fp32 with fp64 dot products.
//
// Launch structure (fixed: cg_max_iter iterations, no host synchronisation, so that a caller can capture it):
//   k3p_init                      x = 0, r = b (in place), per-workgroup partials of |b|^2, done = 0
//   G, k3p_dot                    z = G r, convergence test, partials of <r, z>
//   cg_max_iter x [ k3p_stencil   p = z + beta p (into the other p buffer), q = M p, partials of <p, q>
//                   k3p_update    alpha = <r, z> / <p, q>, x += alpha p, r -= alpha q, partials of |r|^2
//                   G, k3p_dot ]  (the last iteration: k3p_dot as the convergence test only)
// Every dot product is a slab of per-workgroup fp64 partials [B][nwg] that the NEXT kernel sums in a fixed order in every one
// of its workgroups (no float atomics: the solve is bit-reproducible).  k3p_dot stops a simulation when the recursively
// updated |r|_2 <= max(cg_rtol |b|_2, cg_atol): it sets the simulation's done word, after which its x, r and p are frozen
// (every per-simulation kernel returns at once; the transforms return at once when every simulation is done).  The iterations
// used and the converged flag go to cfg.cg_info [B][2] (or to the workspace when it is NULL).
#include "common.hpp"

namespace {

constexpr int K3P_T = 256;          // threads per workgroup
constexpr int K3P_MAXWG = 512;      // workgroups per simulation (= partials per slab row)

int k3p_nwg(size_t N) { const size_t g = (N + K3P_T - 1) / K3P_T; return (int)(g < (size_t)K3P_MAXWG ? g : (size_t)K3P_MAXWG); }

struct K3PArgs {
    int Y, X, Z, N, nwg;
    float rtol, atol;
    const float* active;
    float *x, *r, *q;
    double *bb, *rr, *pq;           // slabs [B][nwg]
    int* done;                      // [B]
    int* info;                      // [B][2]
};

// sum of v over the workgroup, the same fixed order every run; the result is valid in every thread
__device__ double k3p_block_sum(double v) {
    __shared__ double red[K3P_T / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                                // (a previous call's readers are done with red)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < K3P_T / 64; ++w) t += red[w];
    return t;
}

__device__ double k3p_slab_sum(const double* row, int n) {
    double v = 0.0;
    for (int k = threadIdx.x; k < n; k += K3P_T) v += row[k];
    return k3p_block_sum(v);
}

__device__ __forceinline__ void k3p_publish(double* slab, int nwg, double part) {
    const double t = k3p_block_sum(part);
    if (threadIdx.x == 0) slab[(size_t)blockIdx.y * nwg + blockIdx.x] = t;
}

__global__ void __launch_bounds__(K3P_T) k3p_init(K3PArgs a) {
    const int b = blockIdx.y;
    const size_t o = (size_t)b * a.N;
    double acc = 0.0;
    for (int c = blockIdx.x * K3P_T + threadIdx.x; c < a.N; c += a.nwg * K3P_T) {
        const float v = a.r[o + c];
        a.x[o + c] = 0.f;
        acc += (double)v * v;
    }
    const double t = k3p_block_sum(acc);
    if (threadIdx.x == 0) {
        a.bb[(size_t)b * a.nwg + blockIdx.x] = t;
        a.rr[(size_t)b * a.nwg + blockIdx.x] = t;
        if (blockIdx.x == 0) a.done[b] = 0;
    }
}

// p_new = z + beta p_old (beta = rz_cur / rz_prev; first: p_new = z), q = M p_new, partials of <p_new, q>
__global__ void __launch_bounds__(K3P_T) k3p_stencil(K3PArgs a, const float* __restrict__ z, const float* __restrict__ pold,
                                                      float* __restrict__ pnew, const double* __restrict__ rzc,
                                                      const double* __restrict__ rzp, int first) {
    const int b = blockIdx.y;
    if (a.done[b]) return;
    float beta = 0.f;
    if (!first) {
        const double cur = k3p_slab_sum(rzc + (size_t)b * a.nwg, a.nwg), prev = k3p_slab_sum(rzp + (size_t)b * a.nwg, a.nwg);
        beta = (float)(cur / fmax(prev, 1e-300));
    }
    const int Y = a.Y, X = a.X, Z = a.Z, XZ = X * Z;
    const size_t o = (size_t)b * a.N;
    const float* zb = z + o;
    const float* pb = pold + o;
    auto pn = [&](int e) { return first ? zb[e] : fmaf(beta, pb[e], zb[e]); };
    auto act = [&](int e) { return a.active[e] != 0.f ? 1.f : 0.f; };
    double acc = 0.0;
    for (int c = blockIdx.x * K3P_T + threadIdx.x; c < a.N; c += a.nwg * K3P_T) {
        const int k = c % Z, i = (c / Z) % X, j = c / XZ;
        const float ac = act(c), pc = pn(c);
        float n = 0.f, s = 0.f;
        auto nb = [&](bool inside, int e) {
            if (inside) { const float an = act(e); n += an; s += an * pn(e); }
            else n += ac;                           // outside the box: accessible iff the cell is (edge padding), p = 0 there
        };
        nb(j > 0, c - XZ); nb(j + 1 < Y, c + XZ);
        nb(i > 0, c - Z);  nb(i + 1 < X, c + Z);
        nb(k > 0, c - 1);  nb(k + 1 < Z, c + 1);
        const float qv = fmaxf(n, 1.f) * pc - ac * s;
        pnew[o + c] = pc;
        a.q[o + c] = qv;
        acc += (double)pc * qv;
    }
    k3p_publish(a.pq, a.nwg, acc);
}

// alpha = <r, z> / <p, q>;  x += alpha p;  r -= alpha q;  partials of |r|^2
__global__ void __launch_bounds__(K3P_T) k3p_update(K3PArgs a, const float* __restrict__ p, const double* __restrict__ rzc) {
    const int b = blockIdx.y;
    if (a.done[b]) return;
    const double rz = k3p_slab_sum(rzc + (size_t)b * a.nwg, a.nwg), pq = k3p_slab_sum(a.pq + (size_t)b * a.nwg, a.nwg);
    const float al = (float)(rz / fmax(pq, 1e-300));
    const size_t o = (size_t)b * a.N;
    double acc = 0.0;
    for (int c = blockIdx.x * K3P_T + threadIdx.x; c < a.N; c += a.nwg * K3P_T) {
        a.x[o + c] = fmaf(al, p[o + c], a.x[o + c]);
        const float r = fmaf(-al, a.q[o + c], a.r[o + c]);
        a.r[o + c] = r;
        acc += (double)r * r;
    }
    k3p_publish(a.rr, a.nwg, acc);
}

// convergence test after `iter` updates (every workgroup of the simulation takes the same decision from the same slabs; the
// first one records it), then the partials of <r, z> unless the simulation stopped or this is the last iteration (z == NULL)
__global__ void __launch_bounds__(K3P_T) k3p_dot(K3PArgs a, const float* __restrict__ z, double* __restrict__ rz, int iter) {
    const int b = blockIdx.y;
    if (a.done[b]) return;
    const double bb = k3p_slab_sum(a.bb + (size_t)b * a.nwg, a.nwg), rr = k3p_slab_sum(a.rr + (size_t)b * a.nwg, a.nwg);
    const double rt = (double)a.rtol, at = (double)a.atol;
    const bool conv = rr <= fmax(rt * rt * bb, at * at);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.info[2 * b] = iter;
        a.info[2 * b + 1] = conv ? 1 : 0;
        if (conv) a.done[b] = 1;
    }
    if (conv || !z) return;
    const size_t o = (size_t)b * a.N;
    double acc = 0.0;
    for (int c = blockIdx.x * K3P_T + threadIdx.x; c < a.N; c += a.nwg * K3P_T) acc += (double)a.r[o + c] * z[o + c];
    k3p_publish(rz, a.nwg, acc);
}

struct K3PLayout {
    double *bb, *rr, *pq, *rz0, *rz1;
    int *done, *info;
    float *x, *p0, *p1, *q;
    size_t bytes;
};

K3PLayout k3p_layout(const sol_karman3d_cfg* c, void* ws) {
    const size_t B = c->B, N = (size_t)c->Y * c->X * c->Z, nwg = k3p_nwg(N);
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    char* w = static_cast<char*>(ws);
    K3PLayout l{};
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = w ? w + off : nullptr; off += up(bytes); return p; };
    l.bb = reinterpret_cast<double*>(take(B * nwg * 8));
    l.rr = reinterpret_cast<double*>(take(B * nwg * 8));
    l.pq = reinterpret_cast<double*>(take(B * nwg * 8));
    l.rz0 = reinterpret_cast<double*>(take(B * nwg * 8));
    l.rz1 = reinterpret_cast<double*>(take(B * nwg * 8));
    l.done = reinterpret_cast<int*>(take(B * 4));
    l.info = reinterpret_cast<int*>(take(B * 8));
    l.x = reinterpret_cast<float*>(take(B * N * 4));
    l.p0 = reinterpret_cast<float*>(take(B * N * 4));
    l.p1 = reinterpret_cast<float*>(take(B * N * 4));
    l.q = reinterpret_cast<float*>(take(B * N * 4));
    l.bytes = off;
    return l;
}

}  // namespace

size_t k3_pcg_workspace_bytes(const sol_karman3d_cfg* c) { return c && c->pressure_solver == 1 ? k3p_layout(c, nullptr).bytes + 256 : 0; }

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
    const int B = c->B, N = c->Y * c->X * c->Z, nwg = k3p_nwg(N), K = c->cg_max_iter;
    void* wa = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(ws) + 255) / 256 * 256);
    const K3PLayout l = k3p_layout(c, wa);
    K3PArgs a{};
    a.Y = c->Y; a.X = c->X; a.Z = c->Z; a.N = N; a.nwg = nwg; a.rtol = c->cg_rtol; a.atol = c->cg_atol;
    a.active = active;
    a.x = l.x; a.r = b; a.q = l.q; a.bb = l.bb; a.rr = l.rr; a.pq = l.pq; a.done = l.done; a.info = c->cg_info ? c->cg_info : l.info;
    double* rz[2] = {l.rz0, l.rz1};
    float* p[2] = {l.p0, l.p1};
    const dim3 grid(nwg, B), blk(K3P_T);
    SOL_LAUNCH(k3p_init, grid, blk, 0, s, a);
    float* z = nullptr;
    if (int e = k3_apply_G(s, c, b, t1, t2, &z, l.done)) return e;
    SOL_LAUNCH(k3p_dot, grid, blk, 0, s, a, (const float*)z, rz[0], 0);
    for (int k = 1; k <= K; ++k) {
        SOL_LAUNCH(k3p_stencil, grid, blk, 0, s, a, (const float*)z, (const float*)p[(k - 1) & 1], p[k & 1], (const double*)rz[(k - 1) & 1], (const double*)rz[k & 1], k == 1 ? 1 : 0);
        SOL_LAUNCH(k3p_update, grid, blk, 0, s, a, (const float*)p[k & 1], (const double*)rz[(k - 1) & 1]);
        if (k < K) {
            if (int e = k3_apply_G(s, c, b, t1, t2, &z, l.done)) return e;
            SOL_LAUNCH(k3p_dot, grid, blk, 0, s, a, (const float*)z, rz[k & 1], k);
        } else {
            SOL_LAUNCH(k3p_dot, grid, blk, 0, s, a, (const float*)nullptr, (double*)nullptr, k);
        }
    }
    SOL_LAUNCH_CHECK();
    *x_out = l.x;
    return SOL_OK;
}
