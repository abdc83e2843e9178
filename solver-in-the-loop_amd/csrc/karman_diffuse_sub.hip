// Diffusion substeps of the karman-2d step (diffusion_substeps = n on the Python surface; include/sol_hip.h, "DIFFUSION SUBSTEPS").
// The step diffuses the velocity with one explicit Euler stencil v += alpha Lap(v), alpha = dt res^2 / Re (k_l_diffuse, dif_y / dif_x of
// the fused kernels), a convex combination only while alpha <= 1/4.  With M = I + (alpha / n) L, L the 5-point Laplacian with replicate
// padding on each face grid, the step with n substeps is the plain step at alpha / n applied to M^(n-1) v: the kernel here computes
// M^m v and every existing kernel stays as it is.  L is symmetric on both face grids, so the same kernel applied to the cotangent of
// M^(n-1) v is the adjoint.
//   k_diffuse_sub   m <= S_MAX substeps in one launch by temporal blocking: a workgroup loads a TY x TX tile of one component and a halo
//                   of m faces (clipped to the grid) into LDS, runs the substeps between two LDS planes on a region that shrinks by one
//                   face per substep towards the tile, and stores the tile.  One launch covers both components and the batch
//                   (blockIdx.y); alpha_b = adt / re[b] as in k_l_diffuse.
// Replicate padding: the ghost of a border face is that face's CURRENT value at every substep, so the neighbour index is clamped to the
// grid inside the LDS stencil (a clipped halo edge IS the grid's edge).  A halo edge inside the grid is no edge: values beside it go
// stale one face per substep and the shrinking region never reads a stale one.
// Each substep is the one expression fmaf(alpha, lap, c) with lap summed in k_l_diffuse's order and contraction off, so a face's value
// does not depend on the tiling or on m: a launch of m substeps equals m launches of one substep bit for bit.
// LDS: two planes of (TY + 2 S_MAX) x (TX + 2 S_MAX) = 48 x 80 floats, 30 KB.  The loops run over whole rows of the plane, so the LDS
// address of a lane is the loop index: consecutive lanes read consecutive dwords for the centre, the row neighbours (+-1) and the
// column neighbours (+-pitch) -- no bank conflict but at the few clamped lanes.  One barrier per substep.
#include "carve.hpp"
#include "common.hpp"

namespace {

constexpr int S_MAX = 8, TY = 32, TX = 64;
constexpr int PY = TY + 2 * S_MAX, PX = TX + 2 * S_MAX;       // the LDS plane
constexpr int DS_THREADS = 256;

struct DsArgs {
    int Y, X, m;
    int tx_y, nt_y, tx_x;                 // tile columns of the v_y grid, its tile count, tile columns of the v_x grid
    float adt;
    const float *vy_in, *vx_in, *re;
    float *vy_out, *vx_out;
};

__global__ void __launch_bounds__(DS_THREADS) k_diffuse_sub(DsArgs a) {
#pragma clang fp contract(off)
    __shared__ float plane[2][PY * PX];
    const int b = blockIdx.y, m = a.m;
    int t = blockIdx.x, H, W, ntx;
    const float* src;
    float* dst;
    if (t < a.nt_y) {
        H = a.Y + 1; W = a.X; ntx = a.tx_y;
        src = a.vy_in + (size_t)b * H * W; dst = a.vy_out + (size_t)b * H * W;
    } else {
        t -= a.nt_y;
        H = a.Y; W = a.X + 1; ntx = a.tx_x;
        src = a.vx_in + (size_t)b * H * W; dst = a.vx_out + (size_t)b * H * W;
    }
    const int j0 = (t / ntx) * TY, i0 = (t % ntx) * TX;                 // the tile's first face
    const int j1 = min(j0 + TY, H), i1 = min(i0 + TX, W);               // one past its last
    // plane row r holds grid row oj + r, plane column c grid column oi + c; [ra, rb) x [ca, cb) is the part inside the grid
    const int oj = j0 - S_MAX, oi = i0 - S_MAX;
    const int ra = max(j0 - m, 0) - oj, rb = min(j1 + m, H) - oj, ca = max(i0 - m, 0) - oi, cb = min(i1 + m, W) - oi;
    for (int k = ra * PX + threadIdx.x; k < rb * PX; k += DS_THREADS) {
        const int r = k / PX, c = k - r * PX;
        if (c >= ca && c < cb) plane[0][k] = src[(size_t)(oj + r) * W + oi + c];
    }
    __syncthreads();
    const float alpha = a.adt / a.re[b];
    int cur = 0;
    for (int s = 1; s <= m; ++s) {
        // faces within m - s of the tile: what the remaining substeps still read
        const int qa = max(j0 - (m - s), 0) - oj, qb = min(j1 + (m - s), H) - oj, pa = max(i0 - (m - s), 0) - oi, pb = min(i1 + (m - s), W) - oi;
        const float* p = plane[cur];
        float* q = plane[cur ^ 1];
        for (int k = qa * PX + threadIdx.x; k < qb * PX; k += DS_THREADS) {
            const int r = k / PX, c = k - r * PX;
            if (c < pa || c >= pb) continue;
            const float v = p[k];
            const float lap = p[min(r + 1, rb - 1) * PX + c] + p[max(r - 1, ra) * PX + c] + p[r * PX + min(c + 1, cb - 1)] + p[r * PX + max(c - 1, ca)] - 4.f * v;
            q[k] = __fmaf_rn(alpha, lap, v);
        }
        __syncthreads();
        cur ^= 1;
    }
    const float* p = plane[cur];
    for (int k = threadIdx.x; k < (j1 - j0) * TX; k += DS_THREADS) {
        const int r = k / TX, c = k - r * TX;
        if (i0 + c < i1) dst[(size_t)(j0 + r) * W + i0 + c] = p[(r + S_MAX) * PX + c + S_MAX];
    }
}

struct DsLayout {
    float *ty, *tx;            // the ping-pong pair of a call of more than one launch
    size_t bytes;
};

int ds_launches(int m, int chunk) { return (m + chunk - 1) / chunk; }

DsLayout ds_layout(const sol_karman_cfg* c, int launches, void* ws) {
    const size_t B = c->B, nVy = (size_t)(c->Y + 1) * c->X, nVx = (size_t)c->Y * (c->X + 1);
    Carve w(ws);
    DsLayout l{};
    if (launches > 1) l = DsLayout{w.take<float>(B * nVy), w.take<float>(B * nVx), 0};
    l.bytes = launches > 1 ? w.bytes() : 0;
    return l;
}

bool ds_shape_ok(const sol_karman_cfg* c) { return c && c->B >= 1 && c->B <= 65535 && c->Y >= 16 && c->X >= 16 && (size_t)c->Y * c->X < ((size_t)1 << 28); }

}  // namespace

extern "C" int32_t sol_karman_diffuse_sub_max(void) { return S_MAX; }

extern "C" size_t sol_karman_diffuse_sub_workspace_bytes(const sol_karman_cfg* c, int32_t m, int32_t chunk) {
    if (!ds_shape_ok(c) || m < 1) return 0;
    if (chunk < 1 || chunk > S_MAX) chunk = S_MAX;
    return ds_layout(c, ds_launches(m, chunk), nullptr).bytes;
}

extern "C" int sol_karman_diffuse_sub(const sol_karman_cfg* c, void* stream, const float* vy_in, const float* vx_in, const float* re,
                                      float* vy_out, float* vx_out, int32_t m, int32_t chunk, void* workspace, size_t workspace_bytes) {
    const char* who = "sol_karman_diffuse_sub";
    SOL_REQUIRE(c != nullptr, "%s: cfg is NULL", who);
    SOL_REQUIRE(c->B >= 1 && c->B <= 65535 && c->Y >= 16 && c->X >= 16, "%s: B in [1, 65535], Y, X >= 16 (got %d, %d, %d)", who, c->B, c->Y, c->X);
    SOL_REQUIRE((size_t)c->Y * c->X < ((size_t)1 << 28), "%s: grid too large for 32-bit face indices", who);
    SOL_REQUIRE(m >= 1 && m <= 4096, "%s: the number of substeps m must be in [1, 4096] (got %d)", who, m);
    SOL_REQUIRE(chunk >= 0 && chunk <= S_MAX, "%s: chunk (substeps per launch) must be in [1, %d], or 0 for %d (got %d)", who, S_MAX, S_MAX, chunk);
    SOL_REQUIRE(vy_in && vx_in && re && vy_out && vx_out, "%s: NULL pointer argument", who);
    const void* outs[] = {vy_out, vx_out};
    const void* ins[] = {vy_in, vx_in, re};
    for (const void* o : outs)
        for (const void* i : ins) SOL_REQUIRE(o != i, "%s: outputs must not alias the inputs", who);
    SOL_REQUIRE(vy_out != vx_out, "%s: vy_out and vx_out must be buffers of their own", who);
    if (chunk == 0) chunk = S_MAX;
    const int launches = ds_launches(m, chunk);
    const DsLayout l = ds_layout(c, launches, workspace);
    SOL_REQUIRE(l.bytes == 0 || workspace != nullptr, "%s: %d launches need a workspace (%zu bytes)", who, launches, l.bytes);
    SOL_REQUIRE(workspace_bytes >= l.bytes, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, l.bytes);
    DsArgs a{};
    a.Y = c->Y; a.X = c->X; a.re = re;
    a.adt = c->dt * c->res * c->res;
    a.tx_y = (c->X + TX - 1) / TX; a.nt_y = ((c->Y + 1 + TY - 1) / TY) * a.tx_y;
    a.tx_x = (c->X + 1 + TX - 1) / TX;
    const int nt_x = ((c->Y + TY - 1) / TY) * a.tx_x;
    hipStream_t s = (hipStream_t)stream;
    // the last launch writes the outputs; going backwards from it the destinations alternate between the outputs and the workspace pair
    const float *sy = vy_in, *sx = vx_in;
    for (int k = 0, left = m; k < launches; ++k) {
        const bool to_out = (launches - 1 - k) % 2 == 0;
        a.m = left < chunk ? left : chunk;
        a.vy_in = sy; a.vx_in = sx;
        a.vy_out = to_out ? vy_out : l.ty; a.vx_out = to_out ? vx_out : l.tx;
        SOL_LAUNCH(k_diffuse_sub, dim3(a.nt_y + nt_x, c->B), dim3(DS_THREADS), 0, s, a);
        SOL_LAUNCH_CHECK();
        sy = a.vy_out; sx = a.vx_out;
        left -= a.m;
    }
    return SOL_OK;
}
