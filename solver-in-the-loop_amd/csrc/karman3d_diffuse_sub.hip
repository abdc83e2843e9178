// Diffusion substeps of the karman-3d step (diffusion_substeps = n on the Python surface; include/sol_hip.h, "DIFFUSION SUBSTEPS of the
// karman-3d step"): the 3-D twin of karman_diffuse_sub.hip.  The step diffuses the velocity with one explicit Euler stencil
// v += alpha Lap(v), alpha = dt res^2 / Re (k3_diffuse), a convex combination only while alpha <= 1/6.  With M = I + (alpha / n) L, L the
// 7-point Laplacian with replicate padding on each of the three face grids, the step with n substeps is the plain step at alpha / n applied
// to M^(n-1) v: the kernel here computes M^m v and every existing kernel stays as it is.  L is symmetric on every face grid, so the same
// kernel applied to the cotangent of M^(n-1) v is the adjoint.
//   k3_diffuse_sub<M>  M <= S_MAX substeps in one launch by temporal blocking: a workgroup loads a TY x TX x TZ tile of one component and
//                      a halo of M faces (clipped to the grid) into LDS, runs the substeps between two LDS planes on a region that shrinks
//                      by one face per substep towards the tile, and stores the tile.  One launch covers the three components and the
//                      batch (blockIdx.y); alpha_b = adt / re[b] as in k3_diffuse.  M is a template argument: the LDS box is the tile plus
//                      exactly M faces a side (M = 1: 27 KB, M = 2: 41 KB, M = 3: 60 KB for the two planes -- five, three and two workgroups
//                      a CU), and the index arithmetic divides by constants.
// Replicate padding: the ghost of a border face is that face's CURRENT value at every substep, so the neighbour index is clamped to the
// grid inside the LDS stencil (a clipped halo edge IS the grid's edge).  A halo edge inside the grid is no edge: values beside it go
// stale one face per substep and the shrinking region never reads a stale one.
// Each substep is the one expression fmaf(alpha, lap, c) with lap summed in lap7's order (karman3d.hip) and contraction off, so a face's
// value does not depend on the tiling or on M: a launch of m substeps equals m launches of one substep bit for bit.
// LDS: lanes run along z, the contiguous axis; the loops run over whole y-slabs of the box, so the LDS address of a lane is the loop
// index: consecutive lanes read consecutive dwords for the centre and the +-z neighbours, and the +-x / +-y neighbours sit at the constant
// pitches PZ and PX * PZ -- consecutive dwords again, whatever the pitch: no bank conflict but at the few clamped lanes.  One barrier per
// substep.
#include "carve.hpp"
#include "common.hpp"

namespace {

constexpr int S_MAX = 3, TY = 8, TX = 8, TZ = 32;
constexpr int DS3_THREADS = 256;

struct Ds3Comp {            // one face grid [H][W][D] and its tiling
    int H, W, D, ntx, ntz, nt;
    const float* in;
    float* out;
};

struct Ds3Args {
    Ds3Comp c[3];
    float adt;
    const float* re;
};

template <int M>
__global__ void __launch_bounds__(DS3_THREADS) k3_diffuse_sub(Ds3Args a) {
#pragma clang fp contract(off)
    constexpr int PY = TY + 2 * M, PX = TX + 2 * M, PZ = TZ + 2 * M, SLAB = PX * PZ;
    __shared__ float plane[2][PY * SLAB];
    const int b = blockIdx.y;
    int t = blockIdx.x, ci = 0;
    if (t >= a.c[0].nt) { t -= a.c[0].nt; ci = 1; }
    if (ci == 1 && t >= a.c[1].nt) { t -= a.c[1].nt; ci = 2; }
    const Ds3Comp g = ci == 0 ? a.c[0] : ci == 1 ? a.c[1] : a.c[2];       // (uniform selects: no dynamic index into the kernel arguments)
    const int H = g.H, W = g.W, D = g.D;
    const size_t base = (size_t)b * H * W * D;
    const float* src = g.in + base;
    float* dst = g.out + base;
    const int tz = t % g.ntz, tx = (t / g.ntz) % g.ntx, ty = t / (g.ntz * g.ntx);
    const int j0 = ty * TY, i0 = tx * TX, k0 = tz * TZ;                                  // the tile's first face
    const int j1 = min(j0 + TY, H), i1 = min(i0 + TX, W), k1 = min(k0 + TZ, D);          // one past its last
    // box element (r, c, z) holds grid face (oj + r, oi + c, ok + z); [ra, rb) x [ca, cb) x [za, zb) is the part inside the grid
    const int oj = j0 - M, oi = i0 - M, ok = k0 - M;
    const int ra = max(oj, 0) - oj, rb = min(j1 + M, H) - oj, ca = max(oi, 0) - oi, cb = min(i1 + M, W) - oi;
    const int za = max(ok, 0) - ok, zb = min(k1 + M, D) - ok;
    for (int k = ra * SLAB + threadIdx.x; k < rb * SLAB; k += DS3_THREADS) {
        const int r = k / SLAB, q = k - r * SLAB, c = q / PZ, z = q - c * PZ;
        if (c >= ca && c < cb && z >= za && z < zb) plane[0][k] = src[((size_t)(oj + r) * W + (oi + c)) * D + (ok + z)];
    }
    __syncthreads();
    const float alpha = a.adt / a.re[b];
    int cur = 0;
#pragma unroll 1
    for (int s = 1; s <= M; ++s) {
        // faces within M - s of the tile: what the remaining substeps still read
        const int h = M - s;
        const int qa = max(j0 - h, 0) - oj, qb = min(j1 + h, H) - oj, pa = max(i0 - h, 0) - oi, pb = min(i1 + h, W) - oi;
        const int wa = max(k0 - h, 0) - ok, wb = min(k1 + h, D) - ok;
        const float* p = plane[cur];
        float* o = plane[cur ^ 1];
        for (int k = qa * SLAB + threadIdx.x; k < qb * SLAB; k += DS3_THREADS) {
            const int r = k / SLAB, q = k - r * SLAB, c = q / PZ, z = q - c * PZ;
            if (c < pa || c >= pb || z < wa || z >= wb) continue;
            const float v = p[k];
            const float lap = p[r + 1 < rb ? k + SLAB : k] + p[r > ra ? k - SLAB : k] + p[c + 1 < cb ? k + PZ : k] + p[c > ca ? k - PZ : k] +
                              p[z + 1 < zb ? k + 1 : k] + p[z > za ? k - 1 : k] - 6.f * v;
            o[k] = __fmaf_rn(alpha, lap, v);
        }
        __syncthreads();
        cur ^= 1;
    }
    const float* p = plane[cur];
    for (int k = threadIdx.x; k < (j1 - j0) * TX * TZ; k += DS3_THREADS) {
        const int r = k / (TX * TZ), q = k - r * (TX * TZ), c = q / TZ, z = q - c * TZ;
        if (i0 + c < i1 && k0 + z < k1) dst[((size_t)(j0 + r) * W + (i0 + c)) * D + (k0 + z)] = p[(r + M) * SLAB + (c + M) * PZ + (z + M)];
    }
}

struct Ds3Layout {
    float* t[2][3];            // the ping-pong triples of a call of more than one launch
    size_t bytes;
};

int ds3_launches(int m, int chunk) { return (m + chunk - 1) / chunk; }

Ds3Layout ds3_layout(const sol_karman3d_cfg* c, int launches, void* ws) {
    const size_t B = c->B, Y = c->Y, X = c->X, Z = c->Z;
    const size_t n[3] = {(Y + 1) * X * Z, Y * (X + 1) * Z, Y * X * (Z + 1)};
    Carve w(ws);
    Ds3Layout l{};
    if (launches > 1)
        for (int k = 0; k < 2; ++k)
            for (int i = 0; i < 3; ++i) l.t[k][i] = w.take<float>(B * n[i]);
    l.bytes = launches > 1 ? w.bytes() : 0;
    return l;
}

bool ds3_shape_ok(const sol_karman3d_cfg* c) {
    return c && c->B >= 1 && c->B <= 65535 && c->Y >= 16 && c->X >= 8 && c->Z >= 8 && (size_t)(c->Y + 1) * (c->X + 1) * (c->Z + 1) < ((size_t)1 << 30);
}

void ds3_launch(int m, dim3 grid, hipStream_t s, const Ds3Args& a) {
    switch (m) {
        case 1: SOL_LAUNCH_NAMED("k3_diffuse_sub<1>", k3_diffuse_sub<1>, grid, dim3(DS3_THREADS), 0, s, a); break;
        case 2: SOL_LAUNCH_NAMED("k3_diffuse_sub<2>", k3_diffuse_sub<2>, grid, dim3(DS3_THREADS), 0, s, a); break;
        default: SOL_LAUNCH_NAMED("k3_diffuse_sub<3>", k3_diffuse_sub<3>, grid, dim3(DS3_THREADS), 0, s, a); break;
    }
}
static_assert(S_MAX == 3, "ds3_launch lists one instantiation per substep count");

}  // namespace

extern "C" int32_t sol_karman3d_diffuse_sub_max(void) { return S_MAX; }

extern "C" size_t sol_karman3d_diffuse_sub_workspace_bytes(const sol_karman3d_cfg* c, int32_t m, int32_t chunk) {
    if (!ds3_shape_ok(c) || m < 1) return 0;
    if (chunk < 1 || chunk > S_MAX) chunk = S_MAX;
    return ds3_layout(c, ds3_launches(m, chunk), nullptr).bytes;
}

extern "C" int sol_karman3d_diffuse_sub(const sol_karman3d_cfg* c, void* stream, const float* vy_in, const float* vx_in, const float* vz_in,
                                        const float* re, float* vy_out, float* vx_out, float* vz_out, int32_t m, int32_t chunk,
                                        void* workspace, size_t workspace_bytes) {
    const char* who = "sol_karman3d_diffuse_sub";
    SOL_REQUIRE(c != nullptr, "%s: cfg is NULL", who);
    SOL_REQUIRE(c->B >= 1 && c->B <= 65535 && c->Y >= 16 && c->X >= 8 && c->Z >= 8, "%s: B in [1, 65535], Y >= 16, X, Z >= 8 (got %d, %d, %d, %d)", who,
                c->B, c->Y, c->X, c->Z);
    SOL_REQUIRE(ds3_shape_ok(c), "%s: grid too large for 32-bit face indices", who);
    SOL_REQUIRE(m >= 1 && m <= 4096, "%s: the number of substeps m must be in [1, 4096] (got %d)", who, m);
    SOL_REQUIRE(chunk >= 0 && chunk <= S_MAX, "%s: chunk (substeps per launch) must be in [1, %d], or 0 for %d (got %d)", who, S_MAX, S_MAX, chunk);
    SOL_REQUIRE(vy_in && vx_in && vz_in && re && vy_out && vx_out && vz_out, "%s: NULL pointer argument", who);
    const float* ins[] = {vy_in, vx_in, vz_in};
    float* outs[] = {vy_out, vx_out, vz_out};
    for (const void* o : outs) {
        for (const void* i : ins) SOL_REQUIRE(o != i, "%s: outputs must not alias the inputs", who);
        SOL_REQUIRE(o != re, "%s: outputs must not alias the inputs", who);
    }
    SOL_REQUIRE(vy_out != vx_out && vy_out != vz_out && vx_out != vz_out, "%s: vy_out, vx_out and vz_out must be buffers of their own", who);
    if (chunk == 0) chunk = S_MAX;
    const int launches = ds3_launches(m, chunk);
    const Ds3Layout l = ds3_layout(c, launches, workspace);
    SOL_REQUIRE(l.bytes == 0 || workspace != nullptr, "%s: %d launches need a workspace (%zu bytes)", who, launches, l.bytes);
    SOL_REQUIRE(workspace_bytes >= l.bytes, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, l.bytes);
    Ds3Args a{};
    a.re = re;
    a.adt = c->dt * c->res * c->res;
    const int dims[3][3] = {{c->Y + 1, c->X, c->Z}, {c->Y, c->X + 1, c->Z}, {c->Y, c->X, c->Z + 1}};
    int tiles = 0;
    for (int i = 0; i < 3; ++i) {
        Ds3Comp& g = a.c[i];
        g.H = dims[i][0]; g.W = dims[i][1]; g.D = dims[i][2];
        g.ntx = (g.W + TX - 1) / TX; g.ntz = (g.D + TZ - 1) / TZ;
        g.nt = ((g.H + TY - 1) / TY) * g.ntx * g.ntz;
        tiles += g.nt;
    }
    hipStream_t s = (hipStream_t)stream;
    // the last launch writes the outputs; the launches before it alternate between the two workspace triples
    const float* src[3] = {vy_in, vx_in, vz_in};
    for (int k = 0, left = m; k < launches; ++k) {
        const int mk = left < chunk ? left : chunk;
        for (int i = 0; i < 3; ++i) {
            a.c[i].in = src[i];
            a.c[i].out = k == launches - 1 ? outs[i] : l.t[k & 1][i];
        }
        ds3_launch(mk, dim3(tiles, c->B), s, a);
        SOL_LAUNCH_CHECK();
        for (int i = 0; i < 3; ++i) src[i] = a.c[i].out;
        left -= mk;
    }
    return SOL_OK;
}
