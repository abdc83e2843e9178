// Buoyancy of the karman-3d step (karman3d.hip): the marker density pushes the velocity, as PhiFlow's IncompressibleFlow.step does with
// buoyancy_factor != 0 -- the 3-D twin of karman_buoyancy.hip.  F = (F_y, F_x, F_z) is a force per unit density (PhiFlow: -gravity *
// buoyancy_factor, Gravity() = -9.81 along y  ->  F = (9.81 beta, 0, 0)); f = dt F travels as three floats.  With dz = the step's OUTPUT
// density (the inflow already in it) inside the grid and 0 outside -- the zero ghost ring of the density's advection --
//   a_y[jf,i,k] = mask_y * ( SL_y(c)[jf,i,k] + f_y * (dz(jf-1,i,k) + dz(jf,i,k)) / 2 )      jf = 0..Y      (a_x, a_z likewise along their axis)
// between the advection (k3_advect / k3_advect_tile) and the divergence (k3_div) of sol_karman3d_step_fwd: one hook for the direct and the
// CG solve, both advection kernels and both inflow orders.  Two linear kernels, exact transposes of each other:
//   k3_buoyancy         face parallel, the three components in one launch: v = fl(v + fl(f * fl(0.5f * (d0 + d1)))) * mask, contraction off.
//                       The advection has applied the mask already and it is 0 or 1, so masking the sum equals masking both terms.
//   k3b_buoyancy_adj    cell parallel gather, no atomics, fixed order (y, x, z):
//                       g_dsum[c] = g_d_out[c] + f_y (m g_y[j] + m g_y[j+1]) / 2 + f_x (m g_x[i] + m g_x[i+1]) / 2 + f_z (m g_z[k] + m g_z[k+1]) / 2
//                       with g = the cotangent of a (inside the step's adjoint: g_a of k3b_gva, which carries the mask already -- applying
//                       it twice changes nothing).  g_dsum then goes through the density adjoint (sol_karman3d_density_bwd, accumulate = 1).
//                       gmax (the absmax slots k3b_gva published, or NULL): a non-finite g_a of a simulation makes ALL of its g_dsum NaN,
//                       so the poisoning rule of fixed_scatter.hpp holds for the density gradient too.
// Work unit of both, as in k3_advect / k3b_gva: one z COLUMN per wave, lanes along the contiguous z.  (component, j, i) and every bound
// that follows from them are wave uniform; no per-point index decoding, loads and stores coalesced.
// A component whose force is zero is not touched (f = (0, 0, 0): the forward kernel is not launched at all).
#include <algorithm>

#include "fixed_scatter.hpp"
#include "karman3d_mask.hpp"

namespace {

struct Buoy3Args {
    int Y, X, Z;
    float fy, fx, fz;                   // dt F
    const float *active, *d;            // [Y,X,Z], [B,Y,X,Z]
    float *vy, *vx, *vz;                // [B,Y+1,X,Z], [B,Y,X+1,Z], [B,Y,X,Z+1], updated in place
};

__global__ void __launch_bounds__(256) k3_buoyancy(Buoy3Args a) {
#pragma clang fp contract(off)
    const int Y = a.Y, X = a.X, Z = a.Z, XZ = X * Z;
    const size_t N = (size_t)Y * XZ, nVy = (size_t)(Y + 1) * XZ, nVx = (size_t)Y * (X + 1) * Z, nVz = (size_t)Y * X * (Z + 1);
    const int b = blockIdx.y;
    const float* d = a.d + b * N;
    const int cY = (Y + 1) * X, cX = Y * (X + 1), cC = Y * X;
    const int lane = threadIdx.x & 63;
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const int nwaves = gridDim.x * (blockDim.x >> 6);
    for (int c = wave0; c < cY + cX + cC; c += nwaves) {
        if (c < cY) {
            if (a.fy == 0.f) continue;
            const int j = c / X, i = c - j * X;
            const int lo = ((j - 1) * X + i) * Z, hi = (j * X + i) * Z;        // cells (j-1, i, .) and (j, i, .); lo is read for j >= 1 only
            float* v = a.vy + b * nVy + hi;
            for (int k = lane; k < Z; k += 64) {
                const float d0 = j >= 1 ? d[lo + k] : 0.f, d1 = j < Y ? d[hi + k] : 0.f;
                const float t = a.fy * (0.5f * (d0 + d1));
                v[k] = (v[k] + t) * face_mask<0>(a.active, Y, X, Z, j, i, k);
            }
        } else if (c < cY + cX) {
            if (a.fx == 0.f) continue;
            const int q = c - cY, j = q / (X + 1), i = q - j * (X + 1);
            const int lo = (j * X + i - 1) * Z, hi = (j * X + i) * Z;          // cells (j, i-1, .) and (j, i, .)
            float* v = a.vx + b * nVx + (size_t)(j * (X + 1) + i) * Z;
            for (int k = lane; k < Z; k += 64) {
                const float d0 = i >= 1 ? d[lo + k] : 0.f, d1 = i < X ? d[hi + k] : 0.f;
                const float t = a.fx * (0.5f * (d0 + d1));
                v[k] = (v[k] + t) * face_mask<1>(a.active, Y, X, Z, j, i, k);
            }
        } else {
            if (a.fz == 0.f) continue;
            const int q = c - cY - cX, j = q / X, i = q - j * X;
            const int col = q * Z;                                             // cells (j, i, .)
            float* v = a.vz + b * nVz + (size_t)q * (Z + 1);
            for (int k = lane; k <= Z; k += 64) {
                const float d0 = k >= 1 ? d[col + k - 1] : 0.f, d1 = k < Z ? d[col + k] : 0.f;
                const float t = a.fz * (0.5f * (d0 + d1));
                v[k] = (v[k] + t) * face_mask<2>(a.active, Y, X, Z, j, i, k);
            }
        }
    }
}

struct Buoy3AdjArgs {
    int Y, X, Z;
    float fy, fx, fz;
    const float *active, *gy, *gx, *gz;     // cotangent of the faces [B,Y+1,X,Z], [B,Y,X+1,Z], [B,Y,X,Z+1]
    const unsigned* gmax;                   // [B][FX_SLOTS] or NULL
    const float* gdo;                       // [B,Y,X,Z] or NULL (= zero)
    float* gds;                             // [B,Y,X,Z]
};

__global__ void __launch_bounds__(256) k3b_buoyancy_adj(Buoy3AdjArgs a) {
#pragma clang fp contract(off)
    const int Y = a.Y, X = a.X, Z = a.Z, XZ = X * Z;
    const size_t N = (size_t)Y * XZ, nVy = (size_t)(Y + 1) * XZ, nVx = (size_t)Y * (X + 1) * Z, nVz = (size_t)Y * X * (Z + 1);
    const int b = blockIdx.y;
    bool poisoned = false;
    if (a.gmax) {
        float qs, qi;
        fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
        poisoned = qi != qi;
    }
    const float* gy = a.gy + b * nVy;
    const float* gx = a.gx + b * nVx;
    const float* gz = a.gz + b * nVz;
    const float* gdo = a.gdo ? a.gdo + b * N : nullptr;
    float* gds = a.gds + b * N;
    const int lane = threadIdx.x & 63;
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const int nwaves = gridDim.x * (blockDim.x >> 6);
    for (int q = wave0; q < Y * X; q += nwaves) {                             // column of cells (j, i, .)
        const int j = q / X, i = q - j * X;
        const int col = q * Z;
        const int y0 = col, y1 = col + XZ;                                     // y faces j, j + 1
        const int x0 = (j * (X + 1) + i) * Z, x1 = x0 + Z;                     // x faces i, i + 1
        const int z0 = q * (Z + 1);                                            // z faces k, k + 1: z0 + k, z0 + k + 1
        for (int k = lane; k < Z; k += 64) {
            float g = gdo ? gdo[col + k] : 0.f;
            if (a.fy != 0.f)
                g += a.fy * (0.5f * (face_mask<0>(a.active, Y, X, Z, j, i, k) * gy[y0 + k] + face_mask<0>(a.active, Y, X, Z, j + 1, i, k) * gy[y1 + k]));
            if (a.fx != 0.f)
                g += a.fx * (0.5f * (face_mask<1>(a.active, Y, X, Z, j, i, k) * gx[x0 + k] + face_mask<1>(a.active, Y, X, Z, j, i + 1, k) * gx[x1 + k]));
            if (a.fz != 0.f)
                g += a.fz * (0.5f * (face_mask<2>(a.active, Y, X, Z, j, i, k) * gz[z0 + k] + face_mask<2>(a.active, Y, X, Z, j, i, k + 1) * gz[z0 + k + 1]));
            gds[col + k] = poisoned ? __uint_as_float(0x7fc00000u) : g;
        }
    }
}

// a few columns per wave, four waves per workgroup: 2 048 workgroups at most (24 768 face columns at 128 x 64 x 64: three trips per wave,
// eight workgroups per CU in flight)
unsigned grid_cols(size_t cols) { return (unsigned)std::min<size_t>(2048, std::max<size_t>(1, (cols + 3) / 4)); }

int shape_check(const char* who, int B, int Y, int X, int Z) {
    SOL_REQUIRE(B >= 1 && B <= 65535 && Y >= 1 && X >= 1 && Z >= 1, "%s: B in [1, 65535], Y, X, Z >= 1 (got %d, %d, %d, %d)", who, B, Y, X, Z);
    SOL_REQUIRE((size_t)(Y + 1) * (X + 1) * (Z + 1) * 3 < ((size_t)1 << 31), "%s: grid too large for 32-bit face indices", who);
    return SOL_OK;
}

}  // namespace

int k3_buoyancy_add(hipStream_t s, int B, int Y, int X, int Z, const float* active, const float* d, float fy, float fx, float fz,
                    float* vy, float* vx, float* vz) {
    if (fy == 0.f && fx == 0.f && fz == 0.f) return SOL_OK;
    const size_t cols = (size_t)(Y + 1) * X + (size_t)Y * (X + 1) + (size_t)Y * X;
    const Buoy3Args a{Y, X, Z, fy, fx, fz, active, d, vy, vx, vz};
    SOL_LAUNCH(k3_buoyancy, dim3(grid_cols(cols), B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

int k3_buoyancy_adj(hipStream_t s, int B, int Y, int X, int Z, const float* active, const float* gy, const float* gx, const float* gz,
                    const unsigned* gmax, float fy, float fx, float fz, const float* g_d_out, float* g_dsum) {
    const Buoy3AdjArgs a{Y, X, Z, fy, fx, fz, active, gy, gx, gz, gmax, g_d_out, g_dsum};
    SOL_LAUNCH(k3b_buoyancy_adj, dim3(grid_cols((size_t)Y * X), B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

extern "C" int sol_karman3d_buoyancy_add(void* stream, int32_t B, int32_t Y, int32_t X, int32_t Z, const float* active, const float* d,
                                         float fy_dt, float fx_dt, float fz_dt, float* vy, float* vx, float* vz) {
    const char* who = "sol_karman3d_buoyancy_add";
    if (int e = shape_check(who, B, Y, X, Z)) return e;
    SOL_REQUIRE(active && d && vy && vx && vz, "%s: NULL pointer argument", who);
    SOL_REQUIRE(fy_dt - fy_dt == 0.f && fx_dt - fx_dt == 0.f && fz_dt - fz_dt == 0.f, "%s: the force must be finite", who);
    const float* outs[] = {vy, vx, vz};
    for (const float* o : outs) SOL_REQUIRE(o != d && o != active, "%s: outputs must not alias the inputs", who);
    SOL_REQUIRE(vy != vx && vy != vz && vx != vz, "%s: outputs must not alias the inputs", who);
    return k3_buoyancy_add((hipStream_t)stream, B, Y, X, Z, active, d, fy_dt, fx_dt, fz_dt, vy, vx, vz);
}

extern "C" int sol_karman3d_buoyancy_add_bwd(void* stream, int32_t B, int32_t Y, int32_t X, int32_t Z, const float* active,
                                             const float* g_vy, const float* g_vx, const float* g_vz, float fy_dt, float fx_dt, float fz_dt,
                                             const float* g_d_out, float* g_dsum) {
    const char* who = "sol_karman3d_buoyancy_add_bwd";
    if (int e = shape_check(who, B, Y, X, Z)) return e;
    SOL_REQUIRE(active && g_vy && g_vx && g_vz && g_dsum, "%s: NULL pointer argument", who);
    SOL_REQUIRE(fy_dt - fy_dt == 0.f && fx_dt - fx_dt == 0.f && fz_dt - fz_dt == 0.f, "%s: the force must be finite", who);
    SOL_REQUIRE(g_dsum != g_vy && g_dsum != g_vx && g_dsum != g_vz && g_dsum != active && g_dsum != g_d_out, "%s: outputs must not alias the inputs", who);
    return k3_buoyancy_adj((hipStream_t)stream, B, Y, X, Z, active, g_vy, g_vx, g_vz, nullptr, fy_dt, fx_dt, fz_dt, g_d_out, g_dsum);
}
