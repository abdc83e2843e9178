// Buoyancy of the large-grid karman-2d step (karman_large.hip): the marker density pushes the velocity, as PhiFlow's
// IncompressibleFlow.step does with buoyancy_factor != 0.  F = (F_y, F_x) is a force per unit density (PhiFlow: -gravity * buoyancy_factor,
// Gravity() = -9.81 along y  ->  F = (9.81 beta, 0)); f = dt F travels as two floats.  With dz = the step's OUTPUT density (the inflow
// already in it) inside the grid and 0 outside -- the zero ghost ring of the density's advection --
//   a_y[jf,i] = mask_y[jf,i] * ( SL_y(c)[jf,i] + f_y * (dz(jf-1,i) + dz(jf,i)) / 2 )      jf = 0..Y
//   a_x[j,if] = mask_x[j,if] * ( SL_x(c)[j,if] + f_x * (dz(j,if-1) + dz(j,if)) / 2 )      if = 0..X
// between the advection (k_l_advect) and the divergence (k_l_div) of sol_large_front: one hook for the direct, the scattered-direct and
// the CG form of the step.  Two linear kernels, exact transposes of each other:
//   k_l_buoyancy        face parallel, both components in one launch: v = fl(v + fl(f * fl(0.5f * (d0 + d1)))) * mask, contraction off.
//                       k_l_advect has applied the mask already and it is 0 or 1, so masking the sum equals masking both terms.
//   k_lb_buoyancy_adj   cell parallel gather, no atomics, fixed order:
//                       g_dsum[j,i] = g_d_out[j,i] + f_y (m g_y[j,i] + m g_y[j+1,i]) / 2 + f_x (m g_x[j,i] + m g_x[j,i+1]) / 2
//                       with g = the cotangent of a (inside the step's adjoint: g_a of k_lb_ga, which carries the mask already -- applying
//                       it twice changes nothing).  g_dsum then goes through the density adjoint (sol_karman_density_bwd, accumulate = 1).
//                       gmax (the absmax slots k_lb_ga published, or NULL): a non-finite g_a of a simulation makes ALL of its g_dsum NaN,
//                       so the poisoning rule of fixed_scatter.hpp holds for the density gradient too.
// A component whose force is zero is not touched (f = (0, 0): the forward kernel is not launched at all).
#include "fixed_scatter.hpp"
#include "large2d.hpp"

namespace {

struct BuoyArgs {
    int Y, X;
    float fy, fx;                       // dt F
    const float *active, *d;            // [Y,X], [B,Y,X]
    float *vy, *vx;                     // [B,Y+1,X], [B,Y,X+1], updated in place
};

__global__ void __launch_bounds__(256) k_l_buoyancy(BuoyArgs a) {
#pragma clang fp contract(off)
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const float* d = a.d + (size_t)b * N;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nVy + nVx; k += gridDim.x * blockDim.x) {
        if (k < nVy) {
            if (a.fy == 0.f) continue;
            const int j = k / X, i = k - j * X;
            const float d0 = j >= 1 ? d[(j - 1) * X + i] : 0.f, d1 = j < Y ? d[j * X + i] : 0.f;
            float* v = a.vy + (size_t)b * nVy + k;
            const float t = a.fy * (0.5f * (d0 + d1));
            *v = (*v + t) * mask_y(a.active, Y, X, j, i);
        } else {
            if (a.fx == 0.f) continue;
            const int q = k - nVy, j = q / XP, i = q - j * XP;
            const float d0 = i >= 1 ? d[j * X + i - 1] : 0.f, d1 = i < X ? d[j * X + i] : 0.f;
            float* v = a.vx + (size_t)b * nVx + q;
            const float t = a.fx * (0.5f * (d0 + d1));
            *v = (*v + t) * mask_x(a.active, Y, X, j, i);
        }
    }
}

struct BuoyAdjArgs {
    int Y, X;
    float fy, fx;
    const float *active, *gy, *gx;      // cotangent of the faces [B,Y+1,X], [B,Y,X+1]
    const unsigned* gmax;               // [B][FX_SLOTS] or NULL
    const float* gdo;                   // [B,Y,X] or NULL (= zero)
    float* gds;                         // [B,Y,X]
};

__global__ void __launch_bounds__(256) k_lb_buoyancy_adj(BuoyAdjArgs a) {
#pragma clang fp contract(off)
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    bool poisoned = false;
    if (a.gmax) {
        float qs, qi;
        fx_scale(a.gmax + b * FX_SLOTS, qs, qi);
        poisoned = qi != qi;
    }
    const float* gy = a.gy + (size_t)b * nVy;
    const float* gx = a.gx + (size_t)b * nVx;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < N; c += gridDim.x * blockDim.x) {
        const int j = c / X, i = c - j * X;
        float g = a.gdo ? a.gdo[(size_t)b * N + c] : 0.f;
        if (a.fy != 0.f)
            g += a.fy * (0.5f * (mask_y(a.active, Y, X, j, i) * gy[j * X + i] + mask_y(a.active, Y, X, j + 1, i) * gy[(j + 1) * X + i]));
        if (a.fx != 0.f)
            g += a.fx * (0.5f * (mask_x(a.active, Y, X, j, i) * gx[j * XP + i] + mask_x(a.active, Y, X, j, i + 1) * gx[j * XP + i + 1]));
        a.gds[(size_t)b * N + c] = poisoned ? __uint_as_float(0x7fc00000u) : g;
    }
}

int shape_check(const char* who, int B, int Y, int X) {
    SOL_REQUIRE(B >= 1 && B <= 65535 && Y >= 1 && X >= 1, "%s: B in [1, 65535], Y, X >= 1 (got %d, %d, %d)", who, B, Y, X);
    SOL_REQUIRE((size_t)Y * X < ((size_t)1 << 28), "%s: grid too large for 32-bit face indices", who);
    return SOL_OK;
}

}  // namespace

int sol_buoyancy_add(hipStream_t s, int B, int Y, int X, const float* active, const float* d, float fy, float fx, float* vy, float* vx) {
    if (fy == 0.f && fx == 0.f) return SOL_OK;
    const int faces = (Y + 1) * X + Y * (X + 1);
    const BuoyArgs a{Y, X, fy, fx, active, d, vy, vx};
    SOL_LAUNCH(k_l_buoyancy, dim3((faces + 255) / 256, B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

int sol_buoyancy_adj(hipStream_t s, int B, int Y, int X, const float* active, const float* gy, const float* gx, const unsigned* gmax,
                     float fy, float fx, const float* g_d_out, float* g_dsum) {
    const BuoyAdjArgs a{Y, X, fy, fx, active, gy, gx, gmax, g_d_out, g_dsum};
    SOL_LAUNCH(k_lb_buoyancy_adj, dim3((Y * X + 255) / 256, B), dim3(256), 0, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

extern "C" int sol_karman_buoyancy_add(void* stream, int32_t B, int32_t Y, int32_t X, const float* active, const float* d,
                                       float fy_dt, float fx_dt, float* vy, float* vx) {
    const char* who = "sol_karman_buoyancy_add";
    if (int e = shape_check(who, B, Y, X)) return e;
    SOL_REQUIRE(active && d && vy && vx, "%s: NULL pointer argument", who);
    SOL_REQUIRE(vy != vx && d != vy && d != vx && active != vy && active != vx, "%s: outputs must not alias the inputs", who);
    return sol_buoyancy_add((hipStream_t)stream, B, Y, X, active, d, fy_dt, fx_dt, vy, vx);
}

extern "C" int sol_karman_buoyancy_add_bwd(void* stream, int32_t B, int32_t Y, int32_t X, const float* active,
                                           const float* g_vy, const float* g_vx, float fy_dt, float fx_dt,
                                           const float* g_d_out, float* g_dsum) {
    const char* who = "sol_karman_buoyancy_add_bwd";
    if (int e = shape_check(who, B, Y, X)) return e;
    SOL_REQUIRE(active && g_vy && g_vx && g_dsum, "%s: NULL pointer argument", who);
    SOL_REQUIRE(g_dsum != g_vy && g_dsum != g_vx && g_dsum != active && g_dsum != g_d_out, "%s: outputs must not alias the inputs", who);
    return sol_buoyancy_adj((hipStream_t)stream, B, Y, X, active, g_vy, g_vx, nullptr, fy_dt, fx_dt, g_d_out, g_dsum);
}
