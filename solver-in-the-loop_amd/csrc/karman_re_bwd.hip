// Gradient of the karman-2d step with respect to the Reynolds number.  The forward step computes u = v_in + alpha L v_in with
// alpha = dt res^2 / re[b] (k_l_diffuse, karman_step.hip's dif_y / dif_x) and then c_y = (1 - bcm) u_y + bc, c_x = u_x; with g' = the
// cotangent of u -- the field the diffusion adjoints apply (I + alpha L^T) to --
//     g_re[b] = -(dt res^2 / re[b]^2) * sum over the faces of both components of  g'_e (L v_in)_e
// re_reduce.hpp states the order and the precision of the sum.  Two launches, chip wide on global memory, issued by the adjoint that owns
// g' right after its own launches (sol_karman_step_bwd_large_re, sol_karman_density_bwd_re):
//   k_re_partial<SRC>  grid (re_nblk(faces), B): every thread walks a fixed strided share of simulation b's (Y+1) X + Y (X+1) faces,
//                      forms g' as the diffusion adjoint of its path does -- RE_FIXED: k_lb_diffuse_adj's fx_get(g_c) (. (1 - bcm) on
//                      v_y); RE_GU: k_kd_diffuse_adj's kd_face_y / kd_face_x -- gathers (L v_in)_e from the step's INPUT velocity and
//                      adds the fp64 product; one double per workgroup goes to partial[b][blk].  A poisoned simulation (a non-finite
//                      cotangent: fixed_scatter.hpp) stores NaN.
//   k_re_final         grid (B): the partial sums in index order, times -adt / re^2, written to g_re[b] or added onto it
#include "karman_re.hpp"

namespace {

struct ReArgs {
    int Y, X, nblk;
    float adt;
    int accumulate;
    ReIn in;
};

template <int SRC>
__global__ void __launch_bounds__(RE_THREADS) k_re_partial(ReArgs a) {
    const int Y = a.Y, X = a.X, XP = X + 1, N = Y * X, nVy = (Y + 1) * X, nVx = Y * XP;
    const int b = blockIdx.y;
    const ReIn& in = a.in;
    const float* vy = in.vy_in + (size_t)b * nVy;
    const float* vx = in.vx_in + (size_t)b * nVx;
    const float* m = in.bcm + (size_t)b * in.bc_stride;
    const long long* gcy = SRC == RE_FIXED ? in.gcy + (size_t)b * nVy : nullptr;
    const long long* gcx = SRC == RE_FIXED ? in.gcx + (size_t)b * nVx : nullptr;
    const float* uy = SRC == RE_GU ? in.gUy + (size_t)b * N : nullptr;
    const float* ux = SRC == RE_GU ? in.gUx + (size_t)b * N : nullptr;
    float qs, qi;
    fx_scale(in.gmax + b * FX_SLOTS, qs, qi);
    double acc = 0.0;
    for (int e = blockIdx.x * RE_THREADS + threadIdx.x; e < nVy + nVx; e += a.nblk * RE_THREADS) {
        float g, lap;
        if (e < nVy) {
            const int j = e / X, i = e - j * X;
            g = SRC == RE_FIXED ? fx_get(gcy, e, qi) * (1.f - m[e]) : kd_face_y(uy, m, Y, X, j, i);
            lap = re_lap<2>(vy, e, {j, i}, {Y + 1, X});
        } else {
            const int q = e - nVy, j = q / XP, i = q - j * XP;
            g = SRC == RE_FIXED ? fx_get(gcx, q, qi) : kd_face_x(ux, X, j, i);
            lap = re_lap<2>(vx, q, {j, i}, {Y, XP});
        }
        acc += (double)g * (double)lap;
    }
    const double s = re_block_sum(acc);
    // RE_FIXED is poisoned through qi = NaN already; RE_GU as k_kd_diffuse_adj does it: every gradient of the simulation is NaN
    if (threadIdx.x == 0) in.partial[(size_t)b * a.nblk + blockIdx.x] = qi != qi ? (double)qi : s;
}

__global__ void __launch_bounds__(64) k_re_final(ReArgs a) {
    const int b = blockIdx.x;
    if (threadIdx.x == 0) re_final(a.in.partial + (size_t)b * a.nblk, a.nblk, a.adt, a.in.re[b], a.in.g_re + b, a.accumulate);
}

size_t faces_of(const sol_karman_cfg* c) { return (size_t)(c->Y + 1) * c->X + (size_t)c->Y * (c->X + 1); }

}  // namespace

double* sol_re_partial_take(Carve& w, const sol_karman_cfg* c) { return w.take<double>((size_t)c->B * re_nblk(faces_of(c))); }

int sol_re_reduce(hipStream_t s, const sol_karman_cfg* c, const ReIn& in) {
    ReArgs a{};
    a.Y = c->Y; a.X = c->X; a.nblk = re_nblk(faces_of(c));
    a.adt = c->dt * c->res * c->res;
    a.accumulate = in.accumulate != 0;
    a.in = in;
    if (in.src == RE_FIXED) SOL_LAUNCH(k_re_partial<RE_FIXED>, dim3(a.nblk, c->B), dim3(RE_THREADS), 0, s, a);
    else SOL_LAUNCH(k_re_partial<RE_GU>, dim3(a.nblk, c->B), dim3(RE_THREADS), 0, s, a);
    SOL_LAUNCH(k_re_final, dim3(c->B), dim3(64), 0, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}
