// Gradient of the karman-3d step with respect to the Reynolds number: the 3-D twin of karman_re_bwd.hip on re_reduce.hpp.  The forward
// step computes u = v_in + alpha L v_in with alpha = dt res^2 / re[b] (k3_diffuse: the replicate-padded 7-point Laplacian) and then
// c_y = (1 - bcm) u_y + bc, c_x = u_x, c_z = u_z; with g' = the cotangent of u -- the field the diffusion adjoints apply (I + alpha L^T) to --
//     g_re[b] = -(dt res^2 / re[b]^2) * sum over the faces of the three components of  g'_e (L v_in)_e
// re_reduce.hpp states the order and the precision of the sum.  Two launches, chip wide on global memory, issued by the adjoint that owns
// g' after its own launches (sol_karman3d_step_bwd_re, sol_karman3d_density_bwd_re):
//   k3_re_partial<SRC> grid (re_nblk(faces), B): every thread walks a fixed strided share of simulation b's faces, forms g' as the
//                      diffusion adjoint of its path does -- RE3_FIXED: k3b_diffuse_adj's fx_get(g_c) (. (1 - bcm) on v_y); RE3_GU:
//                      k3d_diffuse_adj's k3d_face_y / _x / _z -- gathers (L v_in)_e from the step's INPUT velocity and adds the fp64
//                      product; one double per workgroup goes to partial[b][blk].  A poisoned simulation (a non-finite cotangent:
//                      fixed_scatter.hpp) stores NaN.
//   k3_re_final        grid (B): the partial sums (staged in LDS) in index order, times -adt / re^2, written to g_re[b] or added onto it
#include "karman3d_re.hpp"

namespace {

struct Re3Args {
    int Y, X, Z, nblk;
    float adt;
    int accumulate;
    Re3In in;
};

template <int SRC>
__global__ void __launch_bounds__(RE_THREADS) k3_re_partial(Re3Args a) {
    const int Y = a.Y, X = a.X, Z = a.Z, XP = X + 1, ZP = Z + 1, N = Y * X * Z;
    const int nVy = (Y + 1) * X * Z, nVx = Y * XP * Z, nVz = Y * X * ZP;
    const int b = blockIdx.y;
    const Re3In& in = a.in;
    const float* vy = in.vy_in + (size_t)b * nVy;
    const float* vx = in.vx_in + (size_t)b * nVx;
    const float* vz = in.vz_in + (size_t)b * nVz;
    const float* m = in.bcm + (size_t)b * in.bc_stride;
    const long long* gcy = SRC == RE3_FIXED ? in.gcy + (size_t)b * nVy : nullptr;
    const long long* gcx = SRC == RE3_FIXED ? in.gcx + (size_t)b * nVx : nullptr;
    const long long* gcz = SRC == RE3_FIXED ? in.gcz + (size_t)b * nVz : nullptr;
    const float* uy = SRC == RE3_GU ? in.gUy + (size_t)b * N : nullptr;
    const float* ux = SRC == RE3_GU ? in.gUx + (size_t)b * N : nullptr;
    const float* uz = SRC == RE3_GU ? in.gUz + (size_t)b * N : nullptr;
    float qs, qi;
    fx_scale(in.gmax + b * FX_SLOTS, qs, qi);
    double acc = 0.0;
    for (int e = blockIdx.x * RE_THREADS + threadIdx.x; e < nVy + nVx + nVz; e += a.nblk * RE_THREADS) {
        float g, lap;
        if (e < nVy) {
            const int k = e % Z, i = (e / Z) % X, j = e / (Z * X);
            g = SRC == RE3_FIXED ? fx_get(gcy, e, qi) * (1.f - m[e]) : k3d_face_y(uy, m, Y, X, Z, j, i, k);
            lap = re_lap<3>(vy, e, {j, i, k}, {Y + 1, X, Z});
        } else if (e < nVy + nVx) {
            const int q = e - nVy, k = q % Z, i = (q / Z) % XP, j = q / (Z * XP);
            g = SRC == RE3_FIXED ? fx_get(gcx, q, qi) : k3d_face_x(ux, X, Z, j, i, k);
            lap = re_lap<3>(vx, q, {j, i, k}, {Y, XP, Z});
        } else {
            const int q = e - nVy - nVx, k = q % ZP, i = (q / ZP) % X, j = q / (ZP * X);
            g = SRC == RE3_FIXED ? fx_get(gcz, q, qi) : k3d_face_z(uz, X, Z, j, i, k);
            lap = re_lap<3>(vz, q, {j, i, k}, {Y, X, ZP});
        }
        acc += (double)g * (double)lap;
    }
    const double s = re_block_sum(acc);
    // RE3_FIXED is poisoned through qi = NaN already; RE3_GU as k3d_diffuse_adj does it: every gradient of the simulation is NaN
    if (threadIdx.x == 0) in.partial[(size_t)b * a.nblk + blockIdx.x] = qi != qi ? (double)qi : s;
}

// the wave fetches the partial sums side by side into LDS (256 dependent-latency global loads of one thread cost 12 us), then thread 0 adds
// them in index order as re_final states it: the same bits
__global__ void __launch_bounds__(64) k3_re_final(Re3Args a) {
    __shared__ double part[RE_MAX_BLOCKS];
    const int b = blockIdx.x;
    const double* p = a.in.partial + (size_t)b * a.nblk;
    for (int k = threadIdx.x; k < a.nblk; k += 64) part[k] = p[k];
    __syncthreads();
    if (threadIdx.x == 0) re_final(part, a.nblk, a.adt, a.in.re[b], a.in.g_re + b, a.accumulate);
}

size_t faces_of(const sol_karman3d_cfg* c) {
    const size_t Y = c->Y, X = c->X, Z = c->Z;
    return (Y + 1) * X * Z + Y * (X + 1) * Z + Y * X * (Z + 1);
}

}  // namespace

double* sol_re3_partial_behind(const Carve& plain, const sol_karman3d_cfg* c, size_t* bytes) {
    Carve w(plain.end(), 8, 8);
    double* partial = w.take<double>((size_t)c->B * re_nblk(faces_of(c)));
    *bytes = plain.bytes() + align_up(w.bytes(), 256);
    return partial;
}

int sol_re3_reduce(hipStream_t s, const sol_karman3d_cfg* c, const Re3In& in) {
    Re3Args a{};
    a.Y = c->Y; a.X = c->X; a.Z = c->Z; a.nblk = re_nblk(faces_of(c));
    a.adt = c->dt * c->res * c->res;
    a.accumulate = in.accumulate != 0;
    a.in = in;
    if (in.src == RE3_FIXED) SOL_LAUNCH(k3_re_partial<RE3_FIXED>, dim3(a.nblk, c->B), dim3(RE_THREADS), 0, s, a);
    else SOL_LAUNCH(k3_re_partial<RE3_GU>, dim3(a.nblk, c->B), dim3(RE_THREADS), 0, s, a);
    SOL_LAUNCH(k3_re_final, dim3(c->B), dim3(64), 0, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}
