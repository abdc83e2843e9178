// Halo refresh of the correction network's buffers on a periodic scene (include/sol_hip.h, "CIRCULAR PADDING").
//
// A periodic axis gives an activation a two-pixel halo on either side: buf is [B, H + 4 py, P, C] with the valid pixels at rows
// [2 py, 2 py + H) and columns [2 px, 2 px + W); columns >= W + 4 px are the zero pad of the pitched layout (sol_conv5x5_cols).  The
// 5x5 convolutions run on that buffer as they are (zero padding beyond its edge); what they write into the halo is wrong and is
// replaced here: mode 0 by the valid cell at the index modulo H / W (the circular padding), mode 1 by zero (the dz of a weight gradient:
// only valid pixels may contribute).  One thread per float4 of a halo cell; the sources are valid cells and the destinations halo cells,
// so the copy is in place without a race.  Valid cells and pad columns are never written.
#include "common.hpp"

namespace {

template <bool ZERO> __global__ void __launch_bounds__(256) k_conv_halo(float* __restrict__ buf, int B, int H, int W, int P, int C4, int py, int px) {
    const int WV = W + 4 * px, HB = H + 4 * py;
    const size_t nrow = py ? (size_t)4 * WV : 0;          // the four halo rows, halo columns (the corners) included
    const size_t per = nrow + (px ? (size_t)4 * H : 0);   // + the four halo columns of every valid row
    const size_t n = (size_t)B * per * C4;
    float4* const b4 = reinterpret_cast<float4*>(buf);
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const int c = (int)(e % C4);
        const size_t cell = e / C4, b = cell / per, t = cell - b * per;
        int r, q;                                           // the halo cell: buffer row, buffer column
        if (t < nrow) {
            const int k = (int)(t / WV);
            r = k < 2 ? k : H + k;                          // 0, 1, H + 2, H + 3
            q = (int)(t - (size_t)k * WV);
        } else {
            const size_t u = t - nrow;
            const int k = (int)(u & 3);
            r = (int)(u >> 2) + 2 * py;
            q = k < 2 ? k : W + k;                          // 0, 1, W + 2, W + 3
        }
        const size_t dst = ((b * HB + r) * P + q) * C4 + c;
        if (ZERO) {
            b4[dst] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            int sr = r, sq = q;
            if (py) { sr = (r - 2) % H; if (sr < 0) sr += H; sr += 2; }
            if (px) { sq = (q - 2) % W; if (sq < 0) sq += W; sq += 2; }
            b4[dst] = b4[((b * HB + sr) * P + sq) * C4 + c];
        }
    }
}

}  // namespace

extern "C" int sol_conv_halo(void* stream, float* buf, int32_t B, int32_t H, int32_t W, int32_t P, int32_t C, int32_t periodic_bits, int32_t mode) {
    SOL_REQUIRE(buf, "sol_conv_halo: NULL buffer");
    SOL_REQUIRE(B >= 1 && H >= 1 && W >= 1, "sol_conv_halo: B, H, W >= 1 (got %d, %d, %d)", B, H, W);
    SOL_REQUIRE((periodic_bits & ~(SOL_DIRECT_HDR_PERIODIC_Y | SOL_DIRECT_HDR_PERIODIC_X)) == 0, "sol_conv_halo: periodic_bits must be a combination of 2 "
                "(y periodic) and 4 (x periodic), got %d", periodic_bits);
    SOL_REQUIRE(mode == 0 || mode == 1, "sol_conv_halo: mode must be 0 (wrap) or 1 (zero), got %d", mode);
    SOL_REQUIRE(C >= 4 && C <= 32 && C % 4 == 0, "sol_conv_halo: C must be a multiple of 4 up to 32 (got %d)", C);
    const int py = (periodic_bits & SOL_DIRECT_HDR_PERIODIC_Y) ? 1 : 0, px = (periodic_bits & SOL_DIRECT_HDR_PERIODIC_X) ? 1 : 0;
    SOL_REQUIRE(P % 64 == 0 && P >= 64, "sol_conv_halo: the pitch P must be a multiple of 64 (got %d)", P);
    SOL_REQUIRE((int64_t)P >= (int64_t)W + 4 * px, "sol_conv_halo: the pitch P = %d is below W + 4 px = %lld", P, (long long)W + 4 * px);
    if (periodic_bits == 0) return SOL_OK;          // no periodic axis, no halo: nothing is launched
    const size_t n = (size_t)B * ((py ? (size_t)4 * (W + 4 * px) : 0) + (px ? (size_t)4 * H : 0)) * (C / 4), nb = (n + 255) / 256;
    const dim3 grid((unsigned)(nb < 2048 ? nb : 2048));
    hipStream_t s = (hipStream_t)stream;
    if (mode == 1) SOL_LAUNCH_NAMED("k_conv_halo<zero>", (k_conv_halo<true>), grid, dim3(256), 0, s, buf, B, H, W, P, C / 4, py, px);
    else SOL_LAUNCH_NAMED("k_conv_halo<wrap>", (k_conv_halo<false>), grid, dim3(256), 0, s, buf, B, H, W, P, C / 4, py, px);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}
