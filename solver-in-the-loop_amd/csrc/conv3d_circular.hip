// Circular z padding of the 3-D correction network (include/sol_hip.h, "CIRCULAR PADDING, KARMAN-3D").
//
// The network's buffers are [B, Y, X, Z, C] with z as the pixel axis of a row, and a row has no legal width Z + 4.  On a periodic span the
// network therefore runs on the TRANSPOSED volume [B, Y, HB, X, C]: the depth is y, the image rows are z, the pixels are x.  Rows
// [2, 2 + Z) hold the Z planes, rows 0, 1 and Z + 2, Z + 3 are the circular halo, rows [Z + 4, HB) pad HB up to what check_shape of
// csrc/conv5x5.hip asks of a row count.  The convolution kernels run on that buffer as they are (zero padding beyond it, kernel axes 1 and
// 2 swapped by the caller); what they write into halo and pad rows is replaced by k_conv3d_halo before the next consumer reads it.
//
//   k_conv3d_circ_pack    [B,Y,X,Z,4]  -> [B,Y,HB,X,4]   transpose of every (X, Z) plane through a 32 x 32 float4 LDS tile (pitch 33 float4
//                                                        = 132 dwords: lane l of the transposed ds_read_b128 sits on banks 4 l mod 64, so each
//                                                        16-lane group covers the 64 banks once), halo rows by wrap or zero, pad rows zero
//   k_conv3d_circ_unpack  [B,Y,HB,X,C] -> [B,Y,X,Z,C]    the inverse on rows [2, 2 + Z); C = 4 as float4, C = 3 as dwords through a tile
//                                                        whose pitch is 3 mod 64 (lane = 3 z + c reads bank 3 z + c + const)
//   k_conv3d_halo         [planes,HB,X,C] in place       halo rows = wrapped valid rows or zero, pad rows zero
//
// Global reads and writes of all three are contiguous along the fastest axis of their side.  No atomics, no host synchronisation.
#include "common.hpp"

namespace {

constexpr int T = 32;      // tile edge

// one workgroup: rows [r0, r0 + 32) x pixels [x0, x0 + 32) of one plane of dst
template <bool ZERO> __global__ void __launch_bounds__(256) k_conv3d_circ_pack(const float4* __restrict__ src, float4* __restrict__ dst, int X, int Z, int HB,
                                                                              int tx, int tr) {
    __shared__ float4 tile[T][T + 1];
    const int bid = blockIdx.x, x0 = (bid % tx) * T, r0 = (bid / tx % tr) * T;
    const size_t plane = (size_t)(bid / (tx * tr));
    const float4* const s = src + plane * X * Z;
    float4* const d = dst + plane * HB * X;
    const int j = threadIdx.x & 31, i0 = threadIdx.x >> 5;
    {   // load: j runs along z (contiguous in src), i along x
        const int r = r0 + j;
        const bool valid = r >= 2 && r < Z + 2, halo = !valid && r < Z + 4;
        const bool live = valid || (halo && !ZERO);
        int z = (r - 2) % Z;
        if (z < 0) z += Z;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + 8 * k, x = x0 + i;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live && x < X) v = s[(size_t)x * Z + z];
            tile[i][j] = v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // store: j runs along x (contiguous in dst), i along the rows
        const int i = i0 + 8 * k, r = r0 + i, x = x0 + j;
        if (r < HB && x < X) d[(size_t)r * X + x] = tile[j][i];
    }
}

// one workgroup: planes z in [z0, z0 + 32) x pixels [x0, x0 + 32) of one (b, y)
__global__ void __launch_bounds__(256) k_conv3d_circ_unpack4(const float4* __restrict__ src, float4* __restrict__ dst, int X, int Z, int HB, int tx, int tz) {
    __shared__ float4 tile[T][T + 1];
    const int bid = blockIdx.x, x0 = (bid % tx) * T, z0 = (bid / tx % tz) * T;
    const size_t plane = (size_t)(bid / (tx * tz));
    const float4* const s = src + plane * HB * X;
    float4* const d = dst + plane * X * Z;
    const int j = threadIdx.x & 31, i0 = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // load: j along x, i along z
        const int i = i0 + 8 * k, z = z0 + i, x = x0 + j;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (z < Z && x < X) v = s[(size_t)(z + 2) * X + x];
        tile[i][j] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // store: j along z, i along x
        const int i = i0 + 8 * k, x = x0 + i, z = z0 + j;
        if (x < X && z < Z) d[(size_t)x * Z + z] = tile[j][i];
    }
}

// C = 3: the same tile in dwords, 32 z x (32 x 3) floats; the pitch 131 = 3 mod 64
__global__ void __launch_bounds__(256) k_conv3d_circ_unpack3(const float* __restrict__ src, float* __restrict__ dst, int X, int Z, int HB, int tx, int tz) {
    constexpr int C = 3, RW = T * C, PITCH = RW + 35;
    __shared__ float tile[T * PITCH];
    const int bid = blockIdx.x, x0 = (bid % tx) * T, z0 = (bid / tx % tz) * T;
    const size_t plane = (size_t)(bid / (tx * tz));
    const float* const s = src + plane * HB * X * C;
    float* const d = dst + plane * X * Z * C;
    const int nx = min(T, X - x0) * C, nz = min(T, Z - z0) * C;       // live floats of a tile row on either side
    for (int e = threadIdx.x; e < T * RW; e += 256) {   // load: a row of src holds (x, c) contiguously
        const int zi = e / RW, q = e - zi * RW;
        if (z0 + zi < Z && q < nx) tile[zi * PITCH + q] = s[((size_t)(z0 + zi + 2) * X + x0) * C + q];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < T * RW; e += 256) {   // store: a row of dst holds (z, c) contiguously
        const int xi = e / RW, q = e - xi * RW, zi = q / C, c = q - zi * C;
        if (x0 + xi < X && q < nz) d[((size_t)(x0 + xi) * Z + z0) * C + q] = tile[zi * PITCH + xi * C + c];
    }
}

// one thread per float4 of a halo or pad row; sources are valid rows, destinations are not: in place without a race
template <bool ZERO> __global__ void __launch_bounds__(256) k_conv3d_halo(float* __restrict__ buf, int planes, int Z, int HB, int RW4) {
    const int nr = HB - Z;                                   // rows 0, 1, Z + 2, Z + 3 and the pad rows [Z + 4, HB)
    const size_t per = (size_t)nr * RW4, n = (size_t)planes * per;
    float4* const b4 = reinterpret_cast<float4*>(buf);
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const size_t p = e / per, t = e - p * per;
        const int k = (int)(t / RW4), q = (int)(t - (size_t)k * RW4);
        const int r = k < 2 ? k : Z + k;                     // 0, 1, Z + 2, Z + 3, Z + 4, ...
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!ZERO && k < 4) {
            int z = (r - 2) % Z;
            if (z < 0) z += Z;
            v = b4[(p * HB + z + 2) * RW4 + q];
        }
        b4[(p * HB + r) * RW4 + q] = v;
    }
}

int circ_shape(const char* who, int64_t planes, int X, int Z, int HB) {
    SOL_REQUIRE(planes >= 1 && X >= 1, "%s: B, Y (planes), X >= 1 (got %lld planes, X = %d)", who, (long long)planes, X);
    SOL_REQUIRE(Z >= 2, "%s: Z >= 2 (got %d)", who, Z);
    SOL_REQUIRE(HB >= Z + 4, "%s: HB = %d is below Z + 4 = %d (two halo rows on either side of the Z planes)", who, HB, Z + 4);
    SOL_REQUIRE(planes * (int64_t)HB * X < ((int64_t)1 << 31), "%s: %lld planes of %d x %d pixels do not fit a 32-bit pixel index", who,
                (long long)planes, HB, X);
    return SOL_OK;
}

}  // namespace

extern "C" int sol_conv3d_circ_pack(void* stream, const float* src, float* dst, int32_t B, int32_t Y, int32_t X, int32_t Z, int32_t HB, int32_t C, int32_t mode) {
    SOL_REQUIRE(src && dst, "sol_conv3d_circ_pack: NULL buffer");
    SOL_REQUIRE(B >= 1 && Y >= 1, "sol_conv3d_circ_pack: B, Y >= 1 (got %d, %d)", B, Y);
    if (int rc = circ_shape("sol_conv3d_circ_pack", (int64_t)B * Y, X, Z, HB)) return rc;
    SOL_REQUIRE(C == 4, "sol_conv3d_circ_pack: C must be 4 (got %d)", C);
    SOL_REQUIRE(mode == 0 || mode == 1, "sol_conv3d_circ_pack: mode must be 0 (wrap) or 1 (zero), got %d", mode);
    const int tx = (X + T - 1) / T, tr = (HB + T - 1) / T;
    const dim3 grid((unsigned)((int64_t)B * Y * tx * tr));
    hipStream_t s = (hipStream_t)stream;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    if (mode == 1) SOL_LAUNCH_NAMED("k_conv3d_circ_pack<zero>", (k_conv3d_circ_pack<true>), grid, dim3(256), 0, s, s4, d4, X, Z, HB, tx, tr);
    else SOL_LAUNCH_NAMED("k_conv3d_circ_pack<wrap>", (k_conv3d_circ_pack<false>), grid, dim3(256), 0, s, s4, d4, X, Z, HB, tx, tr);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

extern "C" int sol_conv3d_circ_unpack(void* stream, const float* src, float* dst, int32_t B, int32_t Y, int32_t X, int32_t Z, int32_t HB, int32_t C) {
    SOL_REQUIRE(src && dst, "sol_conv3d_circ_unpack: NULL buffer");
    SOL_REQUIRE(B >= 1 && Y >= 1, "sol_conv3d_circ_unpack: B, Y >= 1 (got %d, %d)", B, Y);
    if (int rc = circ_shape("sol_conv3d_circ_unpack", (int64_t)B * Y, X, Z, HB)) return rc;
    SOL_REQUIRE(C == 3 || C == 4, "sol_conv3d_circ_unpack: C must be 3 or 4 (got %d)", C);
    const int tx = (X + T - 1) / T, tz = (Z + T - 1) / T;
    const dim3 grid((unsigned)((int64_t)B * Y * tx * tz));
    hipStream_t s = (hipStream_t)stream;
    if (C == 4)
        SOL_LAUNCH_NAMED("k_conv3d_circ_unpack4", k_conv3d_circ_unpack4, grid, dim3(256), 0, s, reinterpret_cast<const float4*>(src), reinterpret_cast<float4*>(dst),
                         X, Z, HB, tx, tz);
    else SOL_LAUNCH_NAMED("k_conv3d_circ_unpack3", k_conv3d_circ_unpack3, grid, dim3(256), 0, s, src, dst, X, Z, HB, tx, tz);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}

extern "C" int sol_conv3d_halo(void* stream, float* buf, int32_t planes, int32_t Z, int32_t HB, int32_t X, int32_t C, int32_t mode) {
    SOL_REQUIRE(buf, "sol_conv3d_halo: NULL buffer");
    if (int rc = circ_shape("sol_conv3d_halo", planes, X, Z, HB)) return rc;
    SOL_REQUIRE(C == 4 || C == 32, "sol_conv3d_halo: C must be 4 or 32 (got %d)", C);
    SOL_REQUIRE(mode == 0 || mode == 1, "sol_conv3d_halo: mode must be 0 (wrap) or 1 (zero), got %d", mode);
    const int RW4 = X * (C / 4);
    const size_t n = (size_t)planes * (HB - Z) * RW4, nb = (n + 255) / 256;
    const dim3 grid((unsigned)(nb < 2048 ? nb : 2048));
    hipStream_t s = (hipStream_t)stream;
    if (mode == 1) SOL_LAUNCH_NAMED("k_conv3d_halo<zero>", (k_conv3d_halo<true>), grid, dim3(256), 0, s, buf, planes, Z, HB, RW4);
    else SOL_LAUNCH_NAMED("k_conv3d_halo<wrap>", (k_conv3d_halo<false>), grid, dim3(256), 0, s, buf, planes, Z, HB, RW4);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}
