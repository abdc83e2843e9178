// karman-2d: the direct pressure solve of the multi-launch path as ONE launch, one workgroup per simulation, for the grids one workgroup
// holds (Y, X >= 16, at most 8192 cells, X <= 64) -- what sol_large_direct_solve (karman_large.hip) does for a one-window blob ("FD02",
// precond.direct_solver_blob) with eight k_l_gemm, two k_l_scale and one k_l_capacitance launch:
//   1. T2 = (Qy rhs Qx) / lam          2. X0 = Qy[win,:] T2 Qx[:,win]          3. W2 = 0, W2[sidx] = -K' X0[sidx]
//   4. T2 += (Qy[:,win] W2 Qx[win,:]) / lam                                    5. p = Qy T2 Qx
// Runs inside sol_large_direct_solve for a scene built with multi_launch (flag in the host header copy) under the option k2d_solve_one_wg.
//
// Arithmetic: exact fp32, fmaf chains in k order (what the fp32 MFMA computes too, at the same peak rate on gfx950); no split products.
// Every product is one shape: C[m][n] = sum_k Lt[k][m] R[k][n] on 4 x 4 register tiles, both operands read as 16-byte pieces along their
// contiguous index.  Qy and Qx are symmetric (precond.dst_matrix), so a Q factor on the left is its own k-major image; an intermediate
// that the NEXT product takes on the left is stored transposed by the product that makes it.
//
// LDS plan (floats; YP, XP = Y, X rounded up to 4, S = XP * YP <= 8448):
//   A [S]   P1: (Qy rhs)^T [X][YP]    P3: U [Y][win], then V^T [win][YP]    P5: T2 Qx [Y][XP]
//   Bf[S]   rhs [Y][XP], then the spectral coefficients T2^T [X][YP] (the layout of the blob's 1 / lam)
//   W [win * win]  X0, then W2          xs [SP]  the gathered support values          part [512]  partial sums of K' xs
// at most 2 * 33792 + 16384 + 16384 + 2048 = 102400 bytes of the 160 KB.  The Q matrices, 1 / lam and K' are read from the blob: shared by
// all simulations, L2 resident.  The caller's workspace is used for rhs in / p out only (T0 of the chain's layout); nothing else of it is
// touched, so no size function moves.  Synchronisation: __syncthreads() only; no workgroup waits for another.
#include "common.hpp"

namespace {

constexpr int OW_T = 512;             // threads per workgroup
constexpr int OW_HEADER = 16;         // words of the blob's header
constexpr int OW_MAXSP = 4096;

struct OwArgs {
    const float *Qy, *Qx, *ilT, *KpT, *QxW;
    const int* sidx;
    float* T0;                        // [B][Y][X]: rhs in, p out
    int Y, X, YP, XP, win, wy0, wx0, nS, SP;
};

// p[i .. i + 3] from global memory; AL: 16-byte aligned and in range by construction, else element by element, zero beyond n
template <bool AL>
__device__ __forceinline__ float4 ldg4(const float* __restrict__ p, int i, int n) {
    if (AL) return *reinterpret_cast<const float4*>(p + i);
    float4 v;
    v.x = i < n ? p[i] : 0.f;
    v.y = i + 1 < n ? p[i + 1] : 0.f;
    v.z = i + 2 < n ? p[i + 2] : 0.f;
    v.w = i + 3 < n ? p[i + 3] : 0.f;
    return v;
}

// acc[r][c] = sum_k Lt[k * ldl + m0 + r] * R[k * ldr + n0 + c], k ascending.  LG / RG: the operand lives in global memory (valid
// extents M / N along its row), else in LDS with a pitch that is a multiple of 4 (pad columns are never mixed into valid outputs:
// an output element reads only its own column of either operand)
template <bool LG, bool RG, bool AL>
__device__ __forceinline__ void ow_tile(const float* __restrict__ Lt, int ldl, int M, const float* __restrict__ R, int ldr, int N, int K,
                                        int m0, int n0, float (&acc)[4][4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        const float4 a = LG ? ldg4<AL>(Lt + (size_t)k * ldl, m0, M) : *reinterpret_cast<const float4*>(Lt + k * ldl + m0);
        const float4 b = RG ? ldg4<AL>(R + (size_t)k * ldr, n0, N) : *reinterpret_cast<const float4*>(R + k * ldr + n0);
        const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = fmaf(av[r], bv[c], acc[r][c]);
    }
}

// tile t of an MT x NT tiling -> (m0, n0).  MFAST: consecutive lanes take consecutive m tiles (a product stored transposed: its stores and
// its left operand's reads are then contiguous across lanes), else consecutive n tiles
template <bool MFAST>
__device__ __forceinline__ void ow_tile_of(int t, int MT, int NT, int& m0, int& n0) {
    if (MFAST) { const int nt = t / MT; m0 = (t - nt * MT) * 4; n0 = nt * 4; }
    else { const int mt = t / NT; m0 = mt * 4; n0 = (t - mt * NT) * 4; }
}

// dst[(n0 + c) * pitch + m0 .. + 3] = acc[.][c]: the tile stored transposed, one 16-byte piece per column
__device__ __forceinline__ void ow_store_t(float* dst, int pitch, int m0, int n0, const float (&acc)[4][4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
        *reinterpret_cast<float4*>(dst + (n0 + c) * pitch + m0) = make_float4(acc[0][c], acc[1][c], acc[2][c], acc[3][c]);
}

__device__ __forceinline__ void ow_store_n(float* dst, int pitch, int m0, int n0, const float (&acc)[4][4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
        *reinterpret_cast<float4*>(dst + (m0 + r) * pitch + n0) = make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
}

// AL: Y and X are multiples of 4 -- every 16-byte global access below is aligned and in range
template <bool AL>
__global__ void __launch_bounds__(OW_T) k_solve_one_wg(OwArgs a) {
    extern __shared__ float4 ow_lds[];
    const int Y = a.Y, X = a.X, YP = a.YP, XP = a.XP, win = a.win, SP = a.SP, tid = threadIdx.x;
    const int S = XP * YP, MT = YP / 4, NT = XP / 4, WT = win / 4;
    float* A = reinterpret_cast<float*>(ow_lds);
    float* Bf = A + S;
    float* W = Bf + S;
    float* xs = W + win * win;
    float* part = xs + SP;
    float* T0 = a.T0 + (size_t)blockIdx.x * Y * X;
    float acc[4][4];
    int m0, n0;

    for (int e = tid; e < Y * XP; e += OW_T) {
        const int m = e / XP, c = e - m * XP;
        Bf[e] = c < X ? T0[m * X + c] : 0.f;
    }
    __syncthreads();
    // P1  A^T[c][m] = sum_k Qy[k][m] rhs[k][c]
    for (int t = tid; t < MT * NT; t += OW_T) {
        ow_tile_of<true>(t, MT, NT, m0, n0);
        ow_tile<true, false, AL>(a.Qy, Y, Y, Bf, XP, X, Y, m0, n0, acc);
        ow_store_t(A, YP, m0, n0, acc);
    }
    __syncthreads();
    // P2  T2^T[c][m] = (sum_k A^T[k][m] Qx[k][c]) / lam[m][c]
    for (int t = tid; t < MT * NT; t += OW_T) {
        ow_tile_of<true>(t, MT, NT, m0, n0);
        ow_tile<false, true, AL>(A, YP, Y, a.Qx, X, X, X, m0, n0, acc);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float4 il = n0 + c < X ? ldg4<AL>(a.ilT + (size_t)(n0 + c) * Y, m0, Y) : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(Bf + (n0 + c) * YP + m0) = make_float4(acc[0][c] * il.x, acc[1][c] * il.y, acc[2][c] * il.z, acc[3][c] * il.w);
        }
    }
    __syncthreads();
    // P3a  U[m][j] = sum_c T2^T[c][m] QxW[c][j]
    for (int t = tid; t < MT * WT; t += OW_T) {
        ow_tile_of<false>(t, MT, WT, m0, n0);
        ow_tile<false, true, AL>(Bf, YP, Y, a.QxW, win, win, X, m0, n0, acc);
        ow_store_n(A, win, m0, n0, acc);
    }
    __syncthreads();
    // P3b  X0[i][j] = sum_m Qy[m][wy0 + i] U[m][j]
    for (int t = tid; t < WT * WT; t += OW_T) {
        ow_tile_of<false>(t, WT, WT, m0, n0);
        // (the one operand whose rows start at a column offset: 16-byte pieces only where wy0 allows them)
        if (AL && (a.wy0 & 3) == 0) ow_tile<true, false, true>(a.Qy + a.wy0, Y, win, A, win, win, Y, m0, n0, acc);
        else ow_tile<true, false, false>(a.Qy + a.wy0, Y, win, A, win, win, Y, m0, n0, acc);
        ow_store_n(W, win, m0, n0, acc);
    }
    __syncthreads();
    // P4  xs = X0[sidx];  W2 = 0;  W2[sidx] = -K' xs  (K' stored transposed; rows and columns beyond nS are zero padding)
    const int nW = win * win;
    for (int t = tid; t < SP; t += OW_T) {
        const int si = a.sidx[t];
        xs[t] = (si >= 0 && si < nW) ? W[si] : 0.f;
    }
    __syncthreads();
    for (int t = tid; t < nW; t += OW_T) W[t] = 0.f;
    __syncthreads();
    if (SP >= OW_T) {
        for (int s = tid; s < a.nS; s += OW_T) {
            const int si = a.sidx[s];
            if (si < 0 || si >= nW) continue;
            float c = 0.f;
            for (int q = 0; q < a.nS; ++q) c = fmaf(a.KpT[(size_t)q * SP + s], xs[q], c);
            W[si] = -c;
        }
    } else {
        // G = 512 / SP groups of SP threads split the sum over q; the partials are added in group order (the same bits on every call)
        const int G = OW_T / SP, g = tid / SP, s = tid - g * SP;
        if (g < G) {
            const int q0 = (int)((long)a.nS * g / G), q1 = (int)((long)a.nS * (g + 1) / G);
            float c = 0.f;
            for (int q = q0; q < q1; ++q) c = fmaf(a.KpT[(size_t)q * SP + s], xs[q], c);
            part[g * SP + s] = c;
        }
        __syncthreads();
        if (tid < a.nS) {
            const int si = a.sidx[tid];
            if (si >= 0 && si < nW) {
                float c = 0.f;
                for (int h = 0; h < G; ++h) c += part[h * SP + tid];
                W[si] = -c;
            }
        }
    }
    __syncthreads();
    // P5a  V^T[j][m] = sum_i Qy[wy0 + i][m] W2[i][j]
    for (int t = tid; t < MT * WT; t += OW_T) {
        ow_tile_of<true>(t, MT, WT, m0, n0);
        ow_tile<true, false, AL>(a.Qy + (size_t)a.wy0 * Y, Y, Y, W, win, win, win, m0, n0, acc);
        ow_store_t(A, YP, m0, n0, acc);
    }
    __syncthreads();
    // P5b  T2^T[c][m] += (sum_j V^T[j][m] Qx[wx0 + j][c]) / lam[m][c]
    for (int t = tid; t < MT * NT; t += OW_T) {
        ow_tile_of<true>(t, MT, NT, m0, n0);
        ow_tile<false, true, AL>(A, YP, Y, a.Qx + (size_t)a.wx0 * X, X, X, win, m0, n0, acc);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float4 il = n0 + c < X ? ldg4<AL>(a.ilT + (size_t)(n0 + c) * Y, m0, Y) : make_float4(0.f, 0.f, 0.f, 0.f);
            float4* d = reinterpret_cast<float4*>(Bf + (n0 + c) * YP + m0);
            const float4 o = *d;
            *d = make_float4(fmaf(acc[0][c], il.x, o.x), fmaf(acc[1][c], il.y, o.y), fmaf(acc[2][c], il.z, o.z), fmaf(acc[3][c], il.w, o.w));
        }
    }
    __syncthreads();
    // P6a  T1[m][c] = sum_k T2^T[k][m] Qx[k][c]
    for (int t = tid; t < MT * NT; t += OW_T) {
        ow_tile_of<false>(t, MT, NT, m0, n0);
        ow_tile<false, true, AL>(Bf, YP, Y, a.Qx, X, X, X, m0, n0, acc);
        ow_store_n(A, XP, m0, n0, acc);
    }
    __syncthreads();
    // P6b  p[m][c] = sum_k Qy[k][m] T1[k][c]
    for (int t = tid; t < MT * NT; t += OW_T) {
        ow_tile_of<false>(t, MT, NT, m0, n0);
        ow_tile<true, false, AL>(a.Qy, Y, Y, A, XP, X, Y, m0, n0, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (AL) {
                *reinterpret_cast<float4*>(T0 + (size_t)(m0 + r) * X + n0) = make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
            } else if (m0 + r < Y) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (n0 + c < X) T0[(size_t)(m0 + r) * X + n0 + c] = acc[r][c];
            }
        }
    }
}

size_t ow_lds_bytes(int Y, int X, int win, int SP) {
    const size_t YP = (Y + 3) / 4 * 4, XP = (X + 3) / 4 * 4;
    return (2 * XP * YP + (size_t)win * win + SP + OW_T) * sizeof(float);
}

}  // namespace

bool sol_solve_one_wg_supported(int Y, int X, int win) {
    return Y >= 16 && X >= 16 && (long)Y * X <= 8192 && X <= 64 && (win == 16 || win == 32 || win == 64) && win <= Y && win <= X;
}

extern "C" int sol_karman_solve_one_wg_supported(int32_t Y, int32_t X, int32_t win) { return sol_solve_one_wg_supported(Y, X, win) ? 1 : 0; }

// hdr: the host copy of the blob's header, checked by sol_large_direct_check; base: rhs [B][Y][X] in, p out
int sol_solve_one_wg(hipStream_t s, const sol_karman_cfg* c, const int32_t* hdr, float* base) {
    const int Y = c->Y, X = c->X, wy0 = hdr[3], wx0 = hdr[4], nS = hdr[5], SP = hdr[6], win = hdr[7];
    SOL_REQUIRE(hdr[1] == Y && hdr[2] == X && sol_solve_one_wg_supported(Y, X, win), "sol_solve_one_wg: a %dx%d grid with window %d is not served", Y, X, win);
    SOL_REQUIRE(nS >= 1 && SP >= nS && SP <= OW_MAXSP && SP % 64 == 0 && wy0 >= 0 && wx0 >= 0 && wy0 + win <= Y && wx0 + win <= X,
                "sol_solve_one_wg: direct-solver blob header is inconsistent");
    const size_t words = (size_t)OW_HEADER + (size_t)Y * Y + (size_t)X * X + (size_t)X * Y + (size_t)SP * SP + SP + (size_t)X * win;
    SOL_REQUIRE((size_t)c->direct_n >= words, "sol_solve_one_wg: cfg.direct_n = %d words, the blob of this header has %zu", c->direct_n, words);
    const size_t lds = ow_lds_bytes(Y, X, win, SP);
    SOL_REQUIRE(lds <= 160 * 1024, "sol_solve_one_wg: %zu bytes of LDS", lds);
    static std::atomic<unsigned long long> optin{0};
    if (int e = sol_lds_optin(optin, {SOL_K(k_solve_one_wg<true>), SOL_K(k_solve_one_wg<false>)}, "k_solve_one_wg")) return e;
    OwArgs a{};
    a.Qy = c->direct + OW_HEADER;
    a.Qx = a.Qy + (size_t)Y * Y;
    a.ilT = a.Qx + (size_t)X * X;
    a.KpT = a.ilT + (size_t)X * Y;
    a.sidx = reinterpret_cast<const int*>(a.KpT + (size_t)SP * SP);
    a.QxW = reinterpret_cast<const float*>(a.sidx + SP);
    a.T0 = base;
    a.Y = Y; a.X = X; a.YP = (Y + 3) / 4 * 4; a.XP = (X + 3) / 4 * 4; a.win = win; a.wy0 = wy0; a.wx0 = wx0; a.nS = nS; a.SP = SP;
    const bool aligned = Y % 4 == 0 && X % 4 == 0 && (reinterpret_cast<uintptr_t>(c->direct) & 15) == 0 &&
                         (reinterpret_cast<uintptr_t>(base) & 15) == 0;
    if (aligned) SOL_LAUNCH(k_solve_one_wg<true>, dim3(c->B), dim3(OW_T), lds, s, a);
    else SOL_LAUNCH(k_solve_one_wg<false>, dim3(c->B), dim3(OW_T), lds, s, a);
    SOL_LAUNCH_CHECK();
    return SOL_OK;
}
