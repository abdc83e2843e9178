"""Host-side setup of the two-level CG preconditioner of the fused solver step.

M^-1 = D^-1 + P (P^T M P)^-1 P^T for M = -A, the SPD pressure matrix of the scene
(PhiFlow sparse_pressure_matrix semantics: diagonal = number of accessible neighbours (>= 1),
off-diagonal -1 between two active cells, p = 0 outside the OPEN domain), with P the
piecewise-constant prolongation of 8x8-cell aggregates restricted to active cells.  Only the dense
coarse inverse (nc x nc, nc = Y*X/64) is computed here, once per scene geometry, in float64; the
device kernels apply it inside their CG loop (csrc/karman_step.hip: pcg_solve).  It changes the
iteration count (about 235 -> 56 at 128x64), not the converged solution.
"""
import functools

import numpy as np


def pressure_matrix_dense_coarse(active, block=8):
    """P^T M P as a dense [nc,nc] float64 array, assembled directly from the stencil."""
    act = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
    Y, X = act.shape
    assert Y % block == 0 and X % block == 0
    nby, nbx = Y // block, X // block
    nc = nby * nbx
    acc = np.pad(act, 1, mode="edge")            # accessible: 'boundary' extrapolation (OPEN)
    diag = np.maximum(acc[0:Y, 1:X + 1] + acc[2:Y + 2, 1:X + 1] + acc[1:Y + 1, 0:X] + acc[1:Y + 1, 2:X + 2], 1.0)
    jj, ii = np.meshgrid(np.arange(Y), np.arange(X), indexing="ij")
    blk = (jj // block) * nbx + (ii // block)
    Ac = np.zeros((nc, nc))
    # diagonal contributions (P has the active mask as entries)
    np.add.at(Ac, (blk.ravel(), blk.ravel()), (act * diag * act).ravel())
    # off-diagonal contributions: -act[c]*act[n] for the 4 neighbours inside the domain
    for sj, si in ((1, 0), (0, 1)):
        a = act[0:Y - sj, 0:X - si] * act[sj:Y, si:X]
        b0 = blk[0:Y - sj, 0:X - si].ravel()
        b1 = blk[sj:Y, si:X].ravel()
        np.add.at(Ac, (b0, b1), -a.ravel())
        np.add.at(Ac, (b1, b0), -a.ravel())
    return Ac


def coarse_inverse(active, block=8):
    """float32 [nc,nc] inverse of the coarse matrix (aggregates without active cells get 1)."""
    Ac = pressure_matrix_dense_coarse(active, block)
    empty = np.diag(Ac) == 0
    Ac[empty, empty] = 1.0
    return np.linalg.inv(Ac).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# Direct pressure solver: fast diagonalisation of the rectangle + capacitance correction
# ---------------------------------------------------------------------------------------------
# On the OPEN rectangle without obstacle M is the 5-point Dirichlet Laplacian M_r = T_Y (x) I + I (x) T_X,
# diagonalised by the orthonormal sine transforms Q_Y, Q_X:  M_r^-1 = (Q_Y (x) Q_X) diag(1/lam) (Q_Y (x) Q_X).
# The obstacle changes M only on the set S of obstacle cells and their neighbours (164 cells at
# 128x64, inside one 16x16 window):  M = M_r + U_S E_SS U_S^T.  Then
#     x = G (b - U_S E_SS x_S),   x_S = (I + G_SS E_SS)^-1 (G b)_S,   G = M_r^-1
# i.e. one forward transform, a window-sized dense correction, one inverse transform: NO iteration,
# same solution as the converged CG up to fp32 round-off (csrc/karman_step.hip: fd_solve).
FD_MAGIC = 0x46443032          # "FD02"
FD_HEADER = 16                 # int32 words
FD_WIN = 16                    # window edge (cells) of the one-workgroup kernels; the large-grid path takes 16/32/64


def dst_matrix(n):
    k = np.arange(1, n + 1)
    return np.sqrt(2.0 / (n + 1)) * np.sin(np.pi * np.outer(k, k) / (n + 1))


def hartley_matrix(n):
    """The discrete Hartley matrix H[j,k] = (cos(2 pi j k / n) + sin(2 pi j k / n)) / sqrt(n): symmetric, its own inverse, and it
    diagonalises the PERIODIC second difference (2 on the diagonal, -1 to both neighbours, the last cell coupled to the first) with the
    eigenvalues 2 - 2 cos(2 pi k / n).  The table of a periodic axis where an open one has dst_matrix."""
    k = np.arange(n)
    a = 2.0 * np.pi * (np.outer(k, k) % n) / n
    return (np.cos(a) + np.sin(a)) / np.sqrt(n)


PERIODIC_Y, PERIODIC_X = 2, 4      # header flag bits of a blob built with periodic=(py, px): FD02 word 8, FDS1 word 9 (its word 8 is CP)


def _ints(a):
    """the int32 words of a blob section: a float32 device blob holds their bits, a dtype=np.float64 host blob their values"""
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a.astype(np.int32)


def _periodic_arg(periodic):
    py, px = periodic
    return bool(py), bool(px)


def _periodic_flags(periodic):
    py, px = _periodic_arg(periodic)
    return PERIODIC_Y * py + PERIODIC_X * px


def blob_periodic(blob_or_header):
    """(py, px) recorded in the header of a direct, box or scattered blob (or of its 16-word int32 host copy)"""
    hdr = _ints(blob_or_header[:FD_HEADER])
    w = int(hdr[9 if hdr[0] == FDS_MAGIC else 8])
    return bool(w & PERIODIC_Y), bool(w & PERIODIC_X)


def _axis_tables(n, periodic):
    """(Q, lam) of one axis: the symmetric orthogonal transform and the eigenvalues of its second difference"""
    if periodic:
        return hartley_matrix(n), 2 - 2 * np.cos(2 * np.pi * np.arange(n) / n)
    return dst_matrix(n), 2 - 2 * np.cos(np.pi * np.arange(1, n + 1) / (n + 1))


def _box_tables(Y, X, periodic):
    """(Qy, Qx, lam [Y,X], 1/lam) of the empty box; doubly periodic: lam[0,0] = 0 and 1/lam = 0 there (the zero-mean solution)"""
    py, px = _periodic_arg(periodic)
    if not (py or px):      # the expressions the open blobs have always been built with, bit for bit
        Qy, Qx = dst_matrix(Y), dst_matrix(X)
        lam = (2 - 2 * np.cos(np.pi * np.arange(1, Y + 1) / (Y + 1)))[:, None] + (2 - 2 * np.cos(np.pi * np.arange(1, X + 1) / (X + 1)))[None, :]
        return Qy, Qx, lam, 1.0 / lam
    (Qy, ly), (Qx, lx) = _axis_tables(Y, py), _axis_tables(X, px)
    lam = ly[:, None] + lx[None, :]
    il = np.zeros_like(lam)
    np.divide(1.0, lam, out=il, where=lam > 1e-12)
    if py and px:
        lam = lam.copy()
        lam[0, 0] = 0.0
    return Qy, Qx, lam, il


def _accessible(act, periodic=(False, False)):
    """act with one ring of ghost cells: 'boundary' extrapolation on an open axis, the wrapped cells on a periodic one"""
    py, px = _periodic_arg(periodic)
    acc = np.pad(act, ((1, 1), (0, 0)), mode="wrap" if py else "edge")
    return np.pad(acc, ((0, 0), (1, 1)), mode="wrap" if px else "edge")


def _seam_pairs(Y, X, periodic):
    """The cell pairs a periodic axis adds to the stencil, as (row slice, col slice) of the first and the second cell: last -> first"""
    py, px = _periodic_arg(periodic)
    pairs = []
    if py:
        pairs.append(((slice(Y - 1, Y), slice(0, X)), (slice(0, 1), slice(0, X))))
    if px:
        pairs.append(((slice(0, Y), slice(X - 1, X)), (slice(0, Y), slice(0, 1))))
    return pairs


def scene_matrix(active, periodic=(False, False)):
    """Dense float64 M = -A of the scene (small grids / setup only).  periodic=(py, px): the accessible mask wraps along a periodic axis
    and the last cell of each line couples to the first; doubly periodic: M is singular (constants)."""
    act = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
    Y, X = act.shape
    N = Y * X
    acc = _accessible(act, periodic)
    diag = np.maximum(acc[0:Y, 1:X + 1] + acc[2:Y + 2, 1:X + 1] + acc[1:Y + 1, 0:X] + acc[1:Y + 1, 2:X + 2], 1.0)
    idx = np.arange(N).reshape(Y, X)
    M = np.zeros((N, N))
    M[idx.ravel(), idx.ravel()] = diag.ravel()
    for sj, si in ((1, 0), (0, 1)):
        a = (act[0:Y - sj, 0:X - si] * act[sj:Y, si:X]).ravel()
        r = idx[0:Y - sj, 0:X - si].ravel()
        c = idx[sj:Y, si:X].ravel()
        M[r, c] -= a
        M[c, r] -= a
    for first, second in _seam_pairs(Y, X, periodic):
        a = (act[first] * act[second]).ravel()
        r, c = idx[first].ravel(), idx[second].ravel()
        M[r, c] -= a
        M[c, r] -= a
    return M


def _general_perturbation(active, periodic=(False, False)):
    """Sparse difference E = M - M_r as {(row, col): value} restricted to its support set S (M_r: the empty box with the same
    periodic axes)."""
    act = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
    Y, X = act.shape
    acc = _accessible(act, periodic)
    diag = np.maximum(acc[0:Y, 1:X + 1] + acc[2:Y + 2, 1:X + 1] + acc[1:Y + 1, 0:X] + acc[1:Y + 1, 2:X + 2], 1.0)
    ent = {}
    for j, i in zip(*np.nonzero(diag != 4.0)):
        ent[(j * X + i, j * X + i)] = diag[j, i] - 4.0
    for sj, si in ((1, 0), (0, 1)):
        a = act[0:Y - sj, 0:X - si] * act[sj:Y, si:X]
        for j, i in zip(*np.nonzero(a != 1.0)):
            r, c = j * X + i, (j + sj) * X + (i + si)
            ent[(r, c)] = ent[(c, r)] = 1.0 - a[j, i]      # M has -a, M_r has -1
    idx = np.arange(Y * X).reshape(Y, X)
    for first, second in _seam_pairs(Y, X, periodic):
        a = (act[first] * act[second]).ravel()
        for r, c, v in zip(idx[first].ravel(), idx[second].ravel(), a):
            if v != 1.0:
                ent[(int(r), int(c))] = ent[(int(c), int(r))] = 1.0 - v
    return ent


def _refuse_doubly_periodic_obstacle(periodic, ent, who):
    if all(_periodic_arg(periodic)) and ent:
        raise ValueError("%s: a doubly periodic scene must be empty (no obstacle): its pressure matrix is singular and the capacitance "
                         "correction of a singular box solve is not built.  Keep one axis open, or drop the obstacle" % who)


def _general_direct_solver_blob(active, max_window=FD_WIN, periodic=(False, False), dtype=np.float32):
    """float32 blob consumed by sol_karman_cfg.direct, or None when the scene does not qualify
    (perturbed cells do not fit one window, or the capacitance system is ill conditioned).  The window edge is the
    smallest of 16, 32, 64 (<= max_window) that holds the perturbed cells; it is stored in header[7].

    layout (32-bit words): header[16] = {magic, Y, X, wy0, wx0, nS, SP, win, ...};  Qy[Y*Y];  Qx[X*X];
    invlamT[X*Y] (= 1/lam[m][c] stored [c][m]);  KpT[SP*SP] (K' = E_SS (I + G_SS E_SS)^-1, stored
    transposed, zero padded);  sidx[SP] int32 (window-local index j'*win + i', -1 = padding);
    QxW[X*win] (= Qx[c][wx0 + i'], the window columns of Qx as one compact slab).
    periodic=(py, px): the tables of a periodic axis are hartley_matrix and its eigenvalues, header word 8 carries PERIODIC_Y / PERIODIC_X,
    and a scene WITHOUT perturbation gets the box blob (nS = 0) as its direct blob: box forward, box back.  The window does not wrap:
    an obstacle across the seam spans the whole axis and goes to scattered_solver_blob.
    dtype=np.float64 (host checks only, never a device blob): the same words unrounded, integers stored as float64 values."""
    act = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
    Y, X = act.shape
    ent = _perturbation(act, periodic)
    _refuse_doubly_periodic_obstacle(periodic, ent, "direct_solver_blob")
    if not ent:
        return box_solver_blob(Y, X, periodic, dtype) if any(_periodic_arg(periodic)) else None
    S = np.array(sorted({r for r, _ in ent}), dtype=np.int64)
    js, is_ = S // X, S % X
    span = int(max(js.max() - js.min(), is_.max() - is_.min())) + 1
    win = next((w for w in (16, 32, 64) if w >= span and w <= max_window), None)
    if win is None or Y < win or X < win:
        return None
    wy0 = int(min(js.min(), Y - win))
    wx0 = int(min(is_.min(), X - win))
    nS = len(S)
    SP = (nS + 63) // 64 * 64
    pos = {int(s): n for n, s in enumerate(S)}
    ESS = np.zeros((nS, nS))
    for (r, c), v in ent.items():
        ESS[pos[r], pos[c]] = v
    Qy, Qx, lam, il = _box_tables(Y, X, periodic)
    # G_SS[s, t] = sum_{m,c} Qy[js,m] Qx[is,c] / lam[m,c] * Qy[jt,m] Qx[it,c]
    Fy, Fx = Qy[js, :], Qx[is_, :]                                # [nS, Y], [nS, X]
    F = (Fy[:, :, None] * Fx[:, None, :]).reshape(nS, Y * X)
    GSS = (F / lam.reshape(1, Y * X)) @ F.T
    cap = np.eye(nS) + GSS @ ESS
    if np.linalg.cond(cap) > 1e6:
        return None
    Kp = ESS @ np.linalg.inv(cap)
    KpT = np.zeros((SP, SP))
    KpT[:nS, :nS] = Kp.T
    sidx = np.full(SP, -1, dtype=np.int32)
    sidx[:nS] = ((js - wy0) * win + (is_ - wx0)).astype(np.int32)
    header = np.zeros(FD_HEADER, dtype=np.int32)
    header[:8] = [FD_MAGIC, Y, X, wy0, wx0, nS, SP, win]
    header[8] = _periodic_flags(periodic)
    assert dtype in (np.float32, np.float64)
    words = (lambda a: a.view(np.float32)) if dtype == np.float32 else (lambda a: a.astype(np.float64))
    parts = [words(header), Qy.astype(dtype).ravel(), Qx.astype(dtype).ravel(),
             (1.0 / lam).T.astype(dtype).ravel(), KpT.astype(dtype).ravel(), words(sidx),
             np.ascontiguousarray(Qx[:, wx0:wx0 + win]).astype(dtype).ravel()]
    return np.concatenate(parts)


def _general_box_solver_blob(Y, X, periodic=(False, False), dtype=np.float32):
    """float32 blob of the empty-box solve G = M_r^-1 alone: the direct_solver_blob layout with nS = SP = 0 (no capacitance part, no
    window: win = 0), i.e. header[16] = {magic, Y, X, 0, 0, 0, 0, 0, ...}; Qy[Y*Y]; Qx[X*X]; invlamT[X*Y].  The preconditioner of
    the large-grid CG solve (sol_karman_step_fwd_large_cg), which takes any obstacle.
    periodic=(py, px): Hartley tables on a periodic axis, flags in header word 8; doubly periodic: 1/lam = 0 at the zero mode, so the
    solve returns the zero-mean pressure of a zero-mean right-hand side.  An empty periodic scene runs this blob as its direct solve."""
    Qy, Qx, lam, il = _box_tables(Y, X, periodic)
    header = np.zeros(FD_HEADER, dtype=np.int32)
    header[:3] = [FD_MAGIC, Y, X]
    header[8] = _periodic_flags(periodic)
    assert dtype in (np.float32, np.float64)           # float64: host checks only (integers stored as float64 values)
    return np.concatenate([header.view(np.float32) if dtype == np.float32 else header.astype(np.float64), Qy.astype(dtype).ravel(),
                           Qx.astype(dtype).ravel(), il.T.astype(dtype).ravel()])


def box_solve_reference(blob, b):
    """float64 numpy restatement of G b on a box_solver_blob (b [Y, X])."""
    hdr = _ints(blob[:FD_HEADER])
    assert hdr[0] == FD_MAGIC and hdr[5] == 0
    Y, X = int(hdr[1]), int(hdr[2])
    o = FD_HEADER
    Qy = blob[o:o + Y * Y].astype(np.float64).reshape(Y, Y); o += Y * Y
    Qx = blob[o:o + X * X].astype(np.float64).reshape(X, X); o += X * X
    il = blob[o:o + X * Y].astype(np.float64).reshape(X, Y).T
    return Qy @ (((Qy @ b) @ Qx) * il) @ Qx


def pcg_reference(active, blob, b, rtol=1e-6, atol=1e-9, max_iter=2000):
    """float64 numpy restatement of the large-grid CG solve (csrc/pcg.hip) of M x = b, M = scene_matrix(active), with
    the empty-box preconditioner of `blob`; returns (x, iterations, converged)."""
    act = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
    Y, X = act.shape
    acc = np.pad(act, 1, mode="edge")
    diag = np.maximum(acc[0:Y, 1:X + 1] + acc[2:Y + 2, 1:X + 1] + acc[1:Y + 1, 0:X] + acc[1:Y + 1, 2:X + 2], 1.0)

    def apply_M(p):
        pa = np.pad(p * act, 1)
        return diag * p - act * (pa[2:, 1:-1] + pa[:-2, 1:-1] + pa[1:-1, 2:] + pa[1:-1, :-2])

    b = np.asarray(b, dtype=np.float64)
    x, r = np.zeros_like(b), b.copy()
    bb = float((b * b).sum())
    stop = max(rtol * rtol * bb, atol * atol)
    if float((r * r).sum()) <= stop:
        return x, 0, True
    z = box_solve_reference(blob, r)
    p, rz = z, float((r * z).sum())
    for k in range(1, max_iter + 1):
        q = apply_M(p)
        al = rz / float((p * q).sum())
        x, r = x + al * p, r - al * q
        if float((r * r).sum()) <= stop:
            return x, k, True
        z = box_solve_reference(blob, r)
        rz_new = float((r * z).sum())
        p, rz = z + (rz_new / rz) * p, rz_new
    return x, max_iter, False


def _general_direct_solve_reference(blob, b):
    """float64 numpy restatement of the device algorithm on the blob (used by the CPU tests)."""
    hdr = _ints(blob[:FD_HEADER])
    assert hdr[0] == FD_MAGIC
    if hdr[5] == 0:             # the box blob as a direct blob (an empty periodic scene)
        return box_solve_reference(blob, b)
    Y, X, wy0, wx0, nS, SP = (int(v) for v in hdr[1:7])
    FD_WIN = int(hdr[7])
    o = FD_HEADER
    Qy = blob[o:o + Y * Y].astype(np.float64).reshape(Y, Y); o += Y * Y
    Qx = blob[o:o + X * X].astype(np.float64).reshape(X, X); o += X * X
    il = blob[o:o + X * Y].astype(np.float64).reshape(X, Y).T; o += X * Y
    KpT = blob[o:o + SP * SP].astype(np.float64).reshape(SP, SP); o += SP * SP
    sidx = _ints(blob[o:o + SP])
    T2 = (Qy @ b @ Qx) * il
    x0w = Qy[wy0:wy0 + FD_WIN, :] @ T2 @ Qx[:, wx0:wx0 + FD_WIN]
    xs = np.where(sidx >= 0, x0w.ravel()[np.maximum(sidx, 0)], 0.0)
    c = KpT.T @ xs
    w2 = np.zeros(FD_WIN * FD_WIN)
    w2[sidx[sidx >= 0]] = -c[sidx >= 0]
    w2 = w2.reshape(FD_WIN, FD_WIN)
    T2 = T2 + il * (Qy[:, wy0:wy0 + FD_WIN] @ w2 @ Qx[wx0:wx0 + FD_WIN, :])
    return Qy @ T2 @ Qx


# ---------------------------------------------------------------------------------------------
# Scattered direct solver: the same capacitance correction without the window
# ---------------------------------------------------------------------------------------------
# The correction needs G b only ON S and adds a term that lives only ON S.  With R the distinct rows of S and C its distinct
# columns, (G b)_S is a gather from X0 = Qy[R,:] T2 Qx[:,C] (|R| x |C|) and the correction enters the spectral coefficients as
# Qy[:,R] W2 Qx[C,:]: direct_solver_blob's algorithm with a row list and a column list where that one has two contiguous ranges
# (csrc/karman_large.hip: scattered_solve).  Any scene whose support set has at most 4096 cells qualifies, however spread out.
FDS_MAGIC = 0x46445331         # "FDS1"
FDS_MAX_SUPPORT = 4096


def _pad4(n):
    return (int(n) + 3) // 4 * 4


def scattered_solver_blob(active, dtype=np.float32, periodic=(False, False)):
    """float32 blob of the scattered direct solver (SceneMasks(pressure_solver="direct_scattered"), large grids only), or None when
    the scene has no perturbation, more than 4096 support cells, or an ill-conditioned capacitance system (cond > 1e6).

    layout (32-bit words): header[16] = {magic "FDS1", Y, X, nR, nC, nS, SP, RP, CP, ...} (RP, CP = |R|, |C| padded to multiples of
    4, SP = nS padded to a multiple of 64);  Qy[Y*Y];  Qx[X*X];  invlamT[X*Y];  zero words up to a multiple of 4 (16-byte rows of
    K'^T);  KpT[SP*SP] (K' = E_SS (I + G_SS E_SS)^-1 transposed, zero padded);  rows[RP], cols[CP] int32 (-1 = padding);
    sidx[SP] int32 (row-slot * CP + column-slot of a support cell in X0 / W2, -1 = padding);  the slabs the GEMMs read, zero in the
    padding:  QyR[RP*Y] = Qy[R,:];  QxC[X*CP] = Qx[:,C];  QyRt[Y*RP] = Qy[:,R];  QxCr[CP*X] = Qx[C,:].
    dtype=np.float64 (host checks only, never a device blob): the same words unrounded, integers stored as float64 values.
    periodic=(py, px): as direct_solver_blob, the flags in header word 9 (word 8 is CP); the row and column lists do not care where
    the seam is, so this is the blob of an obstacle that straddles it."""
    act = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
    Y, X = act.shape
    ent = _perturbation(act, periodic)
    _refuse_doubly_periodic_obstacle(periodic, ent, "scattered_solver_blob")
    if not ent:
        return None
    S = np.array(sorted({r for r, _ in ent}), dtype=np.int64)
    nS = len(S)
    if nS > FDS_MAX_SUPPORT:
        return None
    js, is_ = S // X, S % X
    R, rslot = np.unique(js, return_inverse=True)
    Cc, cslot = np.unique(is_, return_inverse=True)
    nR, nC = len(R), len(Cc)
    RP, CP = _pad4(nR), _pad4(nC)
    SP = (nS + 63) // 64 * 64
    pos = {int(s): n for n, s in enumerate(S)}
    ESS = np.zeros((nS, nS))
    for (r, c), v in ent.items():
        ESS[pos[r], pos[c]] = v
    Qy, Qx, lam, il = _box_tables(Y, X, periodic)
    Fy, Fx = Qy[js, :], Qx[is_, :]                                # [nS, Y], [nS, X]
    F = (Fy[:, :, None] * Fx[:, None, :]).reshape(nS, Y * X)
    GSS = (F / lam.reshape(1, Y * X)) @ F.T                       # one GEMM, as direct_solver_blob forms it
    del F
    cap = np.eye(nS) + GSS @ ESS
    if np.linalg.cond(cap) > 1e6:
        return None
    Kp = ESS @ np.linalg.inv(cap)
    KpT = np.zeros((SP, SP))
    KpT[:nS, :nS] = Kp.T
    rows = np.full(RP, -1, dtype=np.int32); rows[:nR] = R
    cols = np.full(CP, -1, dtype=np.int32); cols[:nC] = Cc
    sidx = np.full(SP, -1, dtype=np.int32)
    sidx[:nS] = (rslot * CP + cslot).astype(np.int32)
    QyR = np.zeros((RP, Y)); QyR[:nR] = Qy[R, :]
    QxC = np.zeros((X, CP)); QxC[:, :nC] = Qx[:, Cc]
    header = np.zeros(FD_HEADER, dtype=np.int32)
    header[:9] = [FDS_MAGIC, Y, X, nR, nC, nS, SP, RP, CP]
    header[9] = _periodic_flags(periodic)
    lead = Y * Y + X * X + X * Y
    assert dtype in (np.float32, np.float64)
    flt = lambda a: np.ascontiguousarray(a).astype(dtype).ravel()
    words = (lambda a: a.view(np.float32)) if dtype == np.float32 else (lambda a: a.astype(np.float64))
    parts = [words(header), flt(Qy), flt(Qx), flt((1.0 / lam).T), np.zeros(_pad4(lead) - lead, dtype=dtype), flt(KpT),
             words(rows), words(cols), words(sidx), flt(QyR), flt(QxC), flt(QyR.T), flt(QxC.T)]
    return np.concatenate(parts)


def scattered_sections(blob):
    """The sections of a scattered_solver_blob as a dict of views (header fields by name, matrices in their shapes)."""
    ints = (lambda a: a.view(np.int32)) if blob.dtype == np.float32 else (lambda a: a.astype(np.int32))
    hdr = ints(blob[:FD_HEADER])
    assert hdr[0] == FDS_MAGIC
    Y, X, nR, nC, nS, SP, RP, CP = (int(v) for v in hdr[1:9])
    s = dict(Y=Y, X=X, nR=nR, nC=nC, nS=nS, SP=SP, RP=RP, CP=CP)
    o = FD_HEADER

    def take(name, n, shape, integer=False):
        nonlocal o
        a = blob[o:o + n]
        s[name] = (ints(a) if integer else a).reshape(shape)
        o += n

    take("Qy", Y * Y, (Y, Y)); take("Qx", X * X, (X, X)); take("ilT", X * Y, (X, Y))
    o = FD_HEADER + _pad4(o - FD_HEADER)
    take("KpT", SP * SP, (SP, SP))
    take("rows", RP, (RP,), True); take("cols", CP, (CP,), True); take("sidx", SP, (SP,), True)
    take("QyR", RP * Y, (RP, Y)); take("QxC", X * CP, (X, CP)); take("QyRt", Y * RP, (Y, RP)); take("QxCr", CP * X, (CP, X))
    s["words"] = o
    return s


def scattered_solve_reference(blob, b):
    """float64 numpy restatement of the device algorithm on a scattered_solver_blob (b [Y, X]); used by the CPU tests.  On the device's
    float32 blob the result carries the rounding of its matrices; on a dtype=np.float64 blob it is the algorithm alone."""
    s = scattered_sections(blob)
    f = lambda k: s[k].astype(np.float64)
    Qy, Qx, il, sidx = f("Qy"), f("Qx"), f("ilT").T, s["sidx"]
    T2 = (Qy @ b @ Qx) * il
    x0 = f("QyR") @ (T2 @ f("QxC"))                              # [RP, CP]
    xs = np.where(sidx >= 0, x0.ravel()[np.maximum(sidx, 0)], 0.0)
    c = f("KpT").T @ xs
    w2 = np.zeros(s["RP"] * s["CP"])
    w2[sidx[sidx >= 0]] = -c[sidx >= 0]
    T2 = T2 + il * ((f("QyRt") @ w2.reshape(s["RP"], s["CP"])) @ f("QxCr"))
    return Qy @ T2 @ Qx


# ---------------------------------------------------------------------------------------------
# The open builders, and the public names
# ---------------------------------------------------------------------------------------------
# The four functions below are the OPEN builders as they have always been, text and all (tests/test_scattered_direct_cpu.py pins the
# SHA-256 of their source, so that a blob of an open scene cannot move by accident).  The public names are then rebound to thin
# dispatchers: a call without `periodic` (and without the host-only dtype=np.float64) runs the open builder, bit for bit; anything else
# runs the general one above (_general_*), which holds the periodic tables, the seam couplings and the header flags.


def _perturbation(active):
    """Sparse difference E = M - M_r as {(row, col): value} restricted to its support set S."""
    act = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
    Y, X = act.shape
    acc = np.pad(act, 1, mode="edge")
    diag = np.maximum(acc[0:Y, 1:X + 1] + acc[2:Y + 2, 1:X + 1] + acc[1:Y + 1, 0:X] + acc[1:Y + 1, 2:X + 2], 1.0)
    ent = {}
    for j, i in zip(*np.nonzero(diag != 4.0)):
        ent[(j * X + i, j * X + i)] = diag[j, i] - 4.0
    for sj, si in ((1, 0), (0, 1)):
        a = act[0:Y - sj, 0:X - si] * act[sj:Y, si:X]
        for j, i in zip(*np.nonzero(a != 1.0)):
            r, c = j * X + i, (j + sj) * X + (i + si)
            ent[(r, c)] = ent[(c, r)] = 1.0 - a[j, i]      # M has -a, M_r has -1
    return ent


def direct_solver_blob(active, max_window=FD_WIN):
    """float32 blob consumed by sol_karman_cfg.direct, or None when the scene does not qualify
    (perturbed cells do not fit one window, or the capacitance system is ill conditioned).  The window edge is the
    smallest of 16, 32, 64 (<= max_window) that holds the perturbed cells; it is stored in header[7].

    layout (32-bit words): header[16] = {magic, Y, X, wy0, wx0, nS, SP, win, ...};  Qy[Y*Y];  Qx[X*X];
    invlamT[X*Y] (= 1/lam[m][c] stored [c][m]);  KpT[SP*SP] (K' = E_SS (I + G_SS E_SS)^-1, stored
    transposed, zero padded);  sidx[SP] int32 (window-local index j'*win + i', -1 = padding);
    QxW[X*win] (= Qx[c][wx0 + i'], the window columns of Qx as one compact slab)."""
    act = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
    Y, X = act.shape
    ent = _perturbation(act)
    if not ent:
        return None
    S = np.array(sorted({r for r, _ in ent}), dtype=np.int64)
    js, is_ = S // X, S % X
    span = int(max(js.max() - js.min(), is_.max() - is_.min())) + 1
    win = next((w for w in (16, 32, 64) if w >= span and w <= max_window), None)
    if win is None or Y < win or X < win:
        return None
    wy0 = int(min(js.min(), Y - win))
    wx0 = int(min(is_.min(), X - win))
    nS = len(S)
    SP = (nS + 63) // 64 * 64
    pos = {int(s): n for n, s in enumerate(S)}
    ESS = np.zeros((nS, nS))
    for (r, c), v in ent.items():
        ESS[pos[r], pos[c]] = v
    Qy, Qx = dst_matrix(Y), dst_matrix(X)
    lam = (2 - 2 * np.cos(np.pi * np.arange(1, Y + 1) / (Y + 1)))[:, None] + (2 - 2 * np.cos(np.pi * np.arange(1, X + 1) / (X + 1)))[None, :]
    # G_SS[s, t] = sum_{m,c} Qy[js,m] Qx[is,c] / lam[m,c] * Qy[jt,m] Qx[it,c]
    Fy, Fx = Qy[js, :], Qx[is_, :]                                # [nS, Y], [nS, X]
    F = (Fy[:, :, None] * Fx[:, None, :]).reshape(nS, Y * X)
    GSS = (F / lam.reshape(1, Y * X)) @ F.T
    cap = np.eye(nS) + GSS @ ESS
    if np.linalg.cond(cap) > 1e6:
        return None
    Kp = ESS @ np.linalg.inv(cap)
    KpT = np.zeros((SP, SP))
    KpT[:nS, :nS] = Kp.T
    sidx = np.full(SP, -1, dtype=np.int32)
    sidx[:nS] = ((js - wy0) * win + (is_ - wx0)).astype(np.int32)
    header = np.zeros(FD_HEADER, dtype=np.int32)
    header[:8] = [FD_MAGIC, Y, X, wy0, wx0, nS, SP, win]
    parts = [header.view(np.float32), Qy.astype(np.float32).ravel(), Qx.astype(np.float32).ravel(),
             (1.0 / lam).T.astype(np.float32).ravel(), KpT.astype(np.float32).ravel(), sidx.view(np.float32),
             np.ascontiguousarray(Qx[:, wx0:wx0 + win]).astype(np.float32).ravel()]
    return np.concatenate(parts)


def box_solver_blob(Y, X):
    """float32 blob of the empty-box solve G = M_r^-1 alone: the direct_solver_blob layout with nS = SP = 0 (no capacitance part, no
    window: win = 0), i.e. header[16] = {magic, Y, X, 0, 0, 0, 0, 0, ...}; Qy[Y*Y]; Qx[X*X]; invlamT[X*Y].  The preconditioner of
    the large-grid CG solve (sol_karman_step_fwd_large_cg), which takes any obstacle."""
    Qy, Qx = dst_matrix(Y), dst_matrix(X)
    lam = (2 - 2 * np.cos(np.pi * np.arange(1, Y + 1) / (Y + 1)))[:, None] + (2 - 2 * np.cos(np.pi * np.arange(1, X + 1) / (X + 1)))[None, :]
    header = np.zeros(FD_HEADER, dtype=np.int32)
    header[:3] = [FD_MAGIC, Y, X]
    return np.concatenate([header.view(np.float32), Qy.astype(np.float32).ravel(), Qx.astype(np.float32).ravel(),
                           (1.0 / lam).T.astype(np.float32).ravel()])


def direct_solve_reference(blob, b):
    """float64 numpy restatement of the device algorithm on the blob (used by the CPU tests)."""
    hdr = blob[:FD_HEADER].view(np.int32)
    assert hdr[0] == FD_MAGIC
    Y, X, wy0, wx0, nS, SP = (int(v) for v in hdr[1:7])
    FD_WIN = int(hdr[7])
    o = FD_HEADER
    Qy = blob[o:o + Y * Y].astype(np.float64).reshape(Y, Y); o += Y * Y
    Qx = blob[o:o + X * X].astype(np.float64).reshape(X, X); o += X * X
    il = blob[o:o + X * Y].astype(np.float64).reshape(X, Y).T; o += X * Y
    KpT = blob[o:o + SP * SP].astype(np.float64).reshape(SP, SP); o += SP * SP
    sidx = blob[o:o + SP].view(np.int32)
    T2 = (Qy @ b @ Qx) * il
    x0w = Qy[wy0:wy0 + FD_WIN, :] @ T2 @ Qx[:, wx0:wx0 + FD_WIN]
    xs = np.where(sidx >= 0, x0w.ravel()[np.maximum(sidx, 0)], 0.0)
    c = KpT.T @ xs
    w2 = np.zeros(FD_WIN * FD_WIN)
    w2[sidx[sidx >= 0]] = -c[sidx >= 0]
    w2 = w2.reshape(FD_WIN, FD_WIN)
    T2 = T2 + il * (Qy[:, wy0:wy0 + FD_WIN] @ w2 @ Qx[wx0:wx0 + FD_WIN, :])
    return Qy @ T2 @ Qx


_open_perturbation, _open_direct_solver_blob, _open_box_solver_blob, _open_direct_solve_reference = (
    _perturbation, direct_solver_blob, box_solver_blob, direct_solve_reference)


def _is_open(periodic, dtype=np.float32):
    return not any(_periodic_arg(periodic)) and dtype == np.float32


@functools.wraps(_open_perturbation)
def _perturbation(active, periodic=(False, False)):
    return _open_perturbation(active) if _is_open(periodic) else _general_perturbation(active, periodic)


@functools.wraps(_open_direct_solver_blob)
def direct_solver_blob(active, max_window=FD_WIN, periodic=(False, False), dtype=np.float32):
    if _is_open(periodic, dtype):
        return _open_direct_solver_blob(active, max_window)
    return _general_direct_solver_blob(active, max_window, periodic, dtype)


@functools.wraps(_open_box_solver_blob)
def box_solver_blob(Y, X, periodic=(False, False), dtype=np.float32):
    return _open_box_solver_blob(Y, X) if _is_open(periodic, dtype) else _general_box_solver_blob(Y, X, periodic, dtype)


@functools.wraps(_open_direct_solve_reference)
def direct_solve_reference(blob, b):
    if blob.dtype == np.float32 and _ints(blob[:FD_HEADER])[5] != 0:
        return _open_direct_solve_reference(blob, b)
    return _general_direct_solve_reference(blob, b)


for _f, _g in ((_perturbation, _general_perturbation), (direct_solver_blob, _general_direct_solver_blob),
               (box_solver_blob, _general_box_solver_blob), (direct_solve_reference, _general_direct_solve_reference)):
    _f.__doc__ = _g.__doc__          # (the dispatcher documents the whole keyword set; __wrapped__ stays the open builder)
