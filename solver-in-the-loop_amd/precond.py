"""Host-side setup of the two-level CG preconditioner of the fused solver step.

M^-1 = D^-1 + P (P^T M P)^-1 P^T for M = -A, the SPD pressure matrix of the scene
(PhiFlow sparse_pressure_matrix semantics: diagonal = number of accessible neighbours (>= 1),
off-diagonal -1 between two active cells, p = 0 outside the OPEN domain), with P the
piecewise-constant prolongation of 8x8-cell aggregates restricted to active cells.  Only the dense
coarse inverse (nc x nc, nc = Y*X/64) is computed here, once per scene geometry, in float64; the
device kernels apply it inside their CG loop (csrc/karman_step.hip: pcg_solve).  It changes the
iteration count (about 235 -> 56 at 128x64), not the converged solution.
"""
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


def scene_matrix(active):
    """Dense float64 M = -A of the scene (small grids / setup only)."""
    act = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
    Y, X = act.shape
    N = Y * X
    acc = np.pad(act, 1, mode="edge")
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
    return M


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


def box_solve_reference(blob, b):
    """float64 numpy restatement of G b on a box_solver_blob (b [Y, X])."""
    hdr = blob[:FD_HEADER].view(np.int32)
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


def scattered_solver_blob(active, dtype=np.float32):
    """float32 blob of the scattered direct solver (SceneMasks(pressure_solver="direct_scattered"), large grids only), or None when
    the scene has no perturbation, more than 4096 support cells, or an ill-conditioned capacitance system (cond > 1e6).

    layout (32-bit words): header[16] = {magic "FDS1", Y, X, nR, nC, nS, SP, RP, CP, ...} (RP, CP = |R|, |C| padded to multiples of
    4, SP = nS padded to a multiple of 64);  Qy[Y*Y];  Qx[X*X];  invlamT[X*Y];  zero words up to a multiple of 4 (16-byte rows of
    K'^T);  KpT[SP*SP] (K' = E_SS (I + G_SS E_SS)^-1 transposed, zero padded);  rows[RP], cols[CP] int32 (-1 = padding);
    sidx[SP] int32 (row-slot * CP + column-slot of a support cell in X0 / W2, -1 = padding);  the slabs the GEMMs read, zero in the
    padding:  QyR[RP*Y] = Qy[R,:];  QxC[X*CP] = Qx[:,C];  QyRt[Y*RP] = Qy[:,R];  QxCr[CP*X] = Qx[C,:].
    dtype=np.float64 (host checks only, never a device blob): the same words unrounded, integers stored as float64 values."""
    act = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
    Y, X = act.shape
    ent = _perturbation(act)
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
    Qy, Qx = dst_matrix(Y), dst_matrix(X)
    lam = (2 - 2 * np.cos(np.pi * np.arange(1, Y + 1) / (Y + 1)))[:, None] + (2 - 2 * np.cos(np.pi * np.arange(1, X + 1) / (X + 1)))[None, :]
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
