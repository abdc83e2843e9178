"""Host-side setup of the DIRECT pressure solver of the karman-3d step (csrc/karman3d.hip).

Same construction as precond.direct_solver_blob, one axis more.  On the OPEN box without obstacle the pressure matrix
M = -A (PhiFlow sparse_pressure_matrix semantics: diagonal = number of accessible neighbours, -1 between two active cells,
p = 0 outside) is the 7-point Dirichlet Laplacian M_r = T_Y (x) I (x) I + I (x) T_X (x) I + I (x) I (x) T_Z, diagonalised by
the orthonormal sine transforms Q_Y, Q_X, Q_Z.  The obstacle changes M only on the set S of obstacle cells and their
neighbours, M = M_r + U_S E_SS U_S^T, hence

    x = G (b - U_S E_SS x_S),    x_S = (I + G_SS E_SS)^-1 (G b)_S,    G = M_r^-1

i.e. two applications of G (three sine transforms each way = batched fp32 GEMMs on the device) and one dense |S| x |S|
product: NO iteration, the solution equals the converged CG solution up to fp32 round-off.  Everything here is float64
numpy, computed once per scene geometry (about a second at 128 x 64 x 64 with the sphere: |S| = 1 744).
"""
import numpy as np

from .precond import dst_matrix, hartley_matrix

FD3_MAGIC = 0x46443333          # "FD33"
FD3_HEADER = 16                 # int32 words
FD3_MAX_S = 8192                # largest padded perturbation set the device kernels take


def _accessible_diag(act):
    acc = np.pad(act, 1, mode="edge")
    n = np.zeros_like(act)
    for ax in range(3):
        lo = [slice(1, -1)] * 3
        hi = [slice(1, -1)] * 3
        lo[ax] = slice(0, -2)
        hi[ax] = slice(2, None)
        n += acc[tuple(lo)] + acc[tuple(hi)]
    return np.maximum(n, 1.0)


def _perturbation3d(active):
    """Sparse difference E = M - M_r as (rows, cols, vals) over global cell indices."""
    act = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
    Y, X, Z = act.shape
    idx = np.arange(Y * X * Z).reshape(Y, X, Z)
    diag = _accessible_diag(act)
    sel = diag != 6.0
    rows, cols, vals = [idx[sel]], [idx[sel]], [diag[sel] - 6.0]
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax] = slice(0, -1)
        hi[ax] = slice(1, None)
        a = act[tuple(lo)] * act[tuple(hi)]
        sel = a != 1.0
        r, c = idx[tuple(lo)][sel], idx[tuple(hi)][sel]
        rows += [r, c]; cols += [c, r]; vals += [1.0 - a[sel], 1.0 - a[sel]]        # M has -a, M_r has -1
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)


def rect_eigenvalues(Y, X, Z):
    ev = lambda n: 2.0 - 2.0 * np.cos(np.pi * np.arange(1, n + 1) / (n + 1))
    return ev(Y)[:, None, None] + ev(X)[None, :, None] + ev(Z)[None, None, :]


def _green_on_window(Qy, Qx, Qz, lam, wy, wx, wz):
    """G = M_r^-1 restricted to the box window wy x wx x wz (index arrays), as a 6-index array
    Gw[a, a', b, b', c, c'] = G[(wy[a], wx[b], wz[c]), (wy[a'], wx[b'], wz[c'])], contracted one axis at a time."""
    Wy, Wx, Wz = Qy[wy, :], Qx[wx, :], Qz[wz, :]
    H = np.einsum("am,jm,mce->ajce", Wy, Wy, 1.0 / lam, optimize=True)            # y axis contracted
    H = np.einsum("bc,ic,ajce->ajbie", Wx, Wx, H, optimize=True)                   # x axis
    return np.einsum("ke,le,ajbie->ajbikl", Wz, Wz, H, optimize=True)              # z axis


def direct_solver_blob3d(active):
    """float32 blob consumed by sol_karman3d_cfg.direct, or None when the scene does not qualify (no obstacle at all is
    fine: nS = 0; too many perturbed cells, or an ill-conditioned capacitance system, are not).

    layout (32-bit words): header[16] = {magic, Y, X, Z, nS, SP, ...};  Qy[Y*Y];  Qx[X*X];  Qz[Z*Z];  invlam[Y*X*Z];
    KpT[SP*SP] (K' = E_SS (I + G_SS E_SS)^-1, stored transposed, zero padded);  sidx[SP] int32 (global cell index
    (j*X + i)*Z + k, -1 = padding)."""
    act = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
    Y, X, Z = act.shape
    rows, cols, vals = _perturbation3d(act)
    S = np.unique(rows)
    nS = len(S)
    SP = (nS + 63) // 64 * 64
    if SP > FD3_MAX_S:
        return None
    Qy, Qx, Qz = dst_matrix(Y), dst_matrix(X), dst_matrix(Z)
    lam = rect_eigenvalues(Y, X, Z)
    KpT = np.zeros((SP, SP))
    if nS:
        js, is_, ks = S // (X * Z), (S // Z) % X, S % Z
        wy, wx, wz = (np.arange(v.min(), v.max() + 1) for v in (js, is_, ks))
        if (len(wy) * len(wx) * len(wz)) ** 2 > 6e7:
            return None                                   # (an extruded obstacle spanning the domain: not a window-sized perturbation)
        Gw = _green_on_window(Qy, Qx, Qz, lam, wy, wx, wz)
        a, b, c = js - wy[0], is_ - wx[0], ks - wz[0]
        GSS = Gw[a[:, None], a[None, :], b[:, None], b[None, :], c[:, None], c[None, :]]
        pos = np.full(Y * X * Z, -1, dtype=np.int64)
        pos[S] = np.arange(nS)
        ESS = np.zeros((nS, nS))
        np.add.at(ESS, (pos[rows], pos[cols]), vals)
        cap = np.eye(nS) + GSS @ ESS
        if np.linalg.cond(cap) > 1e6:
            return None
        KpT[:nS, :nS] = (ESS @ np.linalg.inv(cap)).T
    sidx = np.full(SP, -1, dtype=np.int32)
    sidx[:nS] = S.astype(np.int32)
    header = np.zeros(FD3_HEADER, dtype=np.int32)
    header[:6] = [FD3_MAGIC, Y, X, Z, nS, SP]
    parts = [header.view(np.float32), Qy.astype(np.float32).ravel(), Qx.astype(np.float32).ravel(), Qz.astype(np.float32).ravel(),
             (1.0 / lam).astype(np.float32).ravel(), KpT.astype(np.float32).ravel(), sidx.view(np.float32)]
    return np.concatenate(parts)


# ---------------------------------------------------------------------------------------------------------------------
# obstacles extruded along z (the cylinder of the wake): active[j, i, k] = a2[j, i] for every k.  The pressure matrix then
# separates along z,
#
#     M = M2' (x) I_Z + diag(a2) (x) T_Z
#
# (M2': the in-plane matrix, diagonal = in-plane accessible neighbours, at least 1 on a solid cell; T_Z: the Dirichlet
# tridiagonal (2, -1): every fluid cell has two accessible z neighbours, every solid cell is decoupled), and Q_Z diagonalises
# T_Z with mu_m = 2 - 2 cos(pi (m + 1) / (Z + 1)).  In the z-spectral basis mode m sees M_m = M2' + mu_m diag(a2) against the
# empty box's T_Y (+) T_X + mu_m, i.e. the perturbation
#
#     E_m = E2 - mu_m diag(1 - a2),    E2 = M2' - (T_Y (+) T_X)
#
# on the 2-D set S2 of obstacle cells and their in-plane neighbours, and the identity at the head of this file holds mode by
# mode: K'_m = E_m,SS (I + G_m,SS E_m,SS)^-1 with G_m = (T_Y (+) T_X + mu_m)^-1.  The dense |S| x |S| product (|S| = |S2| Z)
# becomes Z products of size |S2| between two sine transforms along z of the support columns.
# ---------------------------------------------------------------------------------------------------------------------
FD3E_MAGIC = 0x46443345         # "FD3E"
FD3E_MAX_Z = 128                # the correction kernels hold Q_Z (Z x Z floats) in LDS
FD3E_MAX_SP2 = 1024             # largest padded in-plane set
FD3E_MAX_WORDS = 1 << 26        # Z * SP2^2, the words of the per-mode matrices (256 MB)
FD3E_MAX_COND = 1e6             # the dense blob's rule, per mode


def _perturbation2d(a2):
    """(S2, E2_SS, solid_S): the in-plane set (flat j*X + i, sorted), E2 = M2' - (T_Y (+) T_X) on it, and 1 - a2 on it"""
    Y, X = a2.shape
    acc = np.pad(a2, 1, mode="edge")
    n2 = acc[:-2, 1:-1] + acc[2:, 1:-1] + acc[1:-1, :-2] + acc[1:-1, 2:]
    d2 = np.where(a2 != 0, n2, np.maximum(n2, 1.0))
    idx = np.arange(Y * X).reshape(Y, X)
    sel = (d2 != 4.0) | (a2 == 0)
    rows, cols, vals = [idx[sel]], [idx[sel]], [d2[sel] - 4.0]
    for ax in range(2):
        lo = [slice(None)] * 2
        hi = [slice(None)] * 2
        lo[ax] = slice(0, -1)
        hi[ax] = slice(1, None)
        a = a2[tuple(lo)] * a2[tuple(hi)]
        sel = a != 1.0
        r, c = idx[tuple(lo)][sel], idx[tuple(hi)][sel]
        rows += [r, c]; cols += [c, r]; vals += [1.0 - a[sel], 1.0 - a[sel]]
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    S2 = np.unique(rows)
    pos = np.full(Y * X, -1, dtype=np.int64)
    pos[S2] = np.arange(len(S2))
    E2 = np.zeros((len(S2), len(S2)))
    np.add.at(E2, (pos[rows], pos[cols]), vals)
    return S2, E2, 1.0 - a2.ravel()[S2]


def extruded_solver_refusal3d(active):
    """Why extruded_solver_blob3d refuses `active` (a sentence), or None where it builds.  Cheap: no matrix is formed, so the
    conditioning rule is not evaluated here."""
    act = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
    Y, X, Z = act.shape
    if not np.all(act == act[:, :, :1]):
        return "the mask depends on z (the extruded solve takes masks with active[j, i, k] = a2[j, i] for every k)"
    if np.all(act != 0):
        return "the scene has no obstacle (no solid cell: that scene is the plain direct solve's, nS = 0)"
    if Z > FD3E_MAX_Z:
        return "Z = %d is beyond the %d the correction kernels take" % (Z, FD3E_MAX_Z)
    nS2 = len(_perturbation2d(act[:, :, 0])[0])
    SP2 = (nS2 + 31) // 32 * 32
    if SP2 > FD3E_MAX_SP2 or SP2 > Y * X or Z * SP2 * SP2 > FD3E_MAX_WORDS:
        return ("the obstacle is beyond the size cap (in-plane set %d, padded %d: at most %d, at most Y X = %d, and Z SP2^2 <= 2^26 words)"
                % (nS2, SP2, FD3E_MAX_SP2, Y * X))
    return None


def extruded_solver_blob3d(active, why=None, periodic=False):
    """float32 blob of the direct solve for an obstacle extruded along z, or None where the scene does not qualify: the mask
    depends on z; there is no solid cell (the plain direct solve's scene, nS = 0); a mode's capacitance system has a condition
    number beyond 1e6; Z > 128; or the size is beyond the cap: SP2 <= 1024, SP2 <= Y X (the device's scratch) and
    Z SP2^2 <= 2^26 words (256 MB).  `why`: a list that receives the reason of a refusal.

    layout (32-bit words): header[16] = {magic "FD3E", Y, X, Z, nS2, SP2, ...};  Qy[Y*Y];  Qx[X*X];  Qz[Z*Z];  invlam[Y*X*Z]
    (the positions of the dense blob: the empty-box solve and the CG preconditioner read either);  KpT[Z][SP2][SP2] (K'_m of
    z mode m, stored transposed, zero padded; SP2 = nS2 rounded up to 32);  sidx2[SP2] int32 (in-plane cell index j*X + i,
    -1 = padding).  G_m,SS is built from the nS2 rows of Qy (x) Qx, never as a (Y X)^2 matrix.

    periodic=True: the z axis is periodic.  T_Z is then the circulant second difference, Qz = hartley_matrix(Z), mu_m = 2 - 2 cos(2 pi m /
    Z) -- mode 0 (mu = 0) is the 2-D problem of the plane -- and header word 6 = PERIODIC_Z; the construction, the conditioning rule and
    the size caps are the open one's."""
    say = why.append if why is not None else (lambda s: None)
    reason = extruded_solver_refusal3d(active)
    if reason is not None:
        say(reason)
        return None
    act = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
    Y, X, Z = act.shape
    S2, E2, solid = _perturbation2d(act[:, :, 0])
    nS2 = len(S2)
    SP2 = (nS2 + 31) // 32 * 32
    Qy, Qx, Qz = dst_matrix(Y), dst_matrix(X), (hartley_matrix(Z) if periodic else dst_matrix(Z))
    lam = periodic_eigenvalues3d(Y, X, Z) if periodic else rect_eigenvalues(Y, X, Z)
    R = (Qy[S2 // X, :, None] * Qx[S2 % X, None, :]).reshape(nS2, Y * X)          # rows S2 of Qy (x) Qx
    KpT = np.zeros((Z, SP2, SP2))
    eye = np.eye(nS2)
    for m in range(Z):
        mu = 2.0 - 2.0 * np.cos(2.0 * np.pi * m / Z) if periodic else 2.0 - 2.0 * np.cos(np.pi * (m + 1) / (Z + 1))
        Em = E2 - mu * np.diag(solid)
        GSS = (R / lam[:, :, m].reshape(1, Y * X)) @ R.T
        cap = eye + GSS @ Em
        cond = np.linalg.cond(cap)
        if not cond <= FD3E_MAX_COND:
            say("the capacitance system of z mode %d is ill conditioned (condition number %.3g, at most %.0e)" % (m, cond, FD3E_MAX_COND))
            return None
        KpT[m, :nS2, :nS2] = (Em @ np.linalg.inv(cap)).T
    sidx2 = np.full(SP2, -1, dtype=np.int32)
    sidx2[:nS2] = S2.astype(np.int32)
    header = np.zeros(FD3_HEADER, dtype=np.int32)
    header[:6] = [FD3E_MAGIC, Y, X, Z, nS2, SP2]
    if periodic:
        header[6] = PERIODIC_Z
    parts = [header.view(np.float32), Qy.astype(np.float32).ravel(), Qx.astype(np.float32).ravel(), Qz.astype(np.float32).ravel(),
             (1.0 / lam).astype(np.float32).ravel(), KpT.astype(np.float32).ravel(), sidx2.view(np.float32)]
    return np.concatenate(parts)


def extruded_solve_reference3d(blob, b):
    """float64 numpy restatement of the device algorithm on the extruded blob: b [Y,X,Z] -> x with M x = b (CPU tests)."""
    hdr = blob[:FD3_HEADER].view(np.int32)
    assert hdr[0] == FD3E_MAGIC
    Y, X, Z, nS2, SP2 = (int(v) for v in hdr[1:6])
    o = FD3_HEADER
    Qy = blob[o:o + Y * Y].astype(np.float64).reshape(Y, Y); o += Y * Y
    Qx = blob[o:o + X * X].astype(np.float64).reshape(X, X); o += X * X
    Qz = blob[o:o + Z * Z].astype(np.float64).reshape(Z, Z); o += Z * Z
    il = blob[o:o + Y * X * Z].astype(np.float64).reshape(Y, X, Z); o += Y * X * Z
    KpT = blob[o:o + Z * SP2 * SP2].astype(np.float64).reshape(Z, SP2, SP2); o += Z * SP2 * SP2
    sidx2 = blob[o:o + SP2].view(np.int32)
    q3 = lambda t: np.einsum("am,bc,ke,mce->abk", Qy, Qx, Qz, t, optimize=True)
    G = lambda t: q3(q3(t) * il)
    g = G(b).reshape(Y * X, Z)
    ok = sidx2 >= 0
    xs = np.where(ok[:, None], g[np.maximum(sidx2, 0)], 0.0)           # support columns [SP2][Z]
    xh = xs @ Qz                                                        # 1. along z into the spectral basis
    ch = np.einsum("mqs,qm->sm", KpT, xh)                               # 2. mode by mode: c^[:, m] = K'_m x^[:, m]
    c = ch @ Qz                                                         # 3. back
    r = np.array(b, dtype=np.float64).reshape(Y * X, Z)
    r[sidx2[ok]] -= c[ok]                                               # 4.
    return G(r.reshape(Y, X, Z))


def direct_solve_reference3d(blob, b):
    """float64 numpy restatement of the device algorithm on the blob: b [Y,X,Z] -> x with M x = b (CPU tests)."""
    hdr = blob[:FD3_HEADER].view(np.int32)
    assert hdr[0] == FD3_MAGIC
    Y, X, Z, nS, SP = (int(v) for v in hdr[1:6])
    o = FD3_HEADER
    Qy = blob[o:o + Y * Y].astype(np.float64).reshape(Y, Y); o += Y * Y
    Qx = blob[o:o + X * X].astype(np.float64).reshape(X, X); o += X * X
    Qz = blob[o:o + Z * Z].astype(np.float64).reshape(Z, Z); o += Z * Z
    il = blob[o:o + Y * X * Z].astype(np.float64).reshape(Y, X, Z); o += Y * X * Z
    KpT = blob[o:o + SP * SP].astype(np.float64).reshape(SP, SP); o += SP * SP
    sidx = blob[o:o + SP].view(np.int32)
    q3 = lambda t: np.einsum("am,bc,ke,mce->abk", Qy, Qx, Qz, t, optimize=True)
    G = lambda t: q3(q3(t) * il)
    g = G(b)
    if nS:
        xs = np.where(sidx >= 0, g.ravel()[np.maximum(sidx, 0)], 0.0)
        c = KpT.T @ xs
        b = b.copy().ravel()
        b[sidx[sidx >= 0]] -= c[sidx >= 0]
        g = G(b.reshape(Y, X, Z))
    return g


# ---------------------------------------------------------------------------------------------------------------------
# a PERIODIC z axis (Scene3D(boundaries="periodic-z"), csrc/karman3d_periodic.hip).  Cell (j, i, Z - 1) is the neighbour of
# (j, i, 0): along z the accessible mask wraps instead of taking the edge value, and the empty box's T_Z is the circulant
# second difference, diagonalised by the Hartley matrix (symmetric, its own inverse: the device's transform launches assume
# nothing else of Q_Z) with the eigenvalues 2 - 2 cos(2 pi m / Z).  The z-constant mode has the eigenvalue 0 along z, but the
# two open axes hold it down: lam > 0 everywhere, the solve is non-singular.  The builders of the open box above keep their
# text (a test pins it); these stand beside them.  Header word 6 carries the axes: PERIODIC_Z = 8; 2 and 4 are reserved for y
# and x, which nothing builds.
# ---------------------------------------------------------------------------------------------------------------------
PERIODIC_Y3, PERIODIC_X3, PERIODIC_Z = 2, 4, 8


def periodic_eigenvalues3d(Y, X, Z):
    """rect_eigenvalues with the z axis periodic"""
    ev = lambda n: 2.0 - 2.0 * np.cos(np.pi * np.arange(1, n + 1) / (n + 1))
    return ev(Y)[:, None, None] + ev(X)[None, :, None] + (2.0 - 2.0 * np.cos(2.0 * np.pi * np.arange(Z) / Z))[None, None, :]


def _accessible3d(act, periodic):
    """the accessible mask with one ring around the domain: the edge value along an open axis, the wrapped plane along z when periodic"""
    acc = np.pad(act, ((1, 1), (1, 1), (0, 0)), mode="edge")
    return np.pad(acc, ((0, 0), (0, 0), (1, 1)), mode="wrap" if periodic else "edge")


def _z_pairs(idx, act, periodic):
    """(lo, hi, a) per axis: the index arrays of the two cells of every cell pair and the product of their active values; along a periodic
    z the seam pair (Z - 1, 0) is one of them"""
    out = []
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax] = slice(0, -1)
        hi[ax] = slice(1, None)
        out.append((idx[tuple(lo)], idx[tuple(hi)], act[tuple(lo)] * act[tuple(hi)]))
    if periodic:
        out.append((idx[:, :, -1], idx[:, :, 0], act[:, :, -1] * act[:, :, 0]))
    return out


def scene_matrix3d(active, periodic=False):
    """The pressure matrix M = -A of a scene as a scipy.sparse CSC matrix over the cells (j*X + i)*Z + k (tests; .toarray() for a dense
    one): diagonal = the number of accessible neighbours (at least 1), -1 between two active neighbours.  periodic: the z axis wraps."""
    import scipy.sparse as sp
    act = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
    Y, X, Z = act.shape
    acc = _accessible3d(act, periodic)
    n = (acc[:-2, 1:-1, 1:-1] + acc[2:, 1:-1, 1:-1] + acc[1:-1, :-2, 1:-1] + acc[1:-1, 2:, 1:-1] + acc[1:-1, 1:-1, :-2] + acc[1:-1, 1:-1, 2:])
    idx = np.arange(Y * X * Z).reshape(Y, X, Z)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.maximum(n, 1.0).ravel()]
    for lo, hi, a in _z_pairs(idx, act, periodic):
        rows += [lo.ravel(), hi.ravel()]; cols += [hi.ravel(), lo.ravel()]; vals += [-a.ravel(), -a.ravel()]
    N = Y * X * Z
    return sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))


def _perturbation3d_pz(act):
    """_perturbation3d with the z axis periodic: the accessible mask wrapped along z, the seam couplings among the pairs"""
    Y, X, Z = act.shape
    idx = np.arange(Y * X * Z).reshape(Y, X, Z)
    acc = _accessible3d(act, True)
    n = (acc[:-2, 1:-1, 1:-1] + acc[2:, 1:-1, 1:-1] + acc[1:-1, :-2, 1:-1] + acc[1:-1, 2:, 1:-1] + acc[1:-1, 1:-1, :-2] + acc[1:-1, 1:-1, 2:])
    diag = np.maximum(n, 1.0)
    sel = diag != 6.0
    rows, cols, vals = [idx[sel]], [idx[sel]], [diag[sel] - 6.0]
    for lo, hi, a in _z_pairs(idx, act, True):
        sel = a != 1.0
        rows += [lo[sel], hi[sel]]; cols += [hi[sel], lo[sel]]; vals += [1.0 - a[sel], 1.0 - a[sel]]
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)


def periodic_solver_blob3d(active, why=None):
    """direct_solver_blob3d for a z-periodic scene: the same layout ("FD33") with Qz = hartley_matrix(Z), the periodic eigenvalues, the
    perturbation of _perturbation3d_pz and header word 6 = PERIODIC_Z.  None where the open builder's rules refuse (`why`: a list that
    receives the sentence): more than FD3_MAX_S perturbed cells, a perturbation beyond one window -- an obstacle lying across the seam
    spans the axis, as does an extruded one (extruded_solver_blob3d(periodic=True) takes that) -- or an ill-conditioned capacitance system."""
    say = why.append if why is not None else (lambda s: None)
    act = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
    Y, X, Z = act.shape
    rows, cols, vals = _perturbation3d_pz(act)
    S = np.unique(rows)
    nS = len(S)
    SP = (nS + 63) // 64 * 64
    if SP > FD3_MAX_S or 8 * SP > Y * X * Z:
        say("the obstacle perturbs %d cells (padded %d): at most %d and at most an eighth of the grid" % (nS, SP, FD3_MAX_S))
        return None
    Qy, Qx, Qz = dst_matrix(Y), dst_matrix(X), hartley_matrix(Z)
    lam = periodic_eigenvalues3d(Y, X, Z)
    KpT = np.zeros((SP, SP))
    if nS:
        js, is_, ks = S // (X * Z), (S // Z) % X, S % Z
        wy, wx, wz = (np.arange(v.min(), v.max() + 1) for v in (js, is_, ks))
        if (len(wy) * len(wx) * len(wz)) ** 2 > 6e7:
            say("the perturbation does not fit one window (%d x %d x %d cells; an obstacle across the z seam, or extruded along z, spans the axis)"
                % (len(wy), len(wx), len(wz)))
            return None
        Gw = _green_on_window(Qy, Qx, Qz, lam, wy, wx, wz)
        a, b, c = js - wy[0], is_ - wx[0], ks - wz[0]
        GSS = Gw[a[:, None], a[None, :], b[:, None], b[None, :], c[:, None], c[None, :]]
        pos = np.full(Y * X * Z, -1, dtype=np.int64)
        pos[S] = np.arange(nS)
        ESS = np.zeros((nS, nS))
        np.add.at(ESS, (pos[rows], pos[cols]), vals)
        cap = np.eye(nS) + GSS @ ESS
        cond = np.linalg.cond(cap)
        if not cond <= 1e6:
            say("the capacitance system is ill conditioned (condition number %.3g, at most 1e6)" % cond)
            return None
        KpT[:nS, :nS] = (ESS @ np.linalg.inv(cap)).T
    sidx = np.full(SP, -1, dtype=np.int32)
    sidx[:nS] = S.astype(np.int32)
    header = np.zeros(FD3_HEADER, dtype=np.int32)
    header[:7] = [FD3_MAGIC, Y, X, Z, nS, SP, PERIODIC_Z]
    parts = [header.view(np.float32), Qy.astype(np.float32).ravel(), Qx.astype(np.float32).ravel(), Qz.astype(np.float32).ravel(),
             (1.0 / lam).astype(np.float32).ravel(), KpT.astype(np.float32).ravel(), sidx.view(np.float32)]
    return np.concatenate(parts)


def blob_periodic_bits3d(blob):
    """header word 6 of a blob: 0 (open) or PERIODIC_Z"""
    return int(np.asarray(blob[:FD3_HEADER]).view(np.int32)[6])


def periodic_solve_reference3d(blob, b):
    """float64 numpy restatement of the device algorithm on a z-periodic blob of either layout: b [Y,X,Z] -> x with M x = b (CPU tests).
    The device runs the open blobs' launches on the periodic blob's tables; so does this."""
    hdr = np.asarray(blob[:FD3_HEADER]).view(np.int32)
    assert hdr[6] == PERIODIC_Z, "not a z-periodic blob (header word 6 = %d)" % hdr[6]
    return (extruded_solve_reference3d if hdr[0] == FD3E_MAGIC else direct_solve_reference3d)(blob, np.asarray(b, dtype=np.float64))
