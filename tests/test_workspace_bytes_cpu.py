"""Every solver workspace size function against a recorded table (workspace_bytes_table.json, next to this file), CPU side: a size
function is its layout called with a NULL workspace (csrc/carve.hpp), so a layout that moves a buffer or loses a slack term changes a
number here.  The table was recorded from the library as it stood BEFORE the layouts moved onto the shared carver:
    python tests/test_workspace_bytes_cpu.py --record        (rewrites the table from the library in the tree)
Headers are host arrays in precond.py's formats (FD02: one window, FDS1: scattered); no device is needed."""
import ctypes as C
import json
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sol_amd
from sol_amd import _lib, ops, precond

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "workspace_bytes_table.json")
GRIDS_2D = ((1, 16, 16), (2, 48, 80), (3, 100, 72), (1, 256, 128), (6, 128, 64), (2, 33, 47))
GRIDS_3D = ((1, 8, 8, 8), (2, 32, 16, 16), (1, 128, 64, 64), (3, 20, 10, 12))
GRIDS_BURGERS = ((1, 128, 128), (2, 96, 160), (3, 65, 71), (1, 1024, 1024))
FAKE = 4096          # a device pointer that is never dereferenced: cfg.direct != NULL selects the direct layouts
# the table holds one list per grid and solver, in this order: FUNCS_2D, then FUNCS_2D_FOR for every header of headers_2d by sorted name
FUNCS_2D = ("sol_karman_step_large_workspace_bytes", "sol_karman_step_large_cg_workspace_bytes", "sol_karman_step_bwd_large_workspace_bytes",
            "sol_karman_density_bwd_workspace_bytes", "sol_karman_density_bwd_re_workspace_bytes")
FUNCS_2D_FOR = ("sol_karman_step_large_workspace_bytes_for", "sol_karman_step_bwd_large_workspace_bytes_for",
                "sol_karman_step_bwd_large_re_workspace_bytes_for")
FUNCS_3D = ("sol_karman3d_step_workspace_bytes", "sol_karman3d_step_bwd_workspace_bytes", "sol_karman3d_step_bwd_re_workspace_bytes",
            "sol_karman3d_density_bwd_workspace_bytes", "sol_karman3d_density_bwd_re_workspace_bytes")


def headers_2d(Y, X):
    """name -> host header (None: no header) of every solver variant; the padded counts RP = 60, CP = 76 are test_scattered_direct_cpu.py's"""
    h = {"none": None}
    for win in (16, 32, 64):
        fd = np.zeros(16, dtype=np.int32)
        fd[:8] = [precond.FD_MAGIC, Y, X, 0, 0, win * win // 4, (win * win // 4 + 63) // 64 * 64, win]
        h["fd02_win%d" % win] = fd
    for RP, CP in ((60, 76), (4, 4), (16, 12)):
        sc = np.zeros(16, dtype=np.int32)
        sc[:9] = [precond.FDS_MAGIC, Y, X, RP - 1, CP - 2, 1194, 1216, RP, CP]
        h["fds1_rp%d_cp%d" % (RP, CP)] = sc
    return h


def sizes(lib):
    hp = lambda h: None if h is None else h.ctypes.data_as(C.c_void_p)
    out = {"2d": {}, "3d": {}, "burgers": {}}
    for B, Y, X in GRIDS_2D:
        row = out["2d"]["%d,%d,%d" % (B, Y, X)] = {}
        for direct in (False, True):
            cfg = ops.karman_cfg(B, Y, X, 100.0 / X)
            if direct:
                cfg.direct, cfg.direct_n = FAKE, 1 << 30
            r = row["direct" if direct else "cg"] = [getattr(lib, f)(C.byref(cfg)) for f in FUNCS_2D]
            for name, h in sorted(headers_2d(Y, X).items()):
                r += [getattr(lib, f)(C.byref(cfg), hp(h)) for f in FUNCS_2D_FOR]
    for B, Y, X, Z in GRIDS_3D:
        row = out["3d"]["%d,%d,%d,%d" % (B, Y, X, Z)] = {}
        for solver in (0, 1):
            cfg = _lib.Karman3DCfg(B, Y, X, Z, 100.0 / X, 1.0, float(X), 0, 0, FAKE, 1 << 20, solver, 10, 1e-5, 0.0, None)
            row["pressure_solver=%d" % solver] = [getattr(lib, f)(C.byref(cfg)) for f in FUNCS_3D]
    for B, Y, X in GRIDS_BURGERS:
        cfg = _lib.BurgersCfg(B, Y, X, 1.0, 0.1)
        out["burgers"]["%d,%d,%d" % (B, Y, X)] = lib.sol_burgers_step_bwd_large_workspace_bytes(C.byref(cfg))
    return out


def test_every_size_function_returns_the_recorded_bytes():
    with open(TABLE) as f:
        want = json.load(f)
    got = sizes(sol_amd.load())
    assert sorted(got) == sorted(want)
    for family in want:
        assert sorted(got[family]) == sorted(want[family]), family
        for grid in want[family]:
            assert got[family][grid] == want[family][grid], (family, grid)


def test_a_null_cfg_sizes_to_zero():
    lib = sol_amd.load()
    for f in FUNCS_2D + FUNCS_3D + ("sol_burgers_step_bwd_large_workspace_bytes",):
        assert getattr(lib, f)(None) == 0, f
    for f in FUNCS_2D_FOR:
        assert getattr(lib, f)(None, None) == 0, f


def test_the_adv_size_functions_with_advection_0_return_the_plain_bytes_and_the_three_python_sizers_select_by_mode():
    """ops.large_workspace_bytes / large_bwd_workspace_bytes / density_bwd_workspace_bytes are served by the _adv size functions in every
    mode: with advection = 0 those must return the plain functions' bytes, for a direct, a scattered-direct and a CG cfg at the three
    ragged shapes of the large-grid tests.  (The SAVED _adv form with advection = 0 is smaller than the plain step's scratch, which the
    plain saved step is sized with: the Python sizer takes it under mac_cormack only.)"""
    import types
    lib = sol_amd.load()
    hp = lambda h: None if h is None else h.ctypes.data_as(C.c_void_p)
    mc = ops.StepPhysics.of(advection="mac_cormack", correction_strength=0.5)
    for Y, X in ((130, 65), (144, 72), (160, 80)):
        hs = headers_2d(Y, X)
        for name in ("fd02_win16", "fd02_win64", "fds1_rp60_cp76", "fds1_rp16_cp12", "none"):
            h = hs[name]
            cfg = ops.karman_cfg(2, Y, X, 100.0 / X)
            if h is not None:
                cfg.direct, cfg.direct_n = FAKE, 1 << 30
            r, where = C.byref(cfg), (Y, X, name)
            mk = types.SimpleNamespace(direct_header=h, direct=None if h is None else FAKE)
            plain_fwd = lib.sol_karman_step_large_cg_workspace_bytes(r) if h is None else lib.sol_karman_step_large_workspace_bytes_for(r, hp(h))
            plain_bwd, plain_bwd_re = lib.sol_karman_step_bwd_large_workspace_bytes_for(r, hp(h)), lib.sol_karman_step_bwd_large_re_workspace_bytes_for(r, hp(h))
            plain_d, plain_d_re = lib.sol_karman_density_bwd_workspace_bytes(r), lib.sol_karman_density_bwd_re_workspace_bytes(r)
            assert min(plain_fwd, plain_bwd, plain_d) > 0, where
            # the C side: advection = 0 is the plain layout
            assert lib.sol_karman_step_fwd_large_adv_workspace_bytes_for(r, hp(h), 0) == plain_fwd, where
            assert lib.sol_karman_step_bwd_large_adv_workspace_bytes_for(r, hp(h), 0, 0) == plain_bwd, where
            assert lib.sol_karman_step_bwd_large_adv_workspace_bytes_for(r, hp(h), 1, 0) == plain_bwd_re, where
            assert lib.sol_karman_density_bwd_adv_workspace_bytes(r, 0, 0) == plain_d, where
            assert lib.sol_karman_density_bwd_adv_workspace_bytes(r, 1, 0) == plain_d_re, where
            # the Python sizers: called as ever, and with a physics value that advects semi-Lagrangian, the plain bytes in every form
            for ph in (None, ops.StepPhysics(), ops.StepPhysics((0.3, -0.2), 2, None)):
                kw = {} if ph is None else {"physics": ph}
                assert ops.large_workspace_bytes(cfg, mk, **kw) == ops.large_workspace_bytes(cfg, mk, saved=True, **kw) == plain_fwd, where
                assert ops.large_bwd_workspace_bytes(cfg, mk, **kw) == plain_bwd and ops.large_bwd_workspace_bytes(cfg, mk, re=True, **kw) == plain_bwd_re, where
                assert ops.density_bwd_workspace_bytes(cfg, **kw) == plain_d and ops.density_bwd_workspace_bytes(cfg, re=True, **kw) == plain_d_re, where
            # ... and under mac_cormack the _adv functions' own
            assert ops.large_workspace_bytes(cfg, mk, mc) == lib.sol_karman_step_fwd_large_adv_workspace_bytes_for(r, hp(h), 1) > plain_fwd, where
            assert ops.large_workspace_bytes(cfg, mk, mc, saved=True) == lib.sol_karman_step_fwd_large_saved_adv_workspace_bytes_for(r, hp(h), 1), where
            for re in (0, 1):
                assert ops.large_bwd_workspace_bytes(cfg, mk, mc, re=bool(re)) == lib.sol_karman_step_bwd_large_adv_workspace_bytes_for(r, hp(h), re, 1), where
                assert ops.density_bwd_workspace_bytes(cfg, mc, re=bool(re)) == lib.sol_karman_density_bwd_adv_workspace_bytes(r, re, 1), where


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit(__doc__)
    with open(TABLE, "w") as f:
        json.dump(sizes(sol_amd.load()), f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("recorded", TABLE)
