"""The table of the karman-3d network shape tests, CPU side (no GPU needed).  tests/karman3d_net_shapes.py restates which kernels the
3-D correction network launches at a shape; here the restated rules are tied to their source lines by text, every number the table quotes
is asserted, karman3d.net3d_shape_reason is checked against a direct restatement of the C conditions over Z in 4 .. 130 and X in 4 .. 70,
and the fp32-ALONE figures are measured and pinned: torch fp32 conv3d and its autograd against torch float64 on the same inputs and
LeakyReLU masks, no project code involved -- what the bounds of the GPU tests rest on where a cell would miss the suite's own
(karman3d_net_shapes.NET_BOUNDS; none does)."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import karman3d_net_shapes as kn
from karman3d_net_shapes import CELLS, FP32_ALONE, NET_CELLS, PERSIST_CELLS, WIDE_CELL, sid

from sol_amd import karman3d as k3

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "solver-in-the-loop_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


def test_the_restated_rules_are_the_launchers_own():
    k3h, c5, sb, dx, c3, tr = (source(n) for n in ("karman3d.hip", "conv5x5.hip", "conv5x5_sb.hip", "conv5x5_dx.hip", "conv3d_sb.hip", "train.hip"))
    # the default options the restatement assumes
    for opt in ("d.conv_precision = 0;", "d.conv_r3 = 1;", "d.conv_thin = 1;", "d.conv_bww32 = 1;", "d.k3d_conv_fused = 1;", "d.k3d_conv_rows = 8;",
                "d.conv_dx = 11;", "d.k3d_bww_jobs = 2;", "d.k3d_conv_persist = 0;"):
        assert opt in tr, opt
    # sol_conv3d: the one-launch form, else five passes of the 2-D kernels (2 B + 2 B + 1 launches)
    assert "static bool conv3d_fusable_shape(int cin, int cout) { return cin == 32 && (cout == 32 || cout <= 16); }" in k3h
    assert "if (conv3d_fusable_shape(cin, cout) && W == 64 && x_absmax && sol_opt().conv_precision == 0 && sol_opt().k3d_conv_fused && residual != y)" in k3h
    assert "SOL_REQUIRE(B >= 1 && D >= 3, \"sol_conv3d: B >= 1, D >= 3 (got %d, %d)\", B, D);" in k3h
    assert k3h.count("D - 2, H, W, cin, cout, SOL_EPI_NONE") == 2 and k3h.count("D - 1, H, W, cin, cout, SOL_EPI_NONE") == 2
    assert "B * D, H, W, cin, cout, epilogue, slope, x_absmax, y_absmax);" in k3h
    # the thin layers: one 2-D 32 -> 32 launch over B D planes, any W % 4 == 0 at the entry point
    assert "return sol_conv5x5_scaled(stream, ws, packed, bias, nullptr, act_ref, y, B * D, H, W, 32, 32, epilogue, slope, slots, y_absmax);" in k3h
    assert "sol_conv5x5_scaled(stream, x, packed, nullptr, nullptr, nullptr, ws, B * D, H, W, 32, 32, SOL_EPI_NONE, 0.f, x_absmax, nullptr)" in k3h
    # check_shape and conv_impl
    assert "SOL_REQUIRE(B >= 1 && H >= 1 && W >= 4, \"conv5x5: bad image shape" in c5
    assert "SOL_REQUIRE((W <= 64 && 64 % W == 0 && H % (64 / W) == 0) || W % 64 == 0," in c5
    assert "if (cin == 32 && W % 64 == 0 && use_sb) {" in c5 and "if (cin == 32 && W % 64 == 0 && sol_opt().conv_r3) {" in c5
    assert "a.xmax = use_sh ? x_absmax : nullptr;" in c5 and "a.TW = W < 64 ? W : 64; a.RPW = 64 / a.TW;" in c5
    assert "if (sol_conv_dx_usable(a, NT, ntiles)) return sol_conv_dx_launch(s, a, ntiles);" in sb
    assert "if (NT == 2) return (sol_opt().conv_dx & 1) && a.CO == 32 && !a.cvy;" in dx
    assert "static int dx_rows_per_wg(int nrows, int tiles_x, int H) { return H >= 2 && ((nrows + 2) / 3) * tiles_x >= 128 ? 3 : 1; }" in dx
    assert "if (!thin && R == 1 && (sol_opt().conv_dx & 8)) SOL_LAUNCH((k_conv5x5_dx<1, 1, true>)" in dx
    assert "else if (R == 3) SOL_LAUNCH((k_conv5x5_dx<3, 2>)" in dx
    # the weight gradients
    assert "constexpr int RB = 8;" in c5
    assert "if (rows > 4096) return thin ? (rows + 1023) / 1024 : (rows + 255) / 256;" in c5
    assert "SOL_REQUIRE(W <= 64 || (nblk_layout == 0 && nseg == 1), \"sol_conv5x5_bwd_weight: the batched forms take W <= 64 (got %d)\", W);" in c5
    assert "const bool jobs = cin == 32 && cout == 32 && W == 64 && sol_opt().conv_precision != 2 && sol_opt().k3d_bww_jobs;" in k3h
    assert "if (W == 64 && ((cin == 4 && cout == 32) || (cin == 32 && cout == 2)) && sol_opt().conv_thin) {" in c5
    assert "if (cin == 32 && cout == 32 && W % 64 == 0 && sol_opt().conv_precision != 2) return sol_bww_sb_launch(s, a, nblk_run);" in c5
    assert "else if (cin == 32 && cout == 32) SOL_LAUNCH((k_conv5x5_bww<32, 32>)" in c5 and "else if (cin == 4 && cout == 32) SOL_LAUNCH((k_conv5x5_bww<4, 32>)" in c5
    assert "if (use_sh && a.xmax && a.zmax && (a.B * a.H) % a.rb == 0) SOL_LAUNCH(k_conv5x5_bww_sb<2>" in sb
    assert "if (sh) SOL_LAUNCH(k_conv5x5_bww_sb_jobs<2>" in sb
    assert "\"sol_conv3d_thin_bwd_weight: needs W == 64 and 1..4 input channels" in k3h
    # the one-launch kernel's grid and its persistent form
    assert "const int nt8 = (nrows + 7) / 8, grid8 = (nt8 + 7) / 8 * 8;" in c3
    assert ("if (sol_opt().k3d_conv_persist && nt8 % 256 == 0 && nt8 >= 512) SOL_LAUNCH((k_conv3d_sb8<2, 0, true>), dim3(256), dim3(512), c8_lds(2), s, a, "
            "nrows, D, nt8 / 256);") in c3
    assert "else SOL_LAUNCH((k_conv3d_sb8<2, 0>), dim3(grid8), dim3(512), c8_lds(2), s, a, nrows, D, 1);" in c3
    # schedule3d.NetSchedule3D.backward switches on Z == 64
    with open(os.path.join(os.path.dirname(CSRC), "schedule3d.py")) as f:
        assert "w64 = self.shape[3] == 64" in f.read()


def test_every_cell_reaches_what_the_table_says():
    form = lambda c: kn.conv_form(*c, 32, 32, True)
    assert [c for c in CELLS if form(c) == "one_launch"] == [(2, 5, 10, 64), (1, 3, 8, 64)] + PERSIST_CELLS
    assert kn.conv_form(2, 5, 10, 64, 32, 32, False) == "five_pass" and kn.conv_form(2, 5, 10, 64, 32, 32, True, fused=0) == "five_pass"
    # narrow rows: image rows per tile and tiles per plane
    tiles = lambda c: (64 // c[3], c[2] * c[3] // 64)
    assert [tiles(c) for c in ((2, 5, 6, 32), (2, 5, 12, 16), (1, 6, 8, 8), (1, 3, 16, 4))] == [(2, 3), (4, 3), (8, 1), (16, 1)]
    for c in ((2, 5, 6, 32), (2, 5, 12, 16), (1, 6, 8, 8), (1, 3, 16, 4)):
        B = c[0]
        assert kn.conv3d_launches(*c) == {"k_conv5x5_c32<2>": 4 * B + 1} and kn.thin_launches(*c) == {"k_conv5x5_c32<2>": 1}
        assert kn.bww_launches(*c, 32, 32) == {"k_conv5x5_bww<32,32>": 5 * B} and kn.bww_launches(*c, 4, 32) == {"k_conv5x5_bww<4,32>": 5 * B}
    # the one-launch kernel at 100 rows: 13 tiles on 16 workgroups, tiles that span planes (H = 10) and the two samples (50 rows each)
    assert kn.one_launch(2, 5, 10) == dict(rows=100, tiles=13, grid=16, persistent=False, tiles_per_wg=1, kernel="k_conv3d_sb8<2,0>")
    assert any(t * 8 < 50 < t * 8 + 8 for t in range(13)) and 10 % 8 != 0
    assert kn.bww_launches(2, 5, 10, 64, 32, 32) == {"k_conv5x5_bww_sb_jobs<2>": 2}
    assert kn.thin_bww_kernel(2, 5, 10) == "k_conv5x5_bww_sb<0>" and kn.thin_bww_kernel(1, 3, 8) == "k_conv5x5_bww_sb<2>"
    assert kn.thin_bww_kernel(2, 20, 10) == "k_conv5x5_bww_sb<2>"                     # the trainer cell 20 x 10 x 64
    assert kn.thin_launches(2, 5, 10, 64) == {"k_conv5x5_dx<1,1,true>": 1}
    # Z = 128: five passes of the dx-major kernel over two column tiles per row; no weight gradient
    assert kn.conv3d_launches(*WIDE_CELL) == {"k_conv5x5_dx<1,1,true>": 5} and kn.bww_launches(*WIDE_CELL, 32, 32) is None
    # the persistent form: only under the option, 2 and 3 tiles per workgroup
    assert [kn.one_launch(*c[:3], persist=1)["tiles_per_wg"] for c in PERSIST_CELLS] == [2, 3]
    assert [kn.one_launch(*c[:3], persist=1)["tiles"] for c in PERSIST_CELLS] == [512, 768]
    assert all(kn.one_launch(*c[:3], persist=1)["kernel"] == "k_conv3d_sb8<2,0,true>" and not kn.one_launch(*c[:3])["persistent"] for c in PERSIST_CELLS)
    assert not kn.one_launch(1, 32, 64, persist=1)["persistent"] and not kn.one_launch(1, 65, 64, persist=1)["persistent"]       # 256 tiles; 520
    # the strict-fp32 form of the dynamic-range test: five passes of the fp32-MFMA kernel
    assert kn.conv3d_launches(*kn.SPLIT3D_SHAPE, precision=2) == {"k_conv5x5_r3<2>": 5}
    # the network as a whole
    conv, bww = kn.net_backward_launches(2, 5, 10, 64)
    assert kn.net_forward_launches(2, 5, 10, 64) == {"k_conv3d_sb8<2,0>": 10, "k_conv5x5_dx<1,1,true>": 2} == conv
    assert bww == {"k_conv5x5_bww_sb_jobs<2>": 20, "k_conv5x5_bww_sb<0>": 2}
    conv, bww = kn.net_backward_launches(2, 5, 6, 32)
    assert conv == {"k_conv5x5_c32<2>": 92} and bww == {"k_conv5x5_bww<32,32>": 110, "k_conv5x5_bww<4,32>": 10}
    # trainer cells are network cells with B = 2
    for (Y, X, Z) in kn.TRAIN_CELLS:
        assert k3.net3d_shape_reason(Y, X, Z, True) is None
    assert k3.net3d_shape_reason(*kn.Z128_CELL, False) is None


def test_net3d_shape_reason_against_the_c_conditions():
    for train in (False, True):
        for Z in range(4, 131):
            for X in range(4, 71):
                why = k3.net3d_shape_reason(16, X, Z, train)
                assert (why is not None) == kn.net_shape_reason(16, X, Z, train), (X, Z, train, why)
    assert k3.net3d_shape_reason(2, 8, 8, False) is not None and k3.net3d_shape_reason(3, 8, 8, True) is None
    assert k3.net3d_shape_reason(16, 8, 2, False) is not None and k3.net3d_shape_reason(16, 8, 192, False) is None
    # every cell of the table is accepted, the refusals name the extent and the rule
    for (B, D, H, W) in CELLS:
        assert k3.net3d_shape_reason(D, H, W, W <= 64) is None
    for (Y, X, Z, train_only), words in kn.REFUSED.items():
        why = k3.net3d_shape_reason(Y, X, Z, True)
        assert why is not None and all(w in why for w in words), (why, words)
        assert (k3.net3d_shape_reason(Y, X, Z, False) is None) == train_only


def test_the_schedules_refuse_at_construction_without_a_device():
    """NetSchedule3D asks net3d_shape_reason before it asks for a device: the refusal is the same on a machine without one"""
    from sol_amd import _lib
    from sol_amd.schedule3d import NetSchedule3D
    for (Y, X, Z, train_only), words in kn.REFUSED.items():
        with pytest.raises(_lib.SolError) as e:
            NetSchedule3D(None, 2, Y, X, Z, train=True)
        assert all(w in str(e.value) for w in words), str(e.value)


def test_the_script_refuses_before_it_generates_anything(tmp_path):
    """scripts/karman3d.py --train-sol / --model at a width the corrector does not take: SystemExit with the reason, no output directory"""
    import importlib.util
    import sol_amd
    import torch
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)
    spec = importlib.util.spec_from_file_location("sol_script_karman3d_refusals", os.path.join(sdir, "karman3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(SystemExit, match="Z = 12"):
        mod.main(["-r", "12", "-t", "8", "-o", str(tmp_path / "a"), "--train-sol", "2"])
    with pytest.raises(SystemExit, match="Z <= 64"):
        mod.main(["-r", "128", "-t", "8", "-o", str(tmp_path / "b"), "--train-sol", "2"])
    net = k3.MarsMoon3D(device="cpu")
    torch.save({"name": net.name, "weights": [torch.as_tensor(a) for a in net.get_weights()], "std_v": (0.2, 0.25, 0.3), "std_re": 1e5}, str(tmp_path / "m.pt"))
    with pytest.raises(SystemExit, match="Z = 24"):
        mod.main(["-r", "24", "-t", "4", "-o", str(tmp_path / "c"), "--model", str(tmp_path / "m.pt")])
    assert sorted(os.listdir(tmp_path)) == ["m.pt"]


@pytest.mark.parametrize("cell", NET_CELLS + [WIDE_CELL], ids=sid)
def test_fp32_alone(cell):
    """torch fp32 against torch float64, the fp32 run with the float64 run's LeakyReLU masks: output, input gradient and the largest of the 24
    parameter gradients (Z = 128: output only, the network trains up to Z = 64).  Pinned within a factor of 2 of FP32_ALONE, and every figure
    below the bound the GPU test of the cell asserts (fp32 arithmetic alone can meet it)."""
    grads = cell != WIDE_CELL
    got = kn.fp32_alone(cell, grads)
    print("fp32 alone at %s: out %.2e, dx %s, params %s" % (sid(cell), got[0], *("%.2e" % v if v is not None else "-" for v in got[1:])))
    for g, want, bound in zip(got, FP32_ALONE[cell], kn.NET_BOUNDS[cell]):
        if g is None:
            continue
        assert want / 2 <= g <= want * 2, (cell, got, FP32_ALONE[cell])
        assert g < bound, (cell, got, kn.NET_BOUNDS[cell])
