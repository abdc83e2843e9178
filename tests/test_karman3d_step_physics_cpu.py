"""karman3d.StepPhysics3D, the one value the 3-D step's buoyancy force and diffusion substeps travel in, and karman3d._step_adjoint3d, the
one place that composes the velocity half, the density half and the substep tail of a step's adjoint (CPU side, no device): the
constructor runs the validators of the keywords with their exception types and messages and normalises a force of (0, 0, 0) where the
callers did; the entry points are looked up by name from the mode; the chain's decisions -- which half runs, in which order, on which
density cotangent, whether the pre-diffusion and the factor n follow -- are checked against a table written out by hand below."""
import itertools

import numpy as np
import pytest
import torch

from sol_amd import karman3d as k3
from sol_amd import ops

P = k3.StepPhysics3D
FORCE = (0.3, -0.2, 0.15)
WHO = "Karman3DFlow: diffusion_substeps"
BAD = (  # (keywords, the message the validator raises): the lists of test_karman3d_buoyancy_cpu.py and test_karman3d_diffusion_substeps_cpu.py
    (dict(buoyancy=(1.0, 2.0, 3.0, 4.0)), "buoyancy must be a finite force \\(fy, fx, fz\\), got \\(1.0, 2.0, 3.0, 4.0\\)"),
    (dict(buoyancy=(float("nan"), 0.0, 0.0)), "buoyancy must be a finite force \\(fy, fx, fz\\)"),
    (dict(buoyancy=()), "buoyancy must be a finite force \\(fy, fx, fz\\), got \\(\\)"),
    (dict(buoyancy=1.0, buoyancy_factor=1.0), "give buoyancy=\\(fy, fx, fz\\) or buoyancy_factor \\(with gravity\\), not both"),
    (dict(buoyancy_factor=1.0, gravity=(-9.81, 0.0)), "gravity must be \\(gy, gx, gz\\), got \\(-9.81, 0.0\\)"),
    (dict(diffusion_substeps=0), "Karman3DFlow: diffusion_substeps must be an integer >= 1 \\(got 0\\)"),
    (dict(diffusion_substeps=-3), "Karman3DFlow: diffusion_substeps must be an integer >= 1 \\(got -3\\)"),
    (dict(diffusion_substeps=2.0), "Karman3DFlow: diffusion_substeps must be an integer >= 1 \\(got 2.0\\)"),
    (dict(diffusion_substeps=1.5), "Karman3DFlow: diffusion_substeps must be an integer >= 1 \\(got 1.5\\)"),
    (dict(diffusion_substeps="2"), "Karman3DFlow: diffusion_substeps must be an integer >= 1 \\(got '2'\\)"),
    (dict(diffusion_substeps=None), "Karman3DFlow: diffusion_substeps must be an integer >= 1 \\(got None\\)"),
    (dict(diffusion_substeps=True), "Karman3DFlow: diffusion_substeps must be an integer >= 1 \\(got True\\)"),
)


def test_the_default_is_the_plain_step_and_the_fields_are_normalised():
    assert P() == P(None, 1) == P.of()
    assert P().mode == "" and P().force_tail == ()
    ph = P.of(buoyancy=(0.3, -0.2), diffusion_substeps=np.int64(3))
    assert ph == ((0.3, -0.2, 0.0), 3) and type(ph.nsub) is int and all(type(v) is float for v in ph.buoyancy)
    assert ph.mode == "_buoy" and ph.force_tail == (0.3, -0.2, 0.0)
    assert P.of(buoyancy=np.float32(0.5)).buoyancy == (0.5, 0.0, 0.0) and type(P.of(buoyancy=np.float32(0.5)).force_tail[0]) is float
    f = P.of(buoyancy_factor=0.1).buoyancy                          # PhiFlow's spelling: -gravity * buoyancy_factor
    assert f == k3.buoyancy_force3d(buoyancy_factor=0.1) and abs(f[0] - 0.981) < 1e-12 and f[1:] == (0.0, 0.0)
    assert P.of(buoyancy_factor=2.0, gravity=(0.0, 0.0, -1.0)).buoyancy == (0.0, 0.0, 2.0)
    with pytest.raises(AttributeError):
        ph.nsub = 2                                                 # immutable
    assert P is not ops.StepPhysics and P._fields == ("buoyancy", "nsub")      # a sibling of the 2-D value, not a generalisation


def test_a_zero_force_normalises_to_none_unless_it_is_kept():
    for zero in (0.0, (0, -0.0, 0), (0.0, 0.0, 0.0), (0.0, 0.0)):
        assert P.of(buoyancy=zero) == P() and P.of(buoyancy=zero).mode == ""
    assert P.of(buoyancy_factor=0) == P() and P.of(buoyancy_factor=0.0, diffusion_substeps=2) == (None, 2)
    kept = P.of(buoyancy=(0, -0.0, 0), keep_zero_force=True)
    assert kept.buoyancy == (0.0, 0.0, 0.0) and kept.mode == "_buoy" and kept.force_tail == (0.0, 0.0, 0.0)
    assert P.of(buoyancy_factor=0, keep_zero_force=True).mode == "_buoy" and P.of(keep_zero_force=True) == P()      # (no force given: none kept)
    # moving(): what a differentiable step runs on
    assert kept.moving() == P() and P.of(buoyancy=0.0, diffusion_substeps=3, keep_zero_force=True).moving() == (None, 3)
    moved = P.of(buoyancy=(0.0, 0.0, 0.5), diffusion_substeps=2, keep_zero_force=True)
    assert moved.moving() is moved and P().moving() == P()
    assert k3._buoyant3d((0.0, 0.0, -1e-3)) and not k3._buoyant3d((0.0, 0.0, 0.0)) and not k3._buoyant3d(None)


@pytest.mark.parametrize("kw,message", BAD)
def test_every_bad_keyword_raises_the_validators_message(kw, message):
    with pytest.raises(ValueError, match=message):
        P.of(who=WHO, **kw)
    with pytest.raises(ValueError, match=message):
        P.of(who=WHO, keep_zero_force=True, **kw)
    with pytest.raises(ValueError, match=message):                  # validated before the device is asked for
        k3.Karman3DFlow(None, 1, **kw)
    if "diffusion_substeps" in kw:                                  # `who` is how the message names the count
        with pytest.raises(ValueError, match="^torch.ops.sol.karman3d_step_sub: nsub must be an integer >= 1"):
            P.of(who="torch.ops.sol.karman3d_step_sub: nsub", **kw)
        with pytest.raises(ValueError, match="^diffusion_substeps must be an integer >= 1"):
            P.of(**kw)


def test_the_entry_points_are_looked_up_by_name_from_the_mode():
    class Lib:
        def __init__(self):
            self.names = []

        def __getattr__(self, name):
            self.names.append(name)
            return "<%s>" % name

    lib = Lib()
    got = {}
    for force, re in itertools.product((None, FORCE), (False, True)):
        ph = P(force, 1)
        got[(force is not None, re)] = (k3._adjoint_entry(lib, "step_bwd", ph.mode, re), k3._adjoint_entry(lib, "density_bwd", re=re))
    assert got == {(False, False): ("<sol_karman3d_step_bwd>", "<sol_karman3d_density_bwd>"),
                   (False, True): ("<sol_karman3d_step_bwd_re>", "<sol_karman3d_density_bwd_re>"),
                   (True, False): ("<sol_karman3d_step_bwd_buoy>", "<sol_karman3d_density_bwd>"),
                   (True, True): ("<sol_karman3d_step_bwd_buoy_re>", "<sol_karman3d_density_bwd_re>")}
    assert sorted(set(lib.names)) == ["sol_karman3d_density_bwd", "sol_karman3d_density_bwd_re", "sol_karman3d_step_bwd",
                                      "sol_karman3d_step_bwd_buoy", "sol_karman3d_step_bwd_buoy_re", "sol_karman3d_step_bwd_re"]
    assert len(lib.names) == 8                                      # one lookup per half and call, nothing else is touched


# ---- the chain's decisions ------------------------------------------------------------------------------------------------------------
# Written out by hand from the rules of the chain.  Per (moving force, density, want_re) and cotangent set: the halves that run, in order.
#   "V(x)"  the velocity half, x = the density cotangent it is handed: "gd" (the caller's), "-" (None: a null pointer)
#   "D(x)"  the density half, x = its density cotangent: "gd" (the caller's) or "dsum" (the velocity half's g_dsum); "+" = onto the velocity
#           half's buffers (and its g_re), accumulating
# A missing velocity cotangent of a velocity half that runs is a tensor of zeros.
T, F = True, False
MOVING = {"none": [], "dens": ["V(gd)", "D(dsum)+"], "vel": ["V(-)", "D(dsum)+"], "both": ["V(gd)", "D(dsum)+"]}
PLAIN = {"none": ["V(-)"], "dens": ["V(-)"], "vel": ["V(-)"], "both": ["V(-)"]}
DENSITY = {"none": [], "dens": ["D(gd)"], "vel": ["V(-)"], "both": ["V(-)", "D(gd)+"]}
RE_ONLY = {"none": [], "dens": [], "vel": ["V(-)"], "both": ["V(-)"]}
TABLE = {  # (moving, density, want_re)
    (F, F, F): PLAIN, (F, F, T): RE_ONLY, (F, T, F): DENSITY, (F, T, T): DENSITY,
    (T, F, F): MOVING, (T, F, T): MOVING, (T, T, F): MOVING, (T, T, T): MOVING,      # under a force the density is in the graph whatever `density` says
}
KINDS = ("none", "dens", "vel", "both")


class Recorder:
    """stands in for the simulator's velocity half, density_bwd and diffuse_sub: records every call, returns tagged tensors"""

    def __init__(self):
        self.calls = []
        t = lambda v: torch.full((2,), float(v))
        self.vel_out, self.dsum, self.re_v = [t(10), t(11), t(12)], t(13), torch.tensor([2.0, 4.0])
        self.od, self.dens_out, self.re_d = t(20), [t(21), t(22), t(23)], torch.tensor([3.0, 5.0])
        self.pre = (t(30), t(31), t(32))

    def _bwd(self, saved, re, gvy, gvx, gvz, vel_in=None, g_re=None, buoyancy=None, g_d=None, nsub=1, physics=None):
        assert buoyancy is None and nsub == 1 and g_re is None       # the chain speaks through physics=
        self.calls.append(("V", physics, g_d, (gvy, gvx, gvz), vel_in))
        res = list(self.vel_out) + ([self.re_v] if vel_in is not None else [])
        return res + [self.dsum] if physics.buoyancy is not None else res

    def density_bwd(self, sim, d_in, saved, re, g_d, g_v=None, vel_in=None, g_re=None, nsub=1):
        assert sim is self
        self.calls.append(("D", nsub, g_d, g_v, vel_in, g_re, d_in))
        return (self.od, *self.dens_out) + ((self.re_d,) if vel_in is not None else ())

    def diffuse_sub(self, sim, vy, vx, vz, re, nsub, chunk=None):
        assert sim is self
        self.calls.append(("S", nsub, (vy, vx, vz)))
        return self.pre


@pytest.mark.parametrize("through", (True, False))
@pytest.mark.parametrize("n", (1, 3))
@pytest.mark.parametrize("moving,density,want_re", sorted(TABLE))
def test_the_chain_runs_the_halves_the_table_names(monkeypatch, moving, density, want_re, n, through):
    saved = tuple(torch.ones(2) * k for k in (1, 2, 3))
    d_in, re, vel_in = torch.ones(2) * 4, torch.ones(2) * 5, tuple(torch.ones(2) * k for k in (6, 7, 8))
    GD, GV = torch.ones(2) * 40, tuple(torch.ones(2) * k for k in (41, 42, 43))
    ph = P(FORCE if moving else None, n)
    for kind in KINDS:
        rec = Recorder()
        monkeypatch.setattr(k3, "density_bwd", rec.density_bwd)
        monkeypatch.setattr(k3, "diffuse_sub", rec.diffuse_sub)
        gd = GD if kind in ("dens", "both") else None
        gv = GV if kind in ("vel", "both") else (None, None, None)
        out = k3._step_adjoint3d(rec, ph, density, d_in, saved, re, gd, gv, vel_in if want_re else None, through_substeps=through)
        want = TABLE[(moving, density, want_re)][kind]
        halves = [c for c in rec.calls if c[0] in "VD"]
        assert len(halves) == len(want), (kind, want, rec.calls)
        ran_v = ran_d = False
        for call, name in zip(halves, want):
            assert call[0] == name[0], (kind, want, rec.calls)
            if name[0] == "V":
                _, physics, g_d, cot, vin = call
                ran_v = True
                assert physics is ph and (vin is vel_in if want_re else vin is None)
                assert g_d is {"V(gd)": GD, "V(-)": None}[name]
                for c, g, s in zip(cot, gv, saved):                 # the cotangent itself, or zeros of the saved velocity's shape
                    assert c is g if g is not None else (c.shape == s.shape and not c.any())
            else:
                _, nsub, g_d, g_v, vin, g_re, din = call
                ran_d = True
                assert nsub == n and din is d_in and (vin is vel_in if want_re else vin is None)
                assert g_d is {"D(gd)": GD, "D(dsum)": rec.dsum}[name.rstrip("+")]
                if name.endswith("+"):                              # onto the velocity half's buffers and g_re
                    assert ran_v and all(a is b for a, b in zip(g_v, rec.vel_out)) and (g_re is rec.re_v if want_re else g_re is None)
                else:
                    assert g_v is None and g_re is None
        # what comes back: the last half's buffers; through the pre-diffusion and times n under substeps
        g_d, *g_v, g_re = out
        assert len(out) == 5
        assert g_d is (rec.od if ran_d else None)
        last_v = rec.dens_out if ran_d else rec.vel_out if ran_v else None
        pre = [c for c in rec.calls if c[0] == "S"]
        if last_v is None:
            assert g_v == [None, None, None] and g_re is None and not pre
            continue
        if n > 1 and through:
            assert len(pre) == 1 and pre[0][1] == n and all(a is b for a, b in zip(pre[0][2], last_v)) and rec.calls[-1] is pre[0]
            assert all(a is b for a, b in zip(g_v, rec.pre))
        else:
            assert not pre and all(a is b for a, b in zip(g_v, last_v))
        last_re = (rec.re_d if ran_d else rec.re_v) if want_re else None
        if last_re is None:
            assert g_re is None
        elif n > 1:                                                 # the factor n does not depend on through_substeps
            assert g_re is not last_re and torch.equal(g_re, last_re * float(n))
        else:
            assert g_re is last_re


def test_the_chain_materialises_zeros_for_single_missing_components(monkeypatch):
    """one velocity cotangent alone counts as "a velocity cotangent arrived"; the other two become zeros"""
    saved = (torch.ones(2, 3), torch.ones(3, 2), torch.ones(1, 5))
    g = torch.ones(3, 2) * 7
    for ph, density in ((P(), False), (P(), True), (P(FORCE, 1), True)):
        rec = Recorder()
        monkeypatch.setattr(k3, "density_bwd", rec.density_bwd)
        k3._step_adjoint3d(rec, ph, density, torch.ones(2), saved, torch.ones(2), None, (None, g, None))
        (kind, _, g_d, cot, _), *rest = rec.calls
        assert kind == "V" and g_d is None and cot[1] is g
        assert cot[0].shape == (2, 3) and cot[2].shape == (1, 5) and not cot[0].any() and not cot[2].any()
        assert [c[0] for c in rest] == (["D"] if ph.buoyancy is not None else [])
