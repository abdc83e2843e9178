"""ops.StepPhysics, the one value the 2-D step's buoyancy force, diffusion substeps and advection scheme travel in (CPU side): its
constructor runs the validators of the three keywords with their exception types and messages, normalises a force of (0, 0) where the
callers did, and its require() makes the three grid checks before any device call.  Every public surface that takes the keywords builds
it on entry."""
import types

import numpy as np
import pytest
import torch

import sol_amd
from sol_amd import karman, ops, trainer

P = ops.StepPhysics
BAD = (  # (keywords, the message the validator raises)
    (dict(buoyancy=1.0, buoyancy_factor=1.0), "give buoyancy=\\(fy, fx\\) or buoyancy_factor \\(with gravity\\), not both"),
    (dict(buoyancy_factor=0.1, gravity=(1.0, 2.0, 3.0)), "gravity must be \\(gy, gx\\)"),
    (dict(buoyancy=(1.0, 2.0, 3.0)), "buoyancy must be a finite force \\(fy, fx\\)"),
    (dict(buoyancy=(float("nan"), 0.0)), "buoyancy must be a finite force \\(fy, fx\\)"),
    (dict(buoyancy=float("inf")), "buoyancy must be a finite force \\(fy, fx\\)"),
    (dict(advection="upwind"), "advection must be one of semi_lagrangian, mac_cormack \\(got 'upwind'\\)"),
    (dict(advection=None), "advection must be one of semi_lagrangian, mac_cormack"),
    (dict(advection=1), "advection must be one of semi_lagrangian, mac_cormack"),
    (dict(correction_strength="1"), "correction_strength must be a number in \\[0, 1\\]"),
    (dict(correction_strength=None), "correction_strength must be a number in \\[0, 1\\]"),
    (dict(correction_strength=True), "correction_strength must be a number in \\[0, 1\\]"),
    (dict(correction_strength=-0.01), "correction_strength must be finite and lie in \\[0, 1\\]"),
    (dict(correction_strength=1.01), "correction_strength must be finite and lie in \\[0, 1\\]"),
    (dict(correction_strength=float("nan")), "correction_strength must be finite and lie in \\[0, 1\\]"),
    (dict(advection="mac_cormack", correction_strength=2.0), "correction_strength must be finite and lie in \\[0, 1\\]"),
    (dict(diffusion_substeps=0), "diffusion_substeps must be an integer >= 1 \\(got 0\\)"),
    (dict(diffusion_substeps=-3), "diffusion_substeps must be an integer >= 1 \\(got -3\\)"),
    (dict(diffusion_substeps=2.0), "diffusion_substeps must be an integer >= 1 \\(got 2.0\\)"),
    (dict(diffusion_substeps="2"), "diffusion_substeps must be an integer >= 1"),
    (dict(diffusion_substeps=None), "diffusion_substeps must be an integer >= 1"),
    (dict(diffusion_substeps=True), "diffusion_substeps must be an integer >= 1"),
)


def test_the_default_is_the_plain_step_and_the_fields_are_normalised():
    assert P() == P(None, 1, None) == P.of()
    assert P().mode == "" and P().advection_kw == {} and P().force_tail == (0.0, 0.0)
    ph = P.of(buoyancy=(0.3, -0.2), diffusion_substeps=np.int64(3), advection="mac_cormack", correction_strength=0.5)
    assert ph == ((0.3, -0.2), 3, 0.5) and type(ph.nsub) is int and type(ph.adv) is float
    assert ph.mode == "_adv" and ph.force_tail == (0.3, -0.2, 1, 0.5) and ph.advection_kw == dict(advection="mac_cormack", correction_strength=0.5)
    assert P.of(buoyancy=0.5).buoyancy == (0.5, 0.0) and P.of(buoyancy=0.5).mode == "_buoy" and P.of(buoyancy=0.5).force_tail == (0.5, 0.0)
    f = P.of(buoyancy_factor=0.1).buoyancy                          # PhiFlow's spelling: -gravity * buoyancy_factor
    assert f == ops.buoyancy_force(buoyancy_factor=0.1) and abs(f[0] - 0.981) < 1e-12
    assert P.of(buoyancy_factor=2.0, gravity=(0.0, -1.0)).buoyancy == (0.0, 2.0)
    assert P.of(advection="mac_cormack").adv == 1.0 and P.of(advection="mac_cormack", correction_strength=0).adv == 0.0
    assert P.of(advection="semi_lagrangian", correction_strength=0.3).adv is None
    with pytest.raises(AttributeError):
        ph.nsub = 2                                                 # immutable


def test_a_zero_force_normalises_to_none_where_the_callers_did():
    for zero in ((0.0, 0.0), 0.0, (0, -0.0)):
        assert P.of(buoyancy=zero).buoyancy is None and P.of(buoyancy=zero).mode == ""
    assert P.of(buoyancy_factor=0.0).buoyancy is None
    # the direct calls keep it as given: their buoyant entry points take it
    kept = P.of(buoyancy=(0.0, 0.0), keep_zero_force=True)
    assert kept.buoyancy == (0.0, 0.0) and kept.mode == "_buoy" and kept.moving() == P()
    moved = P.of(buoyancy=(0.0, 0.5), diffusion_substeps=2, keep_zero_force=True)
    assert moved.moving() is moved and P().moving() == P()
    assert karman.KarmanFlow(buoyancy=(0.0, 0.0))._physics == P() and karman.KarmanFlow(buoyancy=(0.0, 0.4))._physics.buoyancy == (0.0, 0.4)


@pytest.mark.parametrize("kw,message", BAD)
def test_every_bad_keyword_raises_the_validators_message(kw, message):
    with pytest.raises(ValueError, match=message):
        P.of(**kw)
    with pytest.raises(ValueError, match=message):
        karman.KarmanFlow(**kw)
    # the direct calls validate before they look at a tensor, a mask or the device
    z, cfg = torch.zeros(1), ops.karman_cfg(2, 130, 65, 100.0 / 65)
    direct = {} if "buoyancy_factor" in kw else kw                  # (the direct calls take the force itself only)
    if direct:
        for call in (ops.karman_step_large, ops.karman_step_saved):
            with pytest.raises(ValueError, match=message):
                call(z, z, z, z, cfg, None, **direct)
    if "buoyancy" not in kw and "buoyancy_factor" not in kw:
        with pytest.raises(ValueError, match=message):
            ops.karman_step_large_bwd(z, z, z, z, z, cfg, None, **kw)
        with pytest.raises(ValueError, match=message):
            ops.karman_step_large_bwd_re(z, z, z, z, z, z, z, cfg, None, **kw)
    # the large-grid classes, at construction
    if direct:
        with pytest.raises(ValueError, match=message):
            trainer.LargeGridRollout(None, None, 1, 256, 128, 100.0 / 128, (0.2, 0.2), 1.0, **direct)
        with pytest.raises(ValueError, match=message):
            trainer.LargeGridTrainer(None, 1, 256, 128, 2, (0.2, 0.2), 1.0, **direct)


def test_the_strength_is_validated_under_semi_lagrangian_too():
    for bad in (-0.01, 1.01, float("nan"), float("inf"), "1", None, True):
        for name in ops.ADVECTIONS:
            with pytest.raises(ValueError, match="correction_strength"):
                P.of(advection=name, correction_strength=bad)
    with pytest.raises(ValueError, match="correction_strength"):
        trainer._refuse_advection("SolTrainer", "semi_lagrangian", 1.5)
    with pytest.raises(ValueError, match="correction_strength"):
        ops.karman_density_bwd(None, None, None, None, None, None, None, correction_strength=1.5)
    with pytest.raises(ValueError, match="correction_strength"):
        ops.karman_density_bwd_re(None, None, None, None, None, None, None, None, None, correction_strength=-1.0)


def test_require_makes_the_three_grid_checks_before_any_device_call():
    small, large = types.SimpleNamespace(large=False), types.SimpleNamespace(large=True)
    cfg, thin = ops.karman_cfg(2, 130, 65, 100.0 / 65), ops.karman_cfg(1, 16, 8, 100.0 / 8)
    for ph in (P(), P((0.3, 0.0), 2, 0.5), P((0.0, 0.0), 1, None)):
        ph.require(cfg, large, "here")
    P().require(thin, None, "here")                                 # the plain step looks at nothing
    P(None, 2, None).require(ops.karman_cfg(1, 64, 32, 100.0 / 32), small, "here")
    with pytest.raises(sol_amd.SolError, match="here: diffusion substeps \\(sol_karman_diffuse_sub\\) take grids with Y, X >= 16; this one is 16x8"):
        P(None, 2, None).require(thin, None, "here")
    with pytest.raises(sol_amd.SolError, match="here: the buoyancy force is built on the multi-launch \\(large-grid\\) step only; a 64x32 grid runs the fused"):
        P((0.1, 0.0), 1, None).require(ops.karman_cfg(1, 64, 32, 100.0 / 32), small, "here")
    with pytest.raises(sol_amd.SolError, match="here: the buoyancy force is built on the multi-launch"):
        P((0.0, 0.0), 1, None).require(ops.karman_cfg(1, 64, 32, 100.0 / 32), small, "here")      # a kept zero force is still a force
    with pytest.raises(sol_amd.SolError, match="here: the mac_cormack advection is built on the multi-launch \\(large-grid\\) step only; a 64x32 grid runs the fused"):
        P(None, 1, 1.0).require(ops.karman_cfg(1, 64, 32, 100.0 / 32), small, "here")
    # the public calls check on entry
    z = torch.zeros(1)
    c64 = ops.karman_cfg(1, 64, 32, 100.0 / 32)
    for call, kw in ((ops.karman_step_large, dict(buoyancy=(0.1, 0.0))), (ops.karman_step_saved, dict(buoyancy=(0.0, 0.0))),
                     (ops.karman_step_large, dict(advection="mac_cormack")), (ops.karman_step_saved, dict(advection="mac_cormack"))):
        with pytest.raises(sol_amd.SolError, match="multi-launch"):
            call(z, z, z, z, c64, small, **kw)
    with pytest.raises(sol_amd.SolError, match="multi-launch"):
        ops.karman_step_saved(z, z, z, z, c64, small, buoyancy=[0.1, 0.0])          # (a list: the value is built per call, not remembered)
    with pytest.raises(sol_amd.SolError, match="multi-launch"):
        ops.karman_step_large_bwd(z, z, z, z, z, c64, small, advection="mac_cormack")
    with pytest.raises(sol_amd.SolError, match="multi-launch"):
        ops.karman_step_large_bwd_buoy(z, z, z, z, z, z, z, c64, small, (0.1, 0.0))


def test_the_one_workgroup_classes_decide_on_the_same_value():
    assert trainer._refuse_buoyancy("SolTrainer", None) is None and trainer._refuse_buoyancy("SolTrainer", (0.0, 0.0)) is None
    assert trainer._refuse_advection("SolTrainer", "semi_lagrangian", 0.5) is None and trainer._refuse_substeps("SolTrainer", 1, 64, 32) == 1
    with pytest.raises(ValueError, match="SolTrainer: buoyancy=\\(0.1, 0.0\\) -- the buoyancy force is built on the multi-launch"):
        trainer._refuse_buoyancy("SolTrainer", (0.1, 0.0))
    with pytest.raises(ValueError, match="SolRollout: advection='mac_cormack' -- the mac_cormack advection is built on the multi-launch"):
        trainer._refuse_advection("SolRollout", "mac_cormack")
    with pytest.raises(ValueError, match="GraphTrainer: diffusion_substeps=2 -- diffusion substeps are built on the multi-launch"):
        trainer._refuse_substeps("GraphTrainer", 2, 64, 32)
    assert trainer.GraphTrainer._check_physics(64, 32, None, 1, "semi_lagrangian", 1.0) == P()
    ph = trainer.LargeGridTrainer._check_physics(256, 128, buoyancy=(0.0, 0.0), diffusion_substeps=2, advection="mac_cormack", correction_strength=0.5)
    assert ph == (None, 2, 0.5)
