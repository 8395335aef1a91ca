"""bzr_illuminate_coated on the GPU: illumination through the coated chain, against land o coat_ref o emit
(coat_ref.illum_reference for the near outputs and the BACK rows, farfield_ref over the same per-ray rows for the far
outputs) -- everything compared is an integer.

Scenes: test_gpu_illum_bidir.py's -- illum_tir_ref's emitter at NEAR and its target, 10 000 Lambert rays; the encapsulant
scene over the cfg2 lens (four channels) and the cemented doublet (one channel); budgets 0 and 4, ghost_seed 2024, axis
(1, 0, 0) -- with the "mixed" coating: quarter-wave MgF2 rows on the front of lens 0 and the back of the last lens.
"""
import numpy as np
import pytest

import coat_ref
import farfield_ref as ffr
import illum_tir_ref as itr
import media_ref
from bidir_ref import AXIS, SEED
from test_gpu_farfield import check_far, target_frame
from test_gpu_illum_bidir import BUDGETS, N, SCENES, check, count_identity
from test_gpu_illum_tir import same

pytestmark = pytest.mark.gpu


def coating_of(bzr, name, lenses):
    table, media = SCENES[name]
    return coat_ref.mixed(bzr, dict(lenses=lenses, table=table, gaps=media[0]))


@pytest.fixture(scope="module")
def world(bzr, orc, ctx):
    """name -> (device meshes, the coating, {budget: the reference}): computed once."""
    out = {}
    for name, (table, media) in SCENES.items():
        lenses = media_ref.doublet_lenses(bzr.TriMesh) if name == "doublet" else itr.lenses_of(bzr, "cfg2")
        dms = [bzr.DeviceMesh(ctx, p) for p in lenses]
        coat = coating_of(bzr, name, lenses)
        out[name] = (dms, coat, {mb: coat_ref.illum_reference(orc, lenses, table, *media, itr.NEAR, mb, coat)
                                 for mb in BUDGETS})
    return out


def run(bzr, ctx, name, dms, coat, far=None, budget=4, mode=0, **kw):
    table, media = SCENES[name]
    c = None if coat is None else bzr.Coating(*coat)
    return bzr.illuminate_coated(ctx, dms, table, *media, itr.emitter(bzr, itr.NEAR), N, itr.target(bzr), far,
                                 max_bounces=budget, ghost_seed=SEED, axis=AXIS, coat=c, mode=mode, **kw)


def run_bidir(bzr, ctx, name, dms, far=None, budget=4, **kw):
    table, media = SCENES[name]
    return bzr.illuminate_bidir(ctx, dms, table, *media, itr.emitter(bzr, itr.NEAR), N, itr.target(bzr), far,
                                max_bounces=budget, ghost_seed=SEED, axis=AXIS, **kw)


def same_with_far(a, b):
    if not same(a[:7], b[:7]):
        return False
    for k in ("back_count", "back_power"):
        if not np.array_equal(a[6][k], b[6][k]):
            return False
    if len(a) == 8:
        for k in ("flux", "hist", "reflected_flux"):
            if not np.array_equal(a[7][k], b[7][k]):
                return False
        return a[7]["stats"] == b[7]["stats"] and a[7]["power"] == b[7]["power"]
    return True


@pytest.mark.parametrize("name", tuple(SCENES))
@pytest.mark.parametrize("budget", BUDGETS)
def test_every_output_bit_exact(bzr, ctx, world, name, budget):
    dms, coat, refs = world[name]
    ref = refs[budget]
    fr = target_frame()
    want = ffr.of_illumination(fr, ref)
    assert int(want.binned.sum()) >= 1000 and int(ref.hist.sum()) >= 1000
    got = run(bzr, ctx, name, dms, coat, ffr.struct(bzr, fr), budget)
    assert len(got) == 8
    check(bzr, dms[0], ref, got[:7], f"{name}, budget {budget}, mixed coating")  # (with the count identity)
    check_far(got[7], want, got[4:6], f"{name}, budget {budget}, far outputs")
    assert int(got[6]["back_count"].sum()) == int((ref.status == coat_ref.RR_BACK).sum())
    # the coating is in the numbers: the uncoated call differs
    bare = run_bidir(bzr, ctx, name, dms, ffr.struct(bzr, fr), budget)
    assert not np.array_equal(bare[0], got[0])


@pytest.mark.parametrize("name", tuple(SCENES))
def test_count_identity(bzr, ctx, world, name):
    dms, coat, _ = world[name]
    for budget in (0, 1, 4, 8):
        count_identity(run(bzr, ctx, name, dms, coat, budget=budget), f"{name}, budget {budget}")


@pytest.mark.parametrize("name", tuple(SCENES))
@pytest.mark.parametrize("budget", BUDGETS)
def test_mask_0_is_illuminate_bidir(bzr, ctx, world, name, budget):
    dms, coat, _ = world[name]
    far = ffr.struct(bzr, target_frame())
    want = run_bidir(bzr, ctx, name, dms, far, budget)
    assert sum(s["landed"] for s in want[4]) >= 1000
    for c in (None, (None, 0), (coat[0], 0)):
        assert same_with_far(run(bzr, ctx, name, dms, c, far, budget), want), (name, budget)


@pytest.mark.parametrize("name", tuple(SCENES))
def test_lossless_ignores_the_table(bzr, ctx, world, name):
    dms, coat, _ = world[name]
    far = ffr.struct(bzr, target_frame())
    want = run_bidir(bzr, ctx, name, dms, far, 4, surface=bzr.SURFACE_LOSSLESS)
    assert sum(s["landed"] for s in want[4]) >= 1000
    mirror = (np.ones_like(coat[0]), (1 << coat[0].shape[0]) - 1)
    for c in (coat, mirror):
        assert same_with_far(run(bzr, ctx, name, dms, c, far, 4, surface=bzr.SURFACE_LOSSLESS), want), name


def test_arguments(bzr, ctx, world):
    dms, coat, _ = world["cfg2"]
    with pytest.raises(bzr.BzrError, match="staged"):
        run(bzr, ctx, "cfg2", dms, coat, mode=bzr.PIPELINE_STAGED)
    with pytest.raises(bzr.BzrError, match="mask"):
        run(bzr, ctx, "cfg2", dms, (coat[0], 4))
    with pytest.raises(bzr.BzrError, match="table"):
        run(bzr, ctx, "cfg2", dms, (None, 1))
    bad = coat[0].copy()
    bad[0, 0, 5] = np.nan
    with pytest.raises(bzr.BzrError, match=r"\[0, 1\]"):
        run(bzr, ctx, "cfg2", dms, (bad, 1))
    assert len(run(bzr, ctx, "cfg2", dms, (bad, 2))) == 7  # the bad row is unmasked
