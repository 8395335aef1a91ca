"""bzr_illuminate_bidir on the GPU: illumination through the bidirectional chain, against land o bidir_ref o emit
(bidir_ref.illum_reference for the near outputs and the BACK rows, farfield_ref over the same per-ray rows for the far
outputs) -- everything compared is an integer.

Scenes: illum_tir_ref's emitter at NEAR and its target, 10 000 Lambert rays; absorb_ref's encapsulant scene over the
cfg2 lens (four channels) and the cemented doublet (one channel); budgets 0 and 4, ghost_seed 2024, axis (1, 0, 0).
"""
import numpy as np
import pytest

import bidir_ref
import farfield_ref as ffr
import illum_tir_ref as itr
import media_ref
import power_ref
from absorb_ref import DOUBLET_GAPA, DOUBLET_GLASS, ILLUM_GAPA, ILLUM_GAPS, ILLUM_GLASS
from bidir_ref import AXIS, SEED
from test_gpu_farfield import check_far, target_frame
from test_gpu_illum_tir import KEYS, same
from test_gpu_power import culled_by_sphere

pytestmark = pytest.mark.gpu

N = itr.N_RAYS
SCENES = {"cfg2": ([itr.ROW1], (ILLUM_GAPS, ILLUM_GLASS, ILLUM_GAPA)),
          "doublet": (media_ref.DOUBLET_RI, (media_ref.DOUBLET_CEMENT, DOUBLET_GLASS, DOUBLET_GAPA))}
BUDGETS = (0, 4)


@pytest.fixture(scope="module")
def world(bzr, orc, ctx):
    """name -> (device meshes, {budget: the reference}): computed once."""
    out = {}
    for name, (table, media) in SCENES.items():
        lenses = media_ref.doublet_lenses(bzr.TriMesh) if name == "doublet" else itr.lenses_of(bzr, "cfg2")
        dms = [bzr.DeviceMesh(ctx, p) for p in lenses]
        out[name] = (dms, {mb: bidir_ref.illum_reference(orc, lenses, table, *media, itr.NEAR, mb) for mb in BUDGETS})
    return out


def run(bzr, ctx, name, dms, far=None, budget=4, mode=0, **kw):
    table, media = SCENES[name]
    return bzr.illuminate_bidir(ctx, dms, table, *media, itr.emitter(bzr, itr.NEAR), N, itr.target(bzr), far,
                                max_bounces=budget, ghost_seed=SEED, axis=AXIS, mode=mode, **kw)


def count_identity(got, label):
    """Per channel: sum over rows of LOST + EXITED, plus sum over rows of BACK, is EMITTED - CULLED; the ledger's EXITED and
    LANDED columns sum to the stats'."""
    stats, power, ledger = got[4], got[5], got[6]
    for c in range(len(stats)):
        traced = stats[c]["emitted"] - stats[c]["culled"]
        assert int(ledger["count"][c, :, :2].sum()) + int(ledger["back_count"][c].sum()) == traced, (label, c)
        for led, tot in ((ledger["count"], stats), (ledger["power"], power)):
            assert int(led[c, :, itr.EXITED].sum()) == tot[c]["exited"], (label, c)
            assert int(led[c, :, itr.LANDED].sum()) == tot[c]["landed"], (label, c)
        assert int(ledger["power"][c, :, :2].sum()) + int(ledger["back_power"][c].sum()) <= \
            power[c]["emitted"] - power[c]["culled"], (label, c)


def check(bzr, dm, ref, got, label):
    """Every near output and the BACK rows against the reference, exactly."""
    flux, hist, rflux, rhist, stats, power, ledger = got
    for a, want in ((flux, ref.flux), (hist, ref.hist), (rflux, ref.rflux), (rhist, ref.rhist)):
        assert a.dtype == want.dtype and np.array_equal(a, want), label
    culled = culled_by_sphere(bzr.bounding_sphere(dm), ref.rays)
    want_count, want_power = itr.ledger_for(ref, culled)
    q0 = power_ref.q32(ref.w0)
    assert len(stats) == len(power) == ref.nchan
    for c in range(ref.nchan):
        mine = culled & (ref.channel == c)
        assert stats[c] == dict(zip(KEYS, (ref.emitted[c], int(mine.sum()), int(want_count[c, :, itr.EXITED].sum()),
                                           int(ref.hist[c].sum())))), (label, c)
        assert power[c] == dict(zip(KEYS, (ref.emitted_q[c], int(q0[mine].sum()),
                                           int(want_power[c, :, itr.EXITED].sum()), int(ref.flux[c].sum())))), (label, c)
    for k, want in (("count", want_count), ("power", want_power), ("back_count", ref.back_count),
                    ("back_power", ref.back_power)):
        assert ledger[k].dtype == np.uint64 and ledger[k].shape == want.shape, (label, k)
        assert np.array_equal(ledger[k], want), (label, k, ledger[k].sum(axis=0), want.sum(axis=0))
    count_identity(got, label)


@pytest.mark.parametrize("name", tuple(SCENES))
@pytest.mark.parametrize("budget", BUDGETS)
def test_every_output_bit_exact(bzr, ctx, world, name, budget):
    dms, refs = world[name]
    ref = refs[budget]
    fr = target_frame()
    want = ffr.of_illumination(fr, ref)
    assert int(want.binned.sum()) >= 1000 and int(ref.hist.sum()) >= 1000
    got = run(bzr, ctx, name, dms, ffr.struct(bzr, fr), budget)
    assert len(got) == 8
    check(bzr, dms[0], ref, got[:7], f"{name}, budget {budget}")
    check_far(got[7], want, got[4:6], f"{name}, budget {budget}, far outputs")
    back = int(got[6]["back_count"].sum())
    assert back == int((ref.status == bidir_ref.RR_BACK).sum())
    if budget == 4:  # the back-reflected power is a number the library reports
        assert back >= 400 and int(got[6]["back_power"].sum()) > 0
        assert int(got[6]["back_count"][:, 1:].sum()) >= 400  # ... most of it after a reflection
    again = run(bzr, ctx, name, dms, ffr.struct(bzr, fr), budget)
    assert same(again[:7], got[:7]) and np.array_equal(again[6]["back_power"], got[6]["back_power"])


@pytest.mark.parametrize("origin,budget", ((itr.NEAR, 0), (itr.FAR, 1)))
def test_lossless_is_illuminate_farfield(bzr, orc, ctx, world, origin, budget):
    """SURFACE_LOSSLESS takes no draw: bzr_illuminate_farfield bit for bit wherever the side rule sends no ray backward.
    The doublet from NEAR at budget 0 and from FAR at budget 1 are such scenes -- in the lossless reference, computed
    here, every exit of every ray faces forward (from FAR at budget 4 three rays turn round inside the doublet, from
    NEAR 92; the cfg2 scene has 66 rim rays that leave through the front face even at budget 0) -- and from FAR total
    reflection acts."""
    dms, _ = world["doublet"]
    table, media = SCENES["doublet"]
    lenses = media_ref.doublet_lenses(bzr.TriMesh)
    log = {}
    ref = bidir_ref.illum_reference(orc, lenses, table, *media, origin, budget, lossless=True, log=log)
    assert all(log["all_back"]) and int(ref.back_count.sum()) == 0 and int(ref.hist.sum()) >= 200
    if budget:
        assert int(ref.uncut_count[:, 1:].sum()) >= 10
    far = ffr.struct(bzr, target_frame())
    em = itr.emitter(bzr, origin)
    want = bzr.illuminate_farfield(ctx, dms, table, *media, em, N, itr.target(bzr), far, max_bounces=budget,
                                   surface=bzr.SURFACE_LOSSLESS, mode=bzr.PIPELINE_FUSED)
    got = bzr.illuminate_bidir(ctx, dms, table, *media, em, N, itr.target(bzr), far, max_bounces=budget, ghost_seed=SEED,
                               axis=AXIS, surface=bzr.SURFACE_LOSSLESS)
    assert sum(s["landed"] for s in want[4]) >= 200
    assert same(got[:7], want[:7])
    for k in ("flux", "hist", "reflected_flux"):
        assert np.array_equal(got[7][k], want[7][k]), k
    assert got[7]["stats"] == want[7]["stats"] and got[7]["power"] == want[7]["power"]
    assert int(got[6]["back_count"].sum()) == 0 and int(got[6]["back_power"].sum()) == 0
    assert np.array_equal(got[0], ref.flux) and np.array_equal(got[6]["count"][:, :, 1:], ref.uncut_count[:, :, 1:])


def test_arguments(bzr, ctx, world):
    dms, _ = world["cfg2"]
    with pytest.raises(bzr.BzrError, match="staged"):
        run(bzr, ctx, "cfg2", dms, mode=bzr.PIPELINE_STAGED)
    for axis in ((0.0, 0.0, 0.0), (np.nan, 0.0, 1.0)):
        table, media = SCENES["cfg2"]
        with pytest.raises(bzr.BzrError, match="axis"):
            bzr.illuminate_bidir(ctx, dms, table, *media, itr.emitter(bzr, itr.NEAR), N, itr.target(bzr), axis=axis)
    no_far = run(bzr, ctx, "cfg2", dms)
    assert len(no_far) == 7
    count_identity(no_far, "no far frame")
