"""bzr_illuminate_ghost on the GPU: illumination through the chain with the Fresnel roulette, against
ghost_ref.illum_reference (near outputs) and farfield_ref over the same reference chain (far outputs), bit for bit --
everything compared is an integer.

Scene: absorb_ref's encapsulant scene (the cfg2 lens, ROW1's four indices, the emitter in a medium), the emitter at
illum_tir_ref.NEAR, 10 000 Lambert rays, budget 4, ghost_seed 2024; emitter ray j draws with ray number j.
"""
import ctypes

import numpy as np
import pytest

import absorb_ref
import farfield_ref as ffr
import ghost_ref
import illum_tir_ref as itr
from absorb_ref import ILLUM_GAPA, ILLUM_GAPS, ILLUM_GLASS
from ghost_ref import SEED
from test_gpu_farfield import check_far, target_frame
from test_gpu_illum_tir import check, identities, same
from test_gpu_power import set_cap

pytestmark = pytest.mark.gpu

F = np.float32
N = itr.N_RAYS
TABLE = [itr.ROW1]
MEDIA = (ILLUM_GAPS, ILLUM_GLASS, ILLUM_GAPA)
BUDGET = 4


@pytest.fixture(scope="module")
def world(bzr, orc, ctx):
    """The lens, its device mesh, the ghost reference with its draw log and the absorbing reference: computed once."""
    lenses = itr.lenses_of(bzr, "cfg2")
    dms = [bzr.DeviceMesh(ctx, p) for p in lenses]
    log = []
    ref = ghost_ref.illum_reference(orc, lenses, TABLE, *MEDIA, itr.NEAR, BUDGET, log=log)
    plain = absorb_ref.illum_reference(orc, lenses, TABLE, *MEDIA, itr.NEAR, BUDGET)
    return lenses, dms, ref, plain, ghost_ref.draw_stats(log)


def run(bzr, ctx, dms, mode, far=None, target="near", budget=BUDGET, seed=SEED, **kw):
    return bzr.illuminate_ghost(ctx, dms, TABLE, *MEDIA, itr.emitter(bzr, itr.NEAR), N,
                                itr.target(bzr) if target == "near" else None, far, max_bounces=budget, ghost_seed=seed,
                                mode=mode, **kw)


def test_reference_floors(world):
    """What the scene must show for the tests below to mean something (the reference alone, no device output)."""
    _, _, ref, plain, (draws, refl, expect, var, close) = world
    row1 = int((ref.uncut_count[:, 1, itr.EXITED]).sum()), int((plain.uncut_count[:, 1, itr.EXITED]).sum())
    print(f"{refl} of {draws} draws reflect (expected {expect:.1f}); row-1 EXITED {row1[0]} against {row1[1]}; landed "
          f"reflected rays {int(ref.rhist.sum())} against {int(plain.rhist.sum())}")
    assert refl >= 300
    assert abs(refl - expect) <= 4.0 * np.sqrt(var)
    assert row1[0] >= 200 and row1[1] < 100
    assert int(ref.rhist.sum()) > int(plain.rhist.sum()) >= 100


def test_near_and_far_bit_exact(bzr, ctx, pipe, world):
    _, dms, ref, _, _ = world
    fr = target_frame()
    want = ffr.of_illumination(fr, ref)
    assert int(want.binned.sum()) >= 1000 and int(want.reflected.sum()) >= 200
    got = run(bzr, ctx, dms, pipe, ffr.struct(bzr, fr))
    assert len(got) == 8
    culled = check(bzr, dms[0], ref, got[:7], "ghost, near outputs")
    assert not culled.any()  # the emitter lies inside the lens's sphere
    check_far(got[7], want, got[4:6], "ghost, far outputs")
    again = run(bzr, ctx, dms, pipe, ffr.struct(bzr, fr))
    assert same(again[:7], got[:7]) and np.array_equal(again[7]["flux"], got[7]["flux"])
    other = run(bzr, ctx, dms, pipe, ffr.struct(bzr, fr), seed=SEED + 1)
    assert not np.array_equal(other[6]["count"], got[6]["count"])


@pytest.fixture(scope="module")
def cctx(bzr, ctx):
    """This module's own context: the session context never sees a lowered chunk cap."""
    c = bzr.Context(0)
    yield c
    c.close()


def test_three_batches(bzr, cctx, pipe, world):
    """A chunk cap of 4 096: batches two and three start at emitter rays 4 096 and 8 192, and draw with those numbers."""
    lenses, _, ref, _, _ = world
    dm = [bzr.DeviceMesh(cctx, lenses[0])]
    fr = target_frame((24, 40))
    far = ffr.struct(bzr, fr)
    try:
        assert set_cap(bzr, cctx, 0) >= 1 << 14
        one = run(bzr, cctx, dm, pipe, far)
        assert set_cap(bzr, cctx, 4096) == 4096
        got = run(bzr, cctx, dm, pipe, far)
    finally:
        set_cap(bzr, cctx, 0)
    want = ffr.of_illumination(fr, ref)
    for label, g in (("one batch", one), ("three batches", got)):
        check(bzr, dm[0], ref, g[:7], label)
        check_far(g[7], want, g[4:6], label)
    assert same(got[:7], one[:7])


@pytest.mark.parametrize("fast", (False, True))
def test_ledger_identities(bzr, ctx, pipe, world, fast):
    _, dms, _, _, _ = world
    got = run(bzr, ctx, dms, pipe | (bzr.MODE_FAST if fast else 0))
    assert len(got) == 7
    identities(got, got[2], f"ghost, fast={fast}")
    assert int(got[6]["count"][:, 1:].sum()) >= 500 and int(got[3].sum()) >= 150


@pytest.mark.parametrize("what", ("budget 0", "lossless"))
def test_no_draw_is_illuminate_farfield(bzr, ctx, pipe, world, what):
    """max_bounces = 0, and SURFACE_LOSSLESS at budget 4 (no draw is taken): bzr_illuminate_farfield bit for bit."""
    _, dms, _, _, _ = world
    far = ffr.struct(bzr, target_frame())
    kw = dict(max_bounces=0) if what == "budget 0" else dict(max_bounces=BUDGET, surface=bzr.SURFACE_LOSSLESS)
    want = bzr.illuminate_farfield(ctx, dms, TABLE, *MEDIA, itr.emitter(bzr, itr.NEAR), N, itr.target(bzr), far, mode=pipe,
                                   **kw)
    got = bzr.illuminate_ghost(ctx, dms, TABLE, *MEDIA, itr.emitter(bzr, itr.NEAR), N, itr.target(bzr), far,
                               ghost_seed=SEED, mode=pipe, **kw)
    assert sum(s["landed"] for s in want[4]) >= 1000
    assert same(got[:7], want[:7])
    for k in ("flux", "hist", "reflected_flux"):
        assert np.array_equal(got[7][k], want[7][k]), k
    assert got[7]["stats"] == want[7]["stats"] and got[7]["power"] == want[7]["power"]
    if what == "lossless":  # total reflection still acts
        assert int(got[6]["count"][:, 1:].sum()) >= 100


def test_without_a_target_and_without_far(bzr, ctx, pipe, world):
    _, dms, ref, _, _ = world
    fr = target_frame()
    far = ffr.struct(bzr, fr)
    want = ffr.of_illumination(fr, ref)
    both = run(bzr, ctx, dms, pipe, far)
    no_target = run(bzr, ctx, dms, pipe, far, target=None)
    assert no_target[:4] == (None, None, None, None)
    check_far(no_target[7], want, no_target[4:6], "no target")
    for k in ("count", "power"):
        assert (no_target[6][k][:, :, itr.LANDED] == 0).all()
        assert np.array_equal(no_target[6][k][:, :, :2], both[6][k][:, :, :2])
    no_far = run(bzr, ctx, dms, pipe)
    assert len(no_far) == 7 and same(no_far, both[:7])
    check(bzr, dms[0], ref, no_far, "no far frame")
    # neither, and far outputs without a frame: refused with nothing touched
    with pytest.raises(bzr.BzrError, match="neither"):
        run(bzr, ctx, dms, pipe, target=None)
    em, rad = itr.emitter(bzr, itr.NEAR), bzr.Radiometry(1, 1)
    tg = itr.target(bzr)
    table = np.array(TABLE, F)
    handles = (ctypes.c_void_p * 1)(dms[0].handle)
    flux, far_flux = np.full((4, 48, 48), 5, np.uint64), np.full((4, 48, 48), 5, np.uint64)

    def raw(target, frame, far_map):
        return bzr.lib().bzr_illuminate_ghost(ctx.handle, handles, table.ctypes.data, None, None, None, 1, 4,
                                              ctypes.byref(em), N, target, ctypes.byref(rad), BUDGET, SEED,
                                              flux.ctypes.data if target is not None else None, None, None, None, None,
                                              None, None, None, pipe, frame, far_map, None, None, None, None)

    assert raw(None, None, None) == 1 and b"neither" in bzr.lib().bzr_last_error()
    assert raw(ctypes.byref(tg), None, far_flux.ctypes.data) == 1 and b"without a far-field frame" in bzr.lib().bzr_last_error()
    assert (flux == 5).all() and (far_flux == 5).all()
