"""bzr_illuminate_media on the GPU: illumination through the chain that reflects, refracts between media and absorbs,
against absorb_ref.illum_reference (illum_tir_ref's composition over absorb_ref.chain) bit for bit -- everything
compared is an integer.

The scenes are test_gpu_illum_tir.py's emitters (10 000 rays, `near` inside the cfg2 lens's bounding sphere, `far` with
most rays culled), here under an encapsulant: gap_table row 0 holds its index per channel, gap_absorb its absorption,
and the lens's glass absorbs too (channel 3's is opaque).
"""
import numpy as np
import pytest

import absorb_ref
import illum_tir_ref as itr
from absorb_ref import ILLUM_GAPA, ILLUM_GAPS, ILLUM_GLASS
from test_gpu_illum_tir import check, identities, same
from test_gpu_power import set_cap

pytestmark = pytest.mark.gpu

F = np.float32
N = itr.N_RAYS
TABLE = [itr.ROW1]
MEDIA = (ILLUM_GAPS, ILLUM_GLASS, ILLUM_GAPA)          # gap_table, glass_absorb, gap_absorb
MEDIA3 = tuple([row[:3] for row in t] for t in MEDIA)   # three channels
TABLE3 = [itr.ROW1[:3]]


@pytest.fixture(scope="module")
def world(bzr, orc, ctx):
    """The lens, its device mesh on the session context and the references, each computed once and frozen."""
    lenses = itr.lenses_of(bzr, "cfg2")
    dms = [bzr.DeviceMesh(ctx, p) for p in lenses]
    cache = {}

    def ref(nchan, origin, budget):
        key = (nchan, origin, budget)
        if key not in cache:
            table, media = (TABLE, MEDIA) if nchan == 4 else (TABLE3, MEDIA3)
            cache[key] = absorb_ref.illum_reference(orc, lenses, table, media[0], media[1], media[2], origin, budget)
        return cache[key]

    return lenses, dms, ref


def run(bzr, ctx, dms, table, media, origin, budget, mode, **kw):
    return bzr.illuminate_media(ctx, dms, table, media[0], media[1], media[2], itr.emitter(bzr, origin), N,
                                itr.target(bzr), max_bounces=budget, mode=mode, **kw)


# ------------------------------------------------------------------ 1. bit-exact, near scene
@pytest.mark.parametrize("budget", (0, 4))
def test_near_scene_bit_exact(bzr, orc, ctx, pipe, world, budget):
    lenses, dms, ref = world
    r = ref(4, itr.NEAR, budget)
    if budget:
        assert int(itr.reflected(r).sum()) >= 100
        # the media and the absorption changed what lands: not illum_tir_ref's maps
        vac = itr.reference(orc, lenses, TABLE, itr.NEAR, budget)
        assert not np.array_equal(vac.flux, r.flux) and not np.array_equal(vac.hist, r.hist)
    assert int(r.hist.sum()) >= 1000 and int((r.w == 0).sum()) >= 100  # opaque glass: rays of weight 0 still land
    got = run(bzr, ctx, dms, TABLE, MEDIA, itr.NEAR, budget, pipe)
    culled = check(bzr, dms[0], r, got, f"near, budget {budget}")
    assert not culled.any()  # the emitter lies inside the lens's sphere


# ------------------------------------------------------------------ 2. far scene: culled and reflecting rays
def test_far_scene(bzr, ctx, pipe, world):
    _, dms, ref = world
    r = ref(4, itr.FAR, 4)
    got = run(bzr, ctx, dms, TABLE, MEDIA, itr.FAR, 4, pipe)
    check(bzr, dms[0], r, got, "far, budget 4")  # (the ledger adjusted by illum_tir_ref.ledger_for)
    assert sum(s["culled"] for s in got[4]) > 2000
    assert int(itr.reflected(r).sum()) >= 20


# ------------------------------------------------------------------ 3. three batches
@pytest.fixture(scope="module")
def cctx(bzr, ctx):
    """This module's own context: the session context never sees a lowered chunk cap."""
    c = bzr.Context(0)
    yield c
    c.close()


def test_three_batches(bzr, cctx, pipe, world):
    """10 000 rays at a chunk cap of 4 096, three channels: batches two and three reuse batch one's bounce, optical path
    and pending rows.  Host maps, then device maps."""
    torch = pytest.importorskip("torch")
    lenses, _, ref = world
    dm = [bzr.DeviceMesh(cctx, lenses[0])]
    fused = pipe == bzr.PIPELINE_FUSED
    shape = (3, 48, 48)
    try:
        assert set_cap(bzr, cctx, 0) >= 1 << 14
        one = run(bzr, cctx, dm, TABLE3, MEDIA3, itr.FAR, 4, pipe)
        assert set_cap(bzr, cctx, 4096) == 4096
        cctx.timing(True)
        cctx.timing_report()
        got = run(bzr, cctx, dm, TABLE3, MEDIA3, itr.FAR, 4, pipe)
        rep = cctx.timing_report()
        cctx.timing(False)
        flux, rflux = (torch.zeros(shape, dtype=torch.int64, device="cuda") for _ in range(2))
        hist, rhist = (torch.zeros(shape, dtype=torch.int32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        cctx.use_torch_stream()
        try:
            dev = run(bzr, cctx, dm, TABLE3, MEDIA3, itr.FAR, 4, pipe, flux=flux, hist=hist, reflected_flux=rflux,
                      reflected_hist=rhist)
            torch.cuda.synchronize()
        finally:
            cctx.use_own_stream()
    finally:
        cctx.timing(False)
        set_cap(bzr, cctx, 0)
    # fused: one k_trace per batch; staged: per batch the INSIDE stage and 1 + 4 OUTSIDE stages
    assert rep["k_trace" if fused else "k_traverse"][1] == (3 if fused else 3 * 6)
    assert same(got, one)
    r3 = ref(3, itr.FAR, 4)
    assert int(itr.reflected(r3).sum()) >= 10
    check(bzr, dm[0], r3, got, "three batches, three channels")
    maps = tuple(a.cpu().numpy().view(t) for a, t in zip(dev[:4], (np.uint64, np.uint32, np.uint64, np.uint32)))
    assert same(maps + tuple(dev[4:]), got)


# ------------------------------------------------------------------ 4. vacuum, no absorption
@pytest.mark.parametrize("fast", (False, True))
@pytest.mark.parametrize("budget", (0, 4))
def test_vacuum_and_zero_tables_are_illuminate_tir(bzr, ctx, pipe, world, budget, fast):
    _, dms, _ = world
    mode = pipe | (bzr.MODE_FAST if fast else 0)
    want = bzr.illuminate_tir(ctx, dms, TABLE, itr.emitter(bzr, itr.NEAR), N, itr.target(bzr), max_bounces=budget,
                              mode=mode)
    assert sum(s["landed"] for s in want[4]) > 2000
    ones, zeros = np.ones((2, 4), F), np.zeros((1, 4), F)
    for media in ((None, None, None), (ones, zeros, zeros), (ones, None, zeros)):
        got = run(bzr, ctx, dms, TABLE, media, itr.NEAR, budget, mode)
        assert same(got, want), (budget, fast)


# ------------------------------------------------------------------ 5. where the power went
def test_lossless_surfaces_lose_what_the_media_absorb(bzr, ctx, pipe, world):
    """BZR_SURFACE_LOSSLESS with absorption: every count identity holds, and LOST + EXITED power is strictly less than
    EMITTED - CULLED in every channel that absorbs (all four here)."""
    _, dms, _ = world
    got = run(bzr, ctx, dms, TABLE, MEDIA, itr.FAR, 4, pipe, surface=bzr.SURFACE_LOSSLESS)
    identities(got, got[2], "lossless, absorbing")  # the counts, and the power lines that hold either way (<=)
    _, _, _, _, stats, power, ledger = got
    assert sum(s["culled"] for s in stats) > 2000
    for c in range(4):
        ended = int(ledger["power"][c, :, :2].sum())
        traced = power[c]["emitted"] - power[c]["culled"]
        assert ended < traced, c
    # without absorption (the same media) the line is an equality again
    got = run(bzr, ctx, dms, TABLE, (ILLUM_GAPS, None, None), itr.FAR, 4, pipe, surface=bzr.SURFACE_LOSSLESS)
    identities(got, got[2], "lossless, clear media", lossless=True)


def test_bad_tables_leave_the_outputs_untouched(bzr, ctx, world):
    _, dms, _ = world
    for which in range(3):
        for value in (-1.0, np.nan, np.inf):
            media = [np.array(t, F) for t in MEDIA]
            media[which][0, 1] = value
            flux = np.full((4, 48, 48), 5, np.uint64)
            with pytest.raises(bzr.BzrError, match=("gap_table", "glass_absorb", "gap_absorb")[which]):
                run(bzr, ctx, dms, TABLE, media, itr.NEAR, 4, 0, flux=flux)
            assert (flux == 5).all()
