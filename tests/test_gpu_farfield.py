"""Far-field maps on the GPU: bzr_farfield_bin and bzr_illuminate_farfield against farfield_ref (the cell rule in numpy
float32 over rows from illum_tir_ref / absorb_ref) bit for bit -- everything compared is an integer -- and, through
farfield64, against cells computed independently in binary64 within a derived margin.

Every test uses 10 000 rays or fewer and maps no larger than 48 x 48.
"""
import numpy as np
import pytest

import absorb_ref
import farfield64
import farfield_ref as ffr
import illum_tir_ref as itr
from absorb_ref import ILLUM_GAPA, ILLUM_GAPS, ILLUM_GLASS
from test_farfield_host import X_POLE, tilted
from test_gpu_illum_tir import same
from test_gpu_power import set_cap

pytestmark = pytest.mark.gpu

F = np.float32
N = itr.N_RAYS
TABLE = [itr.ROW1]
MEDIA = (ILLUM_GAPS, ILLUM_GLASS, ILLUM_GAPA)
MEDIA3 = tuple([row[:3] for row in t] for t in MEDIA)
TABLE3 = [itr.ROW1[:3]]
VACUUM = (None, None, None)
FAR_KEYS = ("seen", "binned")


def target_frame(bins=(48, 48)):
    """The frame whose axes are the target's (itr.target: axis_u = +y, axis_v = +z, pole +x), R = sqrt(2)."""
    return ffr.frame(*X_POLE, ffr.SQRT2, *bins)


def inverse(fr, X, Y):
    """Directions [3, n] float32 of map points (X, Y), the inverse projection in binary64."""
    n64, u64, v64 = (np.asarray(a, np.float64) for a in (fr.n, fr.axis_u, fr.axis_v))
    rho2 = X * X + Y * Y
    w = np.sqrt(1 - rho2 / 4)
    return ((X * w)[None] * u64[:, None] + (Y * w)[None] * v64[:, None] + (1 - rho2 / 2)[None] * n64[:, None]).astype(F)


def centres(fr):
    R = float(fr.R)
    X = -R + 2 * R * (np.arange(fr.bins_u) + 0.5) / fr.bins_u
    Y = -R + 2 * R * (np.arange(fr.bins_v) + 0.5) / fr.bins_v
    X, Y = np.meshgrid(X, Y)
    return inverse(fr, X.ravel(), Y.ravel())


def rays_of(d):
    rays = np.zeros((6, d.shape[1]), F)
    rays[:3] = np.random.default_rng(d.shape[1]).uniform(-5, 5, (3, d.shape[1]))  # the starts are not read
    rays[3:] = d
    return rays


def sphere(n, seed):
    d = np.random.default_rng(seed).standard_normal((3, n))
    return (d / np.linalg.norm(d, axis=0)).astype(F)


def rows(n, seed, nchan):
    """weight, status, channel [n]: weights in [0, 1] with 0, 1, NaN and negative ones among them, every status, channels
    0 .. nchan + 1 (two of them out of range)."""
    rng = np.random.default_rng(seed)
    w = rng.random(n, dtype=F)
    for k, v in enumerate((0.0, 1.0, np.nan, -0.5, -0.0, 2.0 ** -33)):
        w[k::11] = v
    status = rng.choice(np.array([0, 1, 2, 2, 2], np.uint32), n)
    channel = rng.integers(0, nchan + 2, n).astype(np.uint8)
    return w, status, channel


def check_bin(got, want, label):
    flux, hist, stats, power = got
    assert flux.dtype == np.uint64 and hist.dtype == np.uint32, label
    assert np.array_equal(flux, want.flux), (label, int(flux.sum()), int(want.flux.sum()))
    assert np.array_equal(hist, want.hist), label
    for c in range(want.stats.shape[0]):
        assert stats[c] == dict(zip(FAR_KEYS, (int(x) for x in want.stats[c]))), (label, c)
        assert power[c] == dict(zip(FAR_KEYS, (int(x) for x in want.power[c]))), (label, c)


# ------------------------------------------------------------------ 1. farfield_bin on synthetic rows
@pytest.mark.parametrize("n", (1, 63, 64, 65, 1000))
def test_bin_partial_waves(bzr, ctx, n):
    """Every row given, four channels, 24 x 40 bins (a u / v transposition would show), tilted frame."""
    fr = ffr.frame(*tilted(), ffr.SQRT2, 24, 40)
    rays = rays_of(sphere(n, 100 + n))
    w, status, channel = rows(n, n, 4)
    want = ffr.bin_rays(fr, rays, w, status, channel, 4)
    if n == 1000:
        assert want.binned.sum() > 200 and (~want.seen).sum() > 200 and np.isnan(w[want.binned]).any()
        assert (w[want.binned] == 0).any() and (w[want.binned] == 1).any() and (w[want.binned] < 0).any()
        assert (channel >= 4).sum() > 100 and all((status == s).sum() > 100 for s in (0, 1, 2))
    check_bin(bzr.farfield_bin(ctx, ffr.struct(bzr, fr), rays, w, status, channel, nchan=4), want, f"n = {n}")


def test_bin_one_cell_map(bzr, ctx):
    """A 1 x 1 map: every lane of every wave holds the same key, the combine's worst case.  The cell's sum is the sum of
    q over the binned rays, exactly."""
    fr = ffr.frame(*X_POLE, 1.0, 1, 1)
    rays = rays_of(sphere(1000, 5))
    w = np.random.default_rng(6).random(1000, dtype=F)
    want = ffr.bin_rays(fr, rays, w)
    assert 300 < want.binned.sum() < 1000  # R = 1: some directions fall outside the map
    got = bzr.farfield_bin(ctx, ffr.struct(bzr, fr), rays, w)
    check_bin(got, want, "1 x 1")
    assert int(got[0][0, 0, 0]) == int(ffr.q32(w)[want.binned].sum(dtype=np.uint64)) == got[3][0]["binned"]


def test_bin_distinct_and_alternating_cells(bzr, ctx):
    """A wave whose 64 lanes hold 64 distinct cells (no round of the combine merges anything: the leftover path), then
    one partial wave of the same, then lanes that alternate between two cells."""
    fr = ffr.frame(*tilted(), 1.0, 8, 8)
    far = ffr.struct(bzr, fr)
    d = centres(fr)
    assert np.array_equal(ffr.cell(fr, d), np.arange(64))
    w = np.random.default_rng(8).random(64 + 37, dtype=F)
    rays = rays_of(np.concatenate([d, d[:, ::-1][:, :37]], axis=1))
    want = ffr.bin_rays(fr, rays, w)
    assert want.hist.max() == 2 and want.hist.sum() == 101
    check_bin(bzr.farfield_bin(ctx, far, rays, w), want, "64 distinct cells")
    two = rays_of(d[:, np.where(np.arange(200) % 2, 9, 54)])
    w2 = np.random.default_rng(9).random(200, dtype=F)
    want2 = ffr.bin_rays(fr, two, w2)
    assert sorted(want2.hist.ravel())[-2:] == [100, 100]
    check_bin(bzr.farfield_bin(ctx, far, two, w2), want2, "two alternating cells")


def test_bin_small_extent_and_null_rows(bzr, ctx, pipe):
    """R = 0.5 rejects most rays; weight, status and channel NULL (1.0f, every ray seen, channel 0); both pipelines' flags
    are accepted and change nothing."""
    fr = ffr.frame(*tilted(), 0.5, 7, 3)
    rays = rays_of(sphere(1000, 21))
    want = ffr.bin_rays(fr, rays)
    assert 20 < want.binned.sum() < 200 and want.stats[0, 0] == 1000
    got = bzr.farfield_bin(ctx, ffr.struct(bzr, fr), rays, mode=pipe)
    check_bin(got, want, "R = 0.5")
    assert int(got[0].sum()) == int(want.binned.sum()) << 32
    plain = bzr.farfield_bin(ctx, ffr.struct(bzr, fr), rays)
    assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1]) and plain[2:] == got[2:]
    only_hist = np.zeros((1, 3, 7), np.uint32)
    L = bzr.lib()
    import ctypes
    assert L.bzr_farfield_bin(ctx.handle, ctypes.byref(ffr.struct(bzr, fr)), rays.ctypes.data, None, None, None, 1000, 1,
                              None, only_hist.ctypes.data, None, None, 0) == 0
    assert np.array_equal(only_hist, want.hist)


def test_bin_accumulates_host_then_device(bzr, ctx):
    """Host maps, then device maps on torch's stream, each onto a non-zero start."""
    torch = pytest.importorskip("torch")
    fr = ffr.frame(*X_POLE, ffr.SQRT2, 24, 40)
    far = ffr.struct(bzr, fr)
    n = 1000
    rays = rays_of(sphere(n, 31))
    w, status, channel = rows(n, 32, 3)
    want = ffr.bin_rays(fr, rays, w, status, channel, 3)
    rng = np.random.default_rng(33)
    flux0 = rng.integers(0, 1 << 50, want.flux.shape, dtype=np.uint64)
    hist0 = rng.integers(0, 1 << 20, want.hist.shape, dtype=np.uint32)
    flux, hist = flux0.copy(), hist0.copy()
    got = bzr.farfield_bin(ctx, far, rays, w, status, channel, nchan=3, flux=flux, hist=hist)
    assert got[0] is flux and np.array_equal(flux, flux0 + want.flux) and np.array_equal(hist, hist0 + want.hist)
    dev = [torch.from_numpy(a).cuda() for a in (rays, w, status.view(np.int32), channel, flux0.view(np.int64),
                                                hist0.view(np.int32))]
    torch.cuda.synchronize()
    out = bzr.farfield_bin(ctx, far, dev[0], dev[1], dev[2], dev[3], nchan=3, flux=dev[4], hist=dev[5])
    torch.cuda.synchronize()
    assert np.array_equal(dev[4].cpu().numpy().view(np.uint64), flux0 + want.flux)
    assert np.array_equal(dev[5].cpu().numpy().view(np.uint32), hist0 + want.hist)
    assert out[2:] == got[2:]


def test_bin_fast_mode_and_every_round_count(bzr, ctx):
    """BZR_MODE_FAST bins exactly as parity does (the rule is correctly rounded in both modes), and the combine gives
    the same bits at 0 rounds (plain atomics), the default and unbounded."""
    fr = target_frame((16, 16))
    far = ffr.struct(bzr, fr)
    n = 5000
    cone = sphere(n, 41) * F(0.05)
    cone[0] += 1                      # a narrow beam about the pole: most lanes of a wave share few cells
    rays = rays_of((cone / np.linalg.norm(cone, axis=0)).astype(F))
    w, status, channel = rows(n, 42, 2)
    want = ffr.bin_rays(fr, rays, w, status, channel, 2)
    assert np.count_nonzero(want.hist) < 16 and want.hist.max() > 150  # (about 1 500 seen rays over 2 x 4 cells)
    parity = bzr.farfield_bin(ctx, far, rays, w, status, channel, nchan=2)
    check_bin(parity, want, "beam")
    check_bin(bzr.farfield_bin(ctx, far, rays, w, status, channel, nchan=2, mode=bzr.MODE_FAST), want, "beam, FAST")
    try:
        for rounds in (0, 1, 64):
            bzr.debug_farfield_rounds(ctx, rounds)
            check_bin(bzr.farfield_bin(ctx, far, rays, w, status, channel, nchan=2), want, f"{rounds} rounds")
    finally:
        bzr.debug_farfield_rounds(ctx, -1)


def test_bin_against_binary64_cells(bzr, ctx):
    """The independent check: per-cell lower and upper bounds from cells computed in binary64 with arccos and arctan2, on
    a tilted, non-square map."""
    fr = ffr.frame(*tilted(), 1.25, 24, 40)
    d = sphere(10_000, 51)
    # (towards the direction opposite the pole the margin grows without bound; the map's corners lie at mu = -0.56)
    d = np.ascontiguousarray(d[:, np.asarray(fr.n, np.float64) @ d > -0.9])
    lower, upper, unsure = farfield64.bounds(fr, d)
    assert unsure < 20 and lower.sum() > 3000
    _, hist, _, _ = bzr.farfield_bin(ctx, ffr.struct(bzr, fr), rays_of(d))
    assert (hist[0] >= lower).all() and (hist[0] <= upper).all()
    assert lower.sum() <= int(hist.sum()) <= upper.sum()


# ------------------------------------------------------------------ illuminate_farfield
@pytest.fixture(scope="module")
def world(bzr, orc, ctx):
    """The lens, its device mesh on the session context and the references, each computed once and frozen."""
    lenses = itr.lenses_of(bzr, "cfg2")
    dms = [bzr.DeviceMesh(ctx, p) for p in lenses]
    cache = {}

    def ref(nchan, origin, budget, vacuum=False):
        key = (nchan, origin, budget, vacuum)
        if key not in cache:
            table, media = (TABLE, MEDIA) if nchan == 4 else (TABLE3, MEDIA3)
            if vacuum:
                cache[key] = itr.reference(orc, lenses, table, origin, budget)
            else:
                cache[key] = absorb_ref.illum_reference(orc, lenses, table, media[0], media[1], media[2], origin, budget)
        return cache[key]

    return lenses, dms, ref


def run(bzr, ctx, dms, table, media, origin, budget, mode, far, target="near", **kw):
    return bzr.illuminate_farfield(ctx, dms, table, media[0], media[1], media[2], itr.emitter(bzr, origin), N,
                                   itr.target(bzr) if target == "near" else None, far, max_bounces=budget, mode=mode, **kw)


def check_far(got_far, want, ref_stats, label):
    """The far dict against farfield_ref.of_illumination; SEEN against the near stats' EXITED."""
    assert np.array_equal(got_far["flux"], want.flux), label
    assert np.array_equal(got_far["hist"], want.hist), label
    assert np.array_equal(got_far["reflected_flux"], want.rflux), label
    stats, power = ref_stats
    for c in range(want.stats.shape[0]):
        assert got_far["stats"][c] == dict(zip(FAR_KEYS, (int(x) for x in want.stats[c]))), (label, c)
        assert got_far["power"][c] == dict(zip(FAR_KEYS, (int(x) for x in want.power[c]))), (label, c)
        assert got_far["stats"][c]["seen"] == stats[c]["exited"] and got_far["power"][c]["seen"] == power[c]["exited"]


@pytest.mark.parametrize("budget", (0, 4))
def test_near_scene_bit_exact(bzr, ctx, pipe, world, budget):
    _, dms, ref = world
    r = ref(4, itr.NEAR, budget)
    fr = target_frame()
    want = ffr.of_illumination(fr, r)
    assert int(want.binned.sum()) >= 1000 and int(r.hist.sum()) >= 1000
    got = run(bzr, ctx, dms, TABLE, MEDIA, itr.NEAR, budget, pipe, ffr.struct(bzr, fr))
    assert len(got) == 8
    check_far(got[7], want, got[4:6], f"near, budget {budget}")
    near = bzr.illuminate_media(ctx, dms, TABLE, MEDIA[0], MEDIA[1], MEDIA[2], itr.emitter(bzr, itr.NEAR), N,
                                itr.target(bzr), max_bounces=budget, mode=pipe)
    assert same(got[:7], near)
    assert np.array_equal(got[0], r.flux) and np.array_equal(got[1], r.hist)


def test_vacuum_reflected_far_map(bzr, ctx, pipe, world):
    """illum_tir_ref's vacuum NEAR scene at four reflections: the stray light in angle."""
    _, dms, ref = world
    r = ref(4, itr.NEAR, 4, vacuum=True)
    fr = target_frame()
    want = ffr.of_illumination(fr, r)
    assert int(want.reflected.sum()) >= 50
    got = run(bzr, ctx, dms, TABLE, VACUUM, itr.NEAR, 4, pipe, ffr.struct(bzr, fr))
    check_far(got[7], want, got[4:6], "vacuum, reflected")
    assert int(got[7]["reflected_flux"].sum()) == int(ffr.q32(r.w)[want.reflected].sum(dtype=np.uint64)) > 0
    assert np.array_equal(got[2], r.rflux)


@pytest.fixture(scope="module")
def cctx(bzr, ctx):
    """This module's own context: the session context never sees a lowered chunk cap."""
    c = bzr.Context(0)
    yield c
    c.close()


def test_three_batches(bzr, cctx, pipe, world):
    """The FAR scene at a chunk cap of 4 096, three channels: three batches add into the same far maps.  Host maps, then
    device maps on the torch stream."""
    torch = pytest.importorskip("torch")
    lenses, _, ref = world
    dm = [bzr.DeviceMesh(cctx, lenses[0])]
    fr = ffr.frame(*X_POLE, ffr.SQRT2, 24, 40)
    far = ffr.struct(bzr, fr)
    try:
        assert set_cap(bzr, cctx, 0) >= 1 << 14
        one = run(bzr, cctx, dm, TABLE3, MEDIA3, itr.FAR, 4, pipe, far)
        assert set_cap(bzr, cctx, 4096) == 4096
        got = run(bzr, cctx, dm, TABLE3, MEDIA3, itr.FAR, 4, pipe, far)
        near = [torch.zeros((3, 48, 48), dtype=t, device="cuda") for t in (torch.int64, torch.int32, torch.int64, torch.int32)]
        fard = [torch.zeros((3, 40, 24), dtype=t, device="cuda") for t in (torch.int64, torch.int32, torch.int64)]
        torch.cuda.synchronize()
        cctx.use_torch_stream()
        try:
            dev = run(bzr, cctx, dm, TABLE3, MEDIA3, itr.FAR, 4, pipe, far, flux=near[0], hist=near[1],
                      reflected_flux=near[2], reflected_hist=near[3], far_flux=fard[0], far_hist=fard[1],
                      far_reflected_flux=fard[2])
            torch.cuda.synchronize()
        finally:
            cctx.use_own_stream()
    finally:
        set_cap(bzr, cctx, 0)
    r3 = ref(3, itr.FAR, 4)
    want = ffr.of_illumination(fr, r3)
    assert int(want.binned.sum()) >= 200 and int(want.reflected.sum()) >= 10
    for label, g in (("one batch", one), ("three batches", got)):
        check_far(g[7], want, g[4:6], label)
    assert same(got[:7], one[:7])
    assert sum(s["culled"] for s in got[4]) > 2000
    maps = tuple(a.cpu().numpy().view(t) for a, t in zip(dev[:4], (np.uint64, np.uint32, np.uint64, np.uint32)))
    assert same(maps + tuple(dev[4:7]), got[:7])
    for k, t in (("flux", np.uint64), ("hist", np.uint32), ("reflected_flux", np.uint64)):
        assert np.array_equal(dev[7][k].cpu().numpy().view(t), got[7][k]), k
    assert dev[7]["stats"] == got[7]["stats"] and dev[7]["power"] == got[7]["power"]


def test_without_a_target(bzr, ctx, pipe, world):
    _, dms, ref = world
    r = ref(4, itr.NEAR, 4)
    fr = target_frame()
    far = ffr.struct(bzr, fr)
    want = ffr.of_illumination(fr, r)
    got = run(bzr, ctx, dms, TABLE, MEDIA, itr.NEAR, 4, pipe, far, target=None)
    assert got[:4] == (None, None, None, None)
    check_far(got[7], want, got[4:6], "no target")
    with_target = run(bzr, ctx, dms, TABLE, MEDIA, itr.NEAR, 4, pipe, far)
    for c in range(4):
        for tot, ref_tot in ((got[4][c], with_target[4][c]), (got[5][c], with_target[5][c])):
            assert tot["landed"] == 0
            assert {k: v for k, v in tot.items() if k != "landed"} == {k: v for k, v in ref_tot.items() if k != "landed"}
    assert sum(s["landed"] for s in with_target[4]) >= 1000  # (channel 3's glass is opaque: its landed power is 0)
    for k in ("count", "power"):
        assert (got[6][k][:, :, itr.LANDED] == 0).all()
        assert np.array_equal(got[6][k][:, :, :2], with_target[6][k][:, :, :2])
    flux = np.full((4, 48, 48), 5, np.uint64)
    far_flux = np.full((4, 48, 48), 5, np.uint64)
    with pytest.raises(bzr.BzrError, match="without a target"):
        run(bzr, ctx, dms, TABLE, MEDIA, itr.NEAR, 4, pipe, far, target=None, flux=flux, far_flux=far_flux)
    import ctypes
    em, rad = itr.emitter(bzr, itr.NEAR), bzr.Radiometry(1, 1)
    table = np.array(TABLE, F)
    handles = (ctypes.c_void_p * 1)(dms[0].handle)
    assert bzr.lib().bzr_illuminate_farfield(ctx.handle, handles, table.ctypes.data, None, None, None, 1, 4,
                                             ctypes.byref(em), N, None, ctypes.byref(rad), 4, flux.ctypes.data, None, None,
                                             None, None, None, None, None, pipe, ctypes.byref(far), far_flux.ctypes.data,
                                             None, None, None, None) == 1
    assert b"without a target" in bzr.lib().bzr_last_error()
    assert (flux == 5).all() and (far_flux == 5).all()


def test_bad_arguments_leave_the_outputs_untouched(bzr, ctx, world):
    _, dms, _ = world
    rays = rays_of(sphere(100, 61))
    flux, hist = np.full((1, 8, 8), 5, np.uint64), np.full((1, 8, 8), 5, np.uint32)
    far_flux = np.full((4, 8, 8), 5, np.uint64)
    for kw, msg in (({"extent": 0.0}, "extent"), ({"extent": 1.5}, "extent"), ({"extent": float("nan")}, "extent"),
                    ({"bins_u": 0}, "bins"), ({"bins_v": 0}, "bins")):
        far = bzr.FarField(axis_u=(0, 1, 0), axis_v=(0, 0, 1), **{"extent": 1.0, "bins_u": 8, "bins_v": 8, **kw})
        with pytest.raises(bzr.BzrError, match=msg):
            bzr.farfield_bin(ctx, far, rays, flux=flux, hist=hist)
        with pytest.raises(bzr.BzrError, match=msg):
            run(bzr, ctx, dms, TABLE, MEDIA, itr.NEAR, 4, 0, far, far_flux=far_flux)
    import ctypes
    good = bzr.FarField(axis_u=(0, 1, 0), axis_v=(0, 0, 1), extent=1.0, bins_u=8, bins_v=8)
    stats = np.full((1, 2), 5, np.uint64)
    assert bzr.lib().bzr_farfield_bin(ctx.handle, ctypes.byref(good), rays.ctypes.data, None, None, None, 100, 1, None,
                                      None, stats.ctypes.data, None, 0) == 1
    assert b"far_flux_q32 and far_hist" in bzr.lib().bzr_last_error()
    assert (flux == 5).all() and (hist == 5).all() and (far_flux == 5).all() and (stats == 5).all()
