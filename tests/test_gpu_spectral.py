"""Spectral ray tracing on the GPU: bzr_trace_chain_spectral and bzr_illuminate_spectral against the oracle, bit for
bit.

A chain over rays with mixed channels is, ray for ray, the union of the single-index chains of each channel's rays
(tests/spectral_ref.py), so the reference is the power reference run once per channel.  The populations the tests rely
on are asserted from the reference, so none passes vacuously.
"""
import ctypes

import numpy as np
import pytest

import power_ref
import spectral_ref
from bzr_amd.configs import CONFIGS, build_lens, grid_rays
from test_chunk_plan import chunk_rule
from test_gpu_illumination import emitter, target
from test_gpu_long_chains import chain_rays, lens_patches
from test_gpu_power import assert_same, bits, culled_by_sphere, flags_of, frozen, set_cap

pytestmark = pytest.mark.gpu

F = np.float32
PATHS = ("fused", "staged", "brute")
SIDE, DROP, NCHAN = 64, 37, 4
ROW1 = [1.290, 1.297, 1.304, 1.312]  # lens 1's index per channel
ROW2 = [1.50, 1.5168, 1.53, 1.62]    # cfg4's second lens
TABLES = {"cfg2": [ROW1], "cfg4": [ROW1, ROW2]}


def run(bzr, ctx, dms, table, rays, channel, path, **kw):
    return bzr.trace_chain_spectral(ctx, dms, table, rays, channel, mode=flags_of(bzr, path), **kw)


@pytest.fixture(scope="module")
def scenes(bzr, orc, ctx):
    """name -> (patches, table, device meshes, rays, channel, random input weights, reference with weight 1, reference
    with the random weights, reference with every ray in channel 0): computed once, never changed."""
    out = {}
    for name, table in TABLES.items():
        cfg = CONFIGS[name]
        lenses = [build_lens(bzr.TriMesh, lens).bezier_patches() for lens in cfg.lenses]
        rays = grid_rays(cfg, side=SIDE)
        n = rays.shape[1] - DROP
        rays = np.ascontiguousarray(rays[:, :n])
        channel = np.random.default_rng(7).integers(0, NCHAN, SIDE * SIDE)[:n].astype(np.uint8)
        w_in = np.random.default_rng(41).random(n, dtype=F)
        ones = frozen(*spectral_ref.chain(orc, lenses, table, rays, channel))
        rand = frozen(*spectral_ref.chain(orc, lenses, table, rays, channel, w_in))
        zero = frozen(*spectral_ref.chain(orc, lenses, table, rays, np.zeros(n, np.uint8)))
        frozen(rays, channel, w_in)
        out[name] = (lenses, table, [bzr.DeviceMesh(ctx, p) for p in lenses], rays, channel, w_in, ones, rand, zero)
    return out


# ------------------------------------------------------------------ 1. mixed channels
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(TABLES))
def test_mixed_channels_bit_exact(bzr, ctx, scenes, name, path):
    _, table, dms, rays, channel, w_in, ones, rand, zero = scenes[name]
    n = rays.shape[1]
    assert n == SIDE * SIDE - DROP and n % 64 != 0
    # populations, from the reference: every channel exits often, every wave holds all four channels, and the colours
    # matter -- status, bits and (two lenses) the segment count differ from the all-channel-0 trace
    for c in range(NCHAN):
        assert int(((channel == c) & (ones[2] == bzr.RR_OUTSIDE)).sum()) >= 550, c
    assert all(len(set(channel[k:k + 64])) == NCHAN for k in range(0, n - 63, 64))
    assert int((ones[2] != zero[2]).sum()) >= 15
    assert int((bits(ones[0]) != bits(zero[0])).any(axis=0).sum()) >= 1500
    if name == "cfg4":
        assert int((ones[3] != zero[3]).sum()) >= 15
    got = run(bzr, ctx, dms, table, rays, channel, path)
    assert_same(got, ones, f"{name} {path}, weight=None: vs the reference")
    w = w_in.copy()  # passed in place
    got = run(bzr, ctx, dms, table, rays, channel, path, weight=w, out_weight=w)
    assert got[1] is w
    assert_same(got, rand, f"{name} {path}, random weights in place: vs the reference")


# ------------------------------------------------------------------ 2. uniform table, FAST
@pytest.mark.parametrize("path", PATHS)
def test_uniform_table_is_the_power_chain(bzr, ctx, scenes, path):
    _, _, dms, rays, channel, w_in, _, _, _ = scenes["cfg4"]
    table = np.full((2, NCHAN), 1.3, F)
    want = bzr.trace_chain_power(ctx, dms, [1.3, 1.3], rays, weight=w_in, mode=flags_of(bzr, path))
    got = run(bzr, ctx, dms, table, rays, channel, path, weight=w_in)
    assert int((want[2] == bzr.RR_OUTSIDE).sum()) > 1500
    assert_same(got, tuple(np.asarray(a) for a in want), f"uniform table, {path}: vs trace_chain_power")


@pytest.mark.parametrize("pipe_name", ("fused", "staged"))
def test_fast_mode(bzr, ctx, scenes, pipe_name):
    """FAST with a uniform table is trace_chain_power's FAST result bit for bit.  With mixed channels, how far the
    FAST weights lie from the parity ones is recorded (printed); the distance from the truth is what tests/test_gpu_fast_chain64.py asserts."""
    _, table, dms, rays, channel, _, ones, _, _ = scenes["cfg4"]
    mode = flags_of(bzr, pipe_name) | bzr.MODE_FAST
    want = bzr.trace_chain_power(ctx, dms, [1.3, 1.3], rays, mode=mode)
    got = bzr.trace_chain_spectral(ctx, dms, np.full((2, NCHAN), 1.3, F), rays, channel, mode=mode)
    assert_same(got, tuple(np.asarray(a) for a in want), f"FAST {pipe_name}, uniform table: vs trace_chain_power")
    got = bzr.trace_chain_spectral(ctx, dms, table, rays, channel, mode=mode)
    assert (got[1] > 0).all() and (got[1] <= 1).all()
    agree = (got[2] == ones[2]) & (got[3] == ones[3])
    rel = np.abs(got[1][agree].astype(np.float64) - ones[1][agree]) / ones[1][agree]
    print(f"FAST {pipe_name}, four channels: {int(agree.sum())} of {len(agree)} rays agree in status and segments; "
          f"|w_fast - w_parity| / w_parity median {np.median(rel):.3g}, p99 {np.quantile(rel, 0.99):.3g}, "
          f"max {rel.max():.3g}")
    assert agree.sum() > 3_900


# ------------------------------------------------------------------ 3. layouts and residency
def test_device_buffers_and_aos(bzr, ctx, scenes):
    """Device tensors for rays, channel and weight (the asynchronous path) and [n, 6] ray records: the same bits."""
    torch = pytest.importorskip("torch")
    _, table, dms, rays, channel, w_in, _, rand, _ = scenes["cfg4"]
    r = torch.from_numpy(np.ascontiguousarray(rays.T)).cuda()
    c = torch.from_numpy(channel.copy()).cuda()
    w = torch.from_numpy(w_in.copy()).cuda()
    for pipe in (bzr.PIPELINE_FUSED, bzr.PIPELINE_STAGED):
        o, ow, s, g = bzr.trace_chain_spectral(ctx, dms, table, r, c, weight=w, mode=pipe | bzr.RAYS_AOS)
        torch.cuda.synchronize()
        got = (np.ascontiguousarray(o.cpu().numpy().T), ow.cpu().numpy(), s.cpu().numpy().astype(np.uint32),
               g.cpu().numpy().astype(np.uint32))
        assert_same(got, rand, f"cfg4 device pointers, AoS, pipeline {pipe}")
    got = bzr.trace_chain_spectral(ctx, dms, table, np.ascontiguousarray(rays.T), channel, weight=w_in,
                                   mode=bzr.RAYS_AOS)
    assert_same((np.ascontiguousarray(got[0].T),) + got[1:], rand, "cfg4 host pointers, AoS")


# ------------------------------------------------------------------ 4. small chunks
@pytest.fixture(scope="module")
def cctx(bzr, ctx):
    """This module's own context: the session context never sees a lowered chunk cap."""
    c = bzr.Context(0)
    yield c
    c.close()


def test_small_chunks(bzr, orc, cctx):
    """The channel row is indexed by the global ray index: a row read without the chunk offset fails here."""
    cfg = CONFIGS["cfg2"]
    lens = build_lens(bzr.TriMesh, cfg.lenses[0]).bezier_patches()
    full = grid_rays(cfg, side=128)
    n = 1000
    first = (full.shape[1] - n) // 2  # the grid's centre in tile order: every ray meets the lens
    rays = np.ascontiguousarray(full[:, first:first + n])
    channel = np.random.default_rng(9).integers(0, NCHAN, n).astype(np.uint8)
    w_in = np.random.default_rng(5).random(n, dtype=F)
    want = spectral_ref.chain(orc, [lens], [ROW1], rays, channel, w_in)
    zero = spectral_ref.chain(orc, [lens], [ROW1], rays, np.zeros(n, np.uint8), w_in)
    assert int((want[2] == bzr.RR_OUTSIDE).sum()) > 900
    assert int((bits(want[0]) != bits(zero[0])).any(axis=0).sum()) > 600  # the channels matter
    dm = bzr.DeviceMesh(cctx, lens)
    try:
        assert set_cap(bzr, cctx, 0) >= 1 << 14
        auto = bzr.trace_chain_spectral(cctx, [dm], [ROW1], rays, channel, weight=w_in, mode=bzr.PIPELINE_STAGED)
        assert_same(auto, want, "automatic cap")
        for cap in (64, 192):
            assert set_cap(bzr, cctx, cap) == cap
            cctx.timing(True)
            cctx.timing_report()
            got = bzr.trace_chain_spectral(cctx, [dm], [ROW1], rays, channel, weight=w_in, mode=bzr.PIPELINE_STAGED)
            launches = cctx.timing_report()["k_traverse"][1]
            cctx.timing(False)
            assert launches == 2 * -(-n // chunk_rule(n, cap)) >= 12, (cap, launches)  # two segments per chunk
            assert_same(got, want, f"cap {cap}: vs the reference")
            assert_same(got, auto, f"cap {cap}: vs the automatic cap")
    finally:
        cctx.timing(False)
        set_cap(bzr, cctx, 0)


# ------------------------------------------------------------------ 5. edges
@pytest.mark.parametrize("path", PATHS)
def test_one_channel_and_sixty_four(bzr, orc, ctx, scenes, path):
    lenses, _, dms, rays, channel, w_in, _, _, _ = scenes["cfg2"]
    n = 1024
    first = (rays.shape[1] - n) // 2
    r = np.ascontiguousarray(rays[:, first:first + n])
    w = w_in[first:first + n]
    want = power_ref.chain(orc, lenses, [1.304], r, w)
    assert int((want[2] == bzr.RR_OUTSIDE).sum()) > 300
    got = run(bzr, ctx, dms, [[1.304]], r, np.zeros(n, np.uint8), path, weight=w)
    assert_same(got, want, f"{path}: nchan = 1")
    table = np.full((1, 64), 7.0, F)  # only columns 0 and 63 may be read
    table[0, 0], table[0, 63] = 1.290, 1.312
    ch = np.where(channel[first:first + n] < 2, 0, 63).astype(np.uint8)
    want = spectral_ref.chain(orc, lenses, table, r, ch, w)
    assert int((ch == 63).sum()) > 400 and int((ch == 0).sum()) > 400
    got = run(bzr, ctx, dms, table, r, ch, path, weight=w)
    assert_same(got, want, f"{path}: nchan = 64, channels 0 and 63")


@pytest.mark.parametrize("path", PATHS)
def test_channel_out_of_range_and_nan_ray(bzr, ctx, scenes, path):
    """A channel at or above nchan ends the ray like a non-finite component does: NONE, one segment, ray and weight
    unchanged, and no word of any other ray changes."""
    _, table, dms, rays, channel, w_in, _, rand, _ = scenes["cfg4"]
    n = rays.shape[1]
    lanes17 = np.nonzero((rand[2] == bzr.RR_OUTSIDE) & (np.arange(n) % 64 == 17))[0]
    assert len(lanes17) > 20
    mid = len(lanes17) // 2
    k255, kn, knan = (int(lanes17[mid - 1]), int(lanes17[mid]), int(lanes17[mid + 1]))  # rays that pass both lenses
    ch = channel.copy()
    ch[k255], ch[kn] = 255, NCHAN
    poisoned = rays.copy()
    poisoned[4, knan] = np.nan
    got = run(bzr, ctx, dms, table, poisoned, ch, path, weight=w_in)
    for k in (k255, kn, knan):
        assert got[2][k] == bzr.RR_NONE and got[3][k] == 1, k
        assert bits(got[1])[k] == bits(w_in)[k] and np.array_equal(bits(got[0])[:, k], bits(poisoned)[:, k]), k
    others = np.ones(n, bool)
    others[[k255, kn, knan]] = False
    assert_same(tuple(a[..., others] for a in got), tuple(a[..., others] for a in rand), f"{path}: the other rays")
    got = run(bzr, ctx, dms, table, rays, ch, path)  # weight=None: the rays start at 1
    assert got[1][k255] == 1 and got[1][kn] == 1 and got[2][kn] == bzr.RR_NONE


def test_bad_arguments_leave_the_outputs_untouched(bzr, ctx, scenes):
    _, table, dms, rays, channel, w_in, _, _, _ = scenes["cfg2"]
    n = 256
    r, c = np.ascontiguousarray(rays[:, :n]), channel[:n].copy()

    def rejected(match, dms_, table_, channel_):
        o, w = np.full((6, n), 7.0, F), np.full(n, 7.0, F)
        s, g = np.full(n, 7, np.uint32), np.full(n, 7, np.uint32)
        with pytest.raises(bzr.BzrError, match=match):
            bzr.trace_chain_spectral(ctx, dms_, table_, r, channel_, weight=w_in[:n].copy(), out_rays=o, out_weight=w,
                                     out_status=s, out_segments=g)
        assert (o == 7).all() and (w == 7).all() and (s == 7).all() and (g == 7).all()

    rejected("nchan", dms, np.zeros((1, 0), F), c)
    rejected("nchan", dms, np.full((1, 65), 1.3, F), c)
    rejected("channel", dms, table, None)
    rejected("nlens", [], np.zeros((0, NCHAN), F), c)
    rejected("nlens", dms * 9, np.full((9, NCHAN), 1.3, F), c)
    null = ctypes.c_void_p(None)
    handles = (ctypes.c_void_p * 1)(dms[0].handle)
    o = np.full((6, n), 7.0, F)
    s = np.full(n, 7, np.uint32)
    tab_f = np.ascontiguousarray(table, F)
    w = np.full(n, 7.0, F)
    for tab, out_w in ((null, w.ctypes.data), (tab_f.ctypes.data, null)):  # NULL ri_table, NULL out_weight
        assert bzr.lib().bzr_trace_chain_spectral(ctx.handle, ctypes.cast(handles, ctypes.c_void_p), tab, 1, NCHAN,
                                                  r.ctypes.data, c.ctypes.data, None, n, o.ctypes.data, out_w,
                                                  s.ctypes.data, None, 0) == 1
    assert (o == 7).all() and (s == 7).all() and (w == 7).all()


# ------------------------------------------------------------------ 6. eight lenses
@pytest.fixture(scope="module")
def eight(orc):
    lenses = [lens_patches(orc, k) for k in range(8)]
    table = [[1.3, 1.31]] * 8
    rays = chain_rays()
    channel = (np.arange(rays.shape[1]) % 2).astype(np.uint8)
    want = frozen(*spectral_ref.chain(orc, lenses, table, rays, channel))
    assert rays.shape[1] == 64 * 64 and int((want[3] == 16).sum()) > 2000
    return lenses, table, rays, channel, want


@pytest.mark.parametrize("path", PATHS)
def test_eight_lens_chain(bzr, ctx, path, eight):
    lenses, table, rays, channel, want = eight
    dms = [bzr.DeviceMesh(ctx, p) for p in lenses]
    got = run(bzr, ctx, dms, table, rays, channel, path)
    assert_same(got, want, f"eight lenses, two channels, {path}")


# ------------------------------------------------------------------ 7. illumination
N_ILLUM = 1 << 16


def illum_reference(bzr, orc, lens, n):
    """Per channel: flux, hist, exited, landed, the emitted and exited power; and the emitted rays."""
    rays, _ = orc.emit(emitter(orc), 0, n)
    channel = (np.arange(n) % NCHAN).astype(np.uint8)
    w0 = rays[3].copy()
    out, w, status, _ = spectral_ref.chain(orc, [lens], [ROW1], rays, channel, w0)
    tg = target(orc)
    per = []
    for c in range(NCHAN):
        st = np.where(channel == c, status, 0).astype(np.uint32)
        hist, exited, landed = orc.land(tg, out, st)
        flux = power_ref.flux(orc, tg, out, st, w)
        per.append((flux, hist, exited, landed, int(power_ref.q32(w0[channel == c]).sum()),
                    int(power_ref.q32(w)[st == 2].sum())))
    return rays, channel, per


@pytest.fixture(scope="module")
def illum(bzr, orc, ctx):
    lens = build_lens(bzr.TriMesh, CONFIGS["cfg2"].lenses[0]).bezier_patches()
    rays, channel, per = illum_reference(bzr, orc, lens, N_ILLUM)
    for c in range(NCHAN):
        assert per[c][3] > 400, c  # landed per channel
    assert int((per[0][1] != per[3][1]).sum()) > 100  # the colours land in different cells
    return lens, bzr.DeviceMesh(ctx, lens), rays, channel, per


def check_illum(bzr, dm, rays, channel, per, got, label):
    flux, hist, stats, power = got
    culled = culled_by_sphere(bzr.bounding_sphere(dm), rays)
    for c in range(NCHAN):
        mine = channel == c
        assert np.array_equal(flux[c], per[c][0]), (label, c)
        assert np.array_equal(hist[c], per[c][1]), (label, c)
        assert stats[c] == {"emitted": int(mine.sum()), "culled": int((culled & mine).sum()), "exited": per[c][2],
                            "landed": per[c][3]}, (label, c)
        assert power[c] == {"emitted": per[c][4], "culled": int(power_ref.q32(rays[3][culled & mine]).sum()),
                            "exited": per[c][5], "landed": int(per[c][0].sum())}, (label, c)


def test_illuminate_spectral(bzr, ctx, pipe, illum):
    _, dm, rays, channel, per = illum
    got = bzr.illuminate_spectral(ctx, [dm], [ROW1], emitter(bzr), N_ILLUM, target(bzr), mode=pipe)
    assert got[0].dtype == np.uint64 and got[0].shape == (NCHAN, 48, 48) and got[1].shape == (NCHAN, 48, 48)
    check_illum(bzr, dm, rays, channel, per, got, "first call")
    # a second call into the same flux and hist accumulates
    bzr.illuminate_spectral(ctx, [dm], [ROW1], emitter(bzr), N_ILLUM, target(bzr), flux=got[0], hist=got[1], mode=pipe)
    for c in range(NCHAN):
        assert np.array_equal(got[0][c], per[c][0] * np.uint64(2)) and np.array_equal(got[1][c], per[c][1] * 2)
    # summed over the channels, what is emitted and culled does not depend on the table: illuminate_power's figures
    _, _, p_stats, p_power = bzr.illuminate_power(ctx, [dm], [1.3], emitter(bzr), N_ILLUM, target(bzr), mode=pipe)
    for key in ("emitted", "culled"):
        assert sum(s[key] for s in got[2]) == p_stats[key]
        assert sum(p[key] for p in got[3]) == p_power[key]
    assert p_stats["culled"] > 0


def test_illuminate_spectral_uniform_lossless_is_the_count(bzr, ctx, pipe, illum):
    _, dm, _, _, per = illum
    flux, hist, stats, power = bzr.illuminate_spectral(ctx, [dm], [ROW1], emitter(bzr), N_ILLUM, target(bzr),
                                                       emission=bzr.EMISSION_UNIFORM, surface=bzr.SURFACE_LOSSLESS,
                                                       mode=pipe)
    for c in range(NCHAN):  # the rays still refract with their channel's index
        assert np.array_equal(hist[c], per[c][1]) and stats[c]["landed"] == per[c][3] and stats[c]["exited"] == per[c][2]
        assert np.array_equal(flux[c], hist[c].astype(np.uint64) << np.uint64(32))
        assert power[c] == {k: v << 32 for k, v in stats[c].items()}


def test_illuminate_spectral_batches(bzr, orc, cctx, pipe):
    """10 000 rays at a chunk cap of 4 096: three batches through the batch loop, the same bits as one batch and as the
    reference.  With four channels every batch starts in channel 0 (4 096 is a multiple of four), so a channel taken
    from the ray's index within its batch would pass; with three channels the batches start in channels 0, 1 and 2."""
    lens = build_lens(bzr.TriMesh, CONFIGS["cfg2"].lenses[0]).bezier_patches()
    dm = bzr.DeviceMesh(cctx, lens)
    n = 10_000
    table3 = [ROW1[:3]]  # three channels: the batches start in channels 0, 1 and 2
    try:
        assert set_cap(bzr, cctx, 0) >= 1 << 14
        one = bzr.illuminate_spectral(cctx, [dm], [ROW1], emitter(bzr), n, target(bzr), mode=pipe)
        one3 = bzr.illuminate_spectral(cctx, [dm], table3, emitter(bzr), n, target(bzr), mode=pipe)
        assert set_cap(bzr, cctx, 4096) == 4096
        cctx.timing(True)
        cctx.timing_report()
        got = bzr.illuminate_spectral(cctx, [dm], [ROW1], emitter(bzr), n, target(bzr), mode=pipe)
        rep = cctx.timing_report()
        cctx.timing(False)
        got3 = bzr.illuminate_spectral(cctx, [dm], table3, emitter(bzr), n, target(bzr), mode=pipe)
    finally:
        cctx.timing(False)
        set_cap(bzr, cctx, 0)
    assert rep["k_trace" if pipe == bzr.PIPELINE_FUSED else "k_traverse"][1] == (3 if pipe == bzr.PIPELINE_FUSED else 6)
    for a, b in ((got, one), (got3, one3)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
    rays, channel, per = illum_reference(bzr, orc, lens, n)
    check_illum(bzr, dm, rays, channel, per, got, "three batches")
    assert sum(s["landed"] for s in got[2]) > 300
    # three channels over three batches: ray i of batch b is global ray 4096 b + i
    ch3 = (np.arange(n) % 3).astype(np.uint8)
    out, w, status, _ = spectral_ref.chain(orc, [lens], table3, rays, ch3, rays[3].copy())
    for c in range(3):
        st = np.where(ch3 == c, status, 0).astype(np.uint32)
        assert np.array_equal(got3[0][c], power_ref.flux(orc, target(orc), out, st, w)), c


def test_illuminate_spectral_rejects_bad_arguments(bzr, ctx, illum):
    _, dm, _, _, _ = illum
    flux = np.full((NCHAN, 48, 48), 5, np.uint64)
    hist = np.full((NCHAN, 48, 48), 5, np.uint32)
    args = (emitter(bzr), 1000, target(bzr))
    for kw, msg in (({"emission": 2}, "emission"), ({"surface": 2}, "surface")):
        with pytest.raises(bzr.BzrError, match=msg):
            bzr.illuminate_spectral(ctx, [dm], [ROW1], *args, flux=flux, hist=hist, **kw)
    with pytest.raises(bzr.BzrError, match="2\\^32"):
        bzr.illuminate_spectral(ctx, [dm], [ROW1], emitter(bzr), 1 << 32, target(bzr), flux=flux, hist=hist)
    for table in (np.zeros((1, 0), F), np.full((1, 65), 1.3, F)):
        with pytest.raises(bzr.BzrError, match="nchan"):
            bzr.illuminate_spectral(ctx, [dm], table, *args, flux=flux, hist=hist)
    for nl in (0, 9):
        with pytest.raises(bzr.BzrError, match="nlens"):
            bzr.illuminate_spectral(ctx, [dm] * nl, np.full((nl, NCHAN), 1.3, F), *args, flux=flux, hist=hist)
    assert (flux == 5).all() and (hist == 5).all()
