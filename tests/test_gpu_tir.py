"""Total internal reflection on the GPU: bzr_trace_chain_tir against the oracle composed with the reflecting step
(tests/tir_ref.py), bit for bit, on the fused kernel, the staged pipeline and the brute-force scan.

The populations the tests rely on are asserted from the reference, so none passes vacuously.
"""
import ctypes

import numpy as np
import pytest

import tir_ref
from bzr_amd.configs import CONFIGS, build_lens, grid_rays
from test_chunk_plan import chunk_rule
from test_gpu_long_chains import chain_rays, lens_patches
from test_gpu_power import assert_same, bits, flags_of, frozen, set_cap

pytestmark = pytest.mark.gpu

F = np.float32
PATHS = ("fused", "staged", "brute")
SIDE, DROP, NCHAN = 64, 37, 4
ROW1 = [1.3, 1.5, 1.8, 2.4]        # lens 1's index per channel
ROW2 = [1.5, 1.5168, 1.53, 1.62]   # cfg4's second lens
TABLES = {"cfg2": [ROW1], "cfg4": [ROW1, ROW2]}
BUDGETS = (1, 4, 8)


def assert_tir(got, want, label):
    """(rays, weight, status, segments, bounces) word for word."""
    assert_same(got[:4], want[:4], label)
    bad = np.asarray(got[4]) != want[4]
    assert not bad.any(), (f"{label}: bounces of {int(bad.sum())} rays differ, first {np.nonzero(bad)[0][:8]}; "
                           f"got {np.asarray(got[4])[bad][:8]} want {want[4][bad][:8]}")


def run(bzr, ctx, dms, table, rays, channel, path, max_bounces, **kw):
    return bzr.trace_chain_tir(ctx, dms, table, rays, channel, max_bounces=max_bounces, mode=flags_of(bzr, path), **kw)


@pytest.fixture(scope="module")
def scenes(bzr, orc, ctx):
    """name -> (patches, table, device meshes, rays, channel, random input weights, {max_bounces: reference with
    weight 1}, {max_bounces: reference with the random weights}): computed once, never changed."""
    out = {}
    for name, table in TABLES.items():
        cfg = CONFIGS[name]
        lenses = [build_lens(bzr.TriMesh, lens).bezier_patches() for lens in cfg.lenses]
        rays = grid_rays(cfg, side=SIDE)
        n = rays.shape[1] - DROP
        rays = np.ascontiguousarray(rays[:, :n])
        channel = np.random.default_rng(7).integers(0, NCHAN, SIDE * SIDE)[:n].astype(np.uint8)
        w_in = np.random.default_rng(41).random(n, dtype=F)
        ones = {mb: frozen(*tir_ref.chain(orc, lenses, table, rays, channel, None, mb)) for mb in (0,) + BUDGETS}
        rand = {mb: frozen(*tir_ref.chain(orc, lenses, table, rays, channel, w_in, mb)) for mb in BUDGETS}
        frozen(rays, channel, w_in)
        out[name] = (lenses, table, [bzr.DeviceMesh(ctx, p) for p in lenses], rays, channel, w_in, ones, rand)
    return out


# ------------------------------------------------------------------ populations
def test_populations(bzr, scenes):
    """What the reference alone says about the scenes: reflections are common, mixed with unreflected lanes in most
    waves, and they change the result."""
    _, _, _, rays, _, _, ones, _ = scenes["cfg2"]
    n = rays.shape[1]
    assert n == SIDE * SIDE - DROP == 4059 and n % 64 != 0
    _, _, st, seg, b = ones[4]
    out = st == bzr.RR_OUTSIDE
    assert int((out & (b > 0)).sum()) >= 400 and int((~out & (b > 0)).sum()) >= 150
    for k in (1, 2, 3, 4):
        assert int((out & (b == k)).sum()) >= 30, k
    assert int(seg.max()) == 6 and int(b.max()) == 4
    waves = [b[k:k + 64] for k in range(0, n - 63, 64)]
    assert sum(1 for w in waves if (w > 0).any() and (w == 0).any()) >= 40
    assert int(ones[8][3].max()) == 10 and int(((ones[8][2] == bzr.RR_OUTSIDE) & (ones[8][4] > 0)).sum()) >= 500
    # the feature matters: status and rays differ from the max_bounces = 0 trace on the reflected rays
    assert int((ones[4][2] != ones[0][2]).sum()) >= 400
    assert int((bits(ones[4][0]) != bits(ones[0][0])).any(axis=0).sum()) >= 550
    _, _, st, _, b = scenes["cfg4"][6][4]
    out = st == bzr.RR_OUTSIDE
    assert int((out & (b > 0)).sum()) >= 100 and int((out & (b == 1)).sum()) == 0


# ------------------------------------------------------------------ 1. bit-exact
@pytest.mark.parametrize("max_bounces", BUDGETS)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(TABLES))
def test_bit_exact(bzr, ctx, scenes, name, path, max_bounces):
    _, table, dms, rays, channel, w_in, ones, rand = scenes[name]
    assert int((ones[max_bounces][4] > 0).sum()) >= 600
    got = run(bzr, ctx, dms, table, rays, channel, path, max_bounces)
    assert_tir(got, ones[max_bounces], f"{name} {path} max_bounces {max_bounces}, weight=None: vs the reference")
    w = w_in.copy()  # passed in place
    got = run(bzr, ctx, dms, table, rays, channel, path, max_bounces, weight=w, out_weight=w)
    assert got[1] is w
    assert_tir(got, rand[max_bounces], f"{name} {path} max_bounces {max_bounces}, random weights in place")


# ------------------------------------------------------------------ 2. zero budget
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(TABLES))
def test_zero_budget_is_the_spectral_chain(bzr, ctx, scenes, name, path):
    _, table, dms, rays, channel, w_in, ones, _ = scenes[name]
    want = bzr.trace_chain_spectral(ctx, dms, table, rays, channel, weight=w_in, mode=flags_of(bzr, path))
    got = run(bzr, ctx, dms, table, rays, channel, path, 0, weight=w_in)
    assert int((want[2] == bzr.RR_OUTSIDE).sum()) > 1500
    assert_same(got[:4], tuple(np.asarray(a) for a in want), f"{name} {path}, max_bounces 0: vs trace_chain_spectral")
    assert not got[4].any()
    assert_tir(run(bzr, ctx, dms, table, rays, channel, path, 0), ones[0], f"{name} {path}, max_bounces 0: vs the reference")


@pytest.mark.parametrize("pipe_name", ("fused", "staged"))
def test_zero_budget_fast(bzr, ctx, scenes, pipe_name):
    """Snell's step and the reflecting step are exact in both modes: the FAST kernels agree with their spectral FAST
    siblings."""
    _, table, dms, rays, channel, w_in, _, _ = scenes["cfg4"]
    mode = flags_of(bzr, pipe_name) | bzr.MODE_FAST
    want = bzr.trace_chain_spectral(ctx, dms, table, rays, channel, weight=w_in, mode=mode)
    got = bzr.trace_chain_tir(ctx, dms, table, rays, channel, weight=w_in, max_bounces=0, mode=mode)
    assert_same(got[:4], tuple(np.asarray(a) for a in want), f"FAST {pipe_name}, max_bounces 0: vs trace_chain_spectral")
    assert not got[4].any()


# ------------------------------------------------------------------ 3. FAST with bounces
@pytest.mark.parametrize("pipe_name", ("fused", "staged"))
@pytest.mark.parametrize("name", list(TABLES))
def test_fast_with_bounces(bzr, ctx, scenes, name, pipe_name):
    """Structure only.  The share of rays that agree with parity is recorded (printed); the share with the
    binary64 chain's structure and the distance from the truth are what tests/test_gpu_fast_chain64.py asserts."""
    _, table, dms, rays, channel, _, ones, _ = scenes[name]
    mb, nl = 4, len(dms)
    mode = flags_of(bzr, pipe_name) | bzr.MODE_FAST
    got = bzr.trace_chain_tir(ctx, dms, table, rays, channel, max_bounces=mb, mode=mode)
    spec = bzr.trace_chain_spectral(ctx, dms, table, rays, channel, mode=mode)
    assert set(np.unique(got[2])) <= {bzr.RR_NONE, bzr.RR_OUTSIDE}
    assert (got[1] > 0).all() and (got[1] <= 1).all()
    assert (got[4] <= nl * mb).all() and (got[3] <= nl * (2 + mb)).all() and (got[3] >= 1).all()
    assert int((got[4] > 0).sum()) >= 600
    same = (got[4] == 0) & (got[2] == spec[2])
    assert int(same.sum()) >= 3000
    assert_same(tuple(np.asarray(a)[..., same] for a in got[:4]), tuple(np.asarray(a)[..., same] for a in spec),
                f"FAST {name} {pipe_name}: the unreflected rays vs trace_chain_spectral")
    want = ones[mb]
    agree = (got[2] == want[2]) & (got[3] == want[3]) & (got[4] == want[4])
    print(f"FAST {name} {pipe_name}, max_bounces {mb}: {int(agree.sum())} of {len(agree)} rays "
          f"({100.0 * agree.mean():.2f} %) agree with parity in status, segments and bounces")


# ------------------------------------------------------------------ 4. channel = None
@pytest.mark.parametrize("path", PATHS)
def test_no_channel_row(bzr, orc, ctx, scenes, path):
    lenses, _, dms, rays, _, w_in, _, _ = scenes["cfg2"]
    want = tir_ref.chain(orc, lenses, [[1.8]], rays, None, w_in, 4)
    assert int(((want[2] == bzr.RR_OUTSIDE) & (want[4] > 0)).sum()) >= 500
    got = run(bzr, ctx, dms, [[1.8]], rays, None, path, 4, weight=w_in)
    assert_tir(got, want, f"{path}: channel=None, nchan = 1, index 1.8")


# ------------------------------------------------------------------ 5. layouts and residency
def test_device_buffers_and_aos(bzr, ctx, scenes):
    """Device tensors for rays, channel and weight (the asynchronous path, synchronised only at the end) and [n, 6]
    ray records: the same bits."""
    torch = pytest.importorskip("torch")
    _, table, dms, rays, channel, w_in, _, rand = scenes["cfg4"]
    r = torch.from_numpy(np.ascontiguousarray(rays.T)).cuda()
    c = torch.from_numpy(channel.copy()).cuda()
    w = torch.from_numpy(w_in.copy()).cuda()
    for pipe in (bzr.PIPELINE_FUSED, bzr.PIPELINE_STAGED):
        o, ow, s, g, b = bzr.trace_chain_tir(ctx, dms, table, r, c, weight=w, max_bounces=4, mode=pipe | bzr.RAYS_AOS)
        torch.cuda.synchronize()
        got = (np.ascontiguousarray(o.cpu().numpy().T), ow.cpu().numpy(), s.cpu().numpy().astype(np.uint32),
               g.cpu().numpy().astype(np.uint32), b.cpu().numpy().astype(np.uint32))
        assert_tir(got, rand[4], f"cfg4 device pointers, AoS, pipeline {pipe}")
    got = bzr.trace_chain_tir(ctx, dms, table, np.ascontiguousarray(rays.T), channel, weight=w_in, max_bounces=4,
                              mode=bzr.RAYS_AOS)
    assert_tir((np.ascontiguousarray(got[0].T),) + got[1:], rand[4], "cfg4 host pointers, AoS")


# ------------------------------------------------------------------ 6. small chunks
@pytest.fixture(scope="module")
def cctx(bzr, ctx):
    """This module's own context: the session context never sees a lowered chunk cap."""
    c = bzr.Context(0)
    yield c
    c.close()


def test_small_chunks(bzr, orc, cctx):
    """The pending and bounce rows are indexed by the global ray index: a row read without the chunk offset fails here."""
    cfg = CONFIGS["cfg2"]
    lens = build_lens(bzr.TriMesh, cfg.lenses[0]).bezier_patches()
    full = grid_rays(cfg, side=128)
    n, mb = 1000, 3
    first = (full.shape[1] - n) // 2  # the grid's centre in tile order: every ray meets the lens
    rays = np.ascontiguousarray(full[:, first:first + n])
    channel = np.random.default_rng(9).integers(0, NCHAN, n).astype(np.uint8)
    w_in = np.random.default_rng(5).random(n, dtype=F)
    want = tir_ref.chain(orc, [lens], [ROW1], rays, channel, w_in, mb)
    assert int((want[4] > 0).sum()) >= 80 and int(((want[2] == bzr.RR_OUTSIDE) & (want[4] > 0)).sum()) >= 35
    dm = bzr.DeviceMesh(cctx, lens)
    kw = dict(weight=w_in, max_bounces=mb, mode=bzr.PIPELINE_STAGED)
    try:
        assert set_cap(bzr, cctx, 0) >= 1 << 14
        auto = bzr.trace_chain_tir(cctx, [dm], [ROW1], rays, channel, **kw)
        assert_tir(auto, want, "automatic cap")
        for cap in (64, 192):
            assert set_cap(bzr, cctx, cap) == cap
            cctx.timing(True)
            cctx.timing_report()
            got = bzr.trace_chain_tir(cctx, [dm], [ROW1], rays, channel, **kw)
            launches = cctx.timing_report()["k_traverse"][1]
            cctx.timing(False)
            # per chunk: the INSIDE stage, the OUTSIDE stage and max_bounces bounce stages
            assert launches == (1 + 1 + mb) * -(-n // chunk_rule(n, cap)) >= 30, (cap, launches)
            assert_tir(got, want, f"cap {cap}: vs the reference")
            assert_tir(got, auto, f"cap {cap}: vs the automatic cap")
    finally:
        cctx.timing(False)
        set_cap(bzr, cctx, 0)


# ------------------------------------------------------------------ 7. budget edge
@pytest.mark.parametrize("path", PATHS)
def test_budget_edge(bzr, ctx, scenes, path):
    """A ray that needs exactly two reflections: with a budget of one it ends NONE where its first reflection left it."""
    _, table, dms, rays, channel, _, ones, _ = scenes["cfg2"]
    two = np.nonzero((ones[4][2] == bzr.RR_OUTSIDE) & (ones[4][4] == 2))[0]
    assert len(two) >= 30
    k = int(two[len(two) // 2])
    lo = k - k % 64
    r, c = np.ascontiguousarray(rays[:, lo:lo + 64]), channel[lo:lo + 64].copy()
    j = k - lo
    want1 = tuple(a[..., lo:lo + 64] for a in ones[1])
    assert want1[2][j] == bzr.RR_NONE and want1[4][j] == 1 and want1[3][j] == 3
    assert (bits(want1[0])[:, j] != bits(r)[:, j]).any()
    got = run(bzr, ctx, dms, table, r, c, path, 1)
    assert got[2][j] == bzr.RR_NONE and got[4][j] == 1 and got[3][j] == 3
    assert np.array_equal(bits(got[0])[:, j], bits(want1[0])[:, j]) and got[1][j] == want1[1][j]
    assert_tir(got, want1, f"{path}: max_bounces 1, the ray's wave")
    got = run(bzr, ctx, dms, table, r, c, path, 2)
    assert got[2][j] == bzr.RR_OUTSIDE and got[4][j] == 2 and got[3][j] == 4
    assert np.array_equal(bits(got[0])[:, j], bits(ones[4][0])[:, k])


# ------------------------------------------------------------------ 8. bad rays beside reflected ones
@pytest.mark.parametrize("path", PATHS)
def test_channel_out_of_range_and_nan_ray(bzr, ctx, scenes, path):
    """A channel at or above nchan and a non-finite component end the ray as in the spectral chain: NONE, one segment,
    no bounce, ray and weight unchanged, and no word of any other ray changes."""
    _, table, dms, rays, channel, w_in, _, rand = scenes["cfg4"]
    n = rays.shape[1]
    want = rand[4]
    cand = np.nonzero(want[4] > 0)[0]  # reflected rays, so their waves hold bounce segments
    assert len(cand) > 300
    mid = len(cand) // 2
    k255, kn, knan = int(cand[mid - 1]), int(cand[mid]), int(cand[mid + 1])
    ch = channel.copy()
    ch[k255], ch[kn] = 255, NCHAN
    poisoned = rays.copy()
    poisoned[4, knan] = np.nan
    got = run(bzr, ctx, dms, table, poisoned, ch, path, 4, weight=w_in)
    for k in (k255, kn, knan):
        assert got[2][k] == bzr.RR_NONE and got[3][k] == 1 and got[4][k] == 0, k
        assert bits(got[1])[k] == bits(w_in)[k] and np.array_equal(bits(got[0])[:, k], bits(poisoned)[:, k]), k
    others = np.ones(n, bool)
    others[[k255, kn, knan]] = False
    assert_tir(tuple(a[..., others] for a in got), tuple(a[..., others] for a in want), f"{path}: the other rays")


# ------------------------------------------------------------------ 9. bad arguments
def test_bad_arguments_leave_the_outputs_untouched(bzr, ctx, scenes):
    _, table, dms, rays, channel, w_in, _, _ = scenes["cfg2"]
    n = 256
    r, c = np.ascontiguousarray(rays[:, :n]), channel[:n].copy()

    def rejected(match, dms_, table_, mb):
        o, w = np.full((6, n), 7.0, F), np.full(n, 7.0, F)
        s, g, b = np.full(n, 7, np.uint32), np.full(n, 7, np.uint32), np.full(n, 7, np.uint32)
        with pytest.raises(bzr.BzrError, match=match):
            bzr.trace_chain_tir(ctx, dms_, table_, r, c, weight=w_in[:n].copy(), max_bounces=mb, out_rays=o,
                                out_weight=w, out_status=s, out_segments=g, out_bounces=b)
        assert (o == 7).all() and (w == 7).all() and (s == 7).all() and (g == 7).all() and (b == 7).all()

    rejected("max_bounces", dms, table, bzr.MAX_BOUNCES + 1)
    rejected("nchan", dms, np.zeros((1, 0), F), 4)
    rejected("nchan", dms, np.full((1, 65), 1.3, F), 4)
    rejected("nlens", [], np.zeros((0, NCHAN), F), 4)
    rejected("nlens", dms * 9, np.full((9, NCHAN), 1.3, F), 4)
    assert bzr.MAX_BOUNCES == 8
    null = ctypes.c_void_p(None)
    handles = (ctypes.c_void_p * 1)(dms[0].handle)
    o, w = np.full((6, n), 7.0, F), np.full(n, 7.0, F)
    s, g, b = np.full(n, 7, np.uint32), np.full(n, 7, np.uint32), np.full(n, 7, np.uint32)
    tab_f = np.ascontiguousarray(table, F)
    for tab, out_w in ((null, w.ctypes.data), (tab_f.ctypes.data, null)):  # NULL ri_table, NULL out_weight
        assert bzr.lib().bzr_trace_chain_tir(ctx.handle, ctypes.cast(handles, ctypes.c_void_p), tab, 1, NCHAN,
                                             r.ctypes.data, c.ctypes.data, None, n, 4, o.ctypes.data, out_w,
                                             s.ctypes.data, g.ctypes.data, b.ctypes.data, 0) == 1
    assert (o == 7).all() and (w == 7).all() and (s == 7).all() and (g == 7).all() and (b == 7).all()


# ------------------------------------------------------------------ 10. eight lenses
@pytest.fixture(scope="module")
def eight(orc):
    """test_gpu_long_chains' scene with the spectral test's table: at indices 1.3 and 1.31 enough rays reflect."""
    lenses = [lens_patches(orc, k) for k in range(8)]
    table = [[1.3, 1.31]] * 8
    rays = chain_rays()
    channel = (np.arange(rays.shape[1]) % 2).astype(np.uint8)
    want = frozen(*tir_ref.chain(orc, lenses, table, rays, channel, None, 2))
    assert rays.shape[1] == 64 * 64 and int((want[3] == 16).sum()) > 2000
    assert int((want[4] > 0).sum()) >= 50 and int(want[3].max()) > 16
    return lenses, table, rays, channel, want


@pytest.mark.parametrize("path", PATHS)
def test_eight_lens_chain(bzr, ctx, path, eight):
    lenses, table, rays, channel, want = eight
    dms = [bzr.DeviceMesh(ctx, p) for p in lenses]
    got = run(bzr, ctx, dms, table, rays, channel, path, 2)
    assert_tir(got, want, f"eight lenses, two channels, max_bounces 2, {path}")
