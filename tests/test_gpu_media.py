"""Surrounding media on the GPU: bzr_trace_chain_media against tests/media_ref.py (the oracle's intersect, Snell's step
with a per-ray eta in numpy float32), bit for bit, on the fused kernel, the staged pipeline and the brute-force scan.

The scenes are test_gpu_tir.py's: 64^2 - 37 rays (a ragged last wave), four channels mixed in every wave; the doublet
is media_ref's (two (1, 4, 2) ellipsoids 0.01 apart, one channel).  tests/test_media_ref.py asserts the populations of
these references without a GPU.
"""
import ctypes

import numpy as np
import pytest

import media_ref
import opl_ref
from bzr_amd.configs import CONFIGS, build_lens, grid_rays
from media_ref import DOUBLET_CEMENT, DOUBLET_RI, GAPS2, GAPS4, GAPS_FRONT
from test_chunk_plan import chunk_rule
from test_gpu_fast_ref64 import BAR, CLASS_ALLOW
from test_gpu_opl import assert_opl
from test_gpu_power import bits, flags_of, frozen, set_cap
from test_gpu_tir import DROP, NCHAN, PATHS, ROW1, SIDE, TABLES

pytestmark = pytest.mark.gpu

F = np.float32
BUDGETS = {"cfg2": (0, 4, 8), "cfg4": (0, 4), "doublet": (4,)}
GAPS = {"cfg2": GAPS2, "cfg4": GAPS4, "doublet": DOUBLET_CEMENT}


def run(bzr, ctx, dms, table, gaps, rays, channel, path, max_bounces, **kw):
    return bzr.trace_chain_media(ctx, dms, table, gaps, rays, channel, max_bounces=max_bounces, mode=flags_of(bzr, path), **kw)


@pytest.fixture(scope="module")
def scenes(bzr, orc, ctx):
    """name -> dict(lenses, table, gaps, dms, rays, channel, w_in, p_in, zero {max_bounces: reference with weight 1 and
    path 0}, rand {max_bounces: reference with the random rows}): computed once, never changed."""
    out = {}
    for name in ("cfg2", "cfg4", "doublet"):
        if name == "doublet":
            lenses, table = media_ref.doublet_lenses(bzr.TriMesh), DOUBLET_RI
            cfg = CONFIGS["cfg2"]
        else:
            cfg = CONFIGS[name]
            lenses, table = [build_lens(bzr.TriMesh, lens).bezier_patches() for lens in cfg.lenses], TABLES[name]
        rays = grid_rays(cfg, side=SIDE)
        n = rays.shape[1] - DROP
        rays = np.ascontiguousarray(rays[:, :n])
        channel = np.random.default_rng(7).integers(0, NCHAN, SIDE * SIDE)[:n].astype(np.uint8)
        if name == "doublet":
            channel[:] = 0  # one channel
        w_in = np.random.default_rng(41).random(n, dtype=F)
        p_in = (np.random.default_rng(43).random(n, dtype=F) * F(8)).astype(F)
        zero, rand = {}, {}
        for mb in BUDGETS[name]:
            zero[mb] = frozen(*media_ref.chain(orc, lenses, table, GAPS[name], rays, channel, None, None, mb))
            rand[mb] = frozen(*media_ref.chain(orc, lenses, table, GAPS[name], rays, channel, w_in, p_in, mb))
        frozen(rays, channel, w_in, p_in)
        out[name] = dict(lenses=lenses, table=table, gaps=GAPS[name], dms=[bzr.DeviceMesh(ctx, p) for p in lenses],
                         rays=rays, channel=channel, w_in=w_in, p_in=p_in, zero=zero, rand=rand)
    return out


@pytest.fixture(scope="module")
def front(orc, scenes):
    """cfg2 immersed in front, air behind (GAPS_FRONT): {max_bounces: reference with the random rows}."""
    s = scenes["cfg2"]
    return {mb: frozen(*media_ref.chain(orc, s["lenses"], s["table"], GAPS_FRONT, s["rays"], s["channel"], s["w_in"],
                                        s["p_in"], mb)) for mb in (0, 4)}


# ------------------------------------------------------------------ 1. bit-exact
CASES = [(name, mb) for name in BUDGETS for mb in BUDGETS[name]]


@pytest.mark.parametrize("name,max_bounces", CASES)
@pytest.mark.parametrize("path", PATHS)
def test_bit_exact(bzr, ctx, scenes, name, path, max_bounces):
    s = scenes[name]
    n = s["rays"].shape[1]
    assert n == SIDE * SIDE - DROP == 4059 and n % 64 != 0
    want = s["zero"][max_bounces]
    assert int((want[2] == bzr.RR_OUTSIDE).sum()) >= 2400
    got = run(bzr, ctx, s["dms"], s["table"], s["gaps"], s["rays"], s["channel"], path, max_bounces)
    assert got[6] is not None
    assert_opl(got, want, f"{name} {path} max_bounces {max_bounces}, weight 1 and opl 0: vs the reference")
    w, p = s["w_in"].copy(), s["p_in"].copy()  # both passed in place
    got = run(bzr, ctx, s["dms"], s["table"], s["gaps"], s["rays"], s["channel"], path, max_bounces, weight=w,
              out_weight=w, opl=p, out_opl=p)
    assert got[1] is w and got[5] is p
    assert_opl(got, s["rand"][max_bounces], f"{name} {path} max_bounces {max_bounces}, random rows in place")


@pytest.mark.parametrize("path", PATHS)
def test_no_glass_row(bzr, ctx, scenes, path):
    """out_glass NULL: no row is staged or stored, and the other six outputs are what they were."""
    s = scenes["cfg4"]
    got = run(bzr, ctx, s["dms"], s["table"], s["gaps"], s["rays"], s["channel"], path, 4, weight=s["w_in"],
              opl=s["p_in"], out_glass=False)
    assert got[6] is None
    assert_opl(got, s["rand"][4], f"cfg4 {path}, out_glass NULL")


# ------------------------------------------------------------------ 2. vacuum
@pytest.mark.parametrize("max_bounces", (0, 4))
@pytest.mark.parametrize("path,fast", [(p, False) for p in PATHS] + [("fused", True), ("staged", True)])
def test_vacuum_is_trace_chain_opl(bzr, ctx, scenes, path, fast, max_bounces):
    """x / 1 = x and 1 x = x: a gap table of ones and a NULL one give bzr_trace_chain_opl's seven outputs bit for bit,
    in parity on all three paths and in FAST on the two that have a FAST form."""
    s = scenes["cfg4"]
    mode = flags_of(bzr, path) | (bzr.MODE_FAST if fast else 0)
    kw = dict(weight=s["w_in"], opl=s["p_in"], max_bounces=max_bounces, mode=mode)
    want = bzr.trace_chain_opl(ctx, s["dms"], s["table"], s["rays"], s["channel"], **kw)
    assert int((want[2] == bzr.RR_OUTSIDE).sum()) > 1500
    want = tuple(np.asarray(a) for a in want)
    for what, gaps in (("ones", np.ones((3, NCHAN), F)), ("NULL", None)):
        got = bzr.trace_chain_media(ctx, s["dms"], s["table"], gaps, s["rays"], s["channel"], **kw)
        assert_opl(got, want, f"cfg4 {path} fast={fast} max_bounces {max_bounces}, gap_table {what}")


# ------------------------------------------------------------------ 3. the table cache
@pytest.mark.parametrize("path", PATHS)
def test_table_cache(bzr, orc, scenes, front, path):
    """One context, one ri_table, two gap tables in turn and the first again: no call sees the other's table, and a
    trace_chain_opl call in between still gets vacuum."""
    s = scenes["cfg2"]
    vac = opl_ref.chain(orc, s["lenses"], s["table"], s["rays"], s["channel"], s["w_in"], s["p_in"], 4)
    c = bzr.Context(0)
    try:
        dms = [bzr.DeviceMesh(c, p) for p in s["lenses"]]
        kw = dict(weight=s["w_in"], opl=s["p_in"])
        for k, (gaps, want) in enumerate(((GAPS2, s["rand"][4]), (GAPS_FRONT, front[4]), (None, vac), (GAPS2, s["rand"][4]))):
            if gaps is None:
                got = bzr.trace_chain_opl(c, dms, s["table"], s["rays"], s["channel"], max_bounces=4,
                                          mode=flags_of(bzr, path), **kw)
            else:
                got = run(bzr, c, dms, s["table"], gaps, s["rays"], s["channel"], path, 4, **kw)
            assert_opl(got, want, f"{path}: call {k}")
    finally:
        c.close()


@pytest.mark.parametrize("pipe_name", ("fused", "staged"))
def test_table_cache_device_pointers(bzr, orc, scenes, front, pipe_name):
    """The same with device rows and no synchronisation between the calls: a table is rewritten only after the kernels
    that read the old one have finished."""
    torch = pytest.importorskip("torch")
    s = scenes["cfg2"]
    vac = opl_ref.chain(orc, s["lenses"], s["table"], s["rays"], s["channel"], s["w_in"], s["p_in"], 4)
    r = torch.from_numpy(s["rays"].copy()).cuda()
    ch = torch.from_numpy(s["channel"].copy()).cuda()
    w = torch.from_numpy(s["w_in"].copy()).cuda()
    p = torch.from_numpy(s["p_in"].copy()).cuda()
    c = bzr.Context(0)
    try:
        dms = [bzr.DeviceMesh(c, q) for q in s["lenses"]]
        mode = flags_of(bzr, pipe_name)
        plan = ((GAPS2, s["rand"][4]), (GAPS_FRONT, front[4]), (None, vac), (GAPS2, s["rand"][4]))
        results = []
        for gaps, _ in plan:
            if gaps is None:
                results.append(bzr.trace_chain_opl(c, dms, s["table"], r, ch, weight=w, opl=p, max_bounces=4, mode=mode))
            else:
                results.append(bzr.trace_chain_media(c, dms, s["table"], gaps, r, ch, weight=w, opl=p, max_bounces=4,
                                                     mode=mode))
        torch.cuda.synchronize()
        c.sync()
        for k, (res, (_, want)) in enumerate(zip(results, plan)):
            o, ow, st, g, b, op, gl = (t.cpu().numpy() for t in res)
            got = (o, ow, st.astype(np.uint32), g.astype(np.uint32), b.astype(np.uint32), op, gl)
            assert_opl(got, want, f"{pipe_name}, device pointers: call {k}")
    finally:
        c.close()


# ------------------------------------------------------------------ 4. chunking and layouts
@pytest.fixture(scope="module")
def cctx(bzr, ctx):
    """This module's own context: the session context never sees a lowered chunk cap."""
    c = bzr.Context(0)
    yield c
    c.close()


def test_small_chunks(bzr, orc, cctx):
    """The gap rows belong to the lens, not to the chunk: every chunk of every stage reads the same two rows."""
    cfg = CONFIGS["cfg2"]
    lens = build_lens(bzr.TriMesh, cfg.lenses[0]).bezier_patches()
    full = grid_rays(cfg, side=128)
    n, mb = 1000, 3
    first = (full.shape[1] - n) // 2  # the grid's centre in tile order: every ray meets the lens
    rays = np.ascontiguousarray(full[:, first:first + n])
    channel = np.random.default_rng(9).integers(0, NCHAN, n).astype(np.uint8)
    w_in = np.random.default_rng(5).random(n, dtype=F)
    p_in = np.random.default_rng(6).random(n, dtype=F)
    want = media_ref.chain(orc, [lens], [ROW1], GAPS2, rays, channel, w_in, p_in, mb)
    assert int((want[4] > 0).sum()) >= 40 and int((want[6] > 0).sum()) >= 900
    dm = bzr.DeviceMesh(cctx, lens)
    kw = dict(weight=w_in, opl=p_in, max_bounces=mb, mode=bzr.PIPELINE_STAGED)
    try:
        for cap in (64, 192):
            assert set_cap(bzr, cctx, cap) == cap
            chunk = chunk_rule(n, cap)
            assert -(-n // chunk) >= 3 and n % chunk != 0, (cap, chunk)  # three chunks or more, a ragged last one
            got = bzr.trace_chain_media(cctx, [dm], [ROW1], GAPS2, rays, channel, **kw)
            assert_opl(got, want, f"cap {cap}: vs the reference")
    finally:
        set_cap(bzr, cctx, 0)


def test_device_buffers_and_aos(bzr, ctx, scenes):
    torch = pytest.importorskip("torch")
    s = scenes["cfg4"]
    want = s["rand"][4]
    r = torch.from_numpy(np.ascontiguousarray(s["rays"].T)).cuda()
    c = torch.from_numpy(s["channel"].copy()).cuda()
    w = torch.from_numpy(s["w_in"].copy()).cuda()
    p = torch.from_numpy(s["p_in"].copy()).cuda()
    for pipe in (bzr.PIPELINE_FUSED, bzr.PIPELINE_STAGED):
        res = bzr.trace_chain_media(ctx, s["dms"], s["table"], s["gaps"], r, c, weight=w, opl=p, max_bounces=4,
                                    mode=pipe | bzr.RAYS_AOS)
        torch.cuda.synchronize()
        o, ow, st, g, b, op, gl = (t.cpu().numpy() for t in res)
        got = (np.ascontiguousarray(o.T), ow, st.astype(np.uint32), g.astype(np.uint32), b.astype(np.uint32), op, gl)
        assert_opl(got, want, f"cfg4 device pointers, AoS, pipeline {pipe}")
    got = bzr.trace_chain_media(ctx, s["dms"], s["table"], s["gaps"], np.ascontiguousarray(s["rays"].T), s["channel"],
                                weight=s["w_in"], opl=s["p_in"], max_bounces=4, mode=bzr.RAYS_AOS)
    assert_opl((np.ascontiguousarray(got[0].T),) + got[1:], want, "cfg4 host pointers, AoS")


# ------------------------------------------------------------------ 5. special rays
@pytest.mark.parametrize("path", PATHS)
def test_channel_out_of_range_and_nan_ray(bzr, ctx, scenes, path):
    """A channel at or above nchan and a non-finite component: NONE, one segment, everything else as it came, glass 0;
    no word of any other ray changes."""
    s = scenes["cfg4"]
    rays, channel, w_in, p_in, want = s["rays"], s["channel"], s["w_in"], s["p_in"], s["rand"][4]
    n = rays.shape[1]
    cand = np.nonzero(want[4] > 0)[0]  # reflected rays, so their waves hold bounce segments
    assert len(cand) > 100
    mid = len(cand) // 2
    k255, kn, knan, kinf = int(cand[mid - 1]), int(cand[mid]), int(cand[mid + 1]), int(cand[mid + 2])
    ch = channel.copy()
    ch[k255], ch[kn] = 255, NCHAN
    poisoned = rays.copy()
    poisoned[4, knan] = np.nan
    poisoned[0, kinf] = np.inf
    got = run(bzr, ctx, s["dms"], s["table"], s["gaps"], poisoned, ch, path, 4, weight=w_in, opl=p_in)
    bad = [k255, kn, knan, kinf]
    for k in bad:
        assert got[2][k] == bzr.RR_NONE and got[3][k] == 1 and got[4][k] == 0, k
        assert bits(got[5])[k] == bits(p_in)[k] and bits(got[6])[k] == 0, k
        assert bits(got[1])[k] == bits(w_in)[k] and np.array_equal(bits(got[0])[:, k], bits(poisoned)[:, k]), k
    others = np.ones(n, bool)
    others[bad] = False
    assert_opl(tuple(a[..., others] for a in got), tuple(a[..., others] for a in want), f"{path}: the other rays")


# ------------------------------------------------------------------ 6. bad arguments
def test_bad_arguments_leave_the_outputs_untouched(bzr, ctx, scenes):
    s = scenes["cfg2"]
    n = 256
    r, c = np.ascontiguousarray(s["rays"][:, :n]), s["channel"][:n].copy()

    def sentinels():
        return (np.full((6, n), 7.0, F), np.full(n, 7.0, F), np.full(n, 7, np.uint32), np.full(n, 7, np.uint32),
                np.full(n, 7, np.uint32), np.full(n, 7.0, F), np.full(n, 7.0, F))

    def rejected(match, table, gaps, mb):
        o, w, st, g, b, p, q = outs = sentinels()
        with pytest.raises(bzr.BzrError, match=match):
            bzr.trace_chain_media(ctx, s["dms"], table, gaps, r, c, weight=s["w_in"][:n].copy(), max_bounces=mb,
                                  out_rays=o, out_weight=w, out_status=st, out_segments=g, out_bounces=b, out_opl=p,
                                  out_glass=q)
        assert all((a == 7).all() for a in outs)

    for value in (0.0, -1.333, np.nan, np.inf):
        for row, col in ((0, 0), (1, NCHAN - 1)):  # the first used entry and the last
            gaps = np.array(GAPS2, F)
            gaps[row, col] = value
            rejected("gap_table", s["table"], gaps, 4)
    rejected("max_bounces", s["table"], GAPS2, bzr.MAX_BOUNCES + 1)
    rejected("nchan", np.zeros((1, 0), F), np.zeros((2, 0), F), 4)
    rejected("nchan", np.full((1, 65), 1.3, F), np.ones((2, 65), F), 4)
    o, w, st, g, b, p, q = outs = sentinels()
    handles = (ctypes.c_void_p * 1)(s["dms"][0].handle)
    tab, gap = np.ascontiguousarray(s["table"], F), np.ascontiguousarray(GAPS2, F)
    assert bzr.lib().bzr_trace_chain_media(ctx.handle, ctypes.cast(handles, ctypes.c_void_p), tab.ctypes.data,
                                           gap.ctypes.data, 1, NCHAN, r.ctypes.data, c.ctypes.data, None, None, n, 4,
                                           o.ctypes.data, w.ctypes.data, st.ctypes.data, g.ctypes.data, b.ctypes.data,
                                           None, q.ctypes.data, 0) == 1  # NULL out_opl
    assert b"out_opl" in bzr.lib().bzr_last_error()
    assert all((a == 7).all() for a in outs)


# ------------------------------------------------------------------ 7. FAST with real gaps
@pytest.mark.parametrize("pipe_name", ("fused", "staged"))
def test_fast_chain_step_is_exact(bzr, ctx, scenes, front, pipe_name):
    """A budget-0 ray that ends NONE after two segments completed one leg, in the medium in front of the lens: out_opl
    is opl_in + n0 leg(input origin, output origin) from FAST's own points, bit for bit, and glass is 0."""
    s = scenes["cfg2"]
    want = front[0]
    assert int(((want[2] == bzr.RR_NONE) & (want[3] == 2)).sum()) >= 500  # measured: 610
    mode = flags_of(bzr, pipe_name) | bzr.MODE_FAST
    got = bzr.trace_chain_media(ctx, s["dms"], s["table"], GAPS_FRONT, s["rays"], s["channel"], opl=s["p_in"],
                                max_bounces=0, mode=mode)
    sel = (got[2] == bzr.RR_NONE) & (got[3] == 2)
    assert int(sel.sum()) >= 500
    n0 = np.asarray(GAPS_FRONT, F)[0][s["channel"][sel]]
    m = n0 * opl_ref.leg(s["rays"][0:3][:, sel], got[0][0:3][:, sel])
    assert m.dtype == F
    expect = s["p_in"][sel] + m
    assert np.array_equal(bits(got[5][sel]), bits(expect))
    assert not bits(got[6][sel]).any()


def shares(got, want):
    """(share of rays with the reference's status, segments and bounces; median |d - d_ref| over the rays OUTSIDE in both)."""
    same = (got[2] == want[2]) & (got[3] == want[3]) & (got[4] == want[4])
    both = (np.asarray(got[2]) == 2) & (want[2] == 2)
    err = np.sqrt(((np.asarray(got[0])[3:6][:, both].astype(np.float64) - want[0][3:6][:, both]) ** 2).sum(axis=0))
    return float(same.mean()), float(np.median(err)), int(both.sum())


@pytest.mark.parametrize("pipe_name", ("fused", "staged"))
@pytest.mark.parametrize("name", ("cfg2", "cfg4"))
def test_fast_quality_against_vacuum(bzr, orc, ctx, scenes, name, pipe_name):
    """FAST with media is judged against FAST without: the share of rays in media_ref's class may fall CLASS_ALLOW below
    the share FAST trace_chain_opl reaches against opl_ref on the same rays in vacuum, and the median direction error
    of the rays OUTSIDE in both may be BAR times the vacuum one."""
    s = scenes[name]
    mode = flags_of(bzr, pipe_name) | bzr.MODE_FAST
    kw = dict(weight=s["w_in"], opl=s["p_in"], max_bounces=4, mode=mode)
    vac_ref = opl_ref.chain(orc, s["lenses"], s["table"], s["rays"], s["channel"], s["w_in"], s["p_in"], 4)
    vac = bzr.trace_chain_opl(ctx, s["dms"], s["table"], s["rays"], s["channel"], **kw)
    med = bzr.trace_chain_media(ctx, s["dms"], s["table"], s["gaps"], s["rays"], s["channel"], **kw)
    share_v, err_v, n_v = shares(vac, vac_ref)
    share_m, err_m, n_m = shares(med, s["rand"][4])
    print(f"FAST {name} {pipe_name}: class share media {share_m:.5f} vacuum {share_v:.5f}; median direction error media "
          f"{err_m:.3g} ({n_m} rays) vacuum {err_v:.3g} ({n_v} rays)")
    assert n_m >= 2400 and n_v >= 1500
    assert share_m >= share_v - CLASS_ALLOW
    assert err_m <= BAR * err_v
