"""Beer-Lambert absorption on the GPU: bzr_trace_chain_absorb against tests/absorb_ref.py (media_ref's chain with the
attenuation step in numpy float32), bit for bit, on the fused kernel, the staged pipeline and the brute-force scan.

The scenes are test_gpu_media.py's: 64^2 - 37 rays (a ragged last wave), four channels mixed in every wave, and the
cemented doublet.  The absorption tables are absorb_ref's: channel 0 absorbs nothing, channel 3's glass is opaque (att
returns 0 there, and rays of weight 0 are traced on).
"""
import ctypes

import numpy as np
import pytest

import absorb_ref
import media_ref
import opl_ref
import tir_ref
from absorb_ref import DOUBLET_GAPA, DOUBLET_GLASS, GAPA2, GAPA4, GLASS2, GLASS4
from bzr_amd.configs import CONFIGS, build_lens, grid_rays
from media_ref import DOUBLET_CEMENT, DOUBLET_RI, GAPS2, GAPS4, GAPS_FRONT
from test_chunk_plan import chunk_rule
from test_gpu_opl import assert_opl
from test_gpu_power import bits, flags_of, frozen, set_cap
from test_gpu_tir import DROP, NCHAN, PATHS, ROW1, SIDE, TABLES, assert_tir

pytestmark = pytest.mark.gpu

F = np.float32
BUDGETS = {"cfg2": (0, 4, 8), "cfg4": (0, 4), "doublet": (4,)}
GAPS = {"cfg2": GAPS2, "cfg4": GAPS4, "doublet": DOUBLET_CEMENT}
GLASS = {"cfg2": GLASS2, "cfg4": GLASS4, "doublet": DOUBLET_GLASS}
GAPA = {"cfg2": GAPA2, "cfg4": GAPA4, "doublet": DOUBLET_GAPA}
GLASS_B, GAPA_B = [[0.3, 0.0, 0.01, 5.0]], [[0.1, 0.4, 0.0, 0.002]]  # cfg2's second pair (the table cache)


def run(bzr, ctx, dms, table, gaps, glass, gapa, rays, channel, path, max_bounces, **kw):
    return bzr.trace_chain_absorb(ctx, dms, table, gaps, glass, gapa, rays, channel, max_bounces=max_bounces,
                                  mode=flags_of(bzr, path), **kw)


@pytest.fixture(scope="module")
def scenes(bzr, orc, ctx):
    """name -> dict(lenses, table, gaps, glass, gapa, dms, rays, channel, w_in, p_in, rand {max_bounces: reference with
    the random rows}, media {max_bounces: media_ref's reference with the same rows}): computed once, never changed."""
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
        rand, media = {}, {}
        for mb in BUDGETS[name]:
            rand[mb] = frozen(*absorb_ref.chain(orc, lenses, table, GAPS[name], GLASS[name], GAPA[name], rays, channel,
                                                w_in, p_in, mb))
            media[mb] = frozen(*media_ref.chain(orc, lenses, table, GAPS[name], rays, channel, w_in, p_in, mb))
        frozen(rays, channel, w_in, p_in)
        out[name] = dict(lenses=lenses, table=table, gaps=GAPS[name], glass=GLASS[name], gapa=GAPA[name],
                         dms=[bzr.DeviceMesh(ctx, p) for p in lenses], rays=rays, channel=channel, w_in=w_in, p_in=p_in,
                         rand=rand, media=media)
    return out


# ------------------------------------------------------------------ 0. the term itself
def test_device_attenuation_is_the_host_form(bzr, ctx):
    x = absorb_ref.att_values()
    host = bzr.debug_attenuation(x)
    dev = bzr.debug_attenuation(x, ctx)
    assert x.size == 1 << 20
    assert np.array_equal(bits(dev), bits(host))
    assert np.array_equal(bits(dev), bits(absorb_ref.att(x)))


# ------------------------------------------------------------------ 1. bit-exact
CASES = [(name, mb) for name in BUDGETS for mb in BUDGETS[name]]


@pytest.mark.parametrize("name,max_bounces", CASES)
@pytest.mark.parametrize("path", PATHS)
def test_bit_exact(bzr, ctx, scenes, name, path, max_bounces):
    s = scenes[name]
    n = s["rays"].shape[1]
    assert n == SIDE * SIDE - DROP == 4059 and n % 64 != 0
    want, med = s["rand"][max_bounces], s["media"][max_bounces]
    # absorption moved weights, those of reflected rays among them; nothing else
    unlike = bits(want[1]) != bits(med[1])
    assert int(unlike.sum()) >= 1000
    # (reflected rays with a weight unlike media_ref's: cfg2 290 of 325, cfg4 167 of 167, the doublet 2 of 2)
    if max_bounces:
        assert int((unlike & (want[4] > 0)).sum()) >= (1 if name == "doublet" else 100), name
    for k in (0, 2, 3, 4, 5, 6):
        assert np.array_equal(bits(want[k]), bits(med[k]))
    if name != "doublet":  # opaque glass: rays of weight 0 that went on to leave the lens
        assert int(((want[1] == 0) & (want[2] == bzr.RR_OUTSIDE) & (s["w_in"] > 0)).sum()) >= 100
    w, p = s["w_in"].copy(), s["p_in"].copy()  # both passed in place
    got = run(bzr, ctx, s["dms"], s["table"], s["gaps"], s["glass"], s["gapa"], s["rays"], s["channel"], path,
              max_bounces, weight=w, out_weight=w, opl=p, out_opl=p)
    assert got[1] is w and got[5] is p
    assert_opl(got, want, f"{name} {path} max_bounces {max_bounces}, random rows in place")


@pytest.mark.parametrize("path", PATHS)
def test_geometry_is_trace_chain_media(bzr, ctx, scenes, path):
    """Absorption moves the weight alone: the other six outputs equal trace_chain_media's, bit for bit."""
    s = scenes["cfg4"]
    kw = dict(weight=s["w_in"], opl=s["p_in"], max_bounces=4, mode=flags_of(bzr, path))
    want = bzr.trace_chain_media(ctx, s["dms"], s["table"], s["gaps"], s["rays"], s["channel"], **kw)
    got = bzr.trace_chain_absorb(ctx, s["dms"], s["table"], s["gaps"], s["glass"], s["gapa"], s["rays"], s["channel"], **kw)
    for k in (0, 2, 3, 4, 5, 6):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert int((bits(got[1]) != bits(want[1])).sum()) >= 1000


# ------------------------------------------------------------------ 2. zero tables
@pytest.mark.parametrize("max_bounces", (0, 4))
@pytest.mark.parametrize("path,fast", [(p, False) for p in PATHS] + [("fused", True), ("staged", True)])
def test_zero_tables_are_trace_chain_media(bzr, ctx, scenes, path, fast, max_bounces):
    """A x 1 = A: zero tables, NULL ones and one of each give bzr_trace_chain_media's seven outputs bit for bit, in
    parity on all three paths and in FAST on the two that have a FAST form."""
    s = scenes["cfg4"]
    mode = flags_of(bzr, path) | (bzr.MODE_FAST if fast else 0)
    kw = dict(weight=s["w_in"], opl=s["p_in"], max_bounces=max_bounces, mode=mode)
    want = bzr.trace_chain_media(ctx, s["dms"], s["table"], s["gaps"], s["rays"], s["channel"], **kw)
    assert int((want[2] == bzr.RR_OUTSIDE).sum()) > 1500
    want = tuple(np.asarray(a) for a in want)
    zeros = np.zeros((2, NCHAN), F)
    for what, glass, gapa in (("zeros", zeros, zeros), ("NULL", None, None), ("glass only", zeros, None),
                              ("gap only", None, zeros)):
        got = bzr.trace_chain_absorb(ctx, s["dms"], s["table"], s["gaps"], glass, gapa, s["rays"], s["channel"], **kw)
        assert_opl(got, want, f"cfg4 {path} fast={fast} max_bounces {max_bounces}, tables {what}")


@pytest.mark.parametrize("path", PATHS)
def test_one_table_only(bzr, orc, ctx, scenes, path):
    """Only one of the two tables non-NULL: the other counts as zero."""
    s = scenes["cfg2"]
    for glass, gapa in ((GLASS2, None), (None, GAPA2)):
        want = absorb_ref.chain(orc, s["lenses"], s["table"], GAPS2, glass, gapa, s["rays"], s["channel"], s["w_in"],
                                s["p_in"], 4)
        got = run(bzr, ctx, s["dms"], s["table"], GAPS2, glass, gapa, s["rays"], s["channel"], path, 4, weight=s["w_in"],
                  opl=s["p_in"])
        assert_opl(got, want, f"cfg2 {path}, glass {glass is not None}, gap {gapa is not None}")


# ------------------------------------------------------------------ 3. the table cache
@pytest.fixture(scope="module")
def cache_plan(orc, scenes):
    """Calls on one context, each changing one table against the call before: (kind, tables, reference)."""
    s = scenes["cfg2"]
    args = (s["rays"], s["channel"], s["w_in"], s["p_in"], 4)

    def ab(gaps, glass, gapa):
        return frozen(*absorb_ref.chain(orc, s["lenses"], s["table"], gaps, glass, gapa, *args))

    a, med = s["rand"][4], s["media"][4]
    tir = frozen(*tir_ref.chain(orc, s["lenses"], s["table"], s["rays"], s["channel"], s["w_in"], 4))
    return (("absorb", (GAPS2, GLASS2, GAPA2), a),
            ("absorb", (GAPS2, GLASS_B, GAPA2), ab(GAPS2, GLASS_B, GAPA2)),        # only glass_absorb
            ("media", (GAPS2,), med),
            ("absorb", (GAPS2, GLASS_B, GAPA_B), ab(GAPS2, GLASS_B, GAPA_B)),      # only gap_absorb
            ("tir", (), tir),
            ("absorb", (GAPS_FRONT, GLASS_B, GAPA_B), ab(GAPS_FRONT, GLASS_B, GAPA_B)),  # only gap_table
            ("absorb", (GAPS_FRONT, None, GAPA_B), ab(GAPS_FRONT, None, GAPA_B)),  # glass_absorb to NULL
            ("absorb", (GAPS2, GLASS2, GAPA2), a))


def cache_call(bzr, c, dms, s, kind, tables, r, ch, w, p, mode):
    if kind == "absorb":
        return bzr.trace_chain_absorb(c, dms, s["table"], *tables, r, ch, weight=w, opl=p, max_bounces=4, mode=mode)
    if kind == "media":
        return bzr.trace_chain_media(c, dms, s["table"], *tables, r, ch, weight=w, opl=p, max_bounces=4, mode=mode)
    return bzr.trace_chain_tir(c, dms, s["table"], r, ch, weight=w, max_bounces=4, mode=mode)


@pytest.mark.parametrize("path", PATHS)
def test_table_cache(bzr, scenes, cache_plan, path):
    s = scenes["cfg2"]
    c = bzr.Context(0)
    try:
        dms = [bzr.DeviceMesh(c, p) for p in s["lenses"]]
        for k, (kind, tables, want) in enumerate(cache_plan):
            got = cache_call(bzr, c, dms, s, kind, tables, s["rays"], s["channel"], s["w_in"], s["p_in"],
                             flags_of(bzr, path))
            (assert_tir if kind == "tir" else assert_opl)(got, want, f"{path}: call {k} ({kind})")
    finally:
        c.close()


@pytest.mark.parametrize("pipe_name", ("fused", "staged"))
def test_table_cache_device_pointers(bzr, scenes, cache_plan, pipe_name):
    """The same with device rows and no synchronisation between the calls: a part is rewritten only after the kernels
    that read the old one have finished."""
    torch = pytest.importorskip("torch")
    s = scenes["cfg2"]
    r = torch.from_numpy(s["rays"].copy()).cuda()
    ch = torch.from_numpy(s["channel"].copy()).cuda()
    w = torch.from_numpy(s["w_in"].copy()).cuda()
    p = torch.from_numpy(s["p_in"].copy()).cuda()
    c = bzr.Context(0)
    try:
        dms = [bzr.DeviceMesh(c, q) for q in s["lenses"]]
        mode = flags_of(bzr, pipe_name)
        results = [cache_call(bzr, c, dms, s, kind, tables, r, ch, w, p, mode) for kind, tables, _ in cache_plan]
        torch.cuda.synchronize()
        c.sync()
        for k, (res, (kind, _, want)) in enumerate(zip(results, cache_plan)):
            a = [t.cpu().numpy() for t in res]
            got = tuple(x.astype(np.uint32) if j in (2, 3, 4) else x for j, x in enumerate(a))
            (assert_tir if kind == "tir" else assert_opl)(got, want, f"{pipe_name}, device pointers: call {k} ({kind})")
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
    """The table rows belong to the lens, not to the chunk: every chunk of every stage reads the same rows."""
    cfg = CONFIGS["cfg2"]
    lens = build_lens(bzr.TriMesh, cfg.lenses[0]).bezier_patches()
    full = grid_rays(cfg, side=128)
    n, mb = 1000, 3
    first = (full.shape[1] - n) // 2  # the grid's centre in tile order: every ray meets the lens
    rays = np.ascontiguousarray(full[:, first:first + n])
    channel = np.random.default_rng(9).integers(0, NCHAN, n).astype(np.uint8)
    w_in = np.random.default_rng(5).random(n, dtype=F)
    p_in = np.random.default_rng(6).random(n, dtype=F)
    want = absorb_ref.chain(orc, [lens], [ROW1], GAPS2, GLASS2, GAPA2, rays, channel, w_in, p_in, mb)
    assert int((want[4] > 0).sum()) >= 40 and int((want[6] > 0).sum()) >= 900
    dm = bzr.DeviceMesh(cctx, lens)
    kw = dict(weight=w_in, opl=p_in, max_bounces=mb, mode=bzr.PIPELINE_STAGED)
    try:
        for cap in (64, 192):
            assert set_cap(bzr, cctx, cap) == cap
            chunk = chunk_rule(n, cap)
            assert -(-n // chunk) >= 3 and n % chunk != 0, (cap, chunk)  # three chunks or more, a ragged last one
            got = bzr.trace_chain_absorb(cctx, [dm], [ROW1], GAPS2, GLASS2, GAPA2, rays, channel, **kw)
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
        res = bzr.trace_chain_absorb(ctx, s["dms"], s["table"], s["gaps"], s["glass"], s["gapa"], r, c, weight=w, opl=p,
                                     max_bounces=4, mode=pipe | bzr.RAYS_AOS)
        torch.cuda.synchronize()
        o, ow, st, g, b, op, gl = (t.cpu().numpy() for t in res)
        got = (np.ascontiguousarray(o.T), ow, st.astype(np.uint32), g.astype(np.uint32), b.astype(np.uint32), op, gl)
        assert_opl(got, want, f"cfg4 device pointers, AoS, pipeline {pipe}")
    got = bzr.trace_chain_absorb(ctx, s["dms"], s["table"], s["gaps"], s["glass"], s["gapa"],
                                 np.ascontiguousarray(s["rays"].T), s["channel"], weight=s["w_in"], opl=s["p_in"],
                                 max_bounces=4, mode=bzr.RAYS_AOS)
    assert_opl((np.ascontiguousarray(got[0].T),) + got[1:], want, "cfg4 host pointers, AoS")


# ------------------------------------------------------------------ 5. special rays
@pytest.mark.parametrize("path", PATHS)
def test_channel_out_of_range_and_nan_ray(bzr, ctx, scenes, path):
    """A channel at or above nchan and a non-finite component: NONE, one segment, weight and everything else as it came;
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
    got = run(bzr, ctx, s["dms"], s["table"], s["gaps"], s["glass"], s["gapa"], poisoned, ch, path, 4, weight=w_in,
              opl=p_in)
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

    def rejected(match, table, gaps, glass, gapa, mb):
        o, w, st, g, b, p, q = outs = sentinels()
        with pytest.raises(bzr.BzrError, match=match):
            bzr.trace_chain_absorb(ctx, s["dms"], table, gaps, glass, gapa, r, c, weight=s["w_in"][:n].copy(),
                                   max_bounces=mb, out_rays=o, out_weight=w, out_status=st, out_segments=g,
                                   out_bounces=b, out_opl=p, out_glass=q)
        assert all((a == 7).all() for a in outs)

    for value in (-1e-6, -3.0, np.nan, np.inf):
        for col in (0, NCHAN - 1):  # the first used entry and the last
            t = np.array(GLASS2, F)
            t[0, col] = value
            rejected("glass_absorb", s["table"], GAPS2, t, GAPA2, 4)
            rejected("gap_absorb", s["table"], GAPS2, GLASS2, t, 4)
    bad_gaps = np.array(GAPS2, F)
    bad_gaps[1, 2] = 0.0
    rejected("gap_table", s["table"], bad_gaps, GLASS2, GAPA2, 4)
    rejected("max_bounces", s["table"], GAPS2, GLASS2, GAPA2, bzr.MAX_BOUNCES + 1)
    rejected("nchan", np.full((1, 65), 1.3, F), np.ones((2, 65), F), np.zeros((1, 65), F), np.zeros((1, 65), F), 4)
    o, w, st, g, b, p, q = outs = sentinels()
    handles = (ctypes.c_void_p * 1)(s["dms"][0].handle)
    tab = np.ascontiguousarray(s["table"], F)
    assert bzr.lib().bzr_trace_chain_absorb(ctx.handle, ctypes.cast(handles, ctypes.c_void_p), tab.ctypes.data, None, None,
                                            None, 1, NCHAN, r.ctypes.data, c.ctypes.data, None, None, n, 4, o.ctypes.data,
                                            w.ctypes.data, st.ctypes.data, g.ctypes.data, b.ctypes.data, None,
                                            q.ctypes.data, 0) == 1  # NULL out_opl
    assert b"out_opl" in bzr.lib().bzr_last_error()
    assert all((a == 7).all() for a in outs)


# ------------------------------------------------------------------ 7. FAST
@pytest.mark.parametrize("pipe_name", ("fused", "staged"))
def test_fast_chain_step_is_exact(bzr, ctx, scenes, pipe_name):
    """cfg2 immersed in front, only gap_absorb non-zero, budget 0, weight 1.  A ray that ends NONE after two segments
    completed one leg, in the medium in front of the lens: its weight is att(g leg(input origin, output origin)) from
    FAST's own points times FAST trace_chain_media's weight (the Fresnel term of its one refraction), bit for bit."""
    s = scenes["cfg2"]
    mode = flags_of(bzr, pipe_name) | bzr.MODE_FAST
    med = bzr.trace_chain_media(ctx, s["dms"], s["table"], GAPS_FRONT, s["rays"], s["channel"], max_bounces=0, mode=mode)
    gapa = [[0.02, 0.3, 1.5, 0.0]]
    got = bzr.trace_chain_absorb(ctx, s["dms"], s["table"], GAPS_FRONT, None, gapa, s["rays"], s["channel"],
                                 max_bounces=0, mode=mode)
    for k in (0, 2, 3, 4, 5, 6):
        assert np.array_equal(bits(got[k]), bits(med[k])), k
    sel = (got[2] == bzr.RR_NONE) & (got[3] == 2)
    assert int(sel.sum()) >= 100  # the media reference has 610
    g = np.asarray(gapa, F)[0][s["channel"][sel]]
    x = g * opl_ref.leg(s["rays"][0:3][:, sel], got[0][0:3][:, sel])
    assert x.dtype == F
    a = np.where(g > 0, absorb_ref.att(x), F(1)).astype(F)
    expect = a * med[1][sel]
    assert expect.dtype == F
    assert np.array_equal(bits(got[1][sel]), bits(expect))
    assert int((bits(got[1][sel]) != bits(med[1][sel])).sum()) >= 50
