"""Refraction chains of 3 to 8 lenses (include/bzr.h: nlens is 1..8) against the oracle, bit for bit.

Every other test traces one or two lenses, so k_trace<kModeStage>'s lens[k >> 1] past index 1, the staged driver's
up to 16 in-place run_segment calls, the dispatch order's key over all eight lens pointers, the compact gather byte's
segment counts past 4 and the nlens == 0 / nlens > 8 rejections are reached here only.

Geometry: lens k is makeEllipsoid(12, 6, (1, 4, 2)) moved to x = 10 + 3 k and standardized (432 patches), k = 0..7,
built with the oracle's mesh code; the rays are cfg2's 64 x 64 grid in tile order (4 096 rays, 64 waves).  The
oracle's segment histogram over the eight lenses (ri 1.3 each) is 1: 1388, 2: 86, 5: 60, 7: 86, 8: 16, 9: 6, 11: 36,
13: 110, 14: 2, 15: 31, 16: 2275 (14 of those end NONE at segment 16); the populations the tests rely on are asserted
from the oracle's output, so no test here passes vacuously.
"""
import ctypes

import numpy as np
import pytest

from bzr_amd.configs import CONFIGS, Lens, build_lens, grid_rays

pytestmark = pytest.mark.gpu

MODES = ("fused", "staged", "brute")
N_LENS = 8
N_PATCH = 432
RI_MIXED = [1.05, 1.9, 1.3, 1.1, 1.5, 1.3, 1.7, 1.2]


def lens_x(k):
    return 10.0 + 3.0 * k


def lens_patches(orc, k):
    """Lens k of the common geometry, from the oracle's Mesh."""
    m = orc.OMesh().make_ellipsoid(12, 6, (1.0, 4.0, 2.0))
    m.translate((lens_x(k), 0.0, 0.0))
    p = m.standardize().bezier_patches()
    assert p.shape == (N_PATCH, 66)
    return p


def chain_rays():
    return grid_rays(CONFIGS["cfg2"], side=64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def mode_of(bzr, m):
    return {"fused": bzr.PIPELINE_FUSED, "staged": bzr.PIPELINE_STAGED, "brute": bzr.ACCEL_NONE}[m]


def assert_chain_equal(got, want, label):
    (g_rays, g_st, g_seg), (w_rays, w_st, w_seg) = got, want
    bad = (bits(g_st) != bits(w_st)) | (bits(g_seg) != bits(w_seg)) | (bits(g_rays) != bits(w_rays)).any(axis=0)
    assert not bad.any(), (f"{label}: {int(bad.sum())} of {len(bad)} rays differ, first {np.nonzero(bad)[0][:8]}; "
                           f"segments got {np.asarray(g_seg)[bad][:8]} want {w_seg[bad][:8]}, "
                           f"status got {np.asarray(g_st)[bad][:8]} want {w_st[bad][:8]}")


@pytest.fixture(scope="module")
def lens8(orc):
    out = [lens_patches(orc, k) for k in range(N_LENS)]
    for p in out:
        p.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def big3(orc):
    """cfg2's 3 072-patch lens at lens 3's place."""
    p = build_lens(orc.OMesh, Lens("ellipsoid", 32, 16, (1.0, 4.0, 2.0), (lens_x(3), 0.0, 0.0))).bezier_patches()
    assert len(p) == 3072
    p.setflags(write=False)
    return p


@pytest.fixture(scope="module")
def rays():
    r = chain_rays()
    assert r.shape == (6, 4096)
    r.setflags(write=False)
    return r


@pytest.fixture(scope="module")
def sets(lens8, big3):
    """name -> (indices into the mesh table, refractive indices); mesh 8 is big3."""
    mixed = list(range(3)) + [8] + list(range(4, 8))
    return {"n3": ([0, 1, 2], [1.3] * 3), "n5": (list(range(5)), [1.3] * 5), "n8": (list(range(8)), [1.3] * 8),
            "ri": (list(range(8)), RI_MIXED), "big3": (mixed, RI_MIXED), "reversed": (mixed[::-1], RI_MIXED[::-1]),
            "same8": ([0] * 8, [1.3] * 8)}


@pytest.fixture(scope="module")
def table(lens8, big3):
    return lens8 + [big3]


@pytest.fixture(scope="module")
def want(orc, table, sets, rays):
    """The oracle's chain over every lens set and its work counters, computed once and never changed."""
    out = {}
    for name, (idx, ri) in sets.items():
        orc.counters_reset()
        res = orc.trace_chain([table[k] for k in idx], ri, rays)
        for a in res:
            a.setflags(write=False)
        out[name] = (res, orc.counters())
    return out


@pytest.fixture(scope="module")
def dms(bzr, ctx, table):
    return [bzr.DeviceMesh(ctx, p) for p in table]


def test_the_long_chain_reaches_every_stage(bzr, want):
    """Non-vacuity, from the oracle alone."""
    (_, st, seg), work = want["n8"]
    hist = np.bincount(seg, minlength=17)
    print("8 lenses: segments", {k: int(v) for k, v in enumerate(hist) if v}, "oracle work", work)
    assert seg.max() == 16 and hist[16] >= 2000             # most rays run all 16 segments
    assert (hist > 0).sum() >= 8                             # rays leave the chain at many different stages
    dead = st == bzr.RR_NONE
    assert (dead & (seg % 2 == 1) & (seg > 1)).any()        # a ray misses a later lens's front ...
    assert (dead & (seg % 2 == 0) & (seg > 2)).any()        # ... and one is lost inside a later lens
    assert (dead & (seg == 16)).any() and (~dead & (seg == 16)).any()
    (_, _, seg3), _ = want["n3"]
    (_, _, seg5), _ = want["n5"]
    assert seg3.max() == 6 and seg5.max() == 10
    (_, _, same), _ = want["same8"]
    assert same.max() <= 3 and (same == 2).any()             # one mesh eight times: nothing gets past it twice
    for name in ("ri", "big3"):
        (_, _, g), _ = want[name]
        assert (g == 16).sum() > 500 and len(np.unique(g)) >= 10, (name, np.bincount(g))
    assert (want["big3"][0][2] != want["ri"][0][2]).any()    # the finer lens 3 changes some rays' fate
    (_, _, back), _ = want["reversed"]
    assert back.max() == 3 and (back == 3).sum() > 2000      # backwards: the second lens lies behind the first


@pytest.mark.parametrize("m", MODES)
@pytest.mark.parametrize("name", ["n3", "n5", "n8", "ri", "big3", "reversed", "same8"])
def test_chain_equals_oracle(bzr, ctx, dms, sets, want, rays, name, m):
    """n3 / n5 / n8: ri 1.3 each.  ri: eight different indices.  big3: lens 3 is the 3 072-patch lens, so the staged
    workspace is sized by the largest lens, not the first, and the small-scan / hipCUB switch falls mid-chain.
    reversed: big3's list backwards.  same8: one DeviceMesh passed eight times (eight equal pointers)."""
    idx, ri = sets[name]
    got = bzr.trace_chain(ctx, [dms[k] for k in idx], ri, rays, mode=mode_of(bzr, m))
    assert_chain_equal(got, want[name][0], f"{name} {m}")


def test_counters_over_the_long_chain(bzr, ctx, dms, sets, want, rays):
    """k_trace's work over 16 segments is the oracle's: every gate pass ran Newton once, every follow retry ran."""
    idx, ri = sets["n8"]
    (_, _, w_seg), work = want["n8"]
    rep = {}
    for m in ("fused", "staged"):
        ctx.counters(True)
        ctx.counters_report()
        got = bzr.trace_chain(ctx, [dms[k] for k in idx], ri, rays, mode=mode_of(bzr, m))
        rep[m] = ctx.counters_report()
        ctx.counters(False)
        assert_chain_equal(got, want["n8"][0], m)
    print("fused", rep["fused"], "staged", rep["staged"], "oracle", work)
    assert rep["fused"]["segments"] == work["segments"] == int(w_seg.sum())
    assert rep["fused"]["pairs"] == work["newton"]
    assert rep["fused"]["follows"] == work["follow"]
    assert rep["fused"]["overflow_rays"] == 0
    assert rep["staged"]["segments"] == work["segments"]


def test_ordered_dispatch_over_a_long_lens_set(bzr, lens8):
    """k_trace's cost-ordered dispatch keys its saved tile order on all the lens pointers: 20 fused calls of one size
    (2 304 tiles), every third over the reversed set, so the order is dropped and rebuilt; each equals its set's
    brute-force result."""
    import torch

    c = bzr.Context(0)  # a fresh context: no order yet
    fwd = [bzr.DeviceMesh(c, p) for p in lens8]
    rev = fwd[::-1]
    ri = [1.3] * N_LENS
    r = torch.from_numpy(grid_rays(CONFIGS["cfg2"], side=384)).cuda()
    assert r.shape[1] // 64 >= 2048
    ref = {id(s): [t.cpu().numpy() for t in bzr.trace_chain(c, s, ri, r, mode=bzr.ACCEL_NONE)] for s in (fwd, rev)}
    assert int(ref[id(fwd)][2].max()) == 16 and int(ref[id(rev)][2].max()) <= 4
    for k in range(20):
        s = rev if k % 3 == 2 else fwd
        got = bzr.trace_chain(c, s, ri, r, mode=bzr.PIPELINE_FUSED)
        for g, w in zip(got, ref[id(s)]):
            assert np.array_equal(bits(g.cpu().numpy()), bits(w)), k


def test_tiled_long_chain_equals_single_context(bzr, ctx, dms, lens8, sets, want, rays):
    idx, ri = sets["n8"]
    ctxs = [bzr.Context(0) for _ in range(2)]
    lenses = [[bzr.DeviceMesh(c, p) for p in lens8] for c in ctxs]
    got = bzr.trace_tiled(ctxs, lenses, ri, rays, tile_rays=1000)
    single = bzr.trace_chain(ctx, [dms[k] for k in idx], ri, rays)
    assert_chain_equal(got, single, "tiled vs single")
    assert_chain_equal(got, want["n8"][0], "tiled vs oracle")


def test_packed_long_chain_keeps_segments_up_to_16(bzr, ctx, dms, sets, want, rays):
    """The traced 8-lens frame through bzr_pack_frame in the three gather layouts: the torch packers' words, and the
    reader (frame.assemble / unpack_compact) returns status, segments up to 16 and the rays unchanged."""
    import torch

    from bzr_amd import frame

    cfg, side = CONFIGS["cfg2"], 64
    _, _, prim = frame.rank_rays(cfg, 0, 1, side, side)
    assert np.array_equal(bits(prim), bits(rays))  # one 64 x 64 tile: the grid's own order
    idx, ri = sets["n8"]
    o, st, sg = bzr.trace_chain(ctx, [dms[k] for k in idx], ri, torch.from_numpy(np.array(rays)).cuda())
    torch.cuda.synchronize()
    (w_rays, w_st, w_seg), _ = want["n8"]
    assert int(sg.max()) == 16
    n, npad = rays.shape[1], frame.padded_count(1, side, side)
    count = int(frame.survivors(st, sg).sum())
    cap = frame.compact_capacity(count, npad)
    rows, cols = frame.shard_pixels(cfg, 0, 1, side=side, height=side, block=frame.TILE)
    flat = rows * side + cols
    for layout in frame.LAYOUTS:
        if layout == "compact":
            shape = (frame.compact_size(npad, cap),)
        else:
            shape = (frame.IMAGE_ROWS if layout == "image" else frame.PACKED_ROWS, npad)
        ref = torch.zeros(shape, dtype=torch.float32, device="cuda")
        got = torch.zeros(shape, dtype=torch.float32, device="cuda")
        if layout == "compact":
            frame.pack_compact(st, sg, o, ref, npad, cap)
        else:
            frame.pack(o if layout == "rays" else None, st, sg, ref)
        bzr.pack_frame(ctx, layout, None if layout == "image" else o, st, sg, got, npad, cap)
        torch.cuda.synchronize()
        if layout == "compact":
            nw = frame.compact_words(npad)
            assert torch.equal(got[:nw + 1].view(torch.int32), ref[:nw + 1].view(torch.int32))
            g6, r6 = got[nw + 1:].view(6, cap + 1), ref[nw + 1:].view(6, cap + 1)
            assert torch.equal(g6[:, :count].view(torch.int32), r6[:, :count].view(torch.int32))
            r, s, g = frame.unpack_compact(got.cpu(), n, npad, cap, prim)
            assert np.array_equal(s, w_st) and np.array_equal(g, w_seg) and np.array_equal(bits(r), bits(w_rays))
        else:
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
        a_rays, a_st, a_seg = frame.assemble([got], cfg, 1, side, side, cap=cap)
        assert np.array_equal(a_st[flat], w_st) and np.array_equal(a_seg[flat], w_seg), layout
        assert a_seg.max() == 16
        if layout != "image":
            assert np.array_equal(bits(a_rays[:, flat]), bits(w_rays)), layout


def test_lens_counts_outside_1_to_8_are_rejected(bzr, ctx, dms, rays):
    """nlens = 0 and nlens = 9: BZR_ERR_INVALID_ARGUMENT with a message, before any output is touched."""
    L = bzr.lib()
    n = 256
    r = np.ascontiguousarray(rays[:, :n])
    handles = (ctypes.c_void_p * 9)(*[dms[k % N_LENS].handle for k in range(9)])
    ris = (ctypes.c_float * 9)(*([1.3] * 9))
    one_ctx = (ctypes.c_void_p * 1)(ctx.handle)
    em = bzr.Emitter(origin=(0.0, -0.5, -0.5), edge_u=(0.0, 1.0, 0.0), edge_v=(0.0, 0.0, 1.0), parts_u=2, parts_v=2,
                     points_per_part=8, rays_per_point=8, belts=16, seed=7)
    tg = bzr.Target(origin=(40.0, -12.0, -12.0), axis_u=(0.0, 1.0, 0.0), axis_v=(0.0, 0.0, 1.0), size_u=24.0,
                    size_v=24.0, bins_u=8, bins_v=8)
    for nlens in (0, 9):
        o = np.full((6, n), 7.5, np.float32)
        st = np.full(n, 0xA5A5A5A5, np.uint32)
        sg = np.full(n, 0xA5A5A5A5, np.uint32)
        hist = np.full((8, 8), 0xA5A5A5A5, np.uint32)
        stats = (ctypes.c_uint64 * 4)(*([0xA5] * 4))
        calls = {
            "bzr_trace_chain": lambda: L.bzr_trace_chain(ctx.handle, ctypes.cast(handles, ctypes.c_void_p),
                                                         ctypes.cast(ris, ctypes.c_void_p), nlens, r.ctypes.data, n,
                                                         o.ctypes.data, st.ctypes.data, sg.ctypes.data, bzr.HOST_PTRS),
            "bzr_trace_tiled": lambda: L.bzr_trace_tiled(ctypes.cast(one_ctx, ctypes.c_void_p), 1,
                                                         ctypes.cast(handles, ctypes.c_void_p),
                                                         ctypes.cast(ris, ctypes.c_void_p), nlens, r.ctypes.data, n, 64,
                                                         o.ctypes.data, st.ctypes.data, sg.ctypes.data, bzr.HOST_PTRS),
            "bzr_illuminate": lambda: L.bzr_illuminate(ctx.handle, handles, ris, nlens, ctypes.byref(em), 256,
                                                       ctypes.byref(tg), hist.ctypes.data, stats, bzr.HOST_PTRS),
        }
        for name, call in calls.items():
            assert call() == 1, (name, nlens)  # BZR_ERR_INVALID_ARGUMENT
            assert len(L.bzr_last_error()) > 0, (name, nlens)
            assert (o == 7.5).all() and (st == 0xA5A5A5A5).all() and (sg == 0xA5A5A5A5).all(), (name, nlens)
            assert (hist == 0xA5A5A5A5).all() and list(stats) == [0xA5] * 4, (name, nlens)
    # the limits themselves are accepted
    got = bzr.trace_chain(ctx, [dms[0]], [1.3], r)
    assert got[2].max() == 2


def test_illuminate_over_three_lenses(bzr, orc, ctx, dms, lens8):
    from test_gpu_illumination import emitter, oracle_illuminate, target

    n, ri = 1 << 15, [1.3, 1.5, 1.3]
    hist, stats = bzr.illuminate(ctx, dms[:3], ri, emitter(bzr), n, target(bzr))
    _, status, seg, want_hist, exited, landed = oracle_illuminate(orc, lens8[:3], ri, emitter(orc), n, target(orc))
    print("3-lens illumination: segments", np.bincount(seg), "exited", exited, "landed", landed, stats)
    assert (seg == 6).sum() > 100 and landed > 50  # rays cross all three lenses and reach the target
    assert stats["emitted"] == n and stats["exited"] == exited and stats["landed"] == landed
    assert np.array_equal(hist, want_hist)
