"""The Fresnel roulette on the GPU: bzr_trace_chain_ghost against tests/ghost_ref.py (absorb_ref's chain with the draw
in numpy float32 / uint64), bit for bit, on the fused kernel, the staged pipeline and the brute-force scan.

The scenes are test_gpu_absorb.py's: 64^2 - 37 rays (a ragged last wave), four channels mixed in every wave, and the
cemented doublet.  ghost_seed 2024, first_ray 2^40 + 5: a ray number above 2^32 that is no multiple of 64.
"""
import ctypes
import math

import numpy as np
import pytest

import ghost_ref
from bzr_amd.configs import CONFIGS, grid_rays
from ghost_ref import FIRST_RAY, SEED
from test_gpu_opl import assert_opl
from test_gpu_power import bits, flags_of, frozen, set_cap
from test_gpu_tir import NCHAN, PATHS

pytestmark = pytest.mark.gpu

F = np.float32
BUDGETS = {"cfg2": (1, 4, 8), "cfg4": (1, 4), "doublet": (4,)}
CULLED = ("fused", "staged")


def ghost(bzr, ctx, s, path, max_bounces, rays=None, channel=None, fast=False, seed=SEED, first_ray=FIRST_RAY, **kw):
    mode = flags_of(bzr, path) | (bzr.MODE_FAST if fast else 0)
    return bzr.trace_chain_ghost(ctx, s["dms"], s["table"], s["gaps"], s["glass"], s["gapa"],
                                 s["rays"] if rays is None else rays, s["channel"] if channel is None else channel,
                                 max_bounces=max_bounces, ghost_seed=seed, first_ray=first_ray, mode=mode, **kw)


def absorb(bzr, ctx, s, path, max_bounces, fast=False, **kw):
    mode = flags_of(bzr, path) | (bzr.MODE_FAST if fast else 0)
    return bzr.trace_chain_absorb(ctx, s["dms"], s["table"], s["gaps"], s["glass"], s["gapa"], s["rays"], s["channel"],
                                  max_bounces=max_bounces, mode=mode, **kw)


@pytest.fixture(scope="module")
def scenes(bzr, orc, ctx):
    """name -> ghost_ref.scene plus dms and want {max_bounces: the reference with the random rows}: computed once."""
    out = {}
    for name in BUDGETS:
        s = ghost_ref.scene(bzr, name)
        s["dms"] = [bzr.DeviceMesh(ctx, p) for p in s["lenses"]]
        s["want"] = {mb: frozen(*ghost_ref.chain(orc, s["lenses"], s["table"], s["gaps"], s["glass"], s["gapa"], s["rays"],
                                                 s["channel"], s["w_in"], s["p_in"], mb)) for mb in BUDGETS[name]}
        out[name] = s
    return out


# ------------------------------------------------------------------ 1. bit-exact
@pytest.mark.parametrize("name,max_bounces", [(name, mb) for name in BUDGETS for mb in BUDGETS[name]])
@pytest.mark.parametrize("path", PATHS)
def test_bit_exact(bzr, ctx, scenes, name, path, max_bounces):
    s = scenes[name]
    n = s["rays"].shape[1]
    assert n == 4059 and n % 64 != 0
    want = s["want"][max_bounces]
    if name != "doublet":  # the roulette acts: far more reflected rays than total reflection alone gives
        assert int((want[4] > 0).sum()) >= 250
    w, p = s["w_in"].copy(), s["p_in"].copy()  # both passed in place
    got = ghost(bzr, ctx, s, path, max_bounces, weight=w, out_weight=w, opl=p, out_opl=p)
    assert got[1] is w and got[5] is p
    assert_opl(got, want, f"{name} {path} max_bounces {max_bounces}, random rows in place")


# ------------------------------------------------------------------ 2. budget 0
@pytest.mark.parametrize("path,fast", [(p, False) for p in PATHS] + [("fused", True), ("staged", True)])
def test_budget_0_is_trace_chain_absorb(bzr, ctx, scenes, path, fast):
    for name in ("cfg2", "cfg4"):
        s = scenes[name]
        want = tuple(np.asarray(a) for a in absorb(bzr, ctx, s, path, 0, fast, weight=s["w_in"], opl=s["p_in"]))
        assert int((want[2] == bzr.RR_OUTSIDE).sum()) > 1500
        got = ghost(bzr, ctx, s, path, 0, fast=fast, weight=s["w_in"], opl=s["p_in"])
        assert_opl(got, want, f"{name} {path} fast={fast}: budget 0")


# ------------------------------------------------------------------ 3. determinism and the seed
@pytest.mark.parametrize("path", PATHS)
def test_deterministic_and_seeded(bzr, ctx, scenes, path):
    s = scenes["cfg4"]
    a = ghost(bzr, ctx, s, path, 4, weight=s["w_in"], opl=s["p_in"])
    b = ghost(bzr, ctx, s, path, 4, weight=s["w_in"], opl=s["p_in"])
    assert_opl(b, a, f"{path}: the same call again")
    c = ghost(bzr, ctx, s, path, 4, seed=SEED + 1, weight=s["w_in"], opl=s["p_in"])
    assert int((c[4] != a[4]).sum()) >= 50
    d = ghost(bzr, ctx, s, path, 4, first_ray=FIRST_RAY + 1, weight=s["w_in"], opl=s["p_in"])
    assert int((d[4] != a[4]).sum()) >= 50


# ------------------------------------------------------------------ 4. the ray number
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("first", (FIRST_RAY, 2 ** 32 - 500, 2 ** 64 - 2000))
def test_split_identity(bzr, ctx, scenes, path, first):
    """One call over all rays at first_ray = F equals the calls over [0, 1000) at F and [1000, n) at F + 1000: an
    ignored, wave-relative or 32-bit-truncated ray number shows here (1000 is no multiple of 64; the second and third
    F cross 2^32 and 2^64 inside the call)."""
    s = scenes["cfg2"]
    n, cut = s["rays"].shape[1], 1000
    whole = ghost(bzr, ctx, s, path, 4, first_ray=first, weight=s["w_in"], opl=s["p_in"])
    if first == FIRST_RAY:
        assert_opl(whole, s["want"][4], f"{path}: the whole call")
    parts = []
    for lo, hi in ((0, cut), (cut, n)):
        parts.append(ghost(bzr, ctx, s, path, 4, rays=np.ascontiguousarray(s["rays"][:, lo:hi]),
                           channel=s["channel"][lo:hi].copy(), first_ray=first + lo, weight=s["w_in"][lo:hi].copy(),
                           opl=s["p_in"][lo:hi].copy()))
    joined = tuple(np.concatenate([a[k] for a in parts], axis=-1) for k in range(7))
    assert_opl(joined, tuple(np.asarray(a) for a in whole), f"{path}: two calls against one, first_ray {first}")
    assert int((whole[4] > 0).sum()) >= 250


# ------------------------------------------------------------------ 5. chunking and layouts
@pytest.fixture(scope="module")
def cctx(bzr, ctx):
    """This module's own context: the session context never sees a lowered chunk cap."""
    c = bzr.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("path", CULLED)
def test_small_chunks(bzr, cctx, scenes, path):
    """A chunk cap of 1 024 rays: the staged chain runs in four chunks, and the draw still reads the ray's number in
    the call (the chunk offset applies to it as to status, weight and the pending row)."""
    s = scenes["cfg4"]
    dms = [bzr.DeviceMesh(cctx, p) for p in s["lenses"]]
    try:
        assert set_cap(bzr, cctx, 1024) == 1024
        got = bzr.trace_chain_ghost(cctx, dms, s["table"], s["gaps"], s["glass"], s["gapa"], s["rays"], s["channel"],
                                    weight=s["w_in"], opl=s["p_in"], max_bounces=4, ghost_seed=SEED, first_ray=FIRST_RAY,
                                    mode=flags_of(bzr, path))
        assert_opl(got, s["want"][4], f"{path}: chunk cap 1024")
    finally:
        set_cap(bzr, cctx, 0)


def test_device_buffers_and_aos(bzr, ctx, scenes):
    torch = pytest.importorskip("torch")
    s = scenes["cfg4"]
    want = s["want"][4]
    r = torch.from_numpy(np.ascontiguousarray(s["rays"].T)).cuda()
    c = torch.from_numpy(s["channel"].copy()).cuda()
    w = torch.from_numpy(s["w_in"].copy()).cuda()
    p = torch.from_numpy(s["p_in"].copy()).cuda()
    for pipe in (bzr.PIPELINE_FUSED, bzr.PIPELINE_STAGED):
        res = bzr.trace_chain_ghost(ctx, s["dms"], s["table"], s["gaps"], s["glass"], s["gapa"], r, c, weight=w, opl=p,
                                    max_bounces=4, ghost_seed=SEED, first_ray=FIRST_RAY, mode=pipe | bzr.RAYS_AOS)
        torch.cuda.synchronize()
        o, ow, st, g, b, op, gl = (t.cpu().numpy() for t in res)
        got = (np.ascontiguousarray(o.T), ow, st.astype(np.uint32), g.astype(np.uint32), b.astype(np.uint32), op, gl)
        assert_opl(got, want, f"cfg4 device pointers, AoS, pipeline {pipe}")
    got = bzr.trace_chain_ghost(ctx, s["dms"], s["table"], s["gaps"], s["glass"], s["gapa"],
                                np.ascontiguousarray(s["rays"].T), s["channel"], weight=s["w_in"], opl=s["p_in"],
                                max_bounces=4, ghost_seed=SEED, first_ray=FIRST_RAY, mode=bzr.RAYS_AOS)
    assert_opl((np.ascontiguousarray(got[0].T),) + got[1:], want, "cfg4 host pointers, AoS")


# ------------------------------------------------------------------ 6. special rays
@pytest.mark.parametrize("path", PATHS)
def test_channel_out_of_range_and_nan_ray(bzr, ctx, scenes, path):
    """A channel at or above nchan and a non-finite component: NONE, one segment, weight and everything else as it came;
    no word of any other ray changes (its draws are its own)."""
    s = scenes["cfg4"]
    rays, channel, w_in, p_in, want = s["rays"], s["channel"], s["w_in"], s["p_in"], s["want"][4]
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
    got = ghost(bzr, ctx, s, path, 4, rays=poisoned, channel=ch, weight=w_in, opl=p_in)
    bad = [k255, kn, knan, kinf]
    for k in bad:
        assert got[2][k] == bzr.RR_NONE and got[3][k] == 1 and got[4][k] == 0, k
        assert bits(got[5])[k] == bits(p_in)[k] and bits(got[6])[k] == 0, k
        assert bits(got[1])[k] == bits(w_in)[k] and np.array_equal(bits(got[0])[:, k], bits(poisoned)[:, k]), k
    others = np.ones(n, bool)
    others[bad] = False
    assert_opl(tuple(a[..., others] for a in got), tuple(a[..., others] for a in want), f"{path}: the other rays")


# ------------------------------------------------------------------ 7. bad arguments
def test_bad_arguments_leave_the_outputs_untouched(bzr, ctx, scenes):
    s = scenes["cfg2"]
    n = 256
    r, c = np.ascontiguousarray(s["rays"][:, :n]), s["channel"][:n].copy()
    glass2, gapa2, gaps2 = s["glass"], s["gapa"], s["gaps"]

    def sentinels():
        return (np.full((6, n), 7.0, F), np.full(n, 7.0, F), np.full(n, 7, np.uint32), np.full(n, 7, np.uint32),
                np.full(n, 7, np.uint32), np.full(n, 7.0, F), np.full(n, 7.0, F))

    def rejected(match, table, gaps, glass, gapa, mb):
        o, w, st, g, b, p, q = outs = sentinels()
        with pytest.raises(bzr.BzrError, match=match):
            bzr.trace_chain_ghost(ctx, s["dms"], table, gaps, glass, gapa, r, c, weight=s["w_in"][:n].copy(),
                                  max_bounces=mb, ghost_seed=SEED, first_ray=FIRST_RAY, out_rays=o, out_weight=w,
                                  out_status=st, out_segments=g, out_bounces=b, out_opl=p, out_glass=q)
        assert all((a == 7).all() for a in outs)

    for value in (-1e-6, -3.0, np.nan, np.inf):
        for col in (0, NCHAN - 1):  # the first used entry and the last
            t = np.array(glass2, F)
            t[0, col] = value
            rejected("glass_absorb", s["table"], gaps2, t, gapa2, 4)
            rejected("gap_absorb", s["table"], gaps2, glass2, t, 4)
    bad_gaps = np.array(gaps2, F)
    bad_gaps[1, 2] = 0.0
    rejected("gap_table", s["table"], bad_gaps, glass2, gapa2, 4)
    rejected("max_bounces", s["table"], gaps2, glass2, gapa2, bzr.MAX_BOUNCES + 1)
    assert bzr.MAX_BOUNCES + 1 == 9
    rejected("nchan", np.full((1, 65), 1.3, F), np.ones((2, 65), F), np.zeros((1, 65), F), np.zeros((1, 65), F), 4)
    o, w, st, g, b, p, q = outs = sentinels()
    handles = (ctypes.c_void_p * 1)(s["dms"][0].handle)
    tab = np.ascontiguousarray(s["table"], F)

    def raw(lenses, table, nlens, rays, out_rays, out_weight, out_status, out_opl, flags):
        return bzr.lib().bzr_trace_chain_ghost(ctx.handle, lenses, table, None, None, None, nlens, NCHAN, rays,
                                               c.ctypes.data, None, None, n, 4, SEED, FIRST_RAY, out_rays, out_weight,
                                               out_status, g.ctypes.data, b.ctypes.data, out_opl, q.ctypes.data, flags)

    hp, tp = ctypes.cast(handles, ctypes.c_void_p), tab.ctypes.data
    good = dict(lenses=hp, table=tp, nlens=1, rays=r.ctypes.data, out_rays=o.ctypes.data, out_weight=w.ctypes.data,
                out_status=st.ctypes.data, out_opl=p.ctypes.data, flags=0)
    for change, word in ((dict(out_opl=None), b"out_opl"), (dict(out_weight=None), b"out_weight"),
                         (dict(out_status=None), b"null buffer"), (dict(out_rays=None), b"null buffer"),
                         (dict(rays=None), b"null buffer"), (dict(rays=o.ctypes.data), b"alias"),
                         (dict(lenses=None), b"null lens list"), (dict(table=None), b"ri_table"),
                         (dict(nlens=0), b"nlens"), (dict(nlens=9), b"nlens"), (dict(flags=1 << 30), b"flag")):
        assert raw(**{**good, **change}) == 1, change
        assert word in bzr.lib().bzr_last_error(), (change, bzr.lib().bzr_last_error())
        assert all((a == 7).all() for a in outs), change
    assert raw(**good) == 0 and not (st == 7).any()  # and the unchanged call is accepted


# ------------------------------------------------------------------ 8. the rays that never reflect
@pytest.mark.parametrize("path", CULLED)
@pytest.mark.parametrize("fast", (False, True))
def test_row_0_invariant(bzr, ctx, scenes, path, fast):
    """Every ray with ghost out_bounces == 0 has trace_chain_absorb's ray, status, segments, opl and glass bit for bit
    at the same budget -- its draws all came out u < T -- and a weight at or above absorb's: its exits did not pay T."""
    for name, mb in (("cfg2", 4), ("cfg4", 4), ("cfg2", 1)):
        s = scenes[name]
        a = absorb(bzr, ctx, s, path, mb, fast, weight=s["w_in"], opl=s["p_in"])
        g = ghost(bzr, ctx, s, path, mb, fast=fast, weight=s["w_in"], opl=s["p_in"])
        z = g[4] == 0
        assert int(z.sum()) > 3000
        for k in (0, 2, 3, 5, 6):
            assert np.array_equal(bits(g[k][..., z]), bits(a[k][..., z])), (name, k)
        assert (a[4][z] == 0).all()
        assert (a[1][z] <= g[1][z]).all()
        assert int((a[1][z] < g[1][z]).sum()) > 1000


# ------------------------------------------------------------------ 9. unbiased
@pytest.fixture(scope="module")
def big(bzr, ctx, scenes):
    out = {}
    for name in ("cfg2", "cfg4"):
        rays = grid_rays(CONFIGS[name], side=512)
        channel = np.random.default_rng(7).integers(0, NCHAN, rays.shape[1]).astype(np.uint8)
        out[name] = frozen(rays, channel)
    return out


@pytest.mark.parametrize("name", ("cfg2", "cfg4"))
@pytest.mark.parametrize("fast", (False, True))
def test_unbiased(bzr, ctx, scenes, big, name, fast):
    """The roulette keeps the expectation: over the rays that leave with no reflection (Z: bounces 0 and OUTSIDE) the
    ghost weights sum to what trace_chain_absorb's sum to, within 5 standard deviations.  A surviving ray's weight is
    w_g = w_a / p with p the product of its exits' T, so its contribution has variance w_g^2 p (1 - p), estimated over
    the survivors by w_g^2 (1 - w_a / w_g).  No absorption, weight 1, budget 4, fused."""
    s = scenes[name]
    rays, channel = big[name]
    mode = bzr.PIPELINE_FUSED | (bzr.MODE_FAST if fast else 0)
    a = bzr.trace_chain_absorb(ctx, s["dms"], s["table"], s["gaps"], None, None, rays, channel, max_bounces=4, mode=mode)
    g = bzr.trace_chain_ghost(ctx, s["dms"], s["table"], s["gaps"], None, None, rays, channel, max_bounces=4,
                              ghost_seed=SEED, first_ray=FIRST_RAY, mode=mode)
    za = (a[4] == 0) & (a[2] == bzr.RR_OUTSIDE)
    zg = (g[4] == 0) & (g[2] == bzr.RR_OUTSIDE)
    assert not (zg & ~za).any() and int(zg.sum()) > 100_000
    wa, wg = a[1].astype(np.float64), g[1].astype(np.float64)
    s_a, s_g = float(wa[za].sum()), float(wg[zg].sum())
    sigma = math.sqrt(float((wg[zg] ** 2 * (1.0 - wa[zg] / wg[zg])).sum()))
    print(f"{name} fast={fast}: S_g = {s_g:.3f}, S_a = {s_a:.3f}, sigma = {sigma:.3f}, z = {(s_g - s_a) / sigma:+.2f}; "
          f"{int(za.sum())} rays in Z(absorb), {int(zg.sum())} in Z(ghost)")
    assert abs(s_g - s_a) <= 5.0 * sigma
