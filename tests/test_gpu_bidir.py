"""The bidirectional chain on the GPU: bzr_trace_chain_bidir against tests/bidir_ref.py (the header's walk in numpy
float32 / uint64), bit for bit, on the fused kernel and the brute-force scan.

The scenes are ghost_ref.scene's: 64^2 - 37 rays (a ragged last wave), four channels mixed in every wave, and the
cemented doublet; axis (1, 0, 0), ghost_seed 2024, first_ray 2^40 + 5.
"""
import ctypes
import math

import numpy as np
import pytest

import bidir_ref
import ghost_ref
from bidir_ref import AXIS, FIRST_RAY, SEED
from bzr_amd.configs import CONFIGS, grid_rays
from test_gpu_opl import assert_opl
from test_gpu_power import bits, flags_of, frozen
from test_gpu_tir import NCHAN

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ("cfg2", "cfg4", "doublet")
BUDGETS = (1, 4, 8)
PATHS = ("fused", "brute")  # there is no staged form
DENSE = 3                   # the tables' densest channel: 2.4 and 1.62


def bidir(bzr, ctx, s, path, max_bounces, rays=None, channel=None, fast=False, seed=SEED, first_ray=FIRST_RAY, axis=AXIS,
          **kw):
    mode = (flags_of(bzr, path) if path else 0) | (bzr.MODE_FAST if fast else 0)
    return bzr.trace_chain_bidir(ctx, s["dms"], s["table"], s["gaps"], s["glass"], s["gapa"],
                                 s["rays"] if rays is None else rays, s["channel"] if channel is None else channel,
                                 max_bounces=max_bounces, ghost_seed=seed, first_ray=first_ray, axis=axis, mode=mode, **kw)


def absorb(bzr, ctx, s, path, max_bounces, fast=False, **kw):
    mode = flags_of(bzr, path) | (bzr.MODE_FAST if fast else 0)
    return bzr.trace_chain_absorb(ctx, s["dms"], s["table"], s["gaps"], s["glass"], s["gapa"], s["rays"], s["channel"],
                                  max_bounces=max_bounces, mode=mode, **kw)


@pytest.fixture(scope="module")
def scenes(bzr, orc, ctx):
    """name -> ghost_ref.scene plus dms and want {max_bounces: the reference with the random rows}: computed once."""
    out = {}
    for name in NAMES:
        s = ghost_ref.scene(bzr, name)
        s["dms"] = [bzr.DeviceMesh(ctx, p) for p in s["lenses"]]
        s["want"] = {mb: frozen(*bidir_ref.chain(orc, s["lenses"], s["table"], s["gaps"], s["glass"], s["gapa"], s["rays"],
                                                 s["channel"], s["w_in"], s["p_in"], mb)) for mb in BUDGETS}
        out[name] = s
    return out


# ------------------------------------------------------------------ 1. bit-exact
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("max_bounces", BUDGETS)
@pytest.mark.parametrize("path", PATHS)
def test_bit_exact(bzr, ctx, scenes, name, path, max_bounces):
    s = scenes[name]
    n = s["rays"].shape[1]
    assert n == 4059 and n % 64 != 0
    want = s["want"][max_bounces]
    assert int((want[2] == bzr.RR_BACK).sum()) >= 200 and int((want[4] > 0).sum()) >= 250
    w, p = s["w_in"].copy(), s["p_in"].copy()  # both passed in place
    got = bidir(bzr, ctx, s, path, max_bounces, weight=w, out_weight=w, opl=p, out_opl=p)
    assert got[1] is w and got[5] is p
    assert_opl(got, want, f"{name} {path} max_bounces {max_bounces}, random rows in place")


def test_automatic_choice_is_fused(bzr, ctx, scenes):
    """No pipeline flag: the fused kernel, whatever the batch size (a sparse batch would otherwise go staged)."""
    s = scenes["cfg4"]
    for n in (40, 4059):
        got = bidir(bzr, ctx, s, None, 4, rays=np.ascontiguousarray(s["rays"][:, :n]), channel=s["channel"][:n].copy(),
                    weight=s["w_in"][:n].copy(), opl=s["p_in"][:n].copy())
        assert_opl(got, tuple(a[..., :n] for a in s["want"][4]), f"cfg4, no pipeline flag, {n} rays")


# ------------------------------------------------------------------ 2. budget 0   3. FAST mode
@pytest.mark.parametrize("path,fast", [(p, False) for p in PATHS] + [("fused", True)])
def test_budget_0_is_trace_chain_absorb(bzr, ctx, scenes, path, fast):
    """Every traced ray of the three scenes leaves glass through forward-facing surfaces only
    (tests/test_bidir_ref.py checks that on the CPU), so every ray is compared."""
    for name in NAMES:
        s = scenes[name]
        want = tuple(np.asarray(a) for a in absorb(bzr, ctx, s, path, 0, fast, weight=s["w_in"], opl=s["p_in"]))
        assert int((want[2] == bzr.RR_OUTSIDE).sum()) > 1200
        got = bidir(bzr, ctx, s, path, 0, fast=fast, weight=s["w_in"], opl=s["p_in"])
        assert_opl(got, want, f"{name} {path} fast={fast}: budget 0")


@pytest.mark.parametrize("fast", (False, True))
def test_rays_that_never_reflect(bzr, ctx, scenes, fast):
    """As test_gpu_ghost.py's row-0 invariant, in both modes: a ray with out_bounces == 0 has trace_chain_absorb's ray,
    status, segments, opl and glass bit for bit -- all its draws came out u < T -- and a weight at or above absorb's."""
    for name, mb in (("cfg2", 4), ("cfg4", 4), ("cfg2", 1)):
        s = scenes[name]
        a = absorb(bzr, ctx, s, "fused", mb, fast, weight=s["w_in"], opl=s["p_in"])
        g = bidir(bzr, ctx, s, "fused", mb, fast=fast, weight=s["w_in"], opl=s["p_in"])
        z = g[4] == 0
        assert int(z.sum()) > 3000
        for k in (0, 2, 3, 5, 6):
            assert np.array_equal(bits(g[k][..., z]), bits(a[k][..., z])), (name, k)
        assert (a[4][z] == 0).all()
        assert (a[1][z] <= g[1][z]).all()
        assert int((a[1][z] < g[1][z]).sum()) > 1000


# ------------------------------------------------------------------ 4. one wave and its edges
@pytest.fixture(scope="module")
def wave(bzr, orc, scenes):
    """cfg4's grid at the dense channel, budget 8, with the reference's log, and the first window of 64 consecutive
    rays in which, at one event ordinal, one lane is in lens 0 and another in lens 1 (found here, on the CPU)."""
    s = scenes["cfg4"]
    n = s["rays"].shape[1]
    channel = np.full(n, DENSE, np.uint8)
    log = {}
    want = frozen(*bidir_ref.chain(orc, s["lenses"], s["table"], s["gaps"], s["glass"], s["gapa"], s["rays"], channel,
                                   s["w_in"], s["p_in"], 8, log=log))
    depth = max(len(x) for x in log["lenses"])
    at = np.full((n, depth), -1)
    for i, x in enumerate(log["lenses"]):
        at[i, :len(x)] = x
    start = None
    for lo in range(0, n - 129):
        win = at[lo:lo + 64]
        if (((win == 0).any(axis=0)) & ((win == 1).any(axis=0))).any():
            start = lo
            break
    assert start is not None
    return channel, want, start, at


@pytest.mark.parametrize("n", (1, 63, 64, 65, 129))
@pytest.mark.parametrize("path", PATHS)
def test_one_wave_and_its_edges(bzr, ctx, scenes, wave, path, n):
    s = scenes["cfg4"]
    channel, want, start, at = wave
    win = at[start:start + 64]
    mixed = ((win == 0).any(axis=0)) & ((win == 1).any(axis=0))
    assert mixed.any()  # lanes of one wave in lens 0 and in lens 1 at the same event ordinal
    lo, hi = start, start + n
    got = bidir(bzr, ctx, s, path, 8, rays=np.ascontiguousarray(s["rays"][:, lo:hi]), channel=channel[lo:hi].copy(),
                first_ray=FIRST_RAY + lo, weight=s["w_in"][lo:hi].copy(), opl=s["p_in"][lo:hi].copy())
    assert_opl(got, tuple(a[..., lo:hi] for a in want), f"{path}: {n} rays from {start}, ordinals {np.nonzero(mixed)[0]}")


# ------------------------------------------------------------------ 5. split identity
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("cut", (1, 64, 1000))
def test_split_identity(bzr, ctx, scenes, path, cut):
    """One call over all rays at first_ray = F equals the calls over [0, m) at F and [m, n) at F + m, F past 2^40."""
    s = scenes["cfg4"]
    n = s["rays"].shape[1]
    assert FIRST_RAY > 2 ** 40
    whole = bidir(bzr, ctx, s, path, 4, weight=s["w_in"], opl=s["p_in"])
    assert_opl(whole, s["want"][4], f"{path}: the whole call")
    parts = []
    for lo, hi in ((0, cut), (cut, n)):
        parts.append(bidir(bzr, ctx, s, path, 4, rays=np.ascontiguousarray(s["rays"][:, lo:hi]),
                           channel=s["channel"][lo:hi].copy(), first_ray=FIRST_RAY + lo, weight=s["w_in"][lo:hi].copy(),
                           opl=s["p_in"][lo:hi].copy()))
    joined = tuple(np.concatenate([a[k] for a in parts], axis=-1) for k in range(7))
    assert_opl(joined, tuple(np.asarray(a) for a in whole), f"{path}: two calls against one, cut {cut}")
    other = bidir(bzr, ctx, s, path, 4, first_ray=FIRST_RAY + 1, weight=s["w_in"], opl=s["p_in"])
    assert int((other[4] != whole[4]).sum()) >= 50  # the ray number is read


# ------------------------------------------------------------------ 6. weight invariant
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", NAMES)
def test_weight_invariant(bzr, ctx, scenes, path, name):
    s = scenes[name]
    w_in = s["w_in"]
    mode = flags_of(bzr, path)
    got = bzr.trace_chain_bidir(ctx, s["dms"], s["table"], s["gaps"], None, None, s["rays"], s["channel"], weight=w_in,
                                max_bounces=4, ghost_seed=SEED, first_ray=FIRST_RAY, axis=AXIS, mode=mode)
    left = got[4] < 4
    assert int(left.sum()) > 3000 and int((~left).sum()) >= (1 if name == "doublet" else 50)  # (doublet: one such ray)
    assert np.array_equal(bits(got[1][left]), bits(w_in[left]))
    assert (got[1][~left] <= w_in[~left]).all()
    assert set(np.unique(got[2])) <= {0, 2, 4} and int((got[2] == 4).sum()) >= 100
    assert (got[3] <= bidir_ref.segment_bound(len(s["dms"]), 4)).all() and (got[3] >= 1).all()


# ------------------------------------------------------------------ 7. unbiased
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
    """test_gpu_ghost.test_unbiased's construction: over the rays that leave OUTSIDE with no reflection (Z) the weights
    sum to what trace_chain_absorb's sum to, within 5 standard deviations.  A surviving ray's weight is w_g = w_a / p
    with p the product of the T of its surfaces, entries included now, so its contribution has variance
    w_g^2 p (1 - p), estimated over the survivors by w_g^2 (1 - w_a / w_g).  No absorption, weight 1, budget 4, fused."""
    s = scenes[name]
    rays, channel = big[name]
    mode = bzr.PIPELINE_FUSED | (bzr.MODE_FAST if fast else 0)
    a = bzr.trace_chain_absorb(ctx, s["dms"], s["table"], s["gaps"], None, None, rays, channel, max_bounces=4, mode=mode)
    g = bzr.trace_chain_bidir(ctx, s["dms"], s["table"], s["gaps"], None, None, rays, channel, max_bounces=4,
                              ghost_seed=SEED, first_ray=FIRST_RAY, axis=AXIS, mode=mode)
    za = (a[4] == 0) & (a[2] == bzr.RR_OUTSIDE)
    zg = (g[4] == 0) & (g[2] == bzr.RR_OUTSIDE)
    assert not (zg & ~za).any() and int(zg.sum()) > 100_000
    assert (g[1][zg] == 1.0).all()  # budget left: the whole weight from emitter to exit
    wa, wg = a[1].astype(np.float64), g[1].astype(np.float64)
    s_a, s_g = float(wa[za].sum()), float(wg[zg].sum())
    sigma = math.sqrt(float((wg[zg] ** 2 * (1.0 - wa[zg] / wg[zg])).sum()))
    print(f"{name} fast={fast}: S_g = {s_g:.3f}, S_a = {s_a:.3f}, sigma = {sigma:.3f}, z = {(s_g - s_a) / sigma:+.2f}; "
          f"{int(za.sum())} rays in Z(absorb), {int(zg.sum())} in Z(bidir)")
    assert abs(s_g - s_a) <= 5.0 * sigma


# ------------------------------------------------------------------ 8. arguments, buffers, special rays
def test_device_buffers(bzr, ctx, scenes):
    torch = pytest.importorskip("torch")
    s = scenes["cfg4"]
    want = s["want"][4]
    r = torch.from_numpy(np.ascontiguousarray(s["rays"].T)).cuda()
    c = torch.from_numpy(s["channel"].copy()).cuda()
    w = torch.from_numpy(s["w_in"].copy()).cuda()
    p = torch.from_numpy(s["p_in"].copy()).cuda()
    res = bzr.trace_chain_bidir(ctx, s["dms"], s["table"], s["gaps"], s["glass"], s["gapa"], r, c, weight=w, opl=p,
                                max_bounces=4, ghost_seed=SEED, first_ray=FIRST_RAY, axis=AXIS,
                                mode=bzr.PIPELINE_FUSED | bzr.RAYS_AOS)
    torch.cuda.synchronize()
    o, ow, st, g, b, op, gl = (t.cpu().numpy() for t in res)
    got = (np.ascontiguousarray(o.T), ow, st.astype(np.uint32), g.astype(np.uint32), b.astype(np.uint32), op, gl)
    assert_opl(got, want, "cfg4 device pointers, AoS")


@pytest.mark.parametrize("path", PATHS)
def test_channel_out_of_range_and_nan_ray(bzr, ctx, scenes, path):
    """A channel at or above nchan and a non-finite component: NONE, one segment, weight and everything else as it came;
    no word of any other ray changes."""
    s = scenes["cfg4"]
    rays, channel, w_in, p_in, want = s["rays"], s["channel"], s["w_in"], s["p_in"], s["want"][4]
    n = rays.shape[1]
    cand = np.nonzero(want[4] > 0)[0]  # reflected rays, so their waves hold lanes in several places
    assert len(cand) > 100
    mid = len(cand) // 2
    k255, kn, knan, kinf = int(cand[mid - 1]), int(cand[mid]), int(cand[mid + 1]), int(cand[mid + 2])
    ch = channel.copy()
    ch[k255], ch[kn] = 255, NCHAN
    poisoned = rays.copy()
    poisoned[4, knan] = np.nan
    poisoned[0, kinf] = np.inf
    got = bidir(bzr, ctx, s, path, 4, rays=poisoned, channel=ch, weight=w_in, opl=p_in)
    bad = [k255, kn, knan, kinf]
    for k in bad:
        assert got[2][k] == bzr.RR_NONE and got[3][k] == 1 and got[4][k] == 0, k
        assert bits(got[5])[k] == bits(p_in)[k] and bits(got[6])[k] == 0, k
        assert bits(got[1])[k] == bits(w_in)[k] and np.array_equal(bits(got[0])[:, k], bits(poisoned)[:, k]), k
    others = np.ones(n, bool)
    others[bad] = False
    assert_opl(tuple(a[..., others] for a in got), tuple(a[..., others] for a in want), f"{path}: the other rays")


def test_bad_arguments_leave_the_outputs_untouched(bzr, ctx, scenes):
    s = scenes["cfg2"]
    n = 256
    r, c = np.ascontiguousarray(s["rays"][:, :n]), s["channel"][:n].copy()

    def sentinels():
        return (np.full((6, n), 7.0, F), np.full(n, 7.0, F), np.full(n, 7, np.uint32), np.full(n, 7, np.uint32),
                np.full(n, 7, np.uint32), np.full(n, 7.0, F), np.full(n, 7.0, F))

    def rejected(match, mb=4, axis=AXIS, mode=0, glass=s["glass"]):
        o, w, st, g, b, p, q = outs = sentinels()
        with pytest.raises(bzr.BzrError, match=match):
            bzr.trace_chain_bidir(ctx, s["dms"], s["table"], s["gaps"], glass, s["gapa"], r, c,
                                  weight=s["w_in"][:n].copy(), max_bounces=mb, ghost_seed=SEED, first_ray=FIRST_RAY,
                                  axis=axis, out_rays=o, out_weight=w, out_status=st, out_segments=g, out_bounces=b,
                                  out_opl=p, out_glass=q, mode=mode)
        assert all((a == 7).all() for a in outs)

    rejected("axis", axis=(0.0, 0.0, 0.0))
    rejected("axis", axis=(-0.0, 0.0, 0.0))
    rejected("axis", axis=(1.0, np.nan, 0.0))
    rejected("axis", axis=(np.inf, 0.0, 0.0))
    rejected("max_bounces", mb=bzr.MAX_BOUNCES + 1)
    assert bzr.MAX_BOUNCES + 1 == 9
    rejected("staged", mode=bzr.PIPELINE_STAGED)
    bad = np.array(s["glass"], F)
    bad[0, 0] = -1.0
    rejected("glass_absorb", glass=bad)
    o, w, st, g, b, p, q = outs = sentinels()
    handles = (ctypes.c_void_p * 1)(s["dms"][0].handle)
    tab = np.ascontiguousarray(s["table"], F)
    ax = np.array(AXIS, F)

    def raw(lenses, table, nlens, rays, out_rays, out_weight, out_status, out_opl, flags, axis):
        return bzr.lib().bzr_trace_chain_bidir(ctx.handle, lenses, table, None, None, None, nlens, NCHAN, rays,
                                               c.ctypes.data, None, None, n, 4, SEED, FIRST_RAY, axis, out_rays, out_weight,
                                               out_status, g.ctypes.data, b.ctypes.data, out_opl, q.ctypes.data, flags)

    hp, tp = ctypes.cast(handles, ctypes.c_void_p), tab.ctypes.data
    good = dict(lenses=hp, table=tp, nlens=1, rays=r.ctypes.data, out_rays=o.ctypes.data, out_weight=w.ctypes.data,
                out_status=st.ctypes.data, out_opl=p.ctypes.data, flags=0, axis=ax.ctypes.data)
    for change, word in ((dict(out_opl=None), b"out_opl"), (dict(out_weight=None), b"out_weight"),
                         (dict(out_status=None), b"null buffer"), (dict(out_rays=None), b"null buffer"),
                         (dict(rays=None), b"null buffer"), (dict(rays=o.ctypes.data), b"alias"),
                         (dict(lenses=None), b"null lens list"), (dict(table=None), b"ri_table"),
                         (dict(nlens=0), b"nlens"), (dict(nlens=9), b"nlens"), (dict(flags=1 << 30), b"flag"),
                         (dict(axis=None), b"axis"), (dict(flags=bzr.PIPELINE_STAGED), b"staged")):
        assert raw(**{**good, **change}) == 1, change
        assert word in bzr.lib().bzr_last_error(), (change, bzr.lib().bzr_last_error())
        assert all((a == 7).all() for a in outs), change
    assert raw(**good) == 0 and not (st == 7).any()  # and the unchanged call is accepted
