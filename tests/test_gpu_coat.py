"""The coated chain on the GPU: bzr_trace_chain_coated against tests/coat_ref.py (the header's walk with the coating in
numpy float32 / uint64), bit for bit, on the fused kernel and the brute-force scan.

The scenes are ghost_ref.scene's: 64^2 - 37 rays (a ragged last wave), four channels mixed in every wave, and the
cemented doublet; axis (1, 0, 0), ghost_seed 2024, first_ray 2^40 + 5.  The rows are quarter-wave MgF2 per channel,
built by coating_reflectance (coat_ref.mgf2_rows).  Coatings: "mixed" (front of lens 0 and back of the last lens),
"all" (every surface; on cfg2 its back face a mirror) and, on cfg2 alone, "front" -- the one-lens scene's only way to
a lens with a coated and a bare face (tests/test_coat_ref.py establishes the draws each of them gives).
"""
import ctypes

import numpy as np
import pytest

import coat_ref
import ghost_ref
from bidir_ref import AXIS, FIRST_RAY, SEED
from test_gpu_opl import assert_opl
from test_gpu_power import bits, flags_of, frozen
from test_gpu_tir import NCHAN

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ("cfg2", "cfg4", "doublet")
BUDGETS = (1, 4, 8)
PATHS = ("fused", "brute")
CASES = [(name, kind) for name in NAMES for kind in ("mixed", "all")] + [("cfg2", "front")]


def coated(bzr, ctx, s, path, max_bounces, coat, rays=None, channel=None, fast=False, first_ray=FIRST_RAY, **kw):
    mode = (flags_of(bzr, path) if path else 0) | (bzr.MODE_FAST if fast else 0)
    c = None if coat is None else coat if isinstance(coat, bzr.Coating) else bzr.Coating(coat[0], coat[1])
    return bzr.trace_chain_coated(ctx, s["dms"], s["table"], s["gaps"], s["glass"], s["gapa"],
                                  s["rays"] if rays is None else rays, s["channel"] if channel is None else channel,
                                  max_bounces=max_bounces, ghost_seed=SEED, first_ray=first_ray, axis=AXIS, coat=c,
                                  mode=mode, **kw)


def bidir(bzr, ctx, s, path, max_bounces, fast=False, **kw):
    mode = flags_of(bzr, path) | (bzr.MODE_FAST if fast else 0)
    return bzr.trace_chain_bidir(ctx, s["dms"], s["table"], s["gaps"], s["glass"], s["gapa"], s["rays"], s["channel"],
                                 max_bounces=max_bounces, ghost_seed=SEED, first_ray=FIRST_RAY, axis=AXIS, mode=mode, **kw)


def reference(orc, s, coat, max_bounces, channel=None, log=None):
    return frozen(*coat_ref.chain(orc, s["lenses"], s["table"], s["gaps"], s["glass"], s["gapa"], s["rays"],
                                  s["channel"] if channel is None else channel, s["w_in"], s["p_in"], max_bounces,
                                  coat=coat, log=log))


@pytest.fixture(scope="module")
def scenes(bzr, orc, ctx):
    """name -> ghost_ref.scene plus dms, coat {kind: (rows, mask)} and want {(kind, max_bounces): the reference with the
    random rows}: computed once."""
    out = {}
    for name in NAMES:
        s = ghost_ref.scene(bzr, name)
        s["dms"] = [bzr.DeviceMesh(ctx, p) for p in s["lenses"]]
        s["coat"] = {"mixed": coat_ref.mixed(bzr, s),
                     "all": coat_ref.all_coated(bzr, s, mirror=1 if name == "cfg2" else None)}
        if name == "cfg2":
            s["coat"]["front"] = (s["coat"]["mixed"][0], 1)
        s["want"] = {(kind, mb): reference(orc, s, coat, mb) for kind, coat in s["coat"].items() for mb in BUDGETS}
        out[name] = s
    return out


# ------------------------------------------------------------------ 1. bit-exact
@pytest.mark.parametrize("name,kind", CASES)
@pytest.mark.parametrize("max_bounces", BUDGETS)
@pytest.mark.parametrize("path", PATHS)
def test_bit_exact(bzr, ctx, scenes, name, kind, path, max_bounces):
    s = scenes[name]
    n = s["rays"].shape[1]
    assert n == 4059 and n % 64 != 0
    want = s["want"][(kind, max_bounces)]
    assert int((want[4] > 0).sum()) >= 50  # (the fewest: the doublet's mixed coating, 73 rays; the draws: test_coat_ref.py)
    w, p = s["w_in"].copy(), s["p_in"].copy()  # both passed in place
    got = coated(bzr, ctx, s, path, max_bounces, s["coat"][kind], weight=w, out_weight=w, opl=p, out_opl=p)
    assert got[1] is w and got[5] is p
    assert_opl(got, want, f"{name} {kind} {path} max_bounces {max_bounces}, random rows in place")


def test_the_mirror_sends_cfg2_back(bzr, ctx, scenes):
    s = scenes["cfg2"]
    got = coated(bzr, ctx, s, "fused", 1, s["coat"]["all"], weight=s["w_in"], opl=s["p_in"])
    outside = got[2] == bzr.RR_OUTSIDE
    assert (bits(got[1])[outside] == 0).all()
    assert int(((got[2] == bzr.RR_BACK) & (got[4] == 1)).sum()) >= 1000


# ------------------------------------------------------------------ 2. mask 0   3. FAST mode
@pytest.mark.parametrize("path,fast", [(p, False) for p in PATHS] + [("fused", True)])
@pytest.mark.parametrize("max_bounces", (0, 4))
def test_mask_0_is_trace_chain_bidir(bzr, ctx, scenes, path, fast, max_bounces):
    for name in NAMES:
        s = scenes[name]
        want = tuple(np.asarray(a) for a in bidir(bzr, ctx, s, path, max_bounces, fast, weight=s["w_in"], opl=s["p_in"]))
        assert int((want[2] == bzr.RR_OUTSIDE).sum()) > 1200
        rows = s["coat"]["all"][0]
        for coat in (None, bzr.Coating(None, 0), bzr.Coating(rows, 0)):
            got = coated(bzr, ctx, s, path, max_bounces, coat, fast=fast, weight=s["w_in"], opl=s["p_in"])
            assert_opl(got, want, f"{name} {path} fast={fast} budget {max_bounces}: no surface coated")


def test_fast_rays_that_never_reflect(bzr, ctx, scenes):
    """test_gpu_bidir.py's test_rays_that_never_reflect under FAST with a coating: a ray with out_bounces == 0 has FAST
    trace_chain_absorb's ray, status, segments, opl and glass bit for bit -- the coating moved no ray that drew u < T --
    and a weight at or above absorb's.  The lookup is exact in both modes: on the rays whose FAST geometry is the parity
    geometry bit for bit (at least 1 000 of them), the FAST weight is the parity weight: their draws and budget-spent
    factors read the parity T."""
    for name, mb in (("cfg2", 4), ("cfg4", 4), ("cfg2", 1)):
        s = scenes[name]
        mode = bzr.PIPELINE_FUSED | bzr.MODE_FAST
        a = bzr.trace_chain_absorb(ctx, s["dms"], s["table"], s["gaps"], s["glass"], s["gapa"], s["rays"], s["channel"],
                                   weight=s["w_in"], opl=s["p_in"], max_bounces=mb, mode=mode)
        g = coated(bzr, ctx, s, "fused", mb, s["coat"]["mixed"], fast=True, weight=s["w_in"], opl=s["p_in"])
        z = g[4] == 0
        assert int(z.sum()) > 3000
        for k in (0, 2, 3, 5, 6):
            assert np.array_equal(bits(g[k][..., z]), bits(a[k][..., z])), (name, k)
        assert (a[4][z] == 0).all() and (a[1][z] <= g[1][z]).all()
        want = s["want"][("mixed", mb)]
        same = z & (want[4] == 0) & (bits(g[0]) == bits(want[0])).all(axis=0) & (bits(g[5]) == bits(want[5]))
        print(f"{name} budget {mb}: {int(same.sum())} never-reflected rays with the parity geometry under FAST")
        assert int(same.sum()) >= 1000  # (1 271 in each of the three: rays FAST's Newton stage leaves bit-identical)
        assert np.array_equal(bits(g[1][same]), bits(want[1][same]))


# ------------------------------------------------------------------ 4. one wave and its edges
@pytest.fixture(scope="module")
def wave(orc, scenes):
    """cfg4 with the mixed coating at budget 8, the reference's log, and the first window of 64 consecutive rays in
    which, at one segment ordinal and in one (lens, phase), one lane draws at a coated surface and another at an
    uncoated one (found here, on the CPU)."""
    s = scenes["cfg4"]
    n = s["rays"].shape[1]
    log = {}
    want = reference(orc, s, s["coat"]["mixed"], 8, log=log)
    seen = {}  # (ordinal, lens, phase) -> per ray: 1 coated, 2 uncoated
    for i, ds in enumerate(log["draws"]):
        for e, sf, is_coated, _, _, gl in ds:
            seen.setdefault((e, sf >> 1, gl), np.zeros(n, np.uint8))[i] |= 1 if is_coated else 2
    start = found = None
    for lo in range(0, n - 129):
        for key, row in seen.items():
            win = row[lo:lo + 64]
            if (win & 1).any() and (win & 2).any():
                start, found = lo, key
                break
        if start is not None:
            break
    assert start is not None
    return want, start, found


@pytest.mark.parametrize("n", (1, 63, 64, 65, 129))
@pytest.mark.parametrize("path", PATHS)
def test_one_wave_and_its_edges(bzr, ctx, scenes, wave, path, n):
    s = scenes["cfg4"]
    want, start, found = wave
    lo, hi = start, start + n
    got = coated(bzr, ctx, s, path, 8, s["coat"]["mixed"], rays=np.ascontiguousarray(s["rays"][:, lo:hi]),
                 channel=s["channel"][lo:hi].copy(), first_ray=FIRST_RAY + lo, weight=s["w_in"][lo:hi].copy(),
                 opl=s["p_in"][lo:hi].copy())
    assert_opl(got, tuple(a[..., lo:hi] for a in want), f"{path}: {n} rays from {start}, (ordinal, lens, glass) {found}")


# ------------------------------------------------------------------ 5. split identity
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("cut", (1, 64, 1000))
def test_split_identity(bzr, ctx, scenes, path, cut):
    s = scenes["cfg4"]
    n = s["rays"].shape[1]
    coat = s["coat"]["mixed"]
    whole = coated(bzr, ctx, s, path, 4, coat, weight=s["w_in"], opl=s["p_in"])
    assert_opl(whole, s["want"][("mixed", 4)], f"{path}: the whole call")
    parts = []
    for lo, hi in ((0, cut), (cut, n)):
        parts.append(coated(bzr, ctx, s, path, 4, coat, rays=np.ascontiguousarray(s["rays"][:, lo:hi]),
                            channel=s["channel"][lo:hi].copy(), first_ray=FIRST_RAY + lo, weight=s["w_in"][lo:hi].copy(),
                            opl=s["p_in"][lo:hi].copy()))
    joined = tuple(np.concatenate([a[k] for a in parts], axis=-1) for k in range(7))
    assert_opl(joined, tuple(np.asarray(a) for a in whole), f"{path}: two calls against one, cut {cut}")


# ------------------------------------------------------------------ 6. buffers, special rays, tables
def test_device_buffers(bzr, ctx, scenes):
    torch = pytest.importorskip("torch")
    s = scenes["cfg4"]
    want = s["want"][("mixed", 4)]
    r = torch.from_numpy(np.ascontiguousarray(s["rays"].T)).cuda()
    c = torch.from_numpy(s["channel"].copy()).cuda()
    w = torch.from_numpy(s["w_in"].copy()).cuda()
    p = torch.from_numpy(s["p_in"].copy()).cuda()
    res = bzr.trace_chain_coated(ctx, s["dms"], s["table"], s["gaps"], s["glass"], s["gapa"], r, c, weight=w, opl=p,
                                 max_bounces=4, ghost_seed=SEED, first_ray=FIRST_RAY, axis=AXIS,
                                 coat=bzr.Coating(*s["coat"]["mixed"]), mode=bzr.PIPELINE_FUSED | bzr.RAYS_AOS)
    torch.cuda.synchronize()
    o, ow, st, g, b, op, gl = (t.cpu().numpy() for t in res)
    got = (np.ascontiguousarray(o.T), ow, st.astype(np.uint32), g.astype(np.uint32), b.astype(np.uint32), op, gl)
    assert_opl(got, want, "cfg4 mixed, device pointers, AoS")


@pytest.mark.parametrize("path", PATHS)
def test_channel_out_of_range_and_nan_ray(bzr, ctx, scenes, path):
    """A channel at or above nchan and a non-finite component: NONE, one segment, weight and everything else as it came;
    no word of any other ray changes."""
    s = scenes["cfg4"]
    rays, channel, w_in, p_in, want = s["rays"], s["channel"], s["w_in"], s["p_in"], s["want"][("mixed", 4)]
    n = rays.shape[1]
    cand = np.nonzero(want[4] > 0)[0]
    assert len(cand) > 100
    mid = len(cand) // 2
    k255, kn, knan, kinf = int(cand[mid - 1]), int(cand[mid]), int(cand[mid + 1]), int(cand[mid + 2])
    ch = channel.copy()
    ch[k255], ch[kn] = 255, NCHAN
    poisoned = rays.copy()
    poisoned[4, knan] = np.nan
    poisoned[0, kinf] = np.inf
    got = coated(bzr, ctx, s, path, 4, s["coat"]["mixed"], rays=poisoned, channel=ch, weight=w_in, opl=p_in)
    bad = [k255, kn, knan, kinf]
    for k in bad:
        assert got[2][k] == bzr.RR_NONE and got[3][k] == 1 and got[4][k] == 0, k
        assert bits(got[5])[k] == bits(p_in)[k] and bits(got[6])[k] == 0, k
        assert bits(got[1])[k] == bits(w_in)[k] and np.array_equal(bits(got[0])[:, k], bits(poisoned)[:, k]), k
    others = np.ones(n, bool)
    others[bad] = False
    assert_opl(tuple(a[..., others] for a in got), tuple(a[..., others] for a in want), f"{path}: the other rays")


@pytest.mark.parametrize("path", PATHS)
def test_unmasked_rows_are_not_read(bzr, ctx, scenes, path):
    s = scenes["cfg4"]
    rows, mask = s["coat"]["mixed"]
    poisoned = rows.copy()
    for sf in range(rows.shape[0]):
        if not (mask >> sf) & 1:
            poisoned[sf] = np.nan
    assert np.isnan(poisoned).any()
    got = coated(bzr, ctx, s, path, 4, (poisoned, mask), weight=s["w_in"], opl=s["p_in"])
    assert_opl(got, s["want"][("mixed", 4)], f"{path}: NaN in the unmasked rows")


@pytest.mark.parametrize("path", PATHS)
def test_masked_rows_follow_the_mask_on_one_context(bzr, orc, scenes, path):
    """The device copy of the table is rewritten when the mask changes, not only when a masked row's values do.  On a
    context of its own, cfg2: mask 3 with a mirror on the back (so the device holds a row of ones there), mask 1 with the
    same front row, then mask 3 again with the back row all zeros -- a legal row, a perfect AR coating, whose values equal
    what an image with zeros for unmasked rows would hold.  Each call against coat_ref; the last must see the zeros."""
    s = dict(scenes["cfg2"])
    own = bzr.Context(0)
    s["dms"] = [bzr.DeviceMesh(own, p) for p in s["lenses"]]
    rows = s["coat"]["mixed"][0]
    ones, zeros = rows.copy(), rows.copy()
    ones[1], zeros[1] = F(1), F(0)
    want_mirror = reference(orc, s, (ones, 3), 4)
    want_zero = reference(orc, s, (zeros, 3), 4)
    assert int((want_mirror[4] != want_zero[4]).sum()) > 1000  # the two back rows give other walks
    for coat, want, label in (((ones, 3), want_mirror, "mask 3, back a mirror"),
                              ((rows, 1), s["want"][("front", 4)], "mask 1"),
                              ((zeros, 3), want_zero, "mask 3, back all zeros"),
                              ((rows, 1), s["want"][("front", 4)], "mask 1 again"),
                              ((ones, 3), want_mirror, "mask 3, back a mirror again")):
        got = coated(bzr, own, s, path, 4, coat, weight=s["w_in"], opl=s["p_in"])
        assert_opl(got, want, f"cfg2 {path}: {label}")


def test_bad_arguments_leave_the_outputs_untouched(bzr, ctx, scenes):
    s = scenes["cfg2"]
    n = 256
    r, c = np.ascontiguousarray(s["rays"][:, :n]), s["channel"][:n].copy()
    rows = s["coat"]["mixed"][0]

    def sentinels():
        return (np.full((6, n), 7.0, F), np.full(n, 7.0, F), np.full(n, 7, np.uint32), np.full(n, 7, np.uint32),
                np.full(n, 7, np.uint32), np.full(n, 7.0, F), np.full(n, 7.0, F))

    def rejected(match, coat, mode=0):
        o, w, st, g, b, p, q = outs = sentinels()
        with pytest.raises(bzr.BzrError, match=match):
            bzr.trace_chain_coated(ctx, s["dms"], s["table"], s["gaps"], s["glass"], s["gapa"], r, c,
                                   weight=s["w_in"][:n].copy(), max_bounces=4, ghost_seed=SEED, first_ray=FIRST_RAY,
                                   axis=AXIS, coat=coat, out_rays=o, out_weight=w, out_status=st, out_segments=g,
                                   out_bounces=b, out_opl=p, out_glass=q, mode=mode)
        assert all((a == 7).all() for a in outs)

    rejected("mask", bzr.Coating(rows, 4))             # one lens: bits 0 and 1 alone
    rejected("mask", bzr.Coating(rows, 1 << 31))
    rejected("table", bzr.Coating(None, 1))
    for value in (np.nan, np.inf, -np.inf, -1e-6, 1.0 + 2.0 ** -23):
        bad = rows.copy()
        bad[1, NCHAN - 1, 128] = value
        rejected(r"\[0, 1\]", bzr.Coating(bad, 2))
        rejected(r"\[0, 1\]", bzr.Coating(bad, 3))
    rejected("staged", bzr.Coating(rows, 3), mode=bzr.PIPELINE_STAGED)
    rejected("staged", None, mode=bzr.PIPELINE_STAGED)
    # and the unchanged call is accepted: the bad entry's row is unmasked
    outs = sentinels()
    bzr.trace_chain_coated(ctx, s["dms"], s["table"], s["gaps"], s["glass"], s["gapa"], r, c, max_bounces=4,
                           ghost_seed=SEED, first_ray=FIRST_RAY, axis=AXIS, coat=bzr.Coating(bad, 1), out_rays=outs[0],
                           out_weight=outs[1], out_status=outs[2], out_segments=outs[3], out_bounces=outs[4],
                           out_opl=outs[5], out_glass=outs[6])
    assert not (outs[2] == 7).any()
    # the raw call with a null coating pointer is the uncoated chain
    coat = ctypes.c_void_p(None)
    handles = (ctypes.c_void_p * 1)(s["dms"][0].handle)
    tab, ax = np.ascontiguousarray(s["table"], F), np.array(AXIS, F)
    o, w, st, g, b, p, q = sentinels()
    assert bzr.lib().bzr_trace_chain_coated(ctx.handle, ctypes.cast(handles, ctypes.c_void_p), tab.ctypes.data, None, None,
                                            None, 1, NCHAN, r.ctypes.data, c.ctypes.data, None, None, n, 4, SEED, FIRST_RAY,
                                            ax.ctypes.data, coat, o.ctypes.data, w.ctypes.data, st.ctypes.data,
                                            g.ctypes.data, b.ctypes.data, p.ctypes.data, q.ctypes.data, 0) == 0
    assert not (st == 7).any()
