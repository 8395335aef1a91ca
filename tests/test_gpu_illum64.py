"""The illumination path's two ends on the GPU against tests/illum64.py, the binary64 restatement of include/bzr.h's
text: bzr_emit's rays, and every illumination entry point as land(chain(emit)) with the landing step in binary64.

The older illumination tests compare with the oracle's orc.emit / orc.land, a statement-for-statement copy of the device
code, in one geometry (a yz emitter of 2 x 2 parts, a square target normal to +x).  Here the emitter lies on no
coordinate plane and has 3 x 5 parts of 77 rays, the ray numbers pass 2^32, and the targets are not square, tilted, and
come with their u / v swapped twins.  The chain in the middle is the device's own bzr_trace_chain* over every emitted
ray (uncut), which tests of its own cover.

Measured on an MI355X, 30 000 rays a case, both pipelines alike (the tests print these figures; none is a bar):
  bzr_emit against emit64, the maxima over 2 emitters x 3 belts x 3 firsts
    direction      7.6e-7 per component (bar 2e-6)
    origin         0.195 of its bar: 5.1e-7 absolute at x = 6, 3.8e-6 at x = -40
    | |d| - 1 |    1.05e-7 (bar 2.4e-7)
    patch numbers  equal for every ray; patch_near covers at most 0.013 % of the rays (bar 0.2 %)
  K = 32 (illum64.K_MARGIN, as pinned on the oracle by tests/test_illum64.py; not raised)
  landing, per case: exited / landed, unsure rays (share of the exited), sum(hi - lo) (share of the landed count)
    illuminate, illuminate_power   plain, plain_swapped    5233 / 4851   7 (0.134 %)   14 (0.289 %)
                                   coarse, coarse_swapped  5233 / 4851   3 (0.057 %)    6 (0.124 %)
                                   tilted, tilted_swapped  5233 / 5002   5 (0.096 %)   10 (0.200 %)
                                   behind                  5233 / 0      0              0
    illuminate_spectral  tilted    5054 / 4941   7 (0.139 %)   14 (0.283 %)
    illuminate_tir       tilted    5130 / 4837   2 (0.039 %)    4 (0.083 %)   499 rays reflect
    illuminate_media     tilted    4790 / 4131   3 (0.063 %)    5 (0.121 %)   568 rays reflect
    far emitter          tilted    50 / 50 (tir: 42)   0   0   29 559 rays culled, none borderline
"""
import ctypes

import numpy as np
import pytest

import illum64
from absorb_ref import ILLUM_GAPA, ILLUM_GAPS, ILLUM_GLASS
from illum64 import BELTS, FIRSTS, N_RAYS
from illum_tir_ref import EXITED, LANDED, LOST, ROWS, lenses_of
from test_gpu_tir import ROW1

pytestmark = pytest.mark.gpu

F = np.float32
N = N_RAYS
KINDS = ("plain", "power", "spectral", "tir", "media")   # bzr_illuminate, _power, _spectral, _tir, _media
NCHAN = {"plain": 1, "power": 1, "spectral": 3, "tir": 4, "media": 4}
BUDGET = 4
RI = 1.3
KEYS = ("emitted", "culled", "exited", "landed")


@pytest.fixture(scope="module")
def dms(bzr, ctx):
    return [bzr.DeviceMesh(ctx, p) for p in lenses_of(bzr, "cfg2")]


# ------------------------------------------------------------------ (a) bzr_emit against emit64
@pytest.mark.parametrize("x", (illum64.OBLIQUE_X, illum64.FAR_X))
@pytest.mark.parametrize("belts", BELTS)
@pytest.mark.parametrize("first", FIRSTS)
def test_emit_is_emit64(bzr, ctx, x, belts, first):
    em = illum64.emitter(bzr, x, belts)
    rays, patch = bzr.emit(ctx, em, first, N)
    m = illum64.check_emit(em, first, rays, patch)
    print(f"emit x {x} belts {belts} first {first}: {m}")
    # any range is independent of the others: the same ray numbers from a wider call, bit for bit
    back = 37 if first else 0
    wide, wide_patch = bzr.emit(ctx, em, first - back, N + 100)
    assert np.array_equal(wide[:, back:back + N].view(np.uint32), rays.view(np.uint32))
    assert np.array_equal(wide_patch[back:back + N], patch)


def test_emit_device_buffers_past_2_32(bzr, ctx):
    torch = pytest.importorskip("torch")
    em = illum64.emitter(bzr, belts=33)
    first = FIRSTS[2]
    r = torch.empty((6, N), dtype=torch.float32, device="cuda")
    p = torch.empty(N, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.use_torch_stream()
    try:
        bzr.emit(ctx, em, first, N, rays=r, patch=p)
        torch.cuda.synchronize()
    finally:
        ctx.use_own_stream()
    hr, hp = bzr.emit(ctx, em, first, N)
    assert np.array_equal(r.cpu().numpy().view(np.uint32), hr.view(np.uint32))
    assert np.array_equal(p.cpu().numpy().astype(np.uint32), hp)
    illum64.check_emit(em, first, r.cpu().numpy(), p.cpu().numpy())


# ------------------------------------------------------------------ the entry points, one shape of result
def illuminate(bzr, ctx, dms, kind, em, tg, pipe, n=N):
    """The entry point `kind` -> dict of hist, flux, rhist, rflux ([nchan, bins_v, bins_u] or None), stats and power
    (lists of nchan dicts, or None), ledger ({"count", "power"} or None)."""
    none = dict.fromkeys(("flux", "rhist", "rflux", "power", "ledger"))
    if kind == "plain":
        hist, stats = bzr.illuminate(ctx, dms, [RI], em, n, tg, mode=pipe)
        return {**none, "hist": hist[None], "stats": [stats]}
    if kind == "power":
        flux, hist, stats, power = bzr.illuminate_power(ctx, dms, [RI], em, n, tg, mode=pipe)
        return {**none, "hist": hist[None], "flux": flux[None], "stats": [stats], "power": [power]}
    if kind == "spectral":
        flux, hist, stats, power = bzr.illuminate_spectral(ctx, dms, [ROW1[:3]], em, n, tg, mode=pipe)
        return {**none, "hist": hist, "flux": flux, "stats": stats, "power": power}
    if kind == "tir":
        got = bzr.illuminate_tir(ctx, dms, [ROW1], em, n, tg, max_bounces=BUDGET, mode=pipe)
    else:
        got = bzr.illuminate_media(ctx, dms, [ROW1], ILLUM_GAPS, ILLUM_GLASS, ILLUM_GAPA, em, n, tg, max_bounces=BUDGET,
                                   mode=pipe)
    flux, hist, rflux, rhist, stats, power, ledger = got
    return {"hist": hist, "flux": flux, "rhist": rhist, "rflux": rflux, "stats": stats, "power": power, "ledger": ledger}


def chain_rows(bzr, ctx, dms, kind, em, pipe, n=N):
    """bzr.emit's rays through the matching bzr.trace_chain*, every ray, uncut: ray number i in channel i mod nchan,
    weight-in d.x (the entry points' default Lambert emission) or 1."""
    rays, _ = bzr.emit(ctx, em, 0, n)
    nchan = NCHAN[kind]
    channel = (np.arange(n) % nchan).astype(np.uint8)
    w0 = np.ones(n, F) if kind == "plain" else rays[3].copy()
    bounces = np.zeros(n, np.uint32)
    if kind == "plain":
        out, status, seg = bzr.trace_chain(ctx, dms, [RI], rays, mode=pipe)
        w = w0
    elif kind == "power":
        out, w, status, seg = bzr.trace_chain_power(ctx, dms, [RI], rays, weight=w0, mode=pipe)
    elif kind == "spectral":
        out, w, status, seg = bzr.trace_chain_spectral(ctx, dms, [ROW1[:3]], rays, channel, weight=w0, mode=pipe)
    elif kind == "tir":
        out, w, status, seg, bounces = bzr.trace_chain_tir(ctx, dms, [ROW1], rays, channel, w0, max_bounces=BUDGET,
                                                          mode=pipe)
    else:
        out, w, status, seg, bounces = bzr.trace_chain_absorb(ctx, dms, [ROW1], ILLUM_GAPS, ILLUM_GLASS, ILLUM_GAPA, rays,
                                                             channel, w0, max_bounces=BUDGET, mode=pipe)[:5]
    assert set(np.unique(status)) <= {0, 2}
    return illum64.SimpleNamespace(rays=rays, out=out, w=w, w0=w0, status=status, seg=seg, bounces=bounces,
                                   channel=channel.astype(np.int64), nchan=nchan)


@pytest.fixture(scope="module")
def rows_of(bzr, ctx, dms):
    """chain_rows per (kind, emitter x, pipeline), each computed once and shared by the targets."""
    cache = {}

    def get(kind, x, pipe):
        if (kind, x, pipe) not in cache:
            cache[kind, x, pipe] = chain_rows(bzr, ctx, dms, kind, illum64.emitter(bzr, x), pipe)
        return cache[kind, x, pipe]

    return get


def sphere_cull(sphere, rays):
    """The binary64 sphere test of include/bzr.h's bzr_illuminate -> (culled [n], borderline [n]): borderline where
    |cc| or the discriminant is within 1e-9 relative of zero, either side is then acceptable."""
    c = sphere.astype(np.float64)
    oc = rays[:3].astype(np.float64) - c[:3, None]
    r2 = c[3] ** 2
    oo = (oc * oc).sum(0)
    cc = oo - r2
    b = (oc * rays[3:].astype(np.float64)).sum(0)
    disc = b * b - cc
    culled = (cc > 0) & ((b >= 0) | (disc < 0))
    borderline = (np.abs(cc) <= 1e-9 * (oo + r2)) | ((cc > 0) & (b < 0) & (np.abs(disc) <= 1e-9 * (b * b + np.abs(cc))))
    return culled, borderline


def check_case(bzr, dm0, kind, r, tg, got, label, want_landed=1000):
    """Every output of one illumination call against the rows of the uncut chain."""
    nchan, ch = r.nchan, r.channel
    outside, none = r.status == 2, r.status == 0
    q, q0 = illum64.q32(r.w), illum64.q32(r.w0)
    row = np.minimum(r.bounces, ROWS - 1).astype(np.int64)
    # the cull: every ray the sphere drops ends NONE after one segment without a bounce in the uncut chain
    culled, borderline = sphere_cull(bzr.bounding_sphere(dm0), r.rays)
    assert (none & (r.seg == 1) & (r.bounces == 0))[culled & ~borderline].all(), label
    # ---- exact, all integers
    for c in range(nchan):
        mine = ch == c
        st = got["stats"][c]
        assert st["emitted"] == int(mine.sum()), (label, c)
        assert st["exited"] == int((mine & outside).sum()), (label, c)
        sure = int((mine & culled & ~borderline).sum())
        assert sure <= st["culled"] <= sure + int((mine & borderline).sum()), (label, c)
        exact_cull = not (mine & borderline).any()
        if got["power"] is not None:
            pw = got["power"][c]
            assert pw["emitted"] == int(q0[mine].sum()), (label, c)
            assert pw["exited"] == int(q[mine & outside].sum()), (label, c)
            if exact_cull:
                assert pw["culled"] == int(q0[mine & culled].sum()), (label, c)
        if got["ledger"] is not None:
            cnt, pwr = got["ledger"]["count"][c], got["ledger"]["power"][c]
            for k in range(ROWS):
                at = mine & (row == k)
                assert int(cnt[k, EXITED]) == int((at & outside).sum()), (label, c, k)
                assert int(pwr[k, EXITED]) == int(q[at & outside].sum()), (label, c, k)
                # culled rays are in no row: they would have been row 0's (a culled ray keeps its weight w0)
                assert int(cnt[k, LOST]) == int((at & none).sum()) - (st["culled"] if k == 0 else 0), (label, c, k)
                assert int(pwr[k, LOST]) == int(q[at & none].sum()) - (got["power"][c]["culled"] if k == 0 else 0), \
                    (label, c, k)
            if exact_cull:
                assert np.array_equal(r.w[mine & culled], r.w0[mine & culled]), (label, c)
    # ---- bounded by the binary64 landing
    cnt_b = illum64.bounds(tg, r.out, r.status, key=ch, nkey=nchan)
    ld = cnt_b.landing
    reflected = np.where(r.bounces > 0, ch, -1)
    checks = [("hist", cnt_b, got["hist"])]
    if got["flux"] is not None:
        checks.append(("flux", illum64.bounds(tg, r.out, r.status, q=q, key=ch, nkey=nchan, landing=ld), got["flux"]))
    if got["rhist"] is not None:
        checks.append(("rhist", illum64.bounds(tg, r.out, r.status, key=reflected, nkey=nchan, landing=ld), got["rhist"]))
        checks.append(("rflux", illum64.bounds(tg, r.out, r.status, q=q, key=reflected, nkey=nchan, landing=ld),
                       got["rflux"]))
    for name, b, a in checks:
        assert a.shape == b.lo.shape == (nchan, tg.bins_v, tg.bins_u), (label, name)
        assert (b.lo <= a).all() and (a <= b.hi).all(), (label, name, int((a < b.lo).sum()), int((a > b.hi).sum()))
        total = a.reshape(nchan, -1).sum(axis=1)
        assert (b.landed_lo <= total).all() and (total <= b.landed_hi).all(), (label, name)
        which = {"hist": "stats", "flux": "power"}.get(name)
        if which:
            assert [d["landed"] for d in got[which]] == [int(v) for v in total], (label, name)
    if got["ledger"] is not None:
        key = ch * ROWS + row
        for name, qq in (("count", None), ("power", q)):
            b = illum64.bounds(tg, r.out, r.status, q=qq, key=key, nkey=nchan * ROWS, landing=ld)
            a = got["ledger"][name][:, :, LANDED].reshape(-1)
            assert (b.landed_lo <= a).all() and (a <= b.landed_hi).all(), (label, "ledger", name)
        assert np.array_equal(got["ledger"]["count"][:, 1:, LANDED].sum(axis=1), got["rhist"].reshape(nchan, -1).sum(axis=1))
        assert np.array_equal(got["ledger"]["power"][:, 1:, LANDED].sum(axis=1), got["rflux"].reshape(nchan, -1).sum(axis=1))
    # ---- the bounds bite
    landed = sum(d["landed"] for d in got["stats"])
    slack = int((cnt_b.hi - cnt_b.lo).sum())
    exited = int(outside.sum())
    print(f"{label}: exited {exited}, landed {landed}, culled {sum(d['culled'] for d in got['stats'])}, unsure "
          f"{cnt_b.unsure} ({100.0 * cnt_b.unsure / max(exited, 1):.3f} % of the exited), sum(hi - lo) {slack} "
          f"({100.0 * slack / max(landed, 1):.3f} % of the landed), reflected {int((r.bounces > 0).sum())}")
    assert landed >= want_landed, label
    assert slack <= 0.01 * landed, (label, slack, landed)
    assert cnt_b.unsure <= 0.01 * max(exited, 1), label
    return landed


# ------------------------------------------------------------------ (b) land(chain(emit))
@pytest.mark.parametrize("kind", ("plain", "power"))
@pytest.mark.parametrize("name", illum64.TARGETS)
def test_every_target(bzr, ctx, pipe, dms, rows_of, kind, name):
    r = rows_of(kind, illum64.OBLIQUE_X, pipe)
    tg = illum64.target(bzr, name)
    got = illuminate(bzr, ctx, dms, kind, illum64.emitter(bzr), tg, pipe)
    landed = check_case(bzr, dms[0], kind, r, tg, got, f"{kind}, {name}", want_landed=0 if name == "behind" else 1000)
    if name == "behind":
        assert landed == 0 and not got["hist"].any()


@pytest.mark.parametrize("kind", ("spectral", "tir", "media"))
def test_tilted_target_with_channels(bzr, ctx, pipe, dms, rows_of, kind):
    r = rows_of(kind, illum64.OBLIQUE_X, pipe)
    tg = illum64.target(bzr, "tilted")
    got = illuminate(bzr, ctx, dms, kind, illum64.emitter(bzr), tg, pipe)
    check_case(bzr, dms[0], kind, r, tg, got, f"{kind}, tilted")
    if kind != "spectral":
        assert int((r.bounces > 0).sum()) >= 100 and int(got["rhist"].sum()) >= 50
        assert int(got["ledger"]["count"][:, 1:].sum()) >= 100


@pytest.mark.parametrize("kind", ("plain", "power", "tir"))
def test_far_emitter_culls(bzr, ctx, pipe, dms, rows_of, kind):
    """The emitter at x = -40: most of the hemisphere misses the lens's sphere.  An extra to the cases above for the
    cull's integers (few rays are left to land, so no landed floor)."""
    r = rows_of(kind, illum64.FAR_X, pipe)
    tg = illum64.target(bzr, "tilted")
    got = illuminate(bzr, ctx, dms, kind, illum64.emitter(bzr, illum64.FAR_X), tg, pipe)
    check_case(bzr, dms[0], kind, r, tg, got, f"{kind}, far", want_landed=0)
    assert sum(d["culled"] for d in got["stats"]) > N // 2 and sum(d["exited"] for d in got["stats"]) > 0


# ------------------------------------------------------------------ (c) exact identities
def same_totals(a, b):
    if a["stats"] != b["stats"] or a["power"] != b["power"]:
        return False
    return a["ledger"] is None or all(np.array_equal(a["ledger"][k], b["ledger"][k]) for k in ("count", "power"))


MAPS = ("hist", "flux", "rhist", "rflux")


@pytest.mark.parametrize("kind", KINDS)
def test_swapped_target_is_the_transposed_map(bzr, ctx, pipe, dms, kind):
    em = illum64.emitter(bzr)
    for name in ("plain", "coarse", "tilted"):
        a = illuminate(bzr, ctx, dms, kind, em, illum64.target(bzr, name), pipe)
        b = illuminate(bzr, ctx, dms, kind, em, illum64.target(bzr, name + "_swapped"), pipe)
        assert a["stats"][0]["landed"] >= 1000 // NCHAN[kind]
        assert same_totals(a, b), (kind, name)
        for m in MAPS:
            if a[m] is not None:
                assert np.array_equal(b[m], a[m].transpose(0, 2, 1)), (kind, name, m)
        k = min(a["hist"].shape[1:])
        assert not np.array_equal(a["hist"][0][:k, :k], a["hist"][0][:k, :k].T)   # the map is not symmetric


@pytest.mark.parametrize("kind", KINDS)
def test_coarse_map_is_the_block_sums(bzr, ctx, pipe, dms, kind):
    em = illum64.emitter(bzr)
    for fine, coarse in (("plain", "coarse"), ("tilted20", "tilted20_coarse")):
        a = illuminate(bzr, ctx, dms, kind, em, illum64.target(bzr, fine), pipe)
        b = illuminate(bzr, ctx, dms, kind, em, illum64.target(bzr, coarse), pipe)
        assert same_totals(a, b), (kind, fine)
        for m in MAPS:
            if a[m] is not None:
                s = a[m].shape
                blocks = a[m].reshape(s[0], s[1] // 2, 2, s[2] // 2, 2).sum(axis=(2, 4), dtype=a[m].dtype)
                assert np.array_equal(blocks, b[m]), (kind, fine, m)


# ------------------------------------------------------------------ (d) belts
@pytest.mark.parametrize("belts", (0, 4097))
def test_bad_belts_are_rejected_before_anything_is_written(bzr, ctx, dms, belts):
    em = illum64.emitter(bzr, belts=belts)
    rays, patch = np.full((6, 256), 5, F), np.full(256, 5, np.uint32)
    with pytest.raises(bzr.BzrError, match="belts"):
        bzr.emit(ctx, em, 0, 256, rays=rays, patch=patch)
    assert (rays == 5).all() and (patch == 5).all()
    tg = illum64.target(bzr, "plain")
    hist = np.full((tg.bins_v, tg.bins_u), 5, np.uint32)
    stats = (ctypes.c_uint64 * 4)(5, 5, 5, 5)
    handles, ris = (ctypes.c_void_p * 1)(dms[0].handle), (ctypes.c_float * 1)(RI)
    rc = bzr.lib().bzr_illuminate(ctx.handle, handles, ris, 1, ctypes.byref(em), 256, ctypes.byref(tg), hist.ctypes.data,
                                  stats, 0)
    assert rc == 1 and b"belts" in bzr.lib().bzr_last_error()   # BZR_ERR_INVALID_ARGUMENT
    assert (hist == 5).all() and list(stats) == [5, 5, 5, 5]
    with pytest.raises(bzr.BzrError, match="belts"):
        bzr.illuminate(ctx, dms, [RI], em, 256, tg, hist=hist)
    assert (hist == 5).all()
    # the context still works
    good, _ = bzr.emit(ctx, illum64.emitter(bzr), 0, 256)
    illum64.check_emit(illum64.emitter(bzr), 0, good, bzr.emit(ctx, illum64.emitter(bzr), 0, 256)[1])
