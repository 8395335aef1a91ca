"""Fresnel-weighted ray power on the GPU: bzr_trace_chain_power and bzr_illuminate_power against the oracle composed
segment by segment with the Fresnel term in numpy float32 (tests/power_ref.py), bit for bit.

Every sum is an integer sum of q(w) = trunc(w x 2^32), so the weighted histogram and the four power sums are compared
for equality.  The populations the tests rely on are asserted from the reference, so none passes vacuously.
"""
import ctypes

import numpy as np
import pytest

import power_ref
from bzr_amd.configs import CONFIGS, build_lens, grid_rays
from test_chunk_plan import chunk_rule
from test_gpu_illumination import emitter, target
from test_gpu_long_chains import chain_rays, lens_patches

pytestmark = pytest.mark.gpu

F = np.float32
PATHS = ("fused", "staged", "brute")
CASES = {"cfg2": (128, 37, 10_000), "cfg4": (96, 0, 5_500)}  # side, rays dropped at the end, exits required


def flags_of(bzr, path):
    return {"fused": bzr.PIPELINE_FUSED, "staged": bzr.PIPELINE_STAGED, "brute": bzr.ACCEL_NONE}[path]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def assert_same(got, want, label):
    """(rays, weight, status, segments) word for word."""
    bad = (bits(got[0]) != bits(want[0])).any(axis=0) | (bits(got[1]) != bits(want[1])) | \
        (np.asarray(got[2]) != want[2]) | (np.asarray(got[3]) != want[3])
    assert not bad.any(), (f"{label}: {int(bad.sum())} of {len(bad)} rays differ, first {np.nonzero(bad)[0][:8]}; "
                           f"weights got {np.asarray(got[1])[bad][:4]} want {want[1][bad][:4]}")


@pytest.fixture(scope="module")
def scenes(bzr, orc, ctx):
    """name -> (patches, ris, device meshes, rays, random input weights, reference with weight 1, reference with the
    random weights): computed once, never changed."""
    out = {}
    for name, (side, drop, _) in CASES.items():
        cfg = CONFIGS[name]
        lenses = [build_lens(bzr.TriMesh, lens).bezier_patches() for lens in cfg.lenses]
        ris = [lens.ri for lens in cfg.lenses]
        rays = grid_rays(cfg, side=side)
        rays = np.ascontiguousarray(rays[:, :rays.shape[1] - drop])
        w_in = np.random.default_rng(31 + side).random(rays.shape[1], dtype=F)
        ones = frozen(*power_ref.chain(orc, lenses, ris, rays))
        rand = frozen(*power_ref.chain(orc, lenses, ris, rays, w_in))
        frozen(rays, w_in)
        out[name] = (lenses, ris, [bzr.DeviceMesh(ctx, p) for p in lenses], rays, w_in, ones, rand)
    return out


# ------------------------------------------------------------------ 1. chain weights
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(CASES))
def test_chain_weights_bit_exact(bzr, ctx, scenes, name, path):
    _, ris, dms, rays, w_in, ones, rand = scenes[name]
    side, drop, need = CASES[name]
    assert rays.shape[1] == side * side - drop
    assert int((ones[2] == bzr.RR_OUTSIDE).sum()) >= need
    ex = ones[2] == bzr.RR_OUTSIDE
    assert ((ones[1][ex] > 0.4) & (ones[1][ex] < 0.97)).all()
    mode = flags_of(bzr, path)
    plain = bzr.trace_chain(ctx, dms, ris, rays, mode=mode)
    got = bzr.trace_chain_power(ctx, dms, ris, rays, mode=mode)
    assert_same(got, ones, f"{name} {path}, weight=None: vs the reference")
    assert np.array_equal(bits(got[0]), bits(plain[0])) and np.array_equal(got[2], plain[1]) and \
        np.array_equal(got[3], plain[2])
    w = w_in.copy()  # passed in place
    got = bzr.trace_chain_power(ctx, dms, ris, rays, weight=w, out_weight=w, mode=mode)
    assert got[1] is w
    assert_same(got, rand, f"{name} {path}, random weights in place: vs the reference")
    # a ray that never refracts keeps its input weight
    never = rand[3] == 1
    assert never.sum() > 1000 and np.array_equal(bits(w[never]), bits(w_in[never]))


def test_chain_weights_device_buffers_and_aos(bzr, ctx, scenes):
    """Device pointers (the asynchronous path) and [n, 6] ray records: the same bits."""
    torch = pytest.importorskip("torch")
    _, ris, dms, rays, w_in, _, rand = scenes["cfg4"]
    r = torch.from_numpy(np.ascontiguousarray(rays.T)).cuda()
    w = torch.from_numpy(w_in.copy()).cuda()
    for pipe in (bzr.PIPELINE_FUSED, bzr.PIPELINE_STAGED):
        o, ow, s, g = bzr.trace_chain_power(ctx, dms, ris, r, weight=w, mode=pipe | bzr.RAYS_AOS)
        torch.cuda.synchronize()
        got = (np.ascontiguousarray(o.cpu().numpy().T), ow.cpu().numpy(), s.cpu().numpy().astype(np.uint32),
               g.cpu().numpy().astype(np.uint32))
        assert_same(got, rand, f"cfg4 device pointers, AoS, pipeline {pipe}")


# ------------------------------------------------------------------ 2. small chunks
@pytest.fixture(scope="module")
def cctx(bzr, ctx):
    """This module's own context: the session context never sees a lowered chunk cap."""
    c = bzr.Context(0)
    yield c
    c.close()


def set_cap(bzr, c, rays):
    eff = ctypes.c_uint32(0)
    assert bzr.lib().bzr_debug_chunk_cap(c.handle, rays, ctypes.byref(eff)) == 0
    return eff.value


def test_small_chunks(bzr, orc, cctx):
    cfg = CONFIGS["cfg2"]
    lens = build_lens(bzr.TriMesh, cfg.lenses[0]).bezier_patches()
    full = grid_rays(cfg, side=128)
    n = 1000
    first = (full.shape[1] - n) // 2  # the grid's centre in tile order: every ray meets the lens
    rays = np.ascontiguousarray(full[:, first:first + n])
    w_in = np.random.default_rng(5).random(n, dtype=F)
    want = power_ref.chain(orc, [lens], [1.3], rays, w_in)
    assert int((want[2] == bzr.RR_OUTSIDE).sum()) > 900
    dm = bzr.DeviceMesh(cctx, lens)
    try:
        assert set_cap(bzr, cctx, 0) >= 1 << 14
        auto = bzr.trace_chain_power(cctx, [dm], [1.3], rays, weight=w_in, mode=bzr.PIPELINE_STAGED)
        assert_same(auto, want, "automatic cap")
        for cap in (64, 192):
            assert set_cap(bzr, cctx, cap) == cap
            cctx.timing(True)
            cctx.timing_report()
            got = bzr.trace_chain_power(cctx, [dm], [1.3], rays, weight=w_in, mode=bzr.PIPELINE_STAGED)
            launches = cctx.timing_report()["k_traverse"][1]
            cctx.timing(False)
            assert launches == 2 * -(-n // chunk_rule(n, cap)) >= 12, (cap, launches)  # two segments per chunk
            assert_same(got, want, f"cap {cap}: vs the reference")
            assert_same(got, auto, f"cap {cap}: vs the automatic cap")
    finally:
        cctx.timing(False)
        set_cap(bzr, cctx, 0)


# ------------------------------------------------------------------ 3. edges
@pytest.mark.parametrize("path", PATHS)
def test_nan_ray_keeps_its_weight(bzr, ctx, scenes, path):
    _, ris, dms, rays, w_in, _, rand = scenes["cfg2"]
    n = rays.shape[1]
    lanes17 = np.nonzero((rand[2] == bzr.RR_OUTSIDE) & (np.arange(n) % 64 == 17))[0]
    assert len(lanes17) > 50
    k = int(lanes17[len(lanes17) // 2])  # a ray that passes the lens: lane 17 of a wave mid-batch
    poisoned = rays.copy()
    poisoned[4, k] = np.nan
    got = bzr.trace_chain_power(ctx, dms, ris, poisoned, weight=w_in, mode=flags_of(bzr, path))
    assert got[2][k] == bzr.RR_NONE and bits(got[1])[k] == bits(w_in)[k]
    assert np.array_equal(bits(got[0])[:, k], bits(poisoned)[:, k])
    others = np.arange(rays.shape[1]) != k
    assert_same(tuple(a[..., others] for a in got), tuple(a[..., others] for a in rand), f"{path}: the other rays")


def test_lens_count_is_validated(bzr, ctx, scenes):
    _, ris, dms, rays, w_in, _, _ = scenes["cfg2"]
    n = 256
    r = np.ascontiguousarray(rays[:, :n])
    for nl in (0, 9):
        o = np.full((6, n), 7.0, F)
        w = np.full(n, 7.0, F)
        s = np.full(n, 7, np.uint32)
        g = np.full(n, 7, np.uint32)
        with pytest.raises(bzr.BzrError, match="nlens"):
            bzr.trace_chain_power(ctx, dms * nl, ris * nl, r, weight=w_in[:n].copy(), out_rays=o, out_weight=w,
                                  out_status=s, out_segments=g)
        assert (o == 7).all() and (w == 7).all() and (s == 7).all() and (g == 7).all()


@pytest.mark.parametrize("path", PATHS)
def test_eight_lens_chain(bzr, ctx, path, eight):
    lenses, ris, rays, want = eight
    dms = [bzr.DeviceMesh(ctx, p) for p in lenses]
    got = bzr.trace_chain_power(ctx, dms, ris, rays, mode=flags_of(bzr, path))
    assert_same(got, want, f"eight lenses, {path}")


@pytest.fixture(scope="module")
def eight(orc):
    lenses = [lens_patches(orc, k) for k in range(8)]
    ris = [1.3] * 8
    rays = chain_rays()
    want = frozen(*power_ref.chain(orc, lenses, ris, rays))
    through = want[3] == 16
    assert rays.shape[1] == 64 * 64 and through.sum() > 2000  # sixteen refractions multiplied in chain order
    assert (want[1][through & (want[2] == 2)] < 0.97 ** 8).all()
    return lenses, ris, rays, want


# ------------------------------------------------------------------ 4. FAST
@pytest.mark.parametrize("pipe_name", ("fused", "staged"))
def test_fast_mode(bzr, ctx, scenes, pipe_name):
    """FAST changes the Newton stage only: rays, status and segments are bzr_trace_chain's FAST ones bit for bit, and
    the Fresnel term itself stays exact.  How far the FAST weights lie from the parity ones is recorded (printed, and
    in DESIGN.md (c)); the distance from the truth is what tests/test_gpu_fast_chain64.py asserts."""
    _, ris, dms, rays, _, ones, _ = scenes["cfg2"]
    mode = flags_of(bzr, pipe_name) | bzr.MODE_FAST
    plain = bzr.trace_chain(ctx, dms, ris, rays, mode=mode)
    got = bzr.trace_chain_power(ctx, dms, ris, rays, mode=mode)
    assert np.array_equal(bits(got[0]), bits(plain[0])) and np.array_equal(got[2], plain[1]) and \
        np.array_equal(got[3], plain[2])
    assert (got[1] > 0).all() and (got[1] <= 1).all()
    agree = (got[2] == ones[2]) & (got[3] == ones[3])
    rel = np.abs(got[1][agree].astype(np.float64) - ones[1][agree]) / ones[1][agree]
    print(f"FAST {pipe_name}: {int(agree.sum())} of {len(agree)} rays agree in status and segments; "
          f"|w_fast - w_parity| / w_parity median {np.median(rel):.3g}, p99 {np.quantile(rel, 0.99):.3g}, "
          f"max {rel.max():.3g}")
    assert agree.sum() > 16_000


# ------------------------------------------------------------------ 5. illumination
N_ILLUM = 1 << 16


@pytest.fixture(scope="module")
def illum(bzr, orc, ctx):
    """cfg2, emitter at x = 0, 65 536 rays: the reference chain over every emitted ray (no cull) with Lambert weights,
    its weighted histogram, counts and power sums."""
    lens = build_lens(bzr.TriMesh, CONFIGS["cfg2"].lenses[0]).bezier_patches()
    rays, _ = orc.emit(emitter(orc), 0, N_ILLUM)
    w0 = rays[3].copy()
    out, w, status, _ = power_ref.chain(orc, [lens], [1.3], rays, w0)
    tg = target(orc)
    hist, exited, landed = orc.land(tg, out, status)
    flux = power_ref.flux(orc, tg, out, status, w)
    q = power_ref.q32(w)
    power = {"emitted": int(power_ref.q32(w0).sum()), "exited": int(q[status == 2].sum()), "landed": int(flux.sum())}
    return lens, bzr.DeviceMesh(ctx, lens), rays, hist, flux, exited, landed, power


def culled_by_sphere(sphere, rays):
    c = sphere.astype(np.float64)
    oc = rays[:3].astype(np.float64) - c[:3, None]
    cc = (oc * oc).sum(0) - c[3] ** 2
    b = (oc * rays[3:].astype(np.float64)).sum(0)
    return (cc > 0) & ((b >= 0) | (b * b - cc < 0))


def test_illuminate_lambert_fresnel(bzr, orc, ctx, pipe, illum):
    _, dm, rays, hist, flux, exited, landed, power = illum
    assert landed > 2000
    got_flux, got_hist, stats, got_power = bzr.illuminate_power(ctx, [dm], [1.3], emitter(bzr), N_ILLUM, target(bzr),
                                                                mode=pipe)
    assert got_flux.dtype == np.uint64 and np.array_equal(got_flux, flux)
    assert np.array_equal(got_hist, hist)
    culled = culled_by_sphere(bzr.bounding_sphere(dm), rays)
    assert stats == {"emitted": N_ILLUM, "culled": int(culled.sum()), "exited": exited, "landed": landed}
    assert got_power == dict(power, culled=int(power_ref.q32(rays[3][culled]).sum()))
    assert got_power["landed"] <= got_power["exited"] <= got_power["emitted"] - got_power["culled"]
    assert abs(float(bzr.flux_to_float(got_flux).sum()) - got_power["landed"] / 2 ** 32) < 1e-6
    # a second call into the same flux and hist accumulates
    bzr.illuminate_power(ctx, [dm], [1.3], emitter(bzr), N_ILLUM, target(bzr), flux=got_flux, hist=got_hist, mode=pipe)
    assert np.array_equal(got_flux, flux * np.uint64(2)) and np.array_equal(got_hist, hist * 2)


def test_illuminate_uniform_lossless_is_the_count(bzr, ctx, pipe, illum):
    _, dm, _, hist, _, exited, landed, _ = illum
    flux, got_hist, stats, power = bzr.illuminate_power(ctx, [dm], [1.3], emitter(bzr), N_ILLUM, target(bzr),
                                                        emission=bzr.EMISSION_UNIFORM, surface=bzr.SURFACE_LOSSLESS,
                                                        mode=pipe)
    plain_hist, plain_stats = bzr.illuminate(ctx, [dm], [1.3], emitter(bzr), N_ILLUM, target(bzr), mode=pipe)
    assert np.array_equal(got_hist, plain_hist) and np.array_equal(got_hist, hist) and stats == plain_stats
    assert np.array_equal(flux, got_hist.astype(np.uint64) << np.uint64(32))
    assert power == {k: v << 32 for k, v in stats.items()}
    assert stats["exited"] == exited and stats["landed"] == landed


def test_illuminate_culled_power_far_emitter(bzr, orc, ctx, pipe, illum):
    """x = -60: most of the hemisphere misses the lens's bounding sphere; the culled power is the Lambert weight of
    exactly the rays the sphere drops."""
    _, dm, _, _, _, _, _, _ = illum
    rays, _ = orc.emit(emitter(orc, x=-60.0), 0, N_ILLUM)
    culled = culled_by_sphere(bzr.bounding_sphere(dm), rays)
    _, _, stats, power = bzr.illuminate_power(ctx, [dm], [1.3], emitter(bzr, x=-60.0), N_ILLUM, target(bzr), mode=pipe)
    assert stats["culled"] == int(culled.sum()) > N_ILLUM // 2
    assert power["culled"] == int(power_ref.q32(rays[3][culled]).sum())
    assert power["emitted"] == int(power_ref.q32(rays[3]).sum())
    assert power["landed"] <= power["exited"] <= power["emitted"] - power["culled"]
    assert stats["exited"] > 0 and power["exited"] > 0


def test_illuminate_batches(bzr, orc, cctx, pipe):
    """10 000 rays at a chunk cap of 4 096: three batches through the batch loop, the same bits as one batch."""
    lens = build_lens(bzr.TriMesh, CONFIGS["cfg2"].lenses[0]).bezier_patches()
    dm = bzr.DeviceMesh(cctx, lens)
    n = 10_000
    try:
        assert set_cap(bzr, cctx, 0) >= 1 << 14
        one = bzr.illuminate_power(cctx, [dm], [1.3], emitter(bzr), n, target(bzr), mode=pipe)
        assert set_cap(bzr, cctx, 4096) == 4096
        cctx.timing(True)
        cctx.timing_report()
        got = bzr.illuminate_power(cctx, [dm], [1.3], emitter(bzr), n, target(bzr), mode=pipe)
        rep = cctx.timing_report()
        cctx.timing(False)
    finally:
        cctx.timing(False)
        set_cap(bzr, cctx, 0)
    assert rep["k_trace" if pipe == bzr.PIPELINE_FUSED else "k_traverse"][1] == (3 if pipe == bzr.PIPELINE_FUSED else 6)
    assert np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1]) and got[2] == one[2] and got[3] == one[3]
    rays, _ = orc.emit(emitter(orc), 0, n)
    out, w, status, _ = power_ref.chain(orc, [lens], [1.3], rays, rays[3].copy())
    assert np.array_equal(got[0], power_ref.flux(orc, target(orc), out, status, w))
    assert got[2]["landed"] > 300


def test_illuminate_power_rejects_bad_arguments(bzr, ctx, illum):
    _, dm, _, _, _, _, _, _ = illum
    flux = np.full((48, 48), 5, np.uint64)
    hist = np.full((48, 48), 5, np.uint32)
    for kw, msg in (({"emission": 2}, "emission"), ({"surface": 2}, "surface")):
        with pytest.raises(bzr.BzrError, match=msg):
            bzr.illuminate_power(ctx, [dm], [1.3], emitter(bzr), 1000, target(bzr), flux=flux, hist=hist, **kw)
    with pytest.raises(bzr.BzrError, match="2\\^32"):
        bzr.illuminate_power(ctx, [dm], [1.3], emitter(bzr), 1 << 32, target(bzr), flux=flux, hist=hist)
    assert (flux == 5).all() and (hist == 5).all()
