"""Every buffer form of every entry point on a context of its own.

A context's staging scratch only grows, so on a long-lived context an earlier, larger call hides a staging layout
that asks for fewer bytes than it carves.  Here every call under test runs on a new Context, whose scratch is then
exactly what that call asked for, at batch sizes (1, 65, 257 rays) whose rows are no multiple of the 256-byte carve
unit.  The expected words are those of the device-pointer, row-layout call on one long-lived context (the form the
parity tests pin to the oracle); every other form must equal them bit for bit.

Geometry: cfg4's lens pair; rays: every 7th of its 64 x 64 grid from ray 127 on, so that the first ray already
crosses a lens and reflects in it and a batch of 257 has hits and misses; kModeTir: test_gpu_tir's cfg4 table,
which makes rays reflect.
"""
import ctypes

import numpy as np
import pytest

from bzr_amd.configs import CONFIGS, build_lens, grid_rays
from test_gpu_illumination import emitter, target
from test_gpu_tir import NCHAN, ROW1, ROW2

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = (1, 65, 257)
START, STRIDE = 127, 7
TABLE = [ROW1, ROW2]
ILLUM_RAYS, ILLUM_CAP = 500, 192  # batches of 192 + 192 + 116 rays


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def scene(bzr, ctx):
    """(ri, device meshes, rays [6, 257], channel, weights): made once, never changed."""
    cfg = CONFIGS["cfg4"]
    lenses = [build_lens(bzr.TriMesh, lens).bezier_patches() for lens in cfg.lenses]
    rays = np.ascontiguousarray(grid_rays(cfg, side=64)[:, START::STRIDE][:, :max(SIZES)])
    assert rays.shape == (6, max(SIZES))
    n = rays.shape[1]
    channel = np.random.default_rng(7).integers(0, NCHAN, n).astype(np.uint8)
    weight = np.random.default_rng(41).random(n, dtype=F)
    for a in (rays, channel, weight):
        a.setflags(write=False)
    return [l.ri for l in cfg.lenses], [bzr.DeviceMesh(ctx, p) for p in lenses], rays, channel, weight


def words(x):
    """A result as host words: float32 as uint32, torch tensors copied back."""
    a = x.cpu().numpy() if hasattr(x, "is_cuda") else np.asarray(x)
    return a.view(np.uint32) if a.dtype in (np.float32, np.int32) else a.view(np.uint64) if a.dtype == np.int64 else a


def in_form(torch, a, device, aos=False):
    if a is None:
        return None
    a = np.array(a.T if aos else a, order="C")  # (a writable copy: the scene's arrays are read-only)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() if device else a


def on_fresh_context(bzr, torch, call):
    """call(context) on a context that has staged nothing yet -> its results as host words."""
    c = bzr.Context(0)
    try:
        out = call(c)
        torch.cuda.synchronize()
        return [None if o is None else words(o) for o in out]
    finally:
        c.close()


def same(got, want, label):
    assert len(got) == len(want), label
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), (label, k)
        if g is not None:
            assert g.shape == w.shape and np.array_equal(g, w), f"{label}: output {k}, {int((g != w).sum())} words differ"


FORMS = (("host", False, False), ("host aos", False, True), ("device", True, False), ("device aos", True, True))


def check_forms(bzr, torch, ctx, call, rays, rows, forms, label, ray_out=True):
    """call(context, rays, *rows, mode) in every form of `forms` on fresh contexts against the device-pointer row-layout
    call on the long-lived context.  ray_out: output 0 holds rays ([n, 6] records under RAYS_AOS).  Returns the
    expected words."""
    want = [None if o is None else words(o)
            for o in call(ctx, in_form(torch, rays, True), *[in_form(torch, r, True) for r in rows], 0)]
    torch.cuda.synchronize()
    for name, device, aos in forms:
        got = on_fresh_context(bzr, torch, lambda c: call(c, in_form(torch, rays, device, aos),
                                                          *[in_form(torch, r, device) for r in rows],
                                                          bzr.RAYS_AOS if aos else 0))
        if aos and ray_out:
            got[0] = np.ascontiguousarray(got[0].T)
        same(got, want, f"{label}, {name}")
    return want


PIPES = ("fused", "staged")


def pipe_flag(bzr, pipe):
    return bzr.PIPELINE_FUSED if pipe == "fused" else bzr.PIPELINE_STAGED


# ------------------------------------------------------------------ single-surface entry points
@pytest.mark.parametrize("n", SIZES)
def test_intersect_and_records(bzr, torch, ctx, scene, n):
    _, dms, rays, _, _ = scene
    rays = rays[:, :n]
    for pipe in PIPES:
        p = pipe_flag(bzr, pipe)
        rows = check_forms(bzr, torch, ctx, lambda c, r, m: [bzr.intersect(c, dms[0], r, mode=m | p)], rays, [],
                           FORMS[:2], f"intersect {pipe} n {n}", ray_out=False)[0]
        hit = rows[11] == bzr.WHAT_INTERSECT
        if n == max(SIZES):
            assert 20 <= hit.sum() <= n - 20, "hits and misses"

        def records(c, r, m, with_patch):
            """bzr_intersect_records with or without a patch row (the wrapper always passes one)."""
            k = bzr._n_of(r, m)
            dev = hasattr(r, "is_cuda")
            rec = torch.empty((k, 13), dtype=torch.int32, device="cuda") if dev else np.empty((k, 13), np.uint32)
            pat = None if not with_patch else (torch.empty(k, dtype=torch.int32, device="cuda") if dev
                                               else np.empty(k, np.uint32))
            rb, ob, pb = bzr._Buf(r, F), bzr._Buf(rec, np.uint32, True), bzr._Buf(pat, np.uint32, True)
            res = bzr._residency(rb, ob)
            with bzr._stream_for(c, res):
                bzr._check(bzr.lib().bzr_intersect_records(c.handle, dms[0].handle, rb.ptr, k, ob.ptr, pb.ptr, res | m | p))
            return [rec, pat]

        for with_patch in (True, False):
            rec, pat = check_forms(bzr, torch, ctx, lambda c, r, m: records(c, r, m, with_patch), rays, [],
                                   (FORMS[0], FORMS[1], FORMS[3]), f"records {pipe} n {n} patch {with_patch}", ray_out=False)
            assert np.array_equal(rec[:, 12], rows[11]) and np.array_equal(rec[:, 5], rows[0])
            assert (pat is None) if not with_patch else np.array_equal(pat, rows[12])


@pytest.mark.parametrize("n", SIZES)
def test_patch_intersect(bzr, torch, ctx, scene, n):
    _, dms, rays, _, _ = scene
    rng = np.random.default_rng(n)
    idx = rng.integers(0, dms[0].n, n).astype(np.uint32)
    idx[-1] = dms[0].n + 5  # no such patch: no hit
    limit = rng.integers(0, 2, n).astype(np.uint32)
    check_forms(bzr, torch, ctx, lambda c, r, i, l, m: [bzr.patch_intersect(c, dms[0], i, l, r, mode=m)], rays[:, :n],
                [idx, limit], FORMS[:1], f"patch_intersect n {n}", ray_out=False)


@pytest.mark.parametrize("n", SIZES)
def test_refract(bzr, torch, ctx, scene, n):
    ri, dms, rays, _, _ = scene
    expected = np.random.default_rng(n).integers(0, 4, n).astype(np.uint32)
    for pipe in PIPES:
        p = pipe_flag(bzr, pipe)
        for exp in (None, expected):
            check_forms(bzr, torch, ctx, lambda c, r, e, m: bzr.refract(c, dms[0], ri[0], r, e, mode=m | p), rays[:, :n],
                        [exp], FORMS[:2], f"refract {pipe} n {n} expected {exp is not None}")


# ------------------------------------------------------------------ chains
@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("n", SIZES)
def test_chains(bzr, torch, ctx, scene, n, pipe):
    ri, dms, rays, channel, weight = scene
    rays, channel, weight = rays[:, :n], channel[:n], weight[:n]
    p = pipe_flag(bzr, pipe)
    want = check_forms(bzr, torch, ctx, lambda c, r, m: bzr.trace_chain(c, dms, ri, r, mode=m | p), rays, [], FORMS,
                       f"chain {pipe} n {n}")
    assert want[2].sum() > n, "segment total"
    for w in (None, weight):
        want = check_forms(bzr, torch, ctx, lambda c, r, wi, m: bzr.trace_chain_power(c, dms, ri, r, wi, mode=m | p), rays,
                           [w], FORMS, f"chain_power {pipe} n {n} weight_in {w is not None}")
        assert want[3].sum() > n
    want = check_forms(bzr, torch, ctx,
                       lambda c, r, ch, wi, m: bzr.trace_chain_spectral(c, dms, TABLE, r, ch, wi, mode=m | p), rays,
                       [channel, weight], FORMS, f"chain_spectral {pipe} n {n}")
    assert want[3].sum() > n


@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("n", SIZES)
def test_chain_tir(bzr, torch, ctx, scene, n, pipe):
    _, dms, rays, channel, weight = scene
    rays, channel, weight = rays[:, :n], channel[:n], weight[:n]
    p = pipe_flag(bzr, pipe)
    handles = (ctypes.c_void_p * 2)(*[m.handle for m in dms])
    table = np.ascontiguousarray(TABLE, dtype=F)

    def tir(c, r, ch, wi, m, max_bounces, with_bounces):
        """bzr_trace_chain_tir with or without out_bounces (the wrapper always passes one)."""
        k = bzr._n_of(r, m)
        outs = [bzr._empty_like(r, 6, F, m), bzr._empty_like(r, 0, F, m), bzr._empty_like(r, 0, np.uint32, m),
                bzr._empty_like(r, 0, np.uint32, m), bzr._empty_like(r, 0, np.uint32, m) if with_bounces else None]
        rb, cb, wb = bzr._Buf(r, F), bzr._Buf(ch, np.uint8), bzr._Buf(wi, F)
        ob = [bzr._Buf(o, F if j < 2 else np.uint32, True) for j, o in enumerate(outs)]
        res = bzr._residency(rb, ob[0])
        with bzr._stream_for(c, res):
            bzr._check(bzr.lib().bzr_trace_chain_tir(c.handle, ctypes.cast(handles, ctypes.c_void_p), table.ctypes.data, 2,
                                                     NCHAN, rb.ptr, cb.ptr, wb.ptr, k, max_bounces, ob[0].ptr, ob[1].ptr,
                                                     ob[2].ptr, ob[3].ptr, ob[4].ptr, res | m | p))
        return outs

    for max_bounces in (0, 2):
        for ch in (None, channel):
            for with_bounces in (False, True):
                want = check_forms(bzr, torch, ctx, lambda c, r, cc, wi, m: tir(c, r, cc, wi, m, max_bounces, with_bounces),
                                   rays, [ch, weight], FORMS,
                                   f"chain_tir {pipe} n {n} max_bounces {max_bounces} channel {ch is not None} "
                                   f"out_bounces {with_bounces}")
                assert want[3].sum() > n
                if with_bounces:
                    assert (want[4].max() >= 1) == (max_bounces > 0), "reflections"


# ------------------------------------------------------------------ tessellation, emitter, illumination
@pytest.mark.parametrize("divisor", [1, 3])
def test_mesh_interpolate(bzr, torch, ctx, scene, divisor):
    _, dms, _, _, _ = scene
    out = torch.empty((divisor * divisor * dms[0].n, 3, 3), dtype=torch.float32, device="cuda")
    want = words(bzr.interpolate(ctx, dms[0], divisor, out=out))
    same(on_fresh_context(bzr, torch, lambda c: [bzr.interpolate(c, dms[0], divisor)]), [want], f"interpolate {divisor}")


@pytest.mark.parametrize("n", SIZES)
def test_emit(bzr, torch, ctx, n):
    em, first = emitter(bzr), 12345
    d_rays, d_patch = bzr.emit(ctx, em, first, n, rays=torch.empty((6, n), dtype=torch.float32, device="cuda"),
                               patch=torch.empty(n, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    want = [words(d_rays), words(d_patch)]
    same(on_fresh_context(bzr, torch, lambda c: bzr.emit(c, em, first, n)), want, f"emit n {n}")

    def no_patch(c):
        rays = np.empty((6, n), F)
        bzr._check(bzr.lib().bzr_emit(c.handle, ctypes.byref(em), first, n, rays.ctypes.data, None, bzr.HOST_PTRS))
        return [rays]

    same(on_fresh_context(bzr, torch, no_patch), want[:1], f"emit n {n}, no patch row")


def set_cap(bzr, c, rays):
    eff = ctypes.c_uint32(0)
    assert bzr.lib().bzr_debug_chunk_cap(c.handle, rays, ctypes.byref(eff)) == 0
    return eff.value


@pytest.fixture(scope="module")
def capped(bzr, ctx):
    """The long-lived context of the illumination cases: this module's own, the session context never sees a lowered
    chunk cap."""
    c = bzr.Context(0)
    assert set_cap(bzr, c, ILLUM_CAP) == ILLUM_CAP
    yield c
    c.close()


@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("kind", ["counts", "power", "spectral"])
def test_illuminate_host_maps_against_device_maps(bzr, torch, capped, scene, kind, pipe):
    ri, dms, _, _, _ = scene
    em, tg, p = emitter(bzr), target(bzr), pipe_flag(bzr, pipe)
    shape = (NCHAN if kind == "spectral" else 1, tg.bins_v, tg.bins_u)

    def run(c, device):
        if device:
            flux = torch.zeros(shape, dtype=torch.int64, device="cuda")
            hist = torch.zeros(shape, dtype=torch.int32, device="cuda")
        else:
            flux, hist = np.zeros(shape, np.uint64), np.zeros(shape, np.uint32)
            assert set_cap(bzr, c, ILLUM_CAP) == ILLUM_CAP
        c.timing(True)
        c.timing_report()
        if kind == "counts":
            h, stats = bzr.illuminate(c, dms, ri, em, ILLUM_RAYS, tg, hist=hist[0], mode=p)
            out = [h, np.array(list(stats.values()), np.uint64)]
        elif kind == "power":
            f, h, stats, power = bzr.illuminate_power(c, dms, ri, em, ILLUM_RAYS, tg, flux=flux[0], hist=hist[0], mode=p)
            out = [h, np.array(list(stats.values()) + list(power.values()), np.uint64), f]
        else:
            f, h, stats, power = bzr.illuminate_spectral(c, dms, TABLE, em, ILLUM_RAYS, tg, flux=flux, hist=hist, mode=p)
            out = [h, np.array([list(s.values()) + list(q.values()) for s, q in zip(stats, power)], np.uint64), f]
        launches = {k: v[1] for k, v in c.timing_report().items()}
        c.timing(False)
        assert launches.get("k_trace", 0) == (3 if pipe == "fused" else 0), launches
        assert launches.get("k_traverse", 0) == (0 if pipe == "fused" else 3 * 2 * len(dms)), launches
        return out

    want = [words(o) for o in run(capped, True)]
    torch.cuda.synchronize()
    totals = want[1].reshape(-1, want[1].shape[-1])[:, :4].sum(axis=0)  # emitted, culled, exited, landed
    assert totals[0] == ILLUM_RAYS and totals[1] < ILLUM_RAYS and totals[3] == want[0].sum()
    same(on_fresh_context(bzr, torch, lambda c: run(c, False)), want, f"illuminate {kind} {pipe}")
