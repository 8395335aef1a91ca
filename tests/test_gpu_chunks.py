"""The staged chunk loop (and bzr_illuminate's batch loop) at small chunk sizes, on every entry point.

The chunk size depends on the device's free memory (trace.hip chunk_for: a quarter of it at ~2.7 KB per ray, at most
8 M rays), so on a busy device a modest batch runs as many small ragged chunks.  bzr_debug_chunk_cap lowers the cap of
one context at run time; here every edge-case batch of the other test files (their recipes, imported) runs at caps of
64 rays (one wave per chunk: a quarter of k_traverse's 256-thread block, nearly every bucket on the k_newton_lane
path), 192 (three waves, no multiple of the block) and 1024, so that every `off + i` of the staged kernels' side paths
(overflow list, follow list, expected, alive, status, counters) and every per-chunk reset (w.ctr, the lazily zeroed
histogram across lens switches) meets an offset that is not zero.

In parity mode every output word equals the CPU oracle's and the same call's on the automatic cap.  Every call first
proves the chunks it ran: with timing on, k_traverse launches = chunks (the rule restated, tests/test_chunk_plan.py)
x segments launched; fused bzr_illuminate: k_trace launches = batches.

The context is this module's own: the session context never sees a lowered cap.
"""
import ctypes

import numpy as np
import pytest

import ref64
from test_chunk_plan import chunk_rule
from test_gpu_fast_ref64 import CLASS_ALLOW, STATUS_AGREE, assert_bars, assert_chain_gates, mesh_rays
from test_gpu_illumination import emitter, oracle_illuminate, target
from test_gpu_long_chains import big3, bits, chain_rays, lens8, lens_patches, sets, table  # noqa: F401 (fixtures)
from test_gpu_ray_edges import (RI3, clean_batch, differing, poisoned, run_gpu, run_orc, tier_batches, tier_classes,
                                tier_radii)
from test_gpu_stacked import MAX_CAND, around_rays, dup_patches

pytestmark = pytest.mark.gpu

CAPS = (64, 192, 1024)
OPS = ("intersect", "chain1", "chain3")
SEGMENTS = {"intersect": 1, "chain1": 2, "chain3": 6}  # run_segment calls per chunk: two per lens, whatever is alive
ILLUM_RAYS, ILLUM_CAP = 10_000, 4096


def chunk_count(n, cap):
    return -(-n // chunk_rule(n, cap))


def set_cap(bzr, c, rays):
    eff = ctypes.c_uint32(0)
    assert bzr.lib().bzr_debug_chunk_cap(c.handle, rays, ctypes.byref(eff)) == 0
    return eff.value


def timed(c, call):
    """(call's result, {kernel: launches})."""
    c.timing(True)
    c.timing_report()
    try:
        out = call()
        rep = c.timing_report()
    finally:
        c.timing(False)
    return out, {k: v[1] for k, v in rep.items()}


def counted(c, call):
    c.counters(True)
    c.counters_report()
    try:
        out = call()
        rep = c.counters_report()
    finally:
        c.counters(False)
    return out, rep


def chunked(bzr, c, cap, call, n, segments, ctxs=None):
    """`call` under a cap of `cap` rays, after proving through the k_traverse launches that it ran
    chunk_count(n, cap) chunks of `segments` segments each.  Returns (result, chunks)."""
    for x in ctxs or [c]:
        assert set_cap(bzr, x, cap) == cap
    out, launches = timed(c, call)
    k = chunk_count(n, cap)
    assert launches.get("k_traverse", 0) == k * segments and "k_trace" not in launches, (cap, n, k, segments, launches)
    return out, k


def same(got, want, label):
    bad = differing(got, want)
    assert not bad.any(), f"{label}: {int(bad.sum())} of {len(bad)} rays differ, first {np.nonzero(bad)[0][:8]}"


def sweep(bzr, c, call, n, segments, want, label, caps=CAPS):
    """`call` on the automatic cap and on every cap that splits n rays: each equals the oracle's words `want` and the
    automatic-cap run.  Returns {cap: chunks}."""
    assert set_cap(bzr, c, 0) >= 1 << 14
    auto, launches = timed(c, call)
    assert launches.get("k_traverse", 0) == segments, (label, launches)
    same(auto, want, f"{label}, automatic cap: vs the oracle")
    ran = {}
    for cap in caps:
        if chunk_count(n, cap) < 2:
            continue
        got, ran[cap] = chunked(bzr, c, cap, call, n, segments)
        same(got, want, f"{label}, cap {cap} ({ran[cap]} chunks): vs the oracle")
        same(got, auto, f"{label}, cap {cap} ({ran[cap]} chunks): vs the automatic cap")
    print(label, "chunks per cap", ran)
    assert ran and all(2 <= k <= 224 for k in ran.values())
    return ran


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def cctx(bzr, ctx):
    c = bzr.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def automatic_cap(bzr, cctx):
    yield
    set_cap(bzr, cctx, 0)


@pytest.fixture(scope="module")
def lenses(orc):
    return [lens_patches(orc, k) for k in range(3)]


@pytest.fixture(scope="module")
def dms(bzr, cctx, lenses):
    return [bzr.DeviceMesh(cctx, p) for p in lenses]


@pytest.fixture(scope="module")
def radii(bzr, lenses):
    return tier_radii(bzr, lenses[0])


@pytest.fixture(scope="module")
def seam(orc, lenses, radii):
    """The first 4 097 rays of test_gpu_ray_edges' clean batch (the 4 096 grid rays and one incoherent ray) with the
    oracle's words per op; the oracle treats every ray on its own, so a prefix's words are the prefix of these."""
    rays = np.ascontiguousarray(clean_batch(lenses[0], radii[0])[:, :4097])
    want = {op: run_orc(orc, lenses, op, rays)[0] for op in OPS}
    assert (want["intersect"][0][11] == 4).sum() > 1000 and (want["chain3"][2] == 6).sum() > 500
    return rays, want


# ------------------------------------------------------------------ the hook itself
def test_the_hook_only_lowers_the_cap(bzr, cctx):
    auto = set_cap(bzr, cctx, 0)
    assert auto % 64 == 0 and 1 << 14 <= auto <= 1 << 23
    for rays, want in ((1, 64), (63, 64), (64, 64), (127, 64), (200, 192), (1024, 1024), (4097, 4096),
                       (auto, auto), (auto + 64, auto), (2 ** 32 - 1, auto)):
        assert set_cap(bzr, cctx, rays) == want, rays
    assert set_cap(bzr, cctx, 0) == auto
    assert bzr.lib().bzr_debug_chunk_cap(cctx.handle, 192, None) == 0 and set_cap(bzr, cctx, 0) == auto
    assert bzr.lib().bzr_debug_chunk_cap(None, 192, None) == 1


# ------------------------------------------------------------------ seams and ragged tails
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("n", [65, 129, 1000, 4097])
def test_seams_and_ragged_tails(bzr, cctx, dms, seam, n, op):
    """65 = a last chunk of one ray; 129 at cap 64 = three chunks 64 + 64 + 1; 1000 and 4097: ragged tails that are no
    whole wave."""
    rays, want = seam
    part = np.ascontiguousarray(rays[:, :n])
    ran = sweep(bzr, cctx, lambda: run_gpu(bzr, cctx, dms, op, part, bzr.PIPELINE_STAGED), n, SEGMENTS[op],
                [w[..., :n] for w in want[op]], f"{op} n {n}")
    assert 64 in ran and (n < 1024 or len(ran) == 3)


def test_restoring_the_automatic_cap(bzr, cctx, dms, seam):
    rays, want = seam
    call = lambda: run_gpu(bzr, cctx, dms, "chain3", rays, bzr.PIPELINE_STAGED)  # noqa: E731
    chunked(bzr, cctx, 64, call, 4097, 6)
    assert bzr.lib().bzr_debug_chunk_cap(cctx.handle, 0, None) == 0
    got, launches = timed(cctx, call)
    assert launches["k_traverse"] == 6, launches
    same(got, want["chain3"], "after the restore")


# ------------------------------------------------------------------ overflow list per chunk
@pytest.fixture(scope="module")
def dup(bzr, orc, cctx):
    """test_gpu_stacked's "dup" mesh under its 1 024 grid rays (gate passes 0, 40, 41, 42, 80 .. 168) followed by the
    1 024 around_rays."""
    from bzr_amd.configs import CONFIGS, grid_rays

    patches = dup_patches(orc)
    rays = np.ascontiguousarray(np.concatenate([grid_rays(CONFIGS["cfg1"], side=32), around_rays()], axis=1))
    gate = orc.planar_gate(patches, rays).sum(axis=1)
    want = {"intersect": [bits(orc.intersect(patches, rays))],
            "chain1": [bits(a) for a in orc.trace_chain([patches], [1.3], rays)]}
    return bzr.DeviceMesh(cctx, patches), rays, gate, want


def test_overflow_list_per_chunk(bzr, cctx, dup):
    dm, rays, gate, want = dup
    n, over = rays.shape[1], int((gate > MAX_CAND).sum())
    for g in (0, MAX_CAND, MAX_CAND + 1, MAX_CAND + 2):
        assert (gate == g).sum() >= 10, g
    assert over > 400 and (gate >= 2 * MAX_CAND).sum() > 100
    waves = gate.reshape(-1, 64)
    assert ((waves <= MAX_CAND).any(1) & (waves > MAX_CAND).any(1)).sum() >= 4  # listed and overflowed rays share chunks
    calls = {"intersect": lambda: [bits(bzr.intersect(cctx, dm, rays, mode=bzr.PIPELINE_STAGED))],
             "chain1": lambda: [bits(a) for a in bzr.trace_chain(cctx, [dm], [1.3], rays, mode=bzr.PIPELINE_STAGED)]}
    for op, call in calls.items():
        sweep(bzr, cctx, call, n, SEGMENTS[op], want[op], f"dup {op}")
        set_cap(bzr, cctx, 0)
        _, auto = counted(cctx, call)
        if op == "intersect":
            assert auto["overflow_rays"] == over and auto["segments"] == n
        for cap in CAPS:
            assert set_cap(bzr, cctx, cap) == cap
            got, rep = counted(cctx, call)
            print("dup", op, "cap", cap, rep)
            same(got, want[op], f"dup {op} cap {cap} with counters")
            for k in ("overflow_rays", "segments", "pairs", "follows"):
                assert rep[k] == auto[k], (op, cap, k, rep, auto)


# ------------------------------------------------------------------ far origins in every wave
@pytest.fixture(scope="module")
def tier_mix(orc, lenses, radii):
    _, mix, _ = tier_batches(lenses[0], tier_classes(*radii))
    beyond = np.abs(mix[:3]).max(axis=0) > radii[1]
    assert beyond.reshape(-1, 64).any(1).all() and not beyond.reshape(-1, 64).all(1).any()
    return mix, int(beyond.sum()), {op: run_orc(orc, lenses, op, mix)[0] for op in OPS}


@pytest.mark.parametrize("op", OPS)
def test_far_origins_in_every_wave(bzr, cctx, dms, tier_mix, op):
    """Origins beyond s_max take the overflow list from k_traverse itself, so every chunk, of one wave even, writes
    w.ovf and runs k_finish_ovf.  In a chain only the first segment starts that far out (later origins lie on a lens)."""
    mix, beyond, want = tier_mix
    n = mix.shape[1]
    call = lambda: run_gpu(bzr, cctx, dms, op, mix, bzr.PIPELINE_STAGED)  # noqa: E731
    sweep(bzr, cctx, call, n, SEGMENTS[op], want[op], f"tier_mix {op}")
    for cap in (0,) + CAPS:
        assert set_cap(bzr, cctx, cap) >= cap
        got, rep = counted(cctx, call)
        same(got, want[op], f"tier_mix {op} cap {cap} with counters")
        assert rep["overflow_rays"] == beyond > 1000, (op, cap, rep, beyond)


# ------------------------------------------------------------------ garbage lanes
@pytest.mark.parametrize("op", ["intersect", "chain1"])
def test_garbage_lanes(bzr, orc, cctx, dms, lenses, radii, op):
    clean = clean_batch(lenses[0], radii[0])
    batch, mask = poisoned(clean, "third")
    bad = ~np.isfinite(batch).all(axis=0)
    assert bad.sum() > 1000 and not bad[~mask].any()
    n = batch.shape[1]
    want = run_orc(orc, lenses, op, batch)[0]
    set_cap(bzr, cctx, 0)
    clean_run = run_gpu(bzr, cctx, dms, op, clean, bzr.PIPELINE_STAGED)
    for cap in CAPS:
        got, k = chunked(bzr, cctx, cap, lambda: run_gpu(bzr, cctx, dms, op, batch, bzr.PIPELINE_STAGED), n, SEGMENTS[op])
        same([g[..., ~mask] for g in got], [c[..., ~mask] for c in clean_run], f"third {op} cap {cap}: clean lanes")
        same(got, want, f"third {op} cap {cap} ({k} chunks): vs the oracle")


# ------------------------------------------------------------------ lens switches across seams
@pytest.mark.parametrize("name", ["n8", "big3"])
def test_lens_switches_across_seams(bzr, orc, cctx, table, sets, name):
    """16 segments per chunk; in big3 the histogram grows from 433 to 3 073 slots and shrinks again inside every chunk
    (the small scan clears what it reads, hipCUB's does not: ctx->zero_hn), and the next chunk starts on 433 again."""
    idx, ri = sets[name]
    rays = chain_rays()
    want = [bits(a) for a in orc.trace_chain([table[k] for k in idx], ri, rays, threads=16)]
    assert (want[2] == 16).sum() > 500
    ls = [bzr.DeviceMesh(cctx, table[k]) for k in idx]
    call = lambda: [bits(a) for a in bzr.trace_chain(cctx, ls, ri, rays, mode=bzr.PIPELINE_STAGED)]  # noqa: E731
    assert sweep(bzr, cctx, call, rays.shape[1], 16, want, name, caps=(192, 1024)) == {192: 22, 1024: 4}


# ------------------------------------------------------------------ per-ray expected
def test_refract_with_per_ray_expected(bzr, orc, cctx, dms, lenses):
    """test_gpu_ray_edges' recipe: expected 0..3 lane by lane, on the front and on the back surface."""
    front = chain_rays()
    back, st1 = orc.refract(lenses[0], 1.3, front, np.full(front.shape[1], bzr.RR_INSIDE, np.uint32))
    exp = np.random.default_rng(9).integers(0, 4, front.shape[1]).astype(np.uint32)
    assert all((exp.reshape(-1, 64) == e).any(1).all() for e in range(4))
    assert not np.array_equal(exp[:192], exp[192:384])  # a chunk that read expected[i] for expected[off + i] shows
    for label, rays in (("front", front), ("back", back)):
        w_rays, w_st = orc.refract(lenses[0], 1.3, rays, exp)
        assert len(np.unique(w_st)) >= 2
        call = lambda: [bits(a) for a in bzr.refract(cctx, dms[0], 1.3, rays, exp, mode=bzr.PIPELINE_STAGED)]  # noqa: E731
        sweep(bzr, cctx, call, rays.shape[1], 1, [bits(w_rays), bits(w_st)], f"refract {label}")


# ------------------------------------------------------------------ buffer forms
@pytest.mark.parametrize("cap", [192, 1024])
def test_buffer_forms(bzr, cctx, dms, seam, cap):
    torch = pytest.importorskip("torch")
    rays, want = seam
    n = rays.shape[1]
    staged = bzr.PIPELINE_STAGED
    aos = np.ascontiguousarray(rays.T)
    dev = torch.from_numpy(rays).cuda()
    dev_aos = torch.from_numpy(aos).cuda()

    def host_of(ts):
        torch.cuda.synchronize()
        return [bits(t.cpu().numpy()) for t in ts]

    rows, _ = chunked(bzr, cctx, cap, lambda: bits(bzr.intersect(cctx, dms[0], rays, mode=staged)), n, 1)
    assert np.array_equal(rows, want["intersect"][0])
    forms = {"device": lambda: host_of([bzr.intersect(cctx, dms[0], dev, mode=staged)])[0],
             "aos": lambda: bits(bzr.intersect(cctx, dms[0], aos, mode=staged | bzr.RAYS_AOS)),
             "device aos": lambda: host_of([bzr.intersect(cctx, dms[0], dev_aos, mode=staged | bzr.RAYS_AOS)])[0]}
    for label, call in forms.items():
        got, _ = chunked(bzr, cctx, cap, call, n, 1)
        assert np.array_equal(got, rows), f"intersect, {label}"
    records = {"records": lambda: [bits(a) for a in bzr.intersect_records(cctx, dms[0], rays, mode=staged)],
               "records aos": lambda: [bits(a) for a in bzr.intersect_records(cctx, dms[0], aos, mode=staged | bzr.RAYS_AOS)],
               "records device": lambda: host_of(bzr.intersect_records(cctx, dms[0], dev, mode=staged))}
    for label, call in records.items():
        (rec, patch), _ = chunked(bzr, cctx, cap, call, n, 1)
        assert np.array_equal(rec[:, 0], (rows[11] == bzr.WHAT_INTERSECT).astype(np.uint32)), label
        assert np.array_equal(rec[:, 1:5], rows[1:5].T) and np.array_equal(rec[:, 5], rows[0]), label
        assert np.array_equal(rec[:, 6:12], rows[5:11].T) and np.array_equal(rec[:, 12], rows[11]), label
        assert np.array_equal(patch, rows[12]), label
    chain, _ = chunked(bzr, cctx, cap, lambda: run_gpu(bzr, cctx, dms, "chain3", rays, staged), n, 6)
    same(chain, want["chain3"], "chain3, host pointers")
    chains = {"device": lambda: host_of(bzr.trace_chain(cctx, dms, RI3, dev, mode=staged)),
              "aos": lambda: [bits(a) for a in bzr.trace_chain(cctx, dms, RI3, aos, mode=staged | bzr.RAYS_AOS)],
              "device aos": lambda: host_of(bzr.trace_chain(cctx, dms, RI3, dev_aos, mode=staged | bzr.RAYS_AOS))}
    for label, call in chains.items():
        got, _ = chunked(bzr, cctx, cap, call, n, 6)
        if "aos" in label:
            got[0] = np.ascontiguousarray(got[0].T)
        same(got, chain, f"chain3, {label}")


# ------------------------------------------------------------------ tiled
def test_tiled_over_two_capped_contexts(bzr, cctx, dms, lenses, seam):
    rays, want = seam
    rays, want = np.ascontiguousarray(rays[:, :4096]), [w[..., :4096] for w in want["chain3"]]
    ctxs = [bzr.Context(0) for _ in range(2)]
    per = [[bzr.DeviceMesh(c, p) for p in lenses] for c in ctxs]
    cap, tile = 192, 1000
    share = [sum(min(tile, 4096 - k * tile) for k in range(d, 5, 2)) for d in range(2)]
    assert share == [2096, 2000]
    for c in ctxs:
        assert set_cap(bzr, c, cap) == cap
        c.timing(True)
        c.timing_report()
    got = [bits(a) for a in bzr.trace_tiled(ctxs, per, RI3, rays, tile_rays=tile, mode=bzr.PIPELINE_STAGED)]
    for c, m in zip(ctxs, share):
        launches = c.timing_report()
        c.timing(False)
        assert launches["k_traverse"][1] == chunk_count(m, cap) * 6 and "k_trace" not in launches, (m, launches)
    single, _ = chunked(bzr, cctx, cap, lambda: run_gpu(bzr, cctx, dms, "chain3", rays, bzr.PIPELINE_STAGED), 4096, 6)
    same(got, single, "tiled vs the single context")
    same(got, want, "tiled vs the oracle")


# ------------------------------------------------------------------ illuminate
def culled_by_sphere(sphere, rays):
    """tests/test_gpu_illumination.py's float64 predicate."""
    c = sphere.astype(np.float64)
    oc = rays[:3].astype(np.float64) - c[:3, None]
    cc = (oc * oc).sum(0) - c[3] ** 2
    b = (oc * rays[3:].astype(np.float64)).sum(0)
    return (cc > 0) & ((b >= 0) | (b * b - cc < 0))


@pytest.fixture(scope="module")
def illum(orc, lenses):
    """(lens count, emitter x) -> the oracle's (rays, hist, exited, landed) over all 10 000 emitted rays."""
    out = {}
    for nl in (1, 3):
        for x in (0.0, -60.0):
            rays, _, seg, hist, exited, landed = oracle_illuminate(orc, lenses[:nl], RI3[:nl], emitter(orc, x=x),
                                                                   ILLUM_RAYS, target(orc))
            assert exited > 0 and hist.sum() == landed
            if x == 0.0:
                assert landed > 20 and (seg == 2 * nl).sum() > 100
            out[(nl, x)] = (rays, hist, exited, landed)
    return out


def illum_launches(bzr, nl, mode, batches):
    """The automatic choice (trace.hip use_staged) takes a batch of 3 392 rays over 432 patches staged."""
    if mode == bzr.PIPELINE_FUSED:
        return {"k_trace": batches}
    return {"k_traverse": batches * 2 * nl}


@pytest.mark.parametrize("x", [0.0, -60.0])
@pytest.mark.parametrize("nl", [1, 3])
def test_illuminate_in_three_batches(bzr, cctx, dms, illum, nl, x):
    """10 000 rays at a cap of 4 096: batches of 3 392 + 3 392 + 3 216 rays, the last no whole number of waves, with
    ld = 3 392 throughout; x = -60: most rays culled, so alive_in decides."""
    torch = pytest.importorskip("torch")
    assert chunk_rule(ILLUM_RAYS, ILLUM_CAP) == 3392 and ILLUM_RAYS - 2 * 3392 == 3216
    rays, w_hist, exited, landed = illum[(nl, x)]
    culled = int(culled_by_sphere(bzr.bounding_sphere(dms[0]), rays).sum())
    assert 0 < culled < ILLUM_RAYS and (x == 0.0 or culled > ILLUM_RAYS // 2)
    want_stats = {"emitted": ILLUM_RAYS, "culled": culled, "exited": exited, "landed": landed}
    em, tg = emitter(bzr, x=x), target(bzr)
    for mode in (bzr.PIPELINE_STAGED, bzr.PIPELINE_FUSED, 0):
        label = f"{nl} lenses, x {x}, mode {mode}"
        set_cap(bzr, cctx, 0)
        (hist, stats), launches = timed(cctx, lambda: bzr.illuminate(cctx, dms[:nl], RI3[:nl], em, ILLUM_RAYS, tg, mode=mode))
        assert {k: v for k, v in launches.items() if k in ("k_traverse", "k_trace")} == illum_launches(bzr, nl, mode, 1)
        assert stats == want_stats and np.array_equal(hist, w_hist), f"{label}, one batch"
        assert set_cap(bzr, cctx, ILLUM_CAP) == ILLUM_CAP
        (hist, stats), launches = timed(cctx, lambda: bzr.illuminate(cctx, dms[:nl], RI3[:nl], em, ILLUM_RAYS, tg, mode=mode))
        assert {k: v for k, v in launches.items() if k in ("k_traverse", "k_trace")} == illum_launches(bzr, nl, mode, 3)
        assert stats == want_stats, (label, stats, want_stats)
        assert np.array_equal(hist, w_hist), label
        # a second call into the same hist doubles every cell
        _, again = bzr.illuminate(cctx, dms[:nl], RI3[:nl], em, ILLUM_RAYS, tg, hist=hist, mode=mode)
        assert again == want_stats and np.array_equal(hist, 2 * w_hist), label
        # hist in device memory
        d_hist = torch.zeros(w_hist.shape, dtype=torch.int32, device="cuda")
        for times in (1, 2):
            _, d_stats = bzr.illuminate(cctx, dms[:nl], RI3[:nl], em, ILLUM_RAYS, tg, hist=d_hist, mode=mode)
            torch.cuda.synchronize()
            assert d_stats == want_stats and np.array_equal(d_hist.cpu().numpy().view(np.uint32), times * w_hist), label
        # no rays: hist untouched, all four stats zero
        full = np.full(w_hist.shape, 0xA5A5A5A5, np.uint32)
        _, none = bzr.illuminate(cctx, dms[:nl], RI3[:nl], em, 0, tg, hist=full, mode=mode)
        assert (full == 0xA5A5A5A5).all() and none == dict.fromkeys(want_stats, 0), label
        d_full = torch.full(w_hist.shape, 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        _, none = bzr.illuminate(cctx, dms[:nl], RI3[:nl], em, 0, tg, hist=d_full, mode=mode)
        torch.cuda.synchronize()
        assert bool((d_full == 0x5A5A5A5A).all()) and none == dict.fromkeys(want_stats, 0), label


# ------------------------------------------------------------------ FAST
def test_fast_intersect_chunked_against_float64(bzr, orc, cctx):
    """test_gpu_fast_ref64's "origin" mesh case, staged, at a cap of 192: the same bars against binary64.  (Chunked
    FAST is not promised bit-equal to unchunked FAST: pairs move between k_newton and k_newton_lane.)"""
    patches = ref64.lens_set(orc)["origin"][0]
    s_max = tier_radii(bzr, patches)[1]
    rays = mesh_rays(patches, s_max, 700)
    n = rays.shape[1]
    gate = orc.planar_gate(patches, rays, threads=16)
    want = orc.intersect(patches, rays, threads=16)
    ref = ref64.intersect64(patches, rays, gate)
    dm = bzr.DeviceMesh(cctx, patches)
    mode = bzr.PIPELINE_STAGED | bzr.MODE_FAST
    (fast, rep), k = chunked(bzr, cctx, 192, lambda: counted(cctx, lambda: bzr.intersect(cctx, dm, rays, mode=mode)), n, 1)
    assert k == 22
    fu, wu = bits(fast), bits(want)
    none = ~gate.any(axis=1)
    assert none.sum() > 100 and np.array_equal(fu[:, none], wu[:, none])
    assert rep["overflow_rays"] == int((np.abs(rays[:3]).max(axis=0) > s_max).sum()) >= 40
    well = ref.well
    assert well.sum() >= 500
    hit = lambda u: (u[11, well] == bzr.WHAT_INTERSECT) & (u[12, well] == ref.patch[well])  # noqa: E731
    assert float(hit(fu).mean()) >= float(hit(wu).mean()) - CLASS_ALLOW
    both = well.copy()
    both[well] = hit(wu) & hit(fu)
    assert_bars("intersect origin staged cap 192", fast, want, ref, both, ref64.mesh_span(patches))


def test_fast_chain_chunked(bzr, orc, cctx, dms, lenses):
    rays = chain_rays()
    want = orc.trace_chain(lenses, RI3, rays, threads=16)
    mode = bzr.PIPELINE_STAGED | bzr.MODE_FAST
    got, k = chunked(bzr, cctx, 192, lambda: bzr.trace_chain(cctx, dms, RI3, rays, mode=mode), rays.shape[1], 6)
    assert k == 22
    assert_chain_gates("three432 staged FAST cap 192", got, want)


@pytest.mark.parametrize("pipe", ["staged", "fused"])
def test_fast_illuminate(bzr, cctx, dms, illum, pipe):
    """FAST may change a ray's status where the chain gates allow it, 1 - STATUS_AGREE of the rays at the most, and a
    ray whose status changes moves `exited` and `landed` by at most one each."""
    rays, w_hist, exited, landed = illum[(3, 0.0)]
    mode = (bzr.PIPELINE_STAGED if pipe == "staged" else bzr.PIPELINE_FUSED) | bzr.MODE_FAST
    assert set_cap(bzr, cctx, ILLUM_CAP) == ILLUM_CAP
    (hist, stats), launches = timed(cctx, lambda: bzr.illuminate(cctx, dms, RI3, emitter(bzr), ILLUM_RAYS, target(bzr), mode=mode))
    assert launches.get("k_traverse", 0) == (18 if pipe == "staged" else 0)
    assert launches.get("k_trace", 0) == (0 if pipe == "staged" else 3)
    allow = (1.0 - STATUS_AGREE) * ILLUM_RAYS
    print(pipe, "FAST illuminate", stats, "oracle exited", exited, "landed", landed, "allowed difference", allow)
    assert stats["emitted"] == ILLUM_RAYS
    assert stats["culled"] == int(culled_by_sphere(bzr.bounding_sphere(dms[0]), rays).sum())
    assert abs(stats["exited"] - exited) <= allow and abs(stats["landed"] - landed) <= allow
    assert hist.sum() == stats["landed"]
