"""k_trace's short passes (trace.hip BZR_TRACE_SHORT): a Newton pass none of whose lanes can win skips the last
iteration's surface normal, after a wave-uniform vote that takes the decision consider() takes.  No output bit may
depend on it, so every case here runs the fused pipeline with the work counters on and asserts three things:

  * every output word equals the oracle's;
  * `pairs` and `follows` equal the oracle's Newton runs and follow-side retries (the schedule -- which pass runs a
    (lane, patch, limit), and since the near-first order which pass runs first -- never changes the work);
  * 0 < short_passes <= newton_rounds, unless the case says otherwise.

The cases put the vote where it could go wrong: waves whose lanes disagree about the candidates (the lens rim; lanes
that start inside the lens beside lanes that start outside, where the far patch loses on one lane and wins on its
neighbour), the other half of the patch indices on the near side (rays along -x), exact ties that only the scanned
index decides (the vote must compare the whole key), NaN lanes, the 13-word intersect kernel and FAST mode.

The cfg2 chain also gets a lower bound: a wave in which the oracle's gate gives all 64 rays the same two patches in
segment 0, both results INTERSECT, runs two passes there, and the second, every lane of which loses, must be short.
At 128 x 128 no wave is that uniform (the 8 x 8-ray tiles are wider than the patches); the grid was enlarged as far as
512 x 512, where 102 waves are, and that size carries the bound.
"""
import numpy as np
import pytest

from bzr_amd.configs import CONFIGS, build_lens, grid_rays
from test_gpu_fast import HIT_AGREE, SAME_PATCH
from test_gpu_stacked import dup_patches, shell_patches, around_rays

pytestmark = pytest.mark.gpu

BOUND_SIDE, BOUND_WAVES = 512, 100


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def counted(ctx, call):
    ctx.counters(True)
    ctx.counters_report()
    got = call()
    rep = ctx.counters_report()
    ctx.counters(False)
    return got, rep


def oracle_counted(orc, call):
    orc.counters_reset()
    want = call()
    return want, orc.counters()


def assert_work(rep, work, label, short_min=1):
    print(label, rep, "oracle", work)
    assert rep["overflow_rays"] == 0, label
    assert rep["pairs"] == work["newton"], label
    assert rep["follows"] == work["follow"], label
    assert short_min <= rep["short_passes"] <= rep["newton_rounds"], label


def assert_chain(got, want, label):
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), f"{label}: status / segments"
    bad = (bits(got[0]) != bits(want[0])).any(axis=0)
    assert not bad.any(), f"{label}: {int(bad.sum())} of {len(bad)} rays differ"


def uniform_two_patch_waves(orc, patches, rays):
    """Waves (64 consecutive rays) in which the oracle's planar gate gives every ray the same two patches and both
    BezierTriangle::intersect results are INTERSECT on every ray.  The corner lanes of each 8 x 8 tile are gated
    first, so the full gate runs on the few waves that can still qualify."""
    n = rays.shape[1]
    corners = (np.arange(0, n, 64)[:, None] + np.array([0, 7, 56, 63])[None, :]).reshape(-1)
    g = orc.planar_gate(patches, rays[:, corners])
    two = (g.sum(axis=1) == 2).reshape(-1, 4).all(axis=1)
    same = (g.reshape(-1, 4, len(patches)) == g.reshape(-1, 4, len(patches))[:, :1]).all(axis=(1, 2))
    count = 0
    for w in np.nonzero(two & same)[0]:
        idx = np.arange(64 * w, 64 * w + 64)
        gw = orc.planar_gate(patches, rays[:, idx])
        if not ((gw.sum(axis=1) == 2).all() and (gw == gw[:1]).all()):
            continue
        pair = np.nonzero(gw[0])[0]
        hits = [bits(orc.patch_intersect(patches, np.full(64, p), np.zeros(64, int), rays[:, idx])) for p in pair]
        count += int(all((h[11] == 4).all() for h in hits))
    return count


@pytest.fixture(scope="module")
def lens2(bzr):
    return build_lens(bzr.TriMesh, CONFIGS["cfg2"].lenses[0]).bezier_patches()


@pytest.fixture(scope="module")
def mesh2(bzr, ctx, lens2):
    return bzr.DeviceMesh(ctx, lens2)


@pytest.fixture(scope="module")
def chain128(orc, lens2):
    """The cfg2 chain at 128 x 128: rays, the oracle's result and work (shared; never changed)."""
    rays = grid_rays(CONFIGS["cfg2"], side=128)
    want, work = oracle_counted(orc, lambda: orc.trace_chain([lens2], [1.3], rays))
    for a in (rays, *want):
        a.setflags(write=False)
    return rays, want, work


def test_cfg2_chain_with_rim_waves(bzr, orc, ctx, lens2, mesh2, chain128):
    rays, want, work = chain128
    gate = orc.planar_gate(lens2, rays).sum(axis=1).reshape(-1, 64)
    rim = ((gate == 0).any(axis=1) & (gate >= 2).any(axis=1)).sum()
    assert rim >= 40, rim  # rim waves: lanes without a candidate beside lanes with two and more (up to 16)
    got, rep = counted(ctx, lambda: bzr.trace_chain(ctx, [mesh2], [1.3], rays, mode=bzr.PIPELINE_FUSED))
    assert_chain(got, want, "cfg2 128")
    assert_work(rep, work, "cfg2 128", short_min=max(1, uniform_two_patch_waves(orc, lens2, rays)))


def test_cfg2_chain_lower_bound(bzr, orc, ctx, lens2, mesh2):
    rays = grid_rays(CONFIGS["cfg2"], side=BOUND_SIDE)
    bound = uniform_two_patch_waves(orc, lens2, rays)
    print(f"cfg2 {BOUND_SIDE}: {bound} waves with the same two intersecting patches on all 64 rays")
    assert bound >= BOUND_WAVES
    want, work = oracle_counted(orc, lambda: orc.trace_chain([lens2], [1.3], rays))
    got, rep = counted(ctx, lambda: bzr.trace_chain(ctx, [mesh2], [1.3], rays, mode=bzr.PIPELINE_FUSED))
    assert_chain(got, want, f"cfg2 {BOUND_SIDE}")
    assert_work(rep, work, f"cfg2 {BOUND_SIDE}", short_min=bound)


def test_cfg4_two_lens_chain(bzr, orc, ctx):
    cfg = CONFIGS["cfg4"]
    lenses = [build_lens(bzr.TriMesh, l).bezier_patches() for l in cfg.lenses]
    ri = [l.ri for l in cfg.lenses]
    rays = grid_rays(cfg, side=96)
    want, work = oracle_counted(orc, lambda: orc.trace_chain(lenses, ri, rays))
    assert (want[2] == 4).sum() > 1000  # rays through both lenses
    meshes = [bzr.DeviceMesh(ctx, p) for p in lenses]
    got, rep = counted(ctx, lambda: bzr.trace_chain(ctx, meshes, ri, rays, mode=bzr.PIPELINE_FUSED))
    assert_chain(got, want, "cfg4 96")
    assert_work(rep, work, "cfg4 96")


def test_intersect_keeps_the_winners_whole(bzr, orc, ctx):
    """bzr_intersect (kModeHits) on the cfg1 sphere from outside: all 13 words -- the winners' normal, cosine and
    barycentrics are those of a whole evaluation."""
    cfg = CONFIGS["cfg1"]
    patches = build_lens(bzr.TriMesh, cfg.lenses[0]).bezier_patches()
    rays = grid_rays(cfg, side=64)
    want, work = oracle_counted(orc, lambda: bits(orc.intersect(patches, rays)))
    hit = want[11] == bzr.WHAT_INTERSECT
    assert hit.sum() > 500 and (want[8:11][:, hit] != 0).any(axis=0).all()
    mesh = bzr.DeviceMesh(ctx, patches)
    got, rep = counted(ctx, lambda: bits(bzr.intersect(ctx, mesh, rays, mode=bzr.PIPELINE_FUSED)))
    bad = (got != want).any(axis=0)
    assert not bad.any(), f"{int(bad.sum())} rays differ, rows {np.nonzero((got != want).any(axis=1))[0]}"
    assert_work(rep, work, "cfg1 intersect 64")


def test_rays_from_the_other_side(bzr, orc, ctx, lens2, mesh2):
    """Along -x from x = 20: the near side is now the other half of the patch indices."""
    rays = grid_rays(CONFIGS["cfg2"], side=96).copy()
    rays[0], rays[3] = 20.0, -1.0
    fwd = bits(orc.intersect(lens2, grid_rays(CONFIGS["cfg2"], side=96)))
    back = bits(orc.intersect(lens2, rays))
    both = (fwd[11] == 4) & (back[11] == 4)
    assert both.sum() > 3000 and (fwd[12][both] != back[12][both]).mean() > 0.99  # other winners than along +x
    want, work = oracle_counted(orc, lambda: orc.trace_chain([lens2], [1.3], rays))
    assert (want[2] == 2).sum() > 3000
    got, rep = counted(ctx, lambda: bzr.trace_chain(ctx, [mesh2], [1.3], rays, mode=bzr.PIPELINE_FUSED))
    assert_chain(got, want, "cfg2 along -x")
    assert_work(rep, work, "cfg2 along -x")
    hits, rep = counted(ctx, lambda: bits(bzr.intersect(ctx, mesh2, rays, mode=bzr.PIPELINE_FUSED)))
    assert np.array_equal(hits, back)
    assert 1 <= rep["short_passes"] <= rep["newton_rounds"]


def test_lanes_with_different_candidate_counts(bzr, orc, ctx, lens2, mesh2):
    """Even lanes start outside the lens (two candidates: the far patch loses), odd lanes inside it at x = 10 (one
    candidate: the far patch wins).  The far patch's pass must take the full path: the odd lanes' words -- normal and
    cosine among them -- are the point.  (No lower bound on the short passes: the waves that decide this case have
    none.)"""
    rays = grid_rays(CONFIGS["cfg2"], side=64).copy()
    odd = np.arange(rays.shape[1]) % 2 == 1
    rays[0, odd] = 10.0
    want, work = oracle_counted(orc, lambda: bits(orc.intersect(lens2, rays)))
    gate = orc.planar_gate(lens2, rays).sum(axis=1)
    hit = want[11] == bzr.WHAT_INTERSECT
    mixed = ((gate.reshape(-1, 64)[:, 0::2] == 2).all(axis=1) & (gate.reshape(-1, 64)[:, 1::2] == 1).all(axis=1)
             & hit.reshape(-1, 64).all(axis=1))
    assert mixed.sum() >= 20, mixed.sum()  # whole waves of the pattern
    inside = odd & hit & (gate == 1)
    assert inside.sum() > 1000 and (want[8:11][:, inside] != 0).any(axis=0).all()
    got, rep = counted(ctx, lambda: bits(bzr.intersect(ctx, mesh2, rays, mode=bzr.PIPELINE_FUSED)))
    bad = (got != want).any(axis=0)
    assert not bad[inside].any(), f"{int(bad[inside].sum())} inside lanes differ"
    assert not bad.any(), f"{int(bad.sum())} rays differ"
    assert_work(rep, work, "mixed candidate counts", short_min=0)
    cwant, cwork = oracle_counted(orc, lambda: orc.trace_chain([lens2], [1.3], rays))
    cgot, crep = counted(ctx, lambda: bzr.trace_chain(ctx, [mesh2], [1.3], rays, mode=bzr.PIPELINE_FUSED))
    assert_chain(cgot, cwant, "mixed candidate counts, chain")
    assert_work(crep, cwork, "mixed candidate counts, chain", short_min=0)


@pytest.mark.parametrize("name", ["dup", "shells"])
def test_exact_ties_and_near_ties(bzr, orc, ctx, name):
    """tests/test_gpu_stacked.py's meshes.  dup: every hit is a 20- or 21-way exact tie in t that the first copy must
    win, so a vote on t alone would call later copies possible winners or earlier ones impossible; shells: 24 keys per
    crossing a step of 2^-8 apart.  short_passes > 0 is asserted on the shells only."""
    grid = grid_rays(CONFIGS["cfg1"], side=32)
    if name == "dup":
        patches, rays = dup_patches(orc), grid
    else:
        patches = shell_patches(orc, 2.0 ** -8)
        rays = np.ascontiguousarray(np.concatenate([grid, around_rays()], axis=1))
    want, work = oracle_counted(orc, lambda: bits(orc.intersect(patches, rays)))
    hit = want[11] == bzr.WHAT_INTERSECT
    assert hit.sum() > 300
    if name == "dup":
        assert (want[12][hit] < 126).all()  # the first copy wins every tie
    mesh = bzr.DeviceMesh(ctx, patches)
    got, rep = counted(ctx, lambda: bits(bzr.intersect(ctx, mesh, rays, mode=bzr.PIPELINE_FUSED)))
    bad = (got != want).any(axis=0)
    assert not bad.any(), f"{name}: {int(bad.sum())} rays differ, patch got {got[12][bad][:8]} want {want[12][bad][:8]}"
    assert_work(rep, work, name, short_min=1 if name == "shells" else 0)
    cwant, cwork = oracle_counted(orc, lambda: orc.trace_chain([patches], [1.3], rays))
    cgot, crep = counted(ctx, lambda: bzr.trace_chain(ctx, [mesh], [1.3], rays, mode=bzr.PIPELINE_FUSED))
    assert_chain(cgot, cwant, f"{name} chain")
    assert_work(crep, cwork, f"{name} chain", short_min=1 if name == "shells" else 0)


def test_one_nan_lane_per_wave(bzr, orc, ctx, lens2, mesh2, chain128):
    """A NaN lane cannot win and must not count as one that may: the other lanes' words equal the run without it."""
    clean, cwant, _ = chain128
    rays = clean.copy()
    lane = (np.arange(rays.shape[1] // 64) * 7) % 64  # another lane in each wave
    nan_at = np.arange(0, rays.shape[1], 64) + lane
    rays[1, nan_at] = np.float32(np.nan)
    others = np.ones(rays.shape[1], bool)
    others[nan_at] = False
    want, work = oracle_counted(orc, lambda: orc.trace_chain([lens2], [1.3], rays))
    got, rep = counted(ctx, lambda: bzr.trace_chain(ctx, [mesh2], [1.3], rays, mode=bzr.PIPELINE_FUSED))
    assert_chain(got, want, "cfg2 128 with NaN lanes")
    assert_work(rep, work, "cfg2 128 with NaN lanes")
    assert (got[1][nan_at] == bzr.RR_NONE).all()
    base = bzr.trace_chain(ctx, [mesh2], [1.3], clean, mode=bzr.PIPELINE_FUSED)
    assert_chain(base, cwant, "cfg2 128")
    for g, b in zip(got, base):
        assert np.array_equal(bits(g)[..., others], bits(b)[..., others])


def test_fast_mode(bzr, ctx, mesh2, chain128):
    """FAST mode on the cfg2 chain: tests/test_gpu_fast.py's status, segment and exit-direction gates with the same
    bars (no bit equality; the later segments' rays differ in their last bits, so the work counts are
    not the oracle's either)."""
    rays, (wo, ws, wg), _ = chain128
    (o, s, g), rep = counted(ctx, lambda: bzr.trace_chain(ctx, [mesh2], [1.3], rays,
                                                          mode=bzr.PIPELINE_FUSED | bzr.MODE_FAST))
    status_agree, seg_agree = float((s == ws).mean()), float((g == wg).mean())
    print(f"fast chain cfg2 128: status agree {status_agree:.5f}, segments agree {seg_agree:.5f}", rep)
    assert status_agree >= HIT_AGREE and seg_agree >= SAME_PATCH
    ok = (s == ws) & (ws != 0)
    assert float(np.quantile(np.abs(o[3:6][:, ok] - wo[3:6][:, ok]).max(axis=0), 0.99)) < 1e-3
    assert 1 <= rep["short_passes"] <= rep["newton_rounds"]
