"""Stacked meshes: candidate-list overflow and exact t ties, against the oracle bit for bit.

Real lenses put a handful of patches through a ray's planar gate and never return one t twice, so three pieces of
trace.hip stay idle on them: the staged pipeline's list limit (kMaxCand = 40: the 41st gate pass publishes the ray
on the overflow list, nothing of it is ranked, placed or run by k_newton, k_resolve scans it in order and k_finish /
k_finish_ovf evaluate its winner again), the winner rule under exact ties (the lexicographic minimum of (t order key,
scanned index), in registers on the fused path and as a packed 64-bit atomicMin on the staged one), and k_trace's
16-entry collected-leaf list running several collect / Newton batches per segment.  Two stacked meshes reach them:

dup     cfg1's 126 patches, 20 full copies and the first 63 records of a 21st (2 583 patches).  Every copy returns
        the same bits, so every hit is a 20- or 21-way exact tie that the first copy must win.  A ray that passes
        the gate of g patches of the lens passes 20 g of the stack plus those of the half copy: over the grid the
        counts are 0 (432 rays), 40 (131: a full list), 41 (12) and 42 (131: the first overflows), and 80 to 168.
shells  24 concentric spheres, makeEllipsoid(3, 7) scaled by 1 - k * step, each standardized and built on its own
        (3 024 patches): no exact ties, but 24 keys per crossing that differ by the step (2^-8, or 2^-12 for keys a
        few ulps apart), and origins all around, so every shell wins rays.

The rays are cfg1's 32 x 32 tiled grid (plus, for the shells, 1 024 seeded rays from a radius-3 sphere aimed into
[-0.8, 0.8]^3).  The populations above are computed from the oracle's planar gate and asserted, so no test here
passes vacuously.
"""
import numpy as np
import pytest

from bzr_amd.configs import CONFIGS, build_lens, grid_rays

pytestmark = pytest.mark.gpu

MAX_CAND = 40     # trace.hip kMaxCand
N_BASE = 126      # patches of cfg1's lens, Lens("ellipsoid", 3, 7)
COPIES, PART = 20, 63
SHELLS = 24
MODES = ("fused", "staged", "brute")


def stack(parts, shift=None):
    """Concatenate patch arrays; each part's patch offset (or shift[k]) is added to its three neighbour words
    (words 16..18 of the 66-word record: bzr_patch::neigh at byte 64), so follow retries stay inside their own part."""
    out, off = [], 0
    for k, p in enumerate(parts):
        q = np.array(p, dtype=np.float32, copy=True)
        q.view(np.uint32)[:, 16:19] += np.uint32(off if shift is None else shift[k])
        out.append(q)
        off += len(q)
    return np.ascontiguousarray(np.concatenate(out))


def dup_patches(orc):
    base = build_lens(orc.OMesh, CONFIGS["cfg1"].lenses[0]).bezier_patches()
    assert base.shape == (N_BASE, 66) and int(base.view(np.uint32)[:, 16:19].max()) < N_BASE
    # the partial copy keeps its neighbour words: they point into copy 0
    return stack([base] * COPIES + [base[:PART]], shift=[k * N_BASE for k in range(COPIES)] + [0])


def shell_patches(orc, step, centre=(0.0, 0.0, 0.0)):
    parts = []
    for k in range(SHELLS):
        m = orc.OMesh().make_ellipsoid(3, 7)
        m.transform(np.eye(3, dtype=np.float32) * np.float32(1.0 - k * step), centre)
        parts.append(m.standardize().bezier_patches())
    return stack(parts)


def around_rays(n=1024, seed=7):
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3))
    o *= 3.0 / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.uniform(-0.8, 0.8, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o.T, d.T]).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Case:
    """A stacked mesh, its rays and everything the oracle says about them (computed once, never changed)."""

    def __init__(self, orc, patches, rays):
        self.patches, self.rays = patches, rays
        self.gate = orc.planar_gate(patches, rays).sum(axis=1)
        orc.counters_reset()
        self.hit = bits(orc.intersect(patches, rays))
        self.work = orc.counters()
        # the listed rays alone: what the staged pipeline's pair counters see (overflow rays take the scan)
        self.listed = self.gate <= MAX_CAND
        orc.counters_reset()
        orc.intersect(patches, rays[:, self.listed])
        self.work_listed = orc.counters()
        self.chain = orc.trace_chain([patches], [1.3], rays)
        for a in (self.patches, self.rays, self.gate, self.hit, *self.chain):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def cases(orc):
    grid = grid_rays(CONFIGS["cfg1"], side=32)
    both = np.ascontiguousarray(np.concatenate([grid, around_rays()], axis=1))
    return {"dup": Case(orc, dup_patches(orc), grid),
            "shells8": Case(orc, shell_patches(orc, 2.0 ** -8), both),
            "shells12": Case(orc, shell_patches(orc, 2.0 ** -12), both)}


@pytest.fixture(scope="module")
def meshes(bzr, ctx, cases):
    return {k: bzr.DeviceMesh(ctx, c.patches) for k, c in cases.items()}


@pytest.fixture(params=["dup", "shells8", "shells12"])
def name(request):
    return request.param


def mode_of(bzr, m):
    return {"fused": bzr.PIPELINE_FUSED, "staged": bzr.PIPELINE_STAGED, "brute": bzr.ACCEL_NONE}[m]


def test_the_stacked_meshes_reach_the_list_limit_and_ties(bzr, cases, name):
    """Non-vacuity, from the oracle alone: the gate-count populations around kMaxCand, who wins the ties."""
    c = cases[name]
    g = c.gate
    hits = c.hit[11] == bzr.WHAT_INTERSECT
    assert (g == 0).sum() > 100  # misses: fewer than kMaxCand, and idle lanes beside the busy ones
    assert (g > MAX_CAND).sum() > 100 and (g >= 2 * MAX_CAND).sum() > 100
    assert g.max() > 3 * 16  # and k_trace's 16-entry batches run more than three times on some wave
    if name == "dup":
        # the boundary itself: a full list (40, no overflow) beside the first overflowing count (41)
        assert (g == MAX_CAND).sum() >= 100 and (g == MAX_CAND + 1).sum() >= 10 and (g == MAX_CAND + 2).sum() >= 100
        assert hits.sum() == 350 and (c.hit[12][hits] < N_BASE).all()  # the first copy wins every tie
        waves = g.reshape(-1, 64)
        mixed = ((waves == 0).any(1) | (waves == MAX_CAND).any(1)) & (waves > MAX_CAND).any(1)
        assert mixed.sum() >= 4  # listed (or missing) and overflowed rays side by side in one wave
    else:
        # short lists beside the long ones (the counts step by two here: the list's very boundary is dup's part)
        assert ((g > 0) & (g < MAX_CAND)).sum() >= (50 if name == "shells8" else 4)
        shells_won = np.unique(c.hit[12][hits] // N_BASE)
        assert len(shells_won) >= 12, shells_won
        assert (c.chain[2] == 2).sum() > 900  # two-segment rays of the one-lens chain


@pytest.mark.parametrize("m", MODES)
def test_intersect_equals_oracle(bzr, ctx, cases, meshes, name, m):
    c = cases[name]
    got = bits(bzr.intersect(ctx, meshes[name], c.rays, mode=mode_of(bzr, m)))
    bad = (got != c.hit).any(axis=0)
    assert not bad.any(), (f"{name} {m}: {int(bad.sum())} of {len(bad)} rays differ; gate counts of the first "
                           f"{c.gate[bad][:8]}, patch got {got[12][bad][:8]} want {c.hit[12][bad][:8]}")


@pytest.mark.parametrize("m", MODES)
def test_chain_equals_oracle(bzr, ctx, cases, meshes, name, m):
    c = cases[name]
    w_rays, w_st, w_seg = c.chain
    g_rays, g_st, g_seg = bzr.trace_chain(ctx, [meshes[name]], [1.3], c.rays, mode=mode_of(bzr, m))
    assert np.array_equal(g_st, w_st) and np.array_equal(g_seg, w_seg), f"{name} {m}: status / segments"
    assert np.array_equal(bits(g_rays), bits(w_rays)), f"{name} {m}: rays"


@pytest.mark.parametrize("m", MODES)
def test_two_lens_chain_equals_oracle(bzr, orc, ctx, cases, meshes, m):
    """dup, then the 2^-8 shells moved +3 in x, each with its own refractive index."""
    a = cases["dup"]
    b = shell_patches(orc, 2.0 ** -8, (3.0, 0.0, 0.0))
    ri = [1.3, 1.5]
    w_rays, w_st, w_seg = orc.trace_chain([a.patches, b], ri, a.rays)
    assert (w_seg > 2).sum() > 100  # rays reach the second lens
    lenses = [meshes["dup"], bzr.DeviceMesh(ctx, b)]
    g_rays, g_st, g_seg = bzr.trace_chain(ctx, lenses, ri, a.rays, mode=mode_of(bzr, m))
    assert np.array_equal(g_st, w_st) and np.array_equal(g_seg, w_seg), f"{m}: status / segments"
    assert np.array_equal(bits(g_rays), bits(w_rays)), f"{m}: rays"


def _counted(bzr, ctx, mesh, rays, mode):
    ctx.counters(True)
    ctx.counters_report()
    got = bits(bzr.intersect(ctx, mesh, rays, mode=mode))
    rep = ctx.counters_report()
    ctx.counters(False)
    return got, rep


def test_staged_overflow_rays_are_the_rays_past_the_list_limit(bzr, ctx, cases, meshes, name):
    """Exactly the rays with more than kMaxCand gate passes take the overflow list (the origins are inside the near
    tier's radius and the 64-entry walk stack holds on these coincident boxes: nothing else feeds the counter), and
    the pairs k_newton runs and the follow retries are the oracle's over the listed rays alone."""
    c = cases[name]
    got, rep = _counted(bzr, ctx, meshes[name], c.rays, bzr.PIPELINE_STAGED)
    print(name, "staged", rep, "oracle", c.work, "oracle, listed rays", c.work_listed, "over", int((~c.listed).sum()))
    assert np.array_equal(got, c.hit)
    assert rep["segments"] == c.rays.shape[1]
    assert rep["overflow_rays"] == int((c.gate > MAX_CAND).sum())
    assert rep["pairs"] == c.work_listed["newton"]
    assert rep["follows"] == c.work_listed["follow"]


def test_fused_never_overflows_and_counts_the_oracles_work(bzr, ctx, cases, meshes, name):
    """k_trace has no list limit: no overflow ray, and its Newton runs and follow retries are the oracle's."""
    c = cases[name]
    got, rep = _counted(bzr, ctx, meshes[name], c.rays, bzr.PIPELINE_FUSED)
    print(name, "fused", rep, "oracle", c.work)
    assert np.array_equal(got, c.hit)
    assert rep["segments"] == c.work["segments"] == c.rays.shape[1]
    assert rep["overflow_rays"] == 0
    assert rep["pairs"] == c.work["newton"]
    assert rep["follows"] == c.work["follow"]


def test_staged_runs_are_deterministic(bzr, ctx, cases, meshes, name):
    """The order of the atomicMins must not reach the result."""
    c = cases[name]
    a = bits(bzr.intersect(ctx, meshes[name], c.rays, mode=bzr.PIPELINE_STAGED)).copy()
    b = bits(bzr.intersect(ctx, meshes[name], c.rays, mode=bzr.PIPELINE_STAGED))
    assert np.array_equal(a, b) and np.array_equal(a, c.hit)


@pytest.mark.parametrize("m", MODES)
def test_permuted_rays_give_the_tiled_runs_bits(bzr, ctx, cases, meshes, m):
    """dup's rays in a seeded permutation: every wave mixes gate counts 0, 40, 41 and 120."""
    c = cases["dup"]
    perm = np.random.default_rng(2024).permutation(c.rays.shape[1])
    waves = c.gate[perm].reshape(-1, 64)
    assert ((waves == 0).any(1) & (waves == MAX_CAND).any(1) & (waves > 2 * MAX_CAND).any(1)).all()
    assert ((waves == MAX_CAND + 1).any(1)).sum() >= 8
    tiled = bits(bzr.intersect(ctx, meshes["dup"], c.rays, mode=mode_of(bzr, m)))
    got = bits(bzr.intersect(ctx, meshes["dup"], np.ascontiguousarray(c.rays[:, perm]), mode=mode_of(bzr, m)))
    back = np.empty_like(got)
    back[:, perm] = got
    assert np.array_equal(back, tiled) and np.array_equal(back, c.hit)
