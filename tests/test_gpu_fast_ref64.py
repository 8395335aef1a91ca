"""BZR_MODE_FAST on every entry point, judged against a binary64 reference (tests/ref64.py).

FAST keeps the planar gate exact and runs the Newton stage with FMA contraction and v_rcp / v_sqrt / v_rsq.  The
float32 oracle is itself off the truth (on the lens at x = 10 its t is 4.5e-5 relative off at the 99th percentile), so
FAST is not compared with the oracle's values but with the oracle's error: both are measured against ref64 on the same
well-conditioned triples or rays, in the same test, and FAST's median and 99th percentile of each error may be at most
BAR = 2 x the oracle's.  The margin: FAST swaps correctly rounded operations (1/2 ulp) for v_rcp_f32, v_sqrt_f32 and
v_rsq_f32 at 1 ulp each; contraction only removes roundings; the four Newton steps self-correct, so the last step's
roundings dominate.  The class agreement with ref64 may fall CLASS_ALLOW = 0.005 below the oracle's (SURVEY.md 8c's
own hit/miss allowance).

What holds exactly in FAST is asserted exactly: the gate-fail and the miss records, the candidate set (a hit lies on a
patch whose gate the ray passed, or on the neighbour such a patch names), finite t on every INTERSECT row, the overflow
counter, and the identities between calls that run the same kernels over the same waves (records / rows, AoS / SoA,
device / host pointers, repeated fused calls).

Out of scope: bzr_illuminate and bzr_trace_tiled in FAST, and stacked exact-tie meshes (their winner depends on
bit-equal t across pass sites, which FAST does not promise).
"""
import numpy as np
import pytest

import ref64
from bzr_amd.configs import CONFIGS, build_lens, grid_rays
from test_gpu_fuzz import _lens as fuzz_lens
from test_gpu_long_chains import bits, chain_rays, lens_patches
from test_gpu_ray_edges import clean_batch, poisoned, tier_radii

pytestmark = pytest.mark.gpu

SEEDS = ref64.SEEDS
BAR = 2.0
CLASS_ALLOW = 0.005
STATUS_AGREE = 0.995   # tests/test_gpu_fast.py's chain gates
SEGMENT_AGREE = 0.99
EXIT_DIR_P99 = 1e-3
PIPES = ("fused", "staged")
N_MESH_RAYS = 4096


def pipe_of(bzr, name):
    return bzr.PIPELINE_FUSED if name == "fused" else bzr.PIPELINE_STAGED


def assert_bars(label, fast_rows, oracle_rows, ref, sel, span):
    """FAST's error quantiles against ref64 are at most BAR x the oracle's on the same columns; prints both."""
    qf = ref64.quantiles(ref64.errors(fast_rows, ref, sel, span))
    qo = ref64.quantiles(ref64.errors(oracle_rows, ref, sel, span))
    ratios = {k: tuple(f / o if o > 0 else (0.0 if f == 0 else np.inf) for f, o in zip(qf[k], qo[k])) for k in qf}
    print(f"{label}: {int(np.count_nonzero(sel))} columns; FAST / oracle error ratio (median, p99): "
          + ", ".join(f"{k} {a:.2f} {b:.2f}" for k, (a, b) in ratios.items())
          + "; oracle median / p99: " + ", ".join(f"{k} {a:.2e} / {b:.2e}" for k, (a, b) in qo.items()))
    for k in qf:
        for which, f, o in zip(("median", "p99"), qf[k], qo[k]):
            assert f <= BAR * o, f"{label}: FAST's {which} {k} error {f:.3e} exceeds {BAR} x the oracle's {o:.3e}"


# ------------------------------------------------------------------ per triple: k_patch<true>
@pytest.fixture(scope="module")
def lenses(orc):
    return ref64.lens_set(orc)


@pytest.mark.parametrize("name", list(SEEDS))
def test_patch_intersect_fast_against_float64(bzr, orc, ctx, lenses, name):
    """The Newton numerics with no selection around them: 8 192 aimed (patch, ray, limit) triples per lens."""
    patches, ox, yz = lenses[name]
    idx, limit, rays = ref64.aimed_triples(patches, ox, yz, SEEDS[name])
    span = ref64.mesh_span(patches)
    h = ref64.patch_intersect64(patches, idx, limit, rays)
    want = orc.patch_intersect(patches, idx, limit, rays)
    wu = bits(want)
    dm = bzr.DeviceMesh(ctx, patches)
    par = bits(bzr.patch_intersect(ctx, dm, idx, limit, rays))
    assert np.array_equal(par, wu), f"{name}: parity differs on {int((par != wu).any(axis=0).sum())} triples"
    fast = bzr.patch_intersect(ctx, dm, idx, limit, rays, mode=bzr.MODE_FAST)
    fu = bits(fast)
    # the exact-gate contract: the all-zero gate-fail record, on exactly the oracle's triples
    gate_fail = (wu[:11] == 0).all(axis=0) & (wu[11] == bzr.WHAT_NONE)
    assert 0 < gate_fail.sum() < len(idx)
    assert np.array_equal(fu[:, gate_fail], wu[:, gate_fail])
    assert np.array_equal((fu[:11] == 0).all(axis=0) & (fu[11] == bzr.WHAT_NONE), gate_fail)
    well = ref64.well_conditioned(h, limit, span)
    assert well.sum() >= 1000
    oracle_share = float((wu[11, well] == bzr.WHAT_INTERSECT).mean())
    fast_share = float((fu[11, well] == bzr.WHAT_INTERSECT).mean())
    print(f"{name}: class agreement with float64 on {int(well.sum())} well-conditioned triples: oracle "
          f"{oracle_share:.5f}, FAST {fast_share:.5f}")
    assert fast_share >= oracle_share - CLASS_ALLOW
    both = well & (wu[11] == bzr.WHAT_INTERSECT) & (fu[11] == bzr.WHAT_INTERSECT)
    assert_bars(f"k_patch {name}", fast, want, h, both, span)


# ------------------------------------------------------------------ mesh level: bzr_intersect
MESH_LENSES = ("origin", "cfg2", "robot", "fuzz0", "fuzz2")


def mesh_rays(patches, s_max, seed, n=N_MESH_RAYS):
    """A third +x grid rays over the lens's box, a third aimed at control points, a third at random points of the
    box; an eighth of the last third starts beyond s_max (the in-order scan)."""
    rng = np.random.default_rng(seed)
    cp = np.asarray(patches)[:, 19:49].reshape(-1, 3).astype(np.float64)
    lo, hi = cp.min(axis=0), cp.max(axis=0)
    span = float((hi - lo).max())
    side = 37
    k = (n - side * side) // 2
    u = (np.arange(side) + 0.5) / side
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * 1.05
    gy, gz = np.meshgrid(mid[1] + (2 * u - 1) * half[1], mid[2] + (2 * u - 1) * half[2])
    grid = np.stack([np.full(side * side, lo[0] - span), gy.ravel(), gz.ravel(), np.ones(side * side),
                     np.zeros(side * side), np.zeros(side * side)])
    tgt = np.concatenate([cp[rng.integers(0, len(cp), k)], rng.uniform(lo, hi, (n - side * side - k, 3))])
    m = len(tgt)
    way = rng.normal(size=(m, 3))
    way /= np.linalg.norm(way, axis=1, keepdims=True)
    dist = span * rng.uniform(0.5, 3.0, (m, 1))
    far = (m - k) // 8
    dist[-far:] = 4.0 * float(s_max)
    o = (tgt + way * dist).astype(np.float32)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    aimed = np.concatenate([o.T.astype(np.float64), d.T])
    return np.ascontiguousarray(np.concatenate([grid, aimed], axis=1).astype(np.float32))


@pytest.fixture(scope="module")
def mesh_cases(bzr, orc, lenses):
    """name -> (patches, rays, gate matrix, oracle rows, intersect64's namespace, s_max), computed once."""
    out = {}
    for k, name in enumerate(MESH_LENSES):
        patches = lenses[name][0] if name in lenses else fuzz_lens(bzr, int(name[4:]))[0]
        assert patches is not None
        s_max = tier_radii(bzr, patches)[1]
        rays = mesh_rays(patches, s_max, 700 + k)
        assert rays.shape == (6, N_MESH_RAYS) and rays.shape[1] * len(patches) <= 1 << 25
        gate = orc.planar_gate(patches, rays, threads=16)
        want = orc.intersect(patches, rays, threads=16)
        ref = ref64.intersect64(patches, rays, gate)
        for a in (rays, gate, want):
            a.setflags(write=False)
        out[name] = (patches, rays, gate, want, ref, s_max)
    return out


@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("name", MESH_LENSES)
def test_intersect_fast_against_float64(bzr, ctx, mesh_cases, name, pipe):
    patches, rays, gate, want, ref, s_max = mesh_cases[name]
    n = rays.shape[1]
    span = ref64.mesh_span(patches)
    dm = bzr.DeviceMesh(ctx, patches)
    mode = pipe_of(bzr, pipe)
    par = bits(bzr.intersect(ctx, dm, rays, mode=mode))
    wu = bits(want)
    assert np.array_equal(par, wu)
    ctx.counters(True)
    ctx.counters_report()
    fast = bzr.intersect(ctx, dm, rays, mode=mode | bzr.MODE_FAST)
    rep = ctx.counters_report()
    ctx.counters(False)
    fu = bits(fast)
    # exact: the miss record where no gate passes
    none = ~gate.any(axis=1)
    assert none.sum() > 100 and (~none).sum() > 1000
    assert np.array_equal(fu[:, none], par[:, none]) and (par[11, none] == bzr.WHAT_NONE).all()
    # exact: a hit lies on a candidate of the exact gate, or on the neighbour a candidate names (the follow-side
    # retry reports the neighbour, whose own cThis gate need not pass)
    neigh = np.ascontiguousarray(patches).view(np.uint32)[:, 16:19]
    for label, u in (("parity", par), ("FAST", fu)):
        hit = np.nonzero(u[11] == bzr.WHAT_INTERSECT)[0]
        p = u[12, hit].astype(np.int64)
        assert (p < len(patches)).all()
        direct = gate[hit, p]
        named = np.zeros(len(hit), bool)
        for j in np.nonzero(~direct)[0]:
            named[j] = bool((neigh[gate[hit[j]]] == p[j]).any())
        assert (direct | named).all(), f"{label}: {int((~(direct | named)).sum())} hits on patches outside the candidate set"
        assert np.isfinite(u.view(np.float32)[0, hit]).all(), f"{label}: INTERSECT with a non-finite t"
    # exact: only origins beyond s_max take the in-order scan
    beyond = int((np.abs(rays[:3]).max(axis=0) > s_max).sum())
    assert beyond >= 40
    assert rep["overflow_rays"] == beyond, (rep, beyond)
    # against float64, on the well-conditioned rays
    well = ref.well
    assert well.sum() >= 500, int(well.sum())
    same = lambda u: (u[11, well] == bzr.WHAT_INTERSECT) & (u[12, well] == ref.patch[well])  # noqa: E731
    oracle_share, fast_share = float(same(wu).mean()), float(same(fu).mean())
    print(f"{name} {pipe}: {int(well.sum())} well-conditioned rays of {n}, {beyond} beyond s_max; same hit as float64: "
          f"oracle {oracle_share:.5f}, FAST {fast_share:.5f}")
    assert fast_share >= oracle_share - CLASS_ALLOW
    both = well.copy()
    both[well] = same(wu) & same(fu)
    assert_bars(f"intersect {name} {pipe}", fast, want, ref, both, span)


# ------------------------------------------------------------------ identities that are exact in FAST
def test_fast_identities_between_calls(bzr, ctx, mesh_cases):
    """Same kernels over the same waves: bit for bit, in FAST as in parity."""
    torch = pytest.importorskip("torch")
    patches, rays, _, _, _, _ = mesh_cases["cfg2"]
    dm = bzr.DeviceMesh(ctx, patches)
    rec_rays = np.ascontiguousarray(rays.T)
    for pipe in PIPES:
        mode = pipe_of(bzr, pipe) | bzr.MODE_FAST
        rows = bits(bzr.intersect(ctx, dm, rays, mode=mode))
        assert (rows[11] == bzr.WHAT_INTERSECT).sum() > 1000
        rec, patch = bzr.intersect_records(ctx, dm, rays, mode=mode)
        rec, patch = bits(rec), bits(patch)
        assert np.array_equal(rec[:, 0], (rows[11] == bzr.WHAT_INTERSECT).astype(np.uint32))
        assert np.array_equal(rec[:, 1:5], rows[1:5].T) and np.array_equal(rec[:, 5], rows[0])
        assert np.array_equal(rec[:, 6:12], rows[5:11].T)
        assert np.array_equal(rec[:, 12], rows[11]) and np.array_equal(patch, rows[12])
        assert np.array_equal(bits(bzr.intersect(ctx, dm, rec_rays, mode=mode | bzr.RAYS_AOS)), rows), f"{pipe}: AoS"
        dev = bzr.intersect(ctx, dm, torch.from_numpy(np.array(rays)).cuda(), mode=mode)
        torch.cuda.synchronize()
        assert np.array_equal(bits(dev.cpu().numpy()), rows), f"{pipe}: device pointers"
        chain = [bits(a) for a in bzr.trace_chain(ctx, [dm], [1.3], rays, mode=mode)]
        chain_aos = bzr.trace_chain(ctx, [dm], [1.3], rec_rays, mode=mode | bzr.RAYS_AOS)
        assert np.array_equal(bits(chain_aos[0]).T, chain[0]) and np.array_equal(bits(chain_aos[1]), chain[1])
    fused = bzr.PIPELINE_FUSED | bzr.MODE_FAST
    runs = [[bits(a) for a in bzr.trace_chain(ctx, [dm], [1.3], rays, mode=fused)] for _ in range(3)]
    for other in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], other))


# ------------------------------------------------------------------ chains and refract
@pytest.fixture(scope="module")
def chains(orc):
    """name -> (lens patch arrays, rays, the oracle's chain, the first lens's rays without a gate pass)."""
    out = {}
    cfg4 = CONFIGS["cfg4"]
    sets = {"cfg4": ([build_lens(orc.OMesh, l).bezier_patches() for l in cfg4.lenses], grid_rays(cfg4, side=96)),
            "three432": ([lens_patches(orc, k) for k in range(3)], chain_rays())}
    for name, (ls, rays) in sets.items():
        want = orc.trace_chain(ls, [1.3] * len(ls), rays, threads=16)
        none = ~orc.planar_gate(ls[0], rays, threads=16).any(axis=1)
        out[name] = (ls, rays, want, none)
    return out


def assert_chain_gates(label, got, want, keep=None):
    """tests/test_gpu_fast.py's gates against the oracle over the rays `keep` (default: all)."""
    (o, s, g), (wo, ws, wg) = got, want
    keep = np.ones(len(ws), bool) if keep is None else keep
    status, seg = float((s == ws)[keep].mean()), float((g == wg)[keep].mean())
    ok = keep & (s == ws) & (ws != 0)
    p99 = float(np.quantile(np.abs(o[3:6][:, ok] - wo[3:6][:, ok]).max(axis=0), 0.99))
    print(f"{label}: status agree {status:.5f}, segments agree {seg:.5f}, exit direction p99 {p99:.2e} over "
          f"{int(ok.sum())} exiting rays")
    assert ok.sum() > 500
    assert status >= STATUS_AGREE and seg >= SEGMENT_AGREE and p99 < EXIT_DIR_P99


@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("name", ["cfg4", "three432"])
def test_fast_chains(bzr, ctx, chains, name, pipe):
    ls, rays, want, none = chains[name]
    dms = [bzr.DeviceMesh(ctx, p) for p in ls]
    got = bzr.trace_chain(ctx, dms, [1.3] * len(ls), rays, mode=pipe_of(bzr, pipe) | bzr.MODE_FAST)
    assert (want[2] == 2 * len(ls)).sum() > 500  # rays do run the whole chain
    assert_chain_gates(f"{name} {pipe}", got, want)
    # exact: no gate pass on the first lens, so the ray comes back as it went in
    o, s, g = got
    assert none.sum() > 100
    assert np.array_equal(bits(o)[:, none], bits(rays)[:, none])
    assert (s[none] == bzr.RR_NONE).all() and (g[none] == 1).all()


@pytest.mark.parametrize("pipe", PIPES)
def test_fast_refract_with_per_ray_expected(bzr, orc, ctx, chains, pipe):
    ls, front, _, _ = chains["three432"]
    dm = bzr.DeviceMesh(ctx, ls[0])
    back, st1 = orc.refract(ls[0], 1.3, front, np.full(front.shape[1], bzr.RR_INSIDE, np.uint32))
    assert (st1 == bzr.RR_INSIDE).sum() > 1000
    exp = np.random.default_rng(9).integers(0, 4, front.shape[1]).astype(np.uint32)
    for label, rays in (("front", front), ("back", back)):
        w_rays, w_st = orc.refract(ls[0], 1.3, rays, exp)
        assert len(np.unique(w_st)) >= 2
        g_rays, g_st = bzr.refract(ctx, dm, 1.3, rays, exp, mode=pipe_of(bzr, pipe) | bzr.MODE_FAST)
        agree = float((g_st == w_st).mean())
        print(f"refract {label} {pipe}: status agree {agree:.5f}")
        assert agree >= STATUS_AGREE
        dead = g_st == bzr.RR_NONE
        assert np.array_equal(bits(g_rays)[:, dead], bits(rays)[:, dead])  # a NONE ray is returned as it came


# ------------------------------------------------------------------ non-finite rays
@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("pattern", ["lane17", "third"])
def test_fast_garbage_lanes(bzr, orc, ctx, chains, pattern, pipe):
    """tests/test_gpu_ray_edges.py's 25 kinds of garbage in one lane per wave and in every third lane.  A ray with a
    non-finite component passes through bit-identical with status NONE and one segment; the finite lanes meet the
    chain gates against the oracle.

    The finite lanes are not required to equal the run without garbage bit for bit, as parity is: in k_trace a
    (lane, patch) pair is evaluated at the joined or at the parked pass site depending on what the wave's other
    lanes do, and in FAST the compiler may contract the two sites differently."""
    ls = chains["three432"][0]
    dms = [bzr.DeviceMesh(ctx, p) for p in ls]
    s_near, _ = tier_radii(bzr, ls[0])
    batch, mask = poisoned(clean_batch(ls[0], s_near), pattern)
    bad = ~np.isfinite(batch).all(axis=0)
    assert bad.sum() >= 0.4 * mask.sum() and not bad[~mask].any() and bad.sum() > 50
    mode = pipe_of(bzr, pipe) | bzr.MODE_FAST
    hits = bits(bzr.intersect(ctx, dms[0], batch, mode=mode))
    par = bits(bzr.intersect(ctx, dms[0], batch, mode=pipe_of(bzr, pipe)))
    assert np.array_equal(hits[:, bad], par[:, bad]) and (hits[11, bad] == bzr.WHAT_NONE).all()
    want = orc.trace_chain(ls, [1.3] * 3, batch, threads=16)
    got = bzr.trace_chain(ctx, dms, [1.3] * 3, batch, mode=mode)
    o, s, g = got
    assert np.array_equal(bits(o)[:, bad], bits(batch)[:, bad])
    assert (s[bad] == bzr.RR_NONE).all() and (g[bad] == 1).all()
    assert_chain_gates(f"garbage {pattern} {pipe}", got, want, keep=~mask)
