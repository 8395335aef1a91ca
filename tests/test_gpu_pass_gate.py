"""k_trace's main Newton site runs patch_intersect without the barycentric re-test (patch_math.hpp kGatePlane): a lane is
in a pass because the planar gate of that same record passed for it (`run0`), or it has limitNone (`joined`, `spec`).
If that promise were broken anywhere -- a lane sent into a pass of a patch whose gate it fails -- the lane would get a
Newton result the reference never computes, and the counting kernels would count one pair less (trace.hip checks the
record's own gate for every run0 lane where the counters are on).

So every case runs the fused pipeline with the counters on and asserts:
  * every output word equals the brute-force scan's (BZR_ACCEL_NONE: patch_intersect with the whole gate, in order),
    and the CPU oracle's where the oracle has the entry point;
  * `pairs` equals the oracle's Newton runs and `follows` its follow retries.

The cases are the places where lanes reach a pass by different routes: rim waves, batches of more than 16 entries with
exact ties, follow retries that join a later pass or take a parked result, lanes inside the lens beside lanes outside,
the in-order full scan (origins beyond the tree's radius), the always list, NaN lanes, FAST mode (against the staged
FAST pipeline: the scan has no FAST mode), and the kernels that share trace_segment (power, spectral, TIR, optical path, media).
"""
import numpy as np
import pytest

from bzr_amd.configs import CONFIGS, build_lens, grid_rays
from test_culling_conservative import always_list, dominated_lens, DOMINATED_LENS_SHIFT
from test_gpu_ray_edges import tier_radii
from test_gpu_short_passes import bits, counted, oracle_counted
from test_gpu_stacked import dup_patches, shell_patches, around_rays

pytestmark = pytest.mark.gpu

RI = 1.3


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def assert_same(got, want, label):
    """Tuples of arrays (or one array), word for word."""
    got = got if isinstance(got, (tuple, list)) else (got,)
    want = want if isinstance(want, (tuple, list)) else (want,)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = bits(host(g)), bits(host(w))
        bad = g != w
        assert not bad.any(), f"{label}: output {k}: {int(bad.sum())} of {bad.size} words differ"


def assert_pairs(rep, work, label):
    print(label, rep, "oracle", work)
    assert rep["pairs"] == work["newton"], label
    assert rep["follows"] == work["follow"], label
    assert rep["newton_rounds"] > 0, label


def three_ways(bzr, orc, ctx, patches, mesh, rays, label, ops=("chain", "refract", "intersect")):
    """The fused pipeline (counted), the brute-force scan and the oracle on one mesh; returns the counters per op."""
    reps = {}
    for op in ops:
        if op == "chain":
            want, work = oracle_counted(orc, lambda: orc.trace_chain([patches], [RI], rays))
            got, rep = counted(ctx, lambda: bzr.trace_chain(ctx, [mesh], [RI], rays, mode=bzr.PIPELINE_FUSED))
            brute = bzr.trace_chain(ctx, [mesh], [RI], rays, mode=bzr.ACCEL_NONE)
        elif op == "refract":
            exp = np.full(rays.shape[1], bzr.RR_INSIDE, np.uint32)
            want, work = oracle_counted(orc, lambda: orc.refract(patches, RI, rays, exp))
            got, rep = counted(ctx, lambda: bzr.refract(ctx, mesh, RI, rays, mode=bzr.PIPELINE_FUSED))
            brute = bzr.refract(ctx, mesh, RI, rays, mode=bzr.ACCEL_NONE)
        else:
            want, work = oracle_counted(orc, lambda: orc.intersect(patches, rays))
            got, rep = counted(ctx, lambda: bzr.intersect(ctx, mesh, rays, mode=bzr.PIPELINE_FUSED))
            brute = bzr.intersect(ctx, mesh, rays, mode=bzr.ACCEL_NONE)
        assert_same(got, brute, f"{label} {op}: fused against the brute-force scan")
        assert_same(got, want, f"{label} {op}: fused against the oracle")
        assert_pairs(rep, work, f"{label} {op}")
        reps[op] = rep
    return reps


@pytest.fixture(scope="module")
def lens2(bzr):
    p = build_lens(bzr.TriMesh, CONFIGS["cfg2"].lenses[0]).bezier_patches()
    p.setflags(write=False)
    return p


@pytest.fixture(scope="module")
def mesh2(bzr, ctx, lens2):
    return bzr.DeviceMesh(ctx, lens2)


@pytest.fixture(scope="module")
def rays128():
    r = grid_rays(CONFIGS["cfg2"], side=128)
    r.setflags(write=False)
    return r


def test_cfg2_rim_waves(bzr, orc, ctx, lens2, mesh2, rays128):
    gate = orc.planar_gate(lens2, rays128).sum(axis=1).reshape(-1, 64)
    assert ((gate == 0).any(axis=1) & (gate >= 2).any(axis=1)).sum() >= 40  # no candidate beside two or more
    reps = three_ways(bzr, orc, ctx, lens2, mesh2, rays128, "cfg2 128")
    assert all(r["overflow_rays"] == 0 for r in reps.values())


@pytest.mark.parametrize("name", ["dup", "shells"])
def test_stacked_meshes(bzr, orc, ctx, name):
    """More than 16 entries per wave-segment (several batches) and exact t ties (tests/test_gpu_stacked.py)."""
    grid = grid_rays(CONFIGS["cfg1"], side=32)
    if name == "dup":
        patches, rays = dup_patches(orc), grid
    else:
        patches = shell_patches(orc, 2.0 ** -8)
        rays = np.ascontiguousarray(np.concatenate([grid, around_rays()], axis=1))
    assert orc.planar_gate(patches, rays).sum(axis=1).max() > 3 * 16
    three_ways(bzr, orc, ctx, patches, bzr.DeviceMesh(ctx, patches), rays, name, ops=("chain", "intersect"))


def edge_rays(patches, per_edge=2, seed=5):
    """Rays along +x through points of every patch's three edges (the straight lines between its corner control points,
    slots 0..2), a hair inside or outside: the Newton result of such a ray is often on the neighbour's side."""
    rng = np.random.default_rng(seed)
    cp = patches[:, 19:49].reshape(len(patches), 10, 3).astype(np.float64)
    pts = []
    for a, b, c in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        u = rng.uniform(0.1, 0.9, (len(patches), per_edge, 1))
        on = (1 - u) * cp[:, None, a] + u * cp[:, None, b]
        pts.append(on + rng.uniform(-2e-3, 2e-3, u.shape) * (cp[:, None, c] - on))
    p = np.concatenate(pts, axis=1).reshape(-1, 3)
    # waves of 64 neighbouring rays, as an image's tiles are: strips of 1024 rays in y, each sorted by z
    p = p[np.argsort(p[:, 1], kind="stable")][:len(p) // 1024 * 1024].reshape(-1, 1024, 3)
    p = np.concatenate([s[np.argsort(s[:, 2], kind="stable")] for s in p])
    rays = np.zeros((6, len(p)), np.float32)
    rays[0] = p[:, 0].min() - 5.0
    rays[1], rays[2] = p[:, 1], p[:, 2]
    rays[3] = 1.0
    return rays


def test_follow_retries_join_and_park(bzr, orc, ctx, lens2, mesh2):
    rays = edge_rays(lens2)
    reps = three_ways(bzr, orc, ctx, lens2, mesh2, rays, "edge rays", ops=("chain", "intersect"))
    assert reps["chain"]["follows"] > 100 and reps["intersect"]["follows"] > 50
    assert all(r["overflow_rays"] == 0 for r in reps.values())


def test_inside_beside_outside(bzr, orc, ctx, lens2, mesh2):
    """Odd lanes start inside the lens (x = 10: the back surface is their only candidate), even lanes outside."""
    rays = grid_rays(CONFIGS["cfg2"], side=64).copy()
    rays[0, 1::2] = 10.0
    gate = orc.planar_gate(lens2, rays).sum(axis=1).reshape(-1, 64)
    assert ((gate[:, 0::2] == 2).all(axis=1) & (gate[:, 1::2] == 1).all(axis=1)).sum() >= 20
    three_ways(bzr, orc, ctx, lens2, mesh2, rays, "inside beside outside")


def test_full_scan_entry_source(bzr, orc, ctx, lens2, mesh2):
    """Every fourth lane's origin lies beyond the tree's radius: those lanes take the in-order scan, whose entries
    reach the same Newton site, in the same waves as lanes that walk the tree."""
    _, s_max = tier_radii(bzr, lens2)
    rays = grid_rays(CONFIGS["cfg2"], side=64).copy()
    far = np.arange(rays.shape[1]) % 4 == 3
    back = np.float32(2.0) * np.float32(s_max)  # the same lines, started 2 s_max further back
    rays[0, far] = rays[0, far] - back * rays[3, far]
    rays[1, far] = rays[1, far] - back * rays[4, far]
    rays[2, far] = rays[2, far] - back * rays[5, far]
    assert (np.abs(rays[:3, far]).max(axis=0) > s_max).all() and (np.abs(rays[:3, ~far]).max(axis=0) <= s_max).all()
    want = bits(orc.intersect(lens2, rays))
    assert (want[11][far] == bzr.WHAT_INTERSECT).sum() > 200  # far lanes that hit
    reps = three_ways(bzr, orc, ctx, lens2, mesh2, rays, "beyond the radius")
    assert reps["intersect"]["overflow_rays"] == int(far.sum())
    assert reps["chain"]["overflow_rays"] >= int(far.sum())


def test_always_list_entry_source(bzr, orc, ctx):
    """tests/test_culling_conservative.py's small lens with one rounding-dominated patch: the patch is in no tree, and
    every wave-segment gate-tests it from the always list.  The rays cross it (gate passes on that very patch)."""
    patches = dominated_lens(bzr)
    alw = always_list(bzr, patches, 0)
    assert len(alw) == 1
    side = 64
    y, z = np.meshgrid(np.linspace(-2.1, 2.1, side), np.linspace(-2.1, 2.1, side), indexing="ij")
    tile = (np.arange(side)[:, None] // 8 * (side // 8) + np.arange(side)[None, :] // 8) * 64 \
        + (np.arange(side)[:, None] % 8) * 8 + np.arange(side)[None, :] % 8  # 8 x 8 pixels per wave
    rays = np.zeros((6, side * side), np.float32)
    rays[0, tile.reshape(-1)] = -3.0
    rays[1, tile.reshape(-1)] = (y + DOMINATED_LENS_SHIFT[1]).reshape(-1)
    rays[2, tile.reshape(-1)] = (z + DOMINATED_LENS_SHIFT[2]).reshape(-1)
    rays[3] = 1.0
    # and a fan from beside the lens straight at the listed patch's control points
    cp = patches[alw[0], 19:49].reshape(10, 3).astype(np.float64)
    rng = np.random.default_rng(3)
    tgt = cp[rng.integers(0, 10, 1024)] * 0.7 + cp.mean(axis=0) * 0.3
    org = np.array(DOMINATED_LENS_SHIFT) + np.array([-4.0, 0.5, 0.5]) + rng.uniform(-0.2, 0.2, (1024, 3))
    d = tgt - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.ascontiguousarray(np.concatenate([rays, np.concatenate([org.T, d.T]).astype(np.float32)], axis=1))
    passes = orc.planar_gate(patches, rays)[:, alw[0]]
    print("gate passes on the always-listed patch:", int(passes.sum()))
    assert passes.sum() >= 20
    three_ways(bzr, orc, ctx, patches, bzr.DeviceMesh(ctx, patches), rays, "always list")


def test_nan_lanes(bzr, orc, ctx, lens2, mesh2, rays128):
    rays = rays128.copy()
    waves = rays.shape[1] // 64
    for row in range(6):  # a NaN in each component, on another lane of each wave
        at = np.arange(row, waves, 6) * 64 + (np.arange(row, waves, 6) * 7 + row) % 64
        rays[row, at] = np.float32(np.nan)
    three_ways(bzr, orc, ctx, lens2, mesh2, rays, "NaN lanes")


def test_fast_mode_equals_the_staged_fast_pipeline(bzr, ctx, lens2, mesh2, rays128):
    """FAST mode evaluates a (lane, patch, limit) with the same arithmetic wherever it runs.  The brute-force scan has
    no FAST mode (bzr.h: BZR_MODE_FAST needs the culled path), so FAST's scan is the staged pipeline, whose Newton
    stage runs behind the whole gate (k_traverse's): the fused kernel gives the same words."""
    fast = bzr.MODE_FAST
    got, rep = counted(ctx, lambda: bzr.intersect(ctx, mesh2, rays128, mode=bzr.PIPELINE_FUSED | fast))
    assert_same(got, bzr.intersect(ctx, mesh2, rays128, mode=bzr.PIPELINE_STAGED | fast), "fast intersect")
    assert rep["pairs"] > 0
    got, rep = counted(ctx, lambda: bzr.trace_chain(ctx, [mesh2], [RI], rays128, mode=bzr.PIPELINE_FUSED | fast))
    assert_same(got, bzr.trace_chain(ctx, [mesh2], [RI], rays128, mode=bzr.PIPELINE_STAGED | fast), "fast chain")
    assert rep["pairs"] > 0 and rep["follows"] > 0


@pytest.fixture(scope="module")
def chain64(bzr, orc, ctx):
    """cfg4's two lenses at 64 x 64, the oracle's chain and its work (shared; never changed)."""
    cfg = CONFIGS["cfg4"]
    lenses = [build_lens(bzr.TriMesh, l).bezier_patches() for l in cfg.lenses]
    rays = grid_rays(cfg, side=64)
    ri = [l.ri for l in cfg.lenses]
    want, work = oracle_counted(orc, lambda: orc.trace_chain(lenses, ri, rays))
    rays.setflags(write=False)
    return [bzr.DeviceMesh(ctx, p) for p in lenses], ri, rays, want, work


@pytest.mark.parametrize("kind", ["power", "spectral", "tir", "opl", "media"])
def test_the_kernels_that_share_trace_segment(bzr, ctx, chain64, kind):
    """One chain each through the power, spectral, TIR, optical-path and media kernels: fused (counters on) against the
    brute-force scan, every output word.  With one index per lens (power; the others get two channels) the geometry is
    the plain chain's, so the counted work is the oracle's there."""
    meshes, ri, rays, want, work = chain64
    n = rays.shape[1]
    chan = (np.arange(n) % 2).astype(np.uint8)
    table = np.array([[r, r + 0.05] for r in ri], np.float32)
    gaps = np.array([[1.0, 1.0], [1.2, 1.25], [1.0, 1.0]], np.float32)
    call = {
        "power": lambda m: bzr.trace_chain_power(ctx, meshes, ri, rays, mode=m),
        "spectral": lambda m: bzr.trace_chain_spectral(ctx, meshes, table, rays, chan, mode=m),
        "tir": lambda m: bzr.trace_chain_tir(ctx, meshes, table, rays, chan, max_bounces=3, mode=m),
        "opl": lambda m: bzr.trace_chain_opl(ctx, meshes, table, rays, chan, max_bounces=3, mode=m),
        "media": lambda m: bzr.trace_chain_media(ctx, meshes, table, gaps, rays, chan, max_bounces=3, mode=m),
    }[kind]
    got, rep = counted(ctx, lambda: call(bzr.PIPELINE_FUSED))
    assert_same(got, call(bzr.ACCEL_NONE), f"{kind}: fused against the brute-force scan")
    print(kind, rep, "plain chain, oracle", work)
    assert rep["pairs"] > 0 and rep["follows"] > 0 and rep["overflow_rays"] == 0
    if kind == "power":
        assert_same((got[0], got[2], got[3]), want, "power: rays, status, segments against the oracle's chain")
        assert_pairs(rep, work, kind)
