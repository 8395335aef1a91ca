"""Build-variant libraries (cuda-bezier-triangle-raytracer_amd/Makefile `variants`, built by build()).

stack4: libbzr with a 4-entry traversal stack (-DBZR_STACK=4).  Lanes whose walk runs out of stack
mid-walk switch to the reference's in-order full scan (reference/bezierMesh.cpp:206-227) while keeping
what the walk already found -- duplicates must collapse under the (t, scanned index) key and parked /
joined retry state must stay valid across the switch.  The default 64-entry stack never overflows on the
bench configs, so only this build exercises that path: fused == staged == brute force (and == the oracle
on cfg2), bit for bit, with the device counters reporting overflow rays.

dense1 / dense64: libbzr with the staged pair layout's two extremes (-DBZR_DENSE_MIN=1: every bucket's last
partial chunk padded, no sparse region; =64: no padding, every remainder in the sparse region): staged ==
brute force (== the oracle on cfg2 and the cfg4 chain) through only the dense or mostly the sparse kernel.

tracebundle / traceperlane: libbzr with k_trace's wave-bundle walk one tree level per batch (-DBZR_TRACE_WIDE=0;
the default takes two) and with k_trace's per-lane walk (-DBZR_TRACE_BUNDLE=0, round 3's default): the same
checks, fused == staged == brute force (== the oracle on cfg2), including the incoherent cfg5 rays whose wide
bundles take the per-lane node tests.

Every variant also runs tests/test_gpu_stacked.py's "dup" mesh (cfg1's lens 20.5 times over: exact ties, 40 / 41 / 42
gate passes beside 0 and 80..168), intersect and chain against the oracle: the staged overflow list is exactly the rays
past 40 gate passes (stack4: at least those), so listed and overflowed rays share waves, chunks and pooled passes.

Every variant also runs tests/test_gpu_long_chains.py's eight-lens chain and, from tests/test_gpu_ray_edges.py, the batch
with an origin of each tier-boundary class in every wave and the batch with NaN, infinite and scaled rays in every third
lane, against the oracle on all three modes: the 4-entry stack overflows mid-walk beside a NaN lane, and the per-lane
walk, the one-level walk and both staged pair layouts see those inputs.

Every variant also runs the cfg2 128^2 chain in BZR_MODE_FAST on both pipelines through tests/test_gpu_fast.py's gates
against the oracle (status, segments, exit directions): the kFast instantiations of each build.

Every variant last lowers the staged chunk cap to 192 rays (bzr_debug_chunk_cap, tests/test_gpu_chunks.py) and runs the
staged stacked-lens, tier-boundary and garbage jobs again against the same oracle words: the 4-entry stack's mid-walk
overflow and both pair-layout extremes at chunk offsets other than zero, 6 to 68 chunks per call.

The variant runs in a child process (BZR_LIBRARY selects the library; one process = one libbzr).
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
PKG = REPO / "cuda-bezier-triangle-raytracer_amd"

WORKER = r"""
import json, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import bzr_amd as bzr
from bzr_amd.configs import CONFIGS, build_lens, grid_rays, pixel_coords, rays_for
from oracle import pyoracle as orc

def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)

ctx = bzr.Context(0)
out = {}
# cfg2: one lens, the refraction chain, 256^2 primaries (oracle too)
lens = build_lens(bzr.TriMesh, CONFIGS["cfg2"].lenses[0]).bezier_patches()
dm = bzr.DeviceMesh(ctx, lens)
rays = grid_rays(CONFIGS["cfg2"], side=256)
want = orc.trace_chain([lens], [1.3], rays)
for name, mode in (("fused", bzr.PIPELINE_FUSED), ("staged", bzr.PIPELINE_STAGED), ("brute", bzr.ACCEL_NONE)):
    ctx.counters(True); ctx.counters_report()
    got = bzr.trace_chain(ctx, [dm], [1.3], rays, mode=mode)
    c = ctx.counters_report(); ctx.counters(False)
    out[f"cfg2_{name}_equal"] = all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))
    out[f"cfg2_{name}_overflow_rays"] = c["overflow_rays"]
# BZR_MODE_FAST in this build: the cfg2 128^2 chain through tests/test_gpu_fast.py's gates against the oracle
rays_f = grid_rays(CONFIGS["cfg2"], side=128)
wo, ws, wg = orc.trace_chain([lens], [1.3], rays_f)
for name, mode in (("fused", bzr.PIPELINE_FUSED), ("staged", bzr.PIPELINE_STAGED)):
    o, s, g = bzr.trace_chain(ctx, [dm], [1.3], rays_f, mode=mode | bzr.MODE_FAST)
    ok = (s == ws) & (ws != 0)
    out[f"fast_{name}_status_agree"] = float((s == ws).mean())
    out[f"fast_{name}_segments_agree"] = float((g == wg).mean())
    out[f"fast_{name}_exiting"] = int(ok.sum())
    out[f"fast_{name}_dir_p99"] = float(np.quantile(np.abs(o[3:6][:, ok] - wo[3:6][:, ok]).max(axis=0), 0.99))
# stacked cfg1 lens (tests/test_gpu_stacked.py's "dup"): 20 copies and the first half of a 21st, every hit an exact tie
# the first copy wins; 40, 41 and 42 gate passes beside 0 and 80..168, so listed and overflowed rays share waves
base = build_lens(orc.OMesh, CONFIGS["cfg1"].lenses[0]).bezier_patches()
def moved(p, k):
    q = p.copy()
    q.view(np.uint32)[:, 16:19] += np.uint32(k * len(p))  # the neighbour words stay inside copy k
    return q
stk = np.ascontiguousarray(np.concatenate([moved(base, k) for k in range(20)] + [base[:len(base) // 2]]))
dms = bzr.DeviceMesh(ctx, stk)
rs = grid_rays(CONFIGS["cfg1"], side=32)
want_hit, want_chain = bits(orc.intersect(stk, rs)), orc.trace_chain([stk], [1.3], rs)
out["stack_gate_over_40"] = int((orc.planar_gate(stk, rs).sum(axis=1) > 40).sum())
for name, mode in (("fused", bzr.PIPELINE_FUSED), ("staged", bzr.PIPELINE_STAGED), ("brute", bzr.ACCEL_NONE)):
    ctx.counters(True); ctx.counters_report()
    got = bits(bzr.intersect(ctx, dms, rs, mode=mode))
    c = ctx.counters_report(); ctx.counters(False)
    out[f"stack_{name}_equal"] = bool(np.array_equal(got, want_hit))
    out[f"stack_{name}_overflow_rays"] = c["overflow_rays"]
    got = bzr.trace_chain(ctx, [dms], [1.3], rs, mode=mode)
    out[f"stack_{name}_chain_equal"] = all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want_chain))
# tests/test_gpu_long_chains.py's eight-lens chain, and tests/test_gpu_ray_edges.py's seven tier-boundary classes in every
# wave and its garbage in every third lane (intersect and the one-lens chain on lens 0): the recipes are the tests' own
sys.path.append(sys.argv[2] + "/tests")
import test_gpu_long_chains as tl
import test_gpu_ray_edges as te
l8 = [tl.lens_patches(orc, k) for k in range(tl.N_LENS)]
d8 = [bzr.DeviceMesh(ctx, p) for p in l8]
s_near, s_max = te.tier_radii(bzr, l8[0])
_, tier_mix, _ = te.tier_batches(l8[0], te.tier_classes(s_near, s_max))
third, third_mask = te.poisoned(te.clean_batch(l8[0], s_near), "third")
out["edges_beyond_s_max"] = int((np.abs(tier_mix[:3]).max(axis=0) > s_max).sum())
out["edges_poisoned"] = int(third_mask.sum())
jobs = [("long8", tl.chain_rays(), "chain8"), ("tiers", tier_mix, "intersect"), ("tiers", tier_mix, "chain1"),
        ("third", third, "intersect"), ("third", third, "chain1")]
wants = {}
for label, rr, op in jobs:
    if op == "chain8":
        want_e = [bits(a) for a in orc.trace_chain(l8, [1.3] * tl.N_LENS, rr)]
        out["long8_full_length_rays"] = int((want_e[2] == 16).sum())
    else:
        want_e = wants[(label, op)] = te.run_orc(orc, l8, op, rr)[0]
    for name, mode in (("fused", bzr.PIPELINE_FUSED), ("staged", bzr.PIPELINE_STAGED), ("brute", bzr.ACCEL_NONE)):
        if op == "chain8":
            got_e = [bits(a) for a in bzr.trace_chain(ctx, d8, [1.3] * tl.N_LENS, rr, mode=mode)]
        else:
            got_e = te.run_gpu(bzr, ctx, d8, op, rr, mode)
        out[f"{label}_{op}_{name}_equal"] = not bool(te.differing(got_e, want_e).any())
# cfg5: 301 056 patches, BezierMesh::intersect on 65 536 grid rays from the lens's middle rows
cfg = CONFIGS["cfg5"]
p5 = build_lens(bzr.TriMesh, cfg.lenses[0]).bezier_patches()
dm5 = bzr.DeviceMesh(ctx, p5)
r, c = pixel_coords(cfg, side=8192, order="tiles")
mid = len(r) // 2
rays5 = rays_for(cfg, r[mid:mid + 65536], c[mid:mid + 65536], side=8192)
# plus incoherent rays from all around the lens (deep, diverging walks: the ones that overflow a tiny stack)
rng = np.random.default_rng(41)
o = rng.uniform(-12, 12, (16384, 3)) + np.array([10.0, 0.0, 0.0])
tgt = np.array([10.0, 0.0, 0.0]) + rng.uniform(-1, 1, (16384, 3)) * np.array([1.0, 4.0, 2.0])
dd = (tgt - o) / np.linalg.norm(tgt - o, axis=1, keepdims=True)
rays5 = np.concatenate([rays5, np.concatenate([o.T, dd.T]).astype(np.float32)], axis=1)
ref = bits(bzr.intersect(ctx, dm5, rays5, mode=bzr.ACCEL_NONE))
out["cfg5_hits"] = int((ref[11] == 4).sum())
for name, mode in (("fused", bzr.PIPELINE_FUSED), ("staged", bzr.PIPELINE_STAGED)):
    ctx.counters(True); ctx.counters_report()
    got = bits(bzr.intersect(ctx, dm5, rays5, mode=mode))
    cnt = ctx.counters_report(); ctx.counters(False)
    out[f"cfg5_{name}_equal"] = bool(np.array_equal(got, ref))
    out[f"cfg5_{name}_overflow_rays"] = cnt["overflow_rays"]
    out[f"cfg5_{name}_lane_chunks"] = cnt["lane_chunks"]
    out[f"cfg5_{name}_pairs"] = cnt["pairs"]
if "--more" in sys.argv:
    # cfg4: two lenses, the chain, 256^2 primaries: fused == brute force == the oracle
    l4 = [build_lens(bzr.TriMesh, l).bezier_patches() for l in CONFIGS["cfg4"].lenses]
    d4 = [bzr.DeviceMesh(ctx, p) for p in l4]
    r4 = grid_rays(CONFIGS["cfg4"], side=256)
    w4 = orc.trace_chain(l4, [1.3, 1.3], r4)
    for name, mode in (("fused", bzr.PIPELINE_FUSED), ("staged", bzr.PIPELINE_STAGED), ("brute", bzr.ACCEL_NONE)):
        g4 = bzr.trace_chain(ctx, d4, [1.3, 1.3], r4, mode=mode)
        out[f"cfg4_{name}_equal"] = all(np.array_equal(bits(g), bits(w)) for g, w in zip(g4, w4))
    # origins beyond s_max mixed into the waves (the in-order scan): robot.stl, 25 % far
    lr = build_lens(bzr.TriMesh, CONFIGS["cfg3"].lenses[0].__class__("stl", split=1)).bezier_patches()
    dr = bzr.DeviceMesh(ctx, lr)
    rng = np.random.default_rng(11)
    o = rng.uniform(-30, 30, (3, 4096)).astype(np.float32)
    far = rng.random(4096) < 0.25
    o[0, far] = np.float32(-5e4)
    t = rng.uniform(-20, 20, (3, 4096)).astype(np.float32)
    dd = t - o
    dd /= np.sqrt((dd * dd).sum(axis=0, keepdims=True)).astype(np.float32)
    rr = np.concatenate([o, dd.astype(np.float32)]).astype(np.float32)
    ctx.counters(True); ctx.counters_report()
    gf = bits(bzr.intersect(ctx, dr, rr, mode=bzr.PIPELINE_FUSED))
    cnt = ctx.counters_report(); ctx.counters(False)
    out["far_fused_equal"] = bool(np.array_equal(gf, bits(orc.intersect(lr, rr))))
    out["far_overflow_rays"] = cnt["overflow_rays"]
    out["far_count"] = int(far.sum())
# the staged stack, tiers and third jobs again in chunks of at most 192 rays (bzr_debug_chunk_cap, tests/test_gpu_chunks.py),
# against the oracle words computed above: this build's overflow paths and pair layout at chunk offsets other than zero
import ctypes
eff = ctypes.c_uint32(0)
assert bzr.lib().bzr_debug_chunk_cap(ctx.handle, 192, ctypes.byref(eff)) == 0
out["chunk_cap"] = eff.value
ctx.counters(True); ctx.counters_report()
got = bits(bzr.intersect(ctx, dms, rs, mode=bzr.PIPELINE_STAGED))
c = ctx.counters_report(); ctx.counters(False)
out["stack_staged192_equal"] = bool(np.array_equal(got, want_hit))
out["stack_staged192_overflow_rays"] = c["overflow_rays"]
got = bzr.trace_chain(ctx, [dms], [1.3], rs, mode=bzr.PIPELINE_STAGED)
out["stack_staged192_chain_equal"] = all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want_chain))
for label, rr, op in jobs[1:]:
    got_e = te.run_gpu(bzr, ctx, d8, op, rr, bzr.PIPELINE_STAGED)
    out[f"{label}_{op}_staged192_equal"] = not bool(te.differing(got_e, wants[(label, op)]).any())
print(json.dumps(out))
"""


def assert_edge_inputs_ran(out):
    """The long chain, the tier boundaries and the garbage lanes were traced on all three modes, over the populations
    tests/test_gpu_long_chains.py and tests/test_gpu_ray_edges.py assert."""
    keys = [k for k in out if k.endswith("_equal") and k.split("_")[0] in ("long8", "tiers", "third")]
    assert len(keys) == 19, keys  # 5 jobs x 3 modes, and the tiers and third jobs staged in chunks of 192 rays
    assert out["chunk_cap"] == 192 and "stack_staged192_equal" in out and "stack_staged192_chain_equal" in out, out
    assert out["stack_staged192_overflow_rays"] == out["stack_staged_overflow_rays"], out
    assert out["long8_full_length_rays"] >= 2000 and out["edges_beyond_s_max"] > 1000 and out["edges_poisoned"] > 2000, out


def assert_fast_gates(out):
    """BZR_MODE_FAST in the variant build: tests/test_gpu_fast.py's chain gates (cfg2, 128^2) on both pipelines."""
    for name in ("fused", "staged"):
        assert out[f"fast_{name}_exiting"] > 1000, out
        assert out[f"fast_{name}_status_agree"] >= 0.995 and out[f"fast_{name}_segments_agree"] >= 0.99, (name, out)
        assert out[f"fast_{name}_dir_p99"] < 1e-3, (name, out)


@pytest.mark.gpu
def test_tiny_stack_overflow_path_is_exact():
    lib = PKG / "lib" / "stack4" / "libbzr.so"
    if not lib.exists():
        pytest.fail(f"{lib} missing: build() makes the `variants` target")
    env = dict(os.environ, BZR_LIBRARY=str(lib))
    res = subprocess.run([sys.executable, "-c", WORKER, str(PKG), str(REPO)], env=env, capture_output=True,
                         text=True, timeout=110)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    for k, v in out.items():
        if k.endswith("_equal"):
            assert v, (k, out)
    assert_edge_inputs_ran(out)
    assert_fast_gates(out)
    # the tiny stack really overflowed on both pipelines (the brute-force scan has no stack)
    for k in ("cfg2_fused", "cfg2_staged", "cfg5_fused", "cfg5_staged"):
        assert out[f"{k}_overflow_rays"] > 0, (k, out)
    # the stacked lens: the walk runs out of stack while the candidate list overflows too
    assert out["stack_fused_overflow_rays"] > 0 and out["stack_staged_overflow_rays"] >= out["stack_gate_over_40"] > 0, out
    assert out["cfg5_hits"] > 10000


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["tracebundle", "traceperlane"])
def test_trace_bundle_walk_is_exact(variant):
    """k_trace's other walks (one level per batch; per lane): exact, and only the far origins take the in-order
    scan (round 3's 4096-of-1026 count came from a pre-release bundle walk whose full-stack batches sent whole
    incoherent waves to the scan; the released one tests wide bundles per lane --
    profiles/r04_bundle_overflow_probe.jsonl)."""
    lib = PKG / "lib" / variant / "libbzr.so"
    if not lib.exists():
        pytest.fail(f"{lib} missing: build() makes the `variants` target")
    env = dict(os.environ, BZR_LIBRARY=str(lib))
    res = subprocess.run([sys.executable, "-c", WORKER, str(PKG), str(REPO), "--more"], env=env, capture_output=True,
                         text=True, timeout=110)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    for k, v in out.items():
        if k.endswith("_equal"):
            assert v, (k, out)
    assert_edge_inputs_ran(out)
    assert_fast_gates(out)
    assert out["far_overflow_rays"] == out["far_count"]
    assert out["cfg2_fused_overflow_rays"] == 0
    # the stacked lens: k_traverse's walk is the default one; k_trace's one-level-per-batch bundle walk (tracebundle)
    # runs out of its 64-entry stack on two waves of the 21 coincident boxes (128 overflow rays measured), which take
    # the in-order scan -- the same bits, checked above; the per-lane walk does not
    assert out["stack_staged_overflow_rays"] == out["stack_gate_over_40"] > 0, out
    if variant == "traceperlane":
        assert out["stack_fused_overflow_rays"] == 0, out
    assert out["cfg5_hits"] > 10000


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["dense1", "dense64"])
def test_staged_pair_layout_extremes_are_exact(variant):
    """The staged path with every remainder padded (dense1) or none (dense64): bit-identical to the brute-force
    scan and the oracle; dense1 runs no sparse chunk, dense64 runs every bucket remainder per lane."""
    lib = PKG / "lib" / variant / "libbzr.so"
    if not lib.exists():
        pytest.fail(f"{lib} missing: build() makes the `variants` target")
    env = dict(os.environ, BZR_LIBRARY=str(lib))
    res = subprocess.run([sys.executable, "-c", WORKER, str(PKG), str(REPO), "--more"], env=env,
                         capture_output=True, text=True, timeout=110)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    for k, v in out.items():
        if k.endswith("_equal"):
            assert v, (k, out)
    assert_edge_inputs_ran(out)
    assert_fast_gates(out)
    assert out["stack_fused_overflow_rays"] == 0 and out["stack_staged_overflow_rays"] == out["stack_gate_over_40"] > 0, out
    if variant == "dense1":
        assert out["cfg5_staged_lane_chunks"] == 0, out
    else:
        assert out["cfg5_staged_lane_chunks"] > 0, out
