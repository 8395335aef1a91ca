"""The short Newton pass on the host: newton_tail with its hook answering "not needed" (the last iteration's
surface normal skipped; csrc/device/patch_math_body.inc) against the whole evaluation, through the debug export
bzr_debug_newton_short (include/bzr_debug.h).

The fused kernel takes the short form for passes none of whose lanes can win (trace.hip BZR_TRACE_SHORT).  Such a
pass still owes t, the point, the barycentrics and the classification: the acceptance test and the divider planes
read the point, and the classification decides whether a follow-side retry runs.  So those words must equal the whole
evaluation's bit for bit; the normal and the cosine are the only words the short form may leave out.

2^16 (patch, ray, limit) triples aimed at the patches of four meshes -- the cfg2 lens, the cfg1 sphere, robot.stl and
the lens at the origin -- with both limits, and with rays that end NONE, follow-side and with a NaN t (asserted
below, so the comparison is not vacuous on any of them).
"""
import ctypes
import dataclasses

import numpy as np
import pytest

from bzr_amd.configs import CONFIGS, Lens, build_lens

PER_MESH = 1 << 14  # x 4 meshes = 2^16 triples
T, POINT, COS, BARY, NORMAL, WHAT = slice(0, 1), slice(1, 4), slice(4, 5), slice(5, 8), slice(8, 11), slice(11, 12)


def meshes(bzr):
    origin = Lens("ellipsoid", 32, 16, (1.0, 4.0, 2.0), (0.0, 0.0, 0.0))
    robot = dataclasses.replace(CONFIGS["cfg3"].lenses[0], split=1)
    recipes = {"cfg2 lens": CONFIGS["cfg2"].lenses[0], "cfg1 sphere": CONFIGS["cfg1"].lenses[0], "robot.stl": robot,
               "origin lens": origin}
    return {k: build_lens(bzr.TriMesh, v).bezier_patches() for k, v in recipes.items()}


def triples(patches, n, rng):
    """(patch index, rays [6, n], limit) aimed at the flat triangles under the patches (control points 300, 030,
    003: words 19..27 of the record).  Four classes of aim point, in barycentrics of that triangle: inside; around
    the edges (-0.5 .. 1.5: NONE and follow-side results); inside but grazing; and, with cNone, 10^3 .. 10^16
    triangle sizes away, where the extrapolated cubic overflows and t ends NaN."""
    idx = rng.integers(0, len(patches), n).astype(np.uint32)
    corners = patches[idx][:, 19:28].astype(np.float64).reshape(n, 3, 3)
    normal = patches[idx][:, 0:3].astype(np.float64)
    limit = rng.integers(0, 2, n).astype(np.uint8)
    kind = rng.choice(4, n, p=[0.5, 0.25, 0.125, 0.125])
    b = rng.dirichlet([1.0, 1.0, 1.0], n)
    around = rng.uniform(-0.5, 1.5, (n, 2))
    b[kind == 1] = np.column_stack([around, 1.0 - around.sum(axis=1)])[kind == 1]
    far = (10.0 ** rng.uniform(3, 16, n))[:, None] * rng.normal(size=(n, 2))
    b[kind == 3] = np.column_stack([far, 1.0 - far.sum(axis=1)])[kind == 3]
    limit[kind == 3] = 1
    target = np.einsum("nk,nkc->nc", b, corners)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    graze = kind == 2  # mostly in the plane, a little along the normal
    d[graze] = d[graze] - (1.0 - rng.uniform(0.0, 0.2, n))[graze, None] * np.einsum("nc,nc->n", d, normal)[graze, None] * normal[graze]
    steep = kind == 3  # along the normal, from either side
    d[steep] = normal[steep] * rng.choice([-1.0, 1.0], n)[steep, None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    size = np.linalg.norm(corners[:, 1] - corners[:, 0], axis=1)
    s = target - d * (size * rng.uniform(0.5, 20.0, n))[:, None]
    return idx, np.ascontiguousarray(np.concatenate([s.T, d.T]).astype(np.float32)), limit


def newton_short(bzr, patches, idx, rays, limit):
    fn = bzr.lib().bzr_debug_newton_short
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = ctypes.c_int32
    p = np.ascontiguousarray(patches, np.float32)
    m = len(idx)
    full, skipped = np.zeros((m, 12), np.float32), np.full((m, 12), 7.0, np.float32)
    assert fn(p.ctypes.data, len(p), 264, idx.ctypes.data, rays.ctypes.data, limit.ctypes.data, m, full.ctypes.data,
              skipped.ctypes.data) == 0
    return full.view(np.uint32), skipped.view(np.uint32)


@pytest.fixture(scope="module")
def runs(bzr):
    out = {}
    for k, (name, patches) in enumerate(meshes(bzr).items()):
        idx, rays, limit = triples(patches, PER_MESH, np.random.default_rng(100 + k))
        out[name] = (patches, idx, rays, limit, *newton_short(bzr, patches, idx, rays, limit))
    return out


def test_the_triples_reach_every_kind_of_result(bzr, runs):
    assert sum(len(r[1]) for r in runs.values()) == 1 << 16
    nan_total = 0
    for name, (_, _, _, limit, full, _) in runs.items():
        what, t = full[:, 11], full[:, 0].view(np.float32)
        ran = (full[:, 1:4] != 0).any(axis=1)  # the gate passed: Newton produced a point
        print(name, "intersect", int((what == 4).sum()), "none after Newton", int((ran & (what == 3)).sum()),
              "follow", int((what <= 2).sum()), "NaN t", int(np.isnan(t).sum()), "cNone", int(limit.sum()))
        assert (what == bzr.WHAT_INTERSECT).sum() > 2000, name
        assert (ran & (what == bzr.WHAT_NONE)).sum() > 200, name
        assert (what <= bzr.WHAT_FOLLOW2).sum() > 200, name
        for lim in (0, 1):  # both limits run Newton and intersect
            assert ((limit == lim) & (what == bzr.WHAT_INTERSECT)).sum() > 1000, (name, lim)
        nan_total += int(np.isnan(t).sum())
    assert nan_total > 100


def test_skipping_the_last_normal_changes_nothing_else(runs):
    for name, (_, _, _, _, full, skipped) in runs.items():
        for words, label in ((T, "t"), (POINT, "point"), (BARY, "barycentrics"), (WHAT, "what")):
            bad = (full[:, words] != skipped[:, words]).any(axis=1)
            assert not bad.any(), f"{name}: {label} differs on {int(bad.sum())} of {len(bad)} triples"
        # and the hook did skip: a whole normal is a unit vector, the skipped evaluation leaves zeros
        hit = full[:, 11] == 4
        assert (skipped[hit][:, NORMAL] == 0).all() and (full[hit][:, NORMAL] != 0).any(axis=1).all(), name


def test_the_whole_evaluation_is_the_oracles(orc, runs):
    """The export's `full` side is the host's BezierTriangle::intersect: the oracle's bits (a sample of each mesh)."""
    for name, (patches, idx, rays, limit, full, _) in runs.items():
        pick = np.arange(0, PER_MESH, 16)
        want = orc.patch_intersect(patches, idx[pick], limit[pick], rays[:, pick]).view(np.uint32)[:12].T
        assert np.array_equal(full[pick], want), name
