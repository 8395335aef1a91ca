"""Split leaf gate boxes (csrc/host/bvh.cpp split_cells): the fused refract and chain kernels walk a tree in which
every narrow patch has one leaf reference per strip of its gate region, all naming the patch's one leaf slot.
Culling stays exact only if the strips' boxes together cover the patch's proven gate region: every extreme point
of the region, and every float plane point that passes the oracle's planar gate, must lie in a cell box of its
patch.  The leaf slots themselves (order, patch_box) are those of the unsplit build, a mesh above the slot cap is
not split at all, and the bundle walk on the split tree misses no leaf a lane reaches.  CPU only."""
import ctypes

import numpy as np
import pytest

from bzr_amd.configs import CONFIGS, build_lens, grid_rays
from test_culling_conservative import coherent_waves, gate_boxes
from test_gpu_fuzz import _lens

TIERS = [0, 1]  # bvh.hpp kTierFar, kTierNear
SPLITS = [0, 3]  # 0: the split the kernels use (bvh.hpp kSplitDefault)
SLOT_CAP = 8192  # bvh.hpp kSplitSlotCap
_P, _U32, _I32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32


def split_boxes(bzr, patches, tier, split):
    """Leaf references of the device tree: patch per reference, box per reference, and the build's order and patch_box."""
    fn = bzr.lib().bzr_debug_split_boxes
    fn.argtypes = [_P, _U32, _U32, _I32, _I32, _P, _P, _P, _P, _P]
    fn.restype = _I32
    p = np.ascontiguousarray(patches, np.float32)
    cnt = np.zeros(1, np.uint32)
    assert fn(p.ctypes.data, len(p), 264, tier, split, None, None, cnt.ctypes.data, None, None) == 0
    who, boxes = np.zeros(int(cnt[0]), np.uint32), np.zeros((int(cnt[0]), 6), np.float32)
    order, pbox = np.zeros(len(p), np.uint32), np.zeros((len(p), 8), np.float32)
    assert fn(p.ctypes.data, len(p), 264, tier, split, who.ctypes.data, boxes.ctypes.data, cnt.ctypes.data,
              order.ctypes.data, pbox.ctypes.data) == 0
    return who, boxes, order, pbox


def region_points(bzr, patches, tier):
    fn = bzr.lib().bzr_debug_region_points
    fn.argtypes = [_P, _U32, _U32, _I32, _P, _P, _P]
    fn.restype = _I32
    p = np.ascontiguousarray(patches, np.float32)
    cnt = np.zeros(1, np.uint32)
    assert fn(p.ctypes.data, len(p), 264, tier, None, None, cnt.ctypes.data) == 0
    who, pts = np.zeros(int(cnt[0]), np.uint32), np.zeros((int(cnt[0]), 3), np.float64)
    assert fn(p.ctypes.data, len(p), 264, tier, who.ctypes.data, pts.ctypes.data, cnt.ctypes.data) == 0
    return who, pts


def nodes4(bzr, patches, tier, split):
    fn = bzr.lib().bzr_debug_nodes4
    fn.argtypes = [_P, _U32, _U32, _I32, _I32, _P, _P]
    fn.restype = _I32
    p = np.ascontiguousarray(patches, np.float32)
    cnt = np.zeros(1, np.uint32)
    assert fn(p.ctypes.data, len(p), 264, tier, split, None, cnt.ctypes.data) == 0
    out = np.zeros(int(cnt[0]) * 128, np.uint8)
    assert fn(p.ctypes.data, len(p), 264, tier, split, out.ctypes.data, cnt.ctypes.data) == 0
    return out


def replay(bzr, patches, rays, split):
    fn = bzr.lib().bzr_debug_traverse_bundle_split
    fn.argtypes = [_P, _U32, _U32, _P, _U32, ctypes.c_float, _I32, _P, _P]
    fn.restype = _I32
    p, r = np.ascontiguousarray(patches, np.float32), np.ascontiguousarray(rays, np.float32)
    st, slots = np.zeros(16, np.uint64), np.zeros(((r.shape[1] + 63) // 64, 2), np.uint32)
    assert fn(p.ctypes.data, len(p), 264, r.ctypes.data, r.shape[1], np.float32(np.inf), split, st.ctypes.data,
              slots.ctypes.data) == 0
    return st, slots


def plane_points_f32(patches, rays, ri, pi):
    """The float plane point of (ray ri[k], patch pi[k]) in the gate's own operation order (bvh.cpp planar_gate_h)."""
    f = np.float32
    n, c = patches[pi, 0:3].astype(f), patches[pi, 3].astype(f)
    s, d = rays[:3, ri].T.astype(f), rays[3:, ri].T.astype(f)
    cs = d[:, 0] * n[:, 0] + (d[:, 1] * n[:, 1] + d[:, 2] * n[:, 2])
    t = (c - (n[:, 0] * s[:, 0] + (n[:, 1] * s[:, 1] + n[:, 2] * s[:, 2]))) / cs
    return (s + d * t[:, None]).astype(f)


def uncovered(who, boxes, pw, pts):
    """How many points (patch pw[k], pts[k]) lie in no cell box of their patch."""
    by = np.argsort(who, kind="stable")
    who, boxes = who[by], boxes[by].astype(np.float64)
    first, last = np.searchsorted(who, pw, "left"), np.searchsorted(who, pw, "right")
    bad = 0
    for b in np.unique(pw):
        sel = pw == b
        bx = boxes[first[sel][0]:last[sel][0]]
        p = pts[sel].astype(np.float64)[:, None, :]
        inside = ((bx[None, :, :3] <= p) & (p <= bx[None, :, 3:])).all(axis=2).any(axis=1)
        bad += int((~inside).sum())
    return bad


def _aimed_rays(patches, rng, n):
    cp = patches[:, 19:49].reshape(-1, 3).astype(np.float64)
    span = float(np.abs(cp.max(0) - cp.min(0)).max())
    tgt = cp[rng.integers(0, len(cp), n)] + rng.normal(size=(n, 3)) * span * 0.01
    o = tgt + rng.normal(size=(n, 3)) * span * rng.uniform(0.2, 2.0, (n, 1))
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o.T, d.T]).astype(np.float32)


@pytest.fixture(scope="module")
def meshes(bzr, orc):
    """name -> (patches, rays, gate-passing (ray, patch) pairs): cfg2's lens, cfg4's second lens, one fuzz lens."""
    out = {}
    for name, cfg, lens in (("cfg2", CONFIGS["cfg2"], 0), ("cfg4", CONFIGS["cfg4"], 1)):
        patches = build_lens(bzr.TriMesh, cfg.lenses[lens]).bezier_patches()
        rays = np.concatenate([grid_rays(cfg, side=96), _aimed_rays(patches, np.random.default_rng(3), 6000)], axis=1)
        out[name] = (patches, rays)
    patches, rng = _lens(bzr, 4)
    assert patches is not None
    out["fuzz"] = (patches, _aimed_rays(patches, rng, 30000))
    for name, (patches, rays) in out.items():
        ri, pi = np.nonzero(orc.planar_gate(patches, rays, threads=8))
        out[name] = (patches, rays, ri, pi)
    return out


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", ["cfg2", "cfg4", "fuzz"])
def test_cell_boxes_cover_the_gate_region(bzr, meshes, name, tier, split):
    patches, rays, ri, pi = meshes[name]
    who, boxes, order, pbox = split_boxes(bzr, patches, tier, split)
    assert len(who) > 1.5 * len(patches), "the mesh is split"
    # every extreme point of every proven region lies in a cell box of its patch
    vw, vpts = region_points(bzr, patches, tier)
    in_tree = np.isin(vw, who)
    assert in_tree.mean() > 0.9
    assert uncovered(who, boxes, vw[in_tree], vpts[in_tree]) == 0
    # and so does every gate-passing float plane point of a ray that starts within the tier's radius
    _, smax = gate_boxes(bzr, patches, tier)
    ok = (np.abs(rays[:3, ri]).max(axis=0) <= smax) & np.isin(pi, who)
    assert ok.sum() >= 10000, int(ok.sum())
    pts = plane_points_f32(patches, rays, ri[ok], pi[ok])
    assert uncovered(who, boxes, pi[ok].astype(np.uint32), pts) == 0
    # a cell box lies within its patch's whole-region box
    slot_of = np.empty(len(patches), np.int64)
    slot_of[order] = np.arange(len(patches))
    whole = pbox[slot_of[who]]
    assert (boxes[:, :3] >= whole[:, 0:3]).all() and (boxes[:, 3:] <= whole[:, 4:7]).all()


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", ["cfg2", "fuzz"])
def test_leaf_slots_are_the_unsplit_build_s(bzr, meshes, name, tier):
    patches = meshes[name][0]
    who1, boxes1, order1, pbox1 = split_boxes(bzr, patches, tier, 1)
    who, _, order, pbox = split_boxes(bzr, patches, tier, 0)
    assert np.array_equal(np.sort(order), np.arange(len(patches)))
    assert np.array_equal(order, order1) and np.array_equal(pbox.view(np.uint32), pbox1.view(np.uint32))
    assert len(who1) == len(np.unique(who1)) and set(who1) == set(who)  # one reference per patch; the same patches
    # the unsplit tree's leaf boxes are the per-patch gate boxes the existing culling tests pin
    gb, _ = gate_boxes(bzr, patches, tier)
    assert np.array_equal(boxes1.view(np.uint32), gb[who1].view(np.uint32))
    assert np.bincount(who).max() <= 6  # bvh.hpp kSplitDefault strips at most


def test_mesh_above_the_slot_cap_is_not_split(bzr):
    patches = bzr.TriMesh().make_ellipsoid(56, 26, (1.0, 4.0, 2.0)).translate((10.0, 0.0, 0.0)).standardize().bezier_patches()
    assert len(patches) > SLOT_CAP + 200
    for tier in TIERS:
        assert np.array_equal(nodes4(bzr, patches, tier, 0), nodes4(bzr, patches, tier, 1))
    small = build_lens(bzr.TriMesh, CONFIGS["cfg2"].lenses[0]).bezier_patches()
    assert len(nodes4(bzr, small, 0, 0)) > len(nodes4(bzr, small, 0, 1))


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", ["cfg2", "cfg4"])
def test_bundle_walk_on_the_split_tree_keeps_every_lane_leaf(bzr, name, split):
    """The host replay behind test_bundle_walk_keeps_every_lane_leaf on the split tree: config primaries (8x8 tiles)
    and coherent random waves."""
    cfg = CONFIGS[name]
    patches = build_lens(bzr.TriMesh, cfg.lenses[-1]).bezier_patches()
    rng = np.random.default_rng(11)
    cp = patches[:, 19:49].reshape(-1, 10, 3)
    lo, hi = cp.min(axis=(0, 1)), cp.max(axis=(0, 1))
    centre, spread = (lo + hi) / 2, float((hi - lo).max()) / 2
    for rays in (grid_rays(cfg, side=256), coherent_waves(rng, 150, centre, spread, 1e-3),
                 coherent_waves(rng, 150, centre, spread, 3e-2)):
        st, slots = replay(bzr, patches, rays, split)
        assert st[0] > 0 and st[4] > 0 and st[14] > 1.5 * len(patches)
        assert st[5] == 0, f"bundle walk missed {int(st[5])} leaf slots"
        assert st[11] == 0
        assert st[12] >= st[2] == slots[:, 0].sum()  # references reached >= distinct slots queued
        assert (slots[:, 1] >= slots[:, 0]).all()  # the two-level walk reaches a superset
