"""Split leaf gate boxes on the device (csrc/host/bvh.cpp split_cells, trace.hip bundle_batch `seen`): the fused
refract and chain kernels walk trees in which a patch has one leaf reference per strip of its gate region, and a
per-wave bit set queues each leaf slot once per wave-segment.  Every output must still be the brute-force scan's,
bit for bit, on both pipelines; in FAST mode, which the scan does not offer (BZR_MODE_FAST needs the culled path),
the reference is the staged pipeline, which walks the unsplit tree: the same candidate pairs through the same FAST
Newton arithmetic give the same bits.  A wave whose bundle straddles a strip boundary of one
patch must gate-test that patch once (leaf fetches = the distinct slots of the host replay), and the staged
pipeline must list each (ray, patch) pair once."""
import numpy as np
import pytest

from bzr_amd.configs import CONFIGS, build_lens, grid_rays
from test_split_leaves import replay, split_boxes

pytestmark = pytest.mark.gpu

SCENES = ["cfg2", "cfg4"]


def _same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def scenes(bzr, ctx):
    """name -> (patch arrays, device meshes, indices, 64x64 primaries) of cfg2's one-lens scene and cfg4's chain."""
    out = {}
    for name in SCENES:
        cfg = CONFIGS[name]
        patches = [build_lens(bzr.TriMesh, l).bezier_patches() for l in cfg.lenses]
        out[name] = (patches, [bzr.DeviceMesh(ctx, p) for p in patches], [l.ri for l in cfg.lenses], grid_rays(cfg, side=64))
    return out


@pytest.fixture(scope="module")
def scan(bzr, ctx, scenes):
    """(scene, arithmetic mode) -> the reference's chain, intersect and refract outputs, computed once: the
    brute-force scan in parity mode, the staged pipeline (unsplit tree) in FAST mode."""
    out = {}
    for name, (_, meshes, ri, rays) in scenes.items():
        for m in (bzr.ACCEL_NONE | bzr.MODE_PARITY, bzr.PIPELINE_STAGED | bzr.MODE_FAST):
            out[name, m & bzr.MODE_FAST] = (bzr.trace_chain(ctx, meshes, ri, rays, mode=m),
                                            (bzr.intersect(ctx, meshes[0], rays, mode=m),),
                                            bzr.refract(ctx, meshes[0], ri[0], rays, mode=m))
    return out


@pytest.mark.parametrize("fast", ["parity", "fast"])
@pytest.mark.parametrize("name", SCENES)
def test_split_tree_bits_match_the_scan(bzr, ctx, scenes, scan, pipe, name, fast):
    _, meshes, ri, rays = scenes[name]
    fm = bzr.MODE_FAST if fast == "fast" else bzr.MODE_PARITY
    want_chain, want_hits, want_refract = scan[name, fm]
    assert int(np.asarray(want_chain[2]).sum()) > rays.shape[1] // 2  # the rays do go through the lens
    m = pipe | fm
    assert _same(bzr.trace_chain(ctx, meshes, ri, rays, mode=m), want_chain)
    assert _same((bzr.intersect(ctx, meshes[0], rays, mode=m),), want_hits)
    assert _same(bzr.refract(ctx, meshes[0], ri[0], rays, mode=m), want_refract)


@pytest.fixture(scope="module")
def straddle(bzr, scenes):
    """A 64-ray wave fanned +-1 strip width about an interior strip boundary of one front patch of cfg2's lens: a
    common origin inside the near radius, targets along the strips' axis through the boundary."""
    patches = scenes["cfg2"][0][0]
    who, boxes, _, _ = split_boxes(bzr, patches, 1, 0)  # the near tier's leaf references
    cp = patches[:, 19:28].reshape(-1, 3, 3).astype(np.float64)  # corner control points
    centre = cp.mean(axis=1)
    front = np.argmin(np.abs(centre[:, 1] - 0.7) + np.abs(centre[:, 2] - 0.4) + 10.0 * (centre[:, 0] > 10.0))
    bx = boxes[who == front].astype(np.float64)
    assert len(bx) >= 3, "the patch is split into strips"
    ext = bx[:, 3:].max(axis=0) - bx[:, :3].min(axis=0)
    axis = int(np.argmax(ext))
    bx = bx[np.argsort(bx[:, axis])]
    edge = 0.5 * (bx[1, 3 + axis] + bx[2, axis])  # between the second and the third strip
    width = ext[axis] / len(bx)
    tgt = np.repeat(centre[front][None, :], 64, axis=0)
    tgt[:, axis] = edge + np.linspace(-1.0, 1.0, 64) * width
    o = np.array([0.0, centre[front][1], centre[front][2]])
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return patches, np.concatenate([np.repeat(o[None, :], 64, axis=0).T, d.T]).astype(np.float32)


def test_straddling_wave_matches_the_scan(bzr, ctx, scenes, straddle, pipe):
    _, rays = straddle
    _, meshes, ri, _ = scenes["cfg2"]
    want = bzr.refract(ctx, meshes[0], ri[0], rays, mode=bzr.ACCEL_NONE)
    assert (np.asarray(want[1]) == bzr.RR_INSIDE).sum() >= 32  # most of the fan enters the lens
    assert _same(bzr.refract(ctx, meshes[0], ri[0], rays, mode=pipe), want)
    assert _same(bzr.trace_chain(ctx, meshes, ri, rays, mode=pipe), bzr.trace_chain(ctx, meshes, ri, rays, mode=bzr.ACCEL_NONE))


def test_straddling_wave_fetches_each_slot_once(bzr, ctx, scenes, straddle):
    """leaf_fetches of the wave's one fused refract segment = the distinct slots its walk reaches, not the
    references: the count comes from the host replay of the device's two-level walk."""
    patches, rays = straddle
    mesh = scenes["cfg2"][1][0]
    st, slots = replay(bzr, patches, rays, 0)
    assert st[0] == 1 and st[8] == 0  # one wave, on the bundle walk
    assert st[12] > st[2], "the bundle reaches a slot through more than one reference"
    assert slots[0, 1] != 0xFFFFFFFF
    ctx.counters(True)
    ctx.counters_report()
    bzr.refract(ctx, mesh, scenes["cfg2"][2][0], rays, mode=bzr.PIPELINE_FUSED)
    got = ctx.counters_report()
    ctx.counters(False)
    assert got["segments"] == 64 and got["overflow_rays"] == 0
    assert got["leaf_fetches"] == int(slots[0, 1])


def test_straddling_wave_staged_lists_each_pair_once(bzr, orc, ctx, scenes, straddle):
    """The staged pipeline's candidate pairs of the wave are the oracle's gate passes: no (ray, patch) pair twice."""
    patches, rays = straddle
    mesh = scenes["cfg2"][1][0]
    ctx.counters(True)
    ctx.counters_report()
    bzr.refract(ctx, mesh, scenes["cfg2"][2][0], rays, mode=bzr.PIPELINE_STAGED)
    got = ctx.counters_report()
    ctx.counters(False)
    orc.counters_reset()
    orc.refract(patches, scenes["cfg2"][2][0], rays, np.full(64, bzr.RR_INSIDE, np.uint32))
    want = orc.counters()
    assert got["overflow_rays"] == 0
    assert got["pairs"] == want["newton"] and got["follows"] == want["follow"]
