#!/usr/bin/env python3
"""Host cost of split leaf gate boxes (bvh.cpp split_cells): the bundle walk replayed on trees whose narrow
patches' gate regions are cut into K = 1, 2, 3, 4, 6, 8 strips, one leaf reference each, all naming the patch's slot.

Waves are 8x8-pixel tiles sampled uniformly over the whole image, so the figures are frame averages; the rays
of every chain segment come from the oracle (refract inside / outside per lens), dead lanes are inactive.  A
"wave-segment" is 64 ray-segments, as in bench.py's leaf_fetches_per_wave_segment: totals are divided by the
active (wave, lane) pairs / 64.  Printed per K: distinct leaf slots the 4-wide bundle walk queues and the device's
two-level walk queues (what k_trace gate-tests, once per slot with the per-wave slot set), leaf references reached
(what it would gate-test without the set), nodes visited, batches, the tree's leaf references, and the model cost
75 x slots + batch_cost x batches in VALU per wave-segment (75: one leaf fetch's planar gates, DESIGN.md (d);
batch_cost: one 16-node batch of bundle box tests, ~60 VALU).  missed must be 0 for every K.
usage: python scripts/split_sim.py [--configs cfg4 cfg2] [--waves 4096] [--seed 1] [--batch-cost 60] [--splits 1 2 ...]
"""
import argparse
import ctypes
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "cuda-bezier-triangle-raytracer_amd"))
sys.path.insert(0, str(REPO))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["cfg4", "cfg2"])
    ap.add_argument("--waves", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--batch-cost", type=float, default=60.0)
    ap.add_argument("--splits", type=int, nargs="+", default=[1, 2, 3, 4, 6, 8])
    a = ap.parse_args()
    import bzr_amd
    from bzr_amd.configs import CONFIGS, build_lens, pixel_coords, rays_for
    from oracle import pyoracle

    fn = bzr_amd.lib().bzr_debug_traverse_bundle_split
    fn.restype = ctypes.c_int32
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float,
                   ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    for name in a.configs:
        cfg = CONFIGS[name]
        lenses = [build_lens(bzr_amd.TriMesh, l).bezier_patches() for l in cfg.lenses]
        rng = np.random.default_rng(a.seed)
        ntile = cfg.side // 8
        tiles = rng.choice(ntile * ntile, min(a.waves, ntile * ntile), replace=False)
        sub_r, sub_c = pixel_coords(cfg, 8, "tiles")
        rows = ((tiles // ntile)[:, None] * 8 + sub_r[None, :]).reshape(-1)
        cols = ((tiles % ntile)[:, None] * 8 + sub_c[None, :]).reshape(-1)
        cur = rays_for(cfg, rows, cols)
        alive = np.ones(cur.shape[1], bool)
        segs = []
        for li, p in enumerate(lenses):
            for exp in (1, 2):  # BZR_RR_INSIDE, BZR_RR_OUTSIDE
                r = cur.copy()
                r[:, ~alive] = np.float32(0.0)  # dead lanes: zero direction -> inactive in the replay
                segs.append((li, np.ascontiguousarray(r, np.float32), int(alive.sum())))
                o, s = pyoracle.refract(p, cfg.lenses[li].ri, cur, np.full(cur.shape[1], exp, np.uint32))
                alive &= s == exp
                cur = np.where(alive[None, :], o, cur).astype(np.float32)
        ws = sum(n for _, _, n in segs) / 64.0
        for g in a.splits:
            tot = np.zeros(16, np.uint64)
            two_level = 0
            for li, r, _ in segs:
                p = np.ascontiguousarray(lenses[li], np.float32)
                st = np.zeros(16, np.uint64)
                per_wave = np.zeros(((r.shape[1] + 63) // 64, 2), np.uint32)
                assert fn(p.ctypes.data, len(p), 264, r.ctypes.data, r.shape[1], np.float32(np.inf), g, st.ctypes.data,
                          per_wave.ctypes.data) == 0
                two_level += int(per_wave[:, 1].sum())
                tot[:14] += st[:14]
                tot[14:] = st[14:]
            slots, batches = float(tot[2]) / ws, float(tot[1]) / ws
            print(json.dumps({
                "config": name, "K": g, "waves": len(tiles), "wave_segments": round(ws, 1),
                "slots_per_wave_segment": round(slots, 3), "two_level_slots_per_wave_segment": round(two_level / ws, 3),
                "leaf_refs_per_wave_segment": round(float(tot[12]) / ws, 3),
                "nodes_per_wave_segment": round(float(tot[13]) / ws, 3), "batches_per_wave_segment": round(batches, 3),
                "lane_walk_slots_per_wave_segment": round(float(tot[4]) / ws, 3),
                "tree_leaf_refs_near_far": [int(tot[14]), int(tot[15])], "patches": int(len(lenses[-1])),
                "missed": int(tot[5]), "overflowing_batches": int(tot[9]),
                "model_valu_per_wave_segment": round(75.0 * slots + a.batch_cost * batches, 1)}), flush=True)


if __name__ == "__main__":
    main()
