#!/usr/bin/env python3
"""Host estimate for k_trace's short passes (trace.hip BZR_TRACE_SHORT): how many Newton runs lose to their ray's
winner, and how many of the fused kernel's patch-uniform passes consist of losers only.  CPU only, the oracle only
(planar gate, BezierTriangle::intersect, BezierLens::refract).

A run is a (ray, patch) pair that passed the planar gate (cThis), or the cNone retry on the neighbour a follow-side
result names.  Its key is (t, scanned patch); the ray's winner is the smallest key among its INTERSECT runs.  A run
loses when it is not the winner -- a far-side loser when its t (whatever its classification: the kernel votes before
it classifies) is above the winner's.  A pass is one patch of one 8 x 8-ray wave: a leaf pass runs the wave's lanes
that passed the patch's gate, joined by the retries of the wave's other leaves that name it; a retry whose neighbour
is no leaf of the wave takes a stand-alone pass.  A pass is wholly dominated when every lane's key in it is above that
lane's final winner: run after the winners (the kernel orders a batch near side first), it can skip the last Newton
iteration's normal.  That is an upper bound for the kernel: batches of 16 leaves, parked retries and winners that run
later all lower it.

Prints per segment of the config's chain: rays, Newton runs, rays with two candidates, winning runs, losers, far-side
losers; then over all segments: passes, wholly dominated passes and the lane-runs in them.
usage: python scripts/dominated_sim.py [--config cfg4] [--tiles 160] [--side 4096]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "cuda-bezier-triangle-raytracer_amd"), str(REPO)]

from bzr_amd.configs import CONFIGS, build_lens, rays_for  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

INTERSECT = 4
FLT_MAX = np.finfo(np.float32).max


def t_order(t):
    """trace.hip t_order: the monotone map of float32 t to uint32 (-0 ties with +0)."""
    u = np.where(t == 0, np.float32(0), t).astype(np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--tiles", type=int, default=160)
    ap.add_argument("--side", type=int, default=0, help="rays per image side (0 = the config's own)")
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    cfg = CONFIGS[a.config]
    side = a.side or cfg.side
    lenses = [build_lens(po.OMesh, l).bezier_patches() for l in cfg.lenses]
    rng = np.random.default_rng(a.seed)
    nt = side // 8
    tiles = rng.choice(nt * nt, a.tiles, replace=False)
    rr, cc = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    rows = ((tiles // nt)[:, None] * 8 + rr.reshape(-1)[None, :]).reshape(-1)
    cols = ((tiles % nt)[:, None] * 8 + cc.reshape(-1)[None, :]).reshape(-1)
    rays = rays_for(cfg, rows, cols, side=side)
    n = rays.shape[1]
    alive = np.ones(n, bool)
    tot = dict(passes=0, follow_passes=0, dominated=0, lane_runs=0, dominated_lane_runs=0)
    nseg = 2 * len(lenses) if cfg.op == "chain" else 1
    for seg in range(nseg):
        lens = lenses[seg // 2]
        neigh = lens[:, 16:19].view(np.uint32)
        gate = po.planar_gate(lens, rays) & alive[:, None]
        ray, patch = np.nonzero(gate)
        first = po.patch_intersect(lens, patch, np.zeros(len(ray), int), rays[:, ray])
        what = first.view(np.uint32)[11]
        # runs: (ray, pass patch, scanned patch, t, intersects)
        runs = [(ray, patch, patch, first[0], what == INTERSECT)]
        fol = what <= 2
        if fol.any():
            nb = neigh[patch[fol], what[fol]]
            second = po.patch_intersect(lens, nb, np.ones(int(fol.sum()), int), rays[:, ray[fol]])
            runs.append((ray[fol], nb, patch[fol], second[0], second.view(np.uint32)[11] == INTERSECT))
        r_ray, r_pass, r_scan, r_t, r_hit = (np.concatenate(x) for x in zip(*runs))
        with np.errstate(invalid="ignore"):
            finite = r_t < FLT_MAX  # false for NaN: such a t cannot win (trace.hip consider())
        key = (t_order(r_t).astype(np.uint64) << np.uint64(32)) | r_scan.astype(np.uint64)  # (t order, scanned patch)
        none = np.uint64(0xFFFFFFFFFFFFFFFF)
        best = np.full(n, none)
        np.minimum.at(best, r_ray, np.where(r_hit & finite, key, none))
        wins = r_hit & finite & (key == best[r_ray])
        above = finite & ((key >> np.uint64(32)) > (best[r_ray] >> np.uint64(32)))
        # the kernel's vote: the lane's key, whatever the run's classification, against its final winner's
        lost = ~(finite & (key < best[r_ray])) & ~wins
        # passes: per (wave, patch); a retry joins its neighbour's leaf pass when the wave collected that leaf
        wave = r_ray // 64
        leaf = set(zip((ray // 64).tolist(), patch.tolist()))
        pid = {}
        for i in range(len(r_ray)):
            k = (int(wave[i]), int(r_pass[i]))
            own = i >= len(ray) and k not in leaf  # a stand-alone follow pass
            pid.setdefault((k, own), []).append(i)
        dom = [(k, v) for k, v in pid.items() if lost[v].all()]
        tot["passes"] += len(pid)
        tot["follow_passes"] += sum(1 for (k, own) in pid if own)
        tot["dominated"] += len(dom)
        tot["lane_runs"] += len(r_ray)
        tot["dominated_lane_runs"] += sum(len(v) for _, v in dom)
        print(json.dumps({"segment": seg, "rays": int(alive.sum()), "newton_runs": int(len(r_ray)),
                          "rays_with_2_candidates": int((gate.sum(axis=1) == 2).sum()), "runs_that_win": int(wins.sum()),
                          "losers": int((~wins).sum()), "far_side_losers": int((~wins & above).sum()),
                          "passes": len(pid), "wholly_dominated": len(dom)}), flush=True)
        if cfg.op != "chain":
            break
        o, st = po.refract(lens, cfg.lenses[seg // 2].ri, rays, np.full(n, 1 + seg % 2, np.uint32))
        alive &= st != 0
        rays = o
    P, R = tot["passes"], tot["lane_runs"]
    print(json.dumps({"config": a.config, "side": side, "tiles": a.tiles, "passes": P,
                      "stand_alone_follow_passes": tot["follow_passes"], "wholly_dominated_passes": tot["dominated"],
                      "dominated_pct": round(100 * tot["dominated"] / max(1, P), 2), "lane_runs": R,
                      "dominated_lane_runs": tot["dominated_lane_runs"],
                      "note": "a wholly dominated pass has no lane whose (t, scanned patch) key is below the lane's "
                              "final winner: run after the winners it skips the last normal (upper bound)"}))


if __name__ == "__main__":
    main()
