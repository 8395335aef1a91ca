#!/usr/bin/env python3
"""k_trace<kModeBidir>'s wave schedule on the host: rounds per wave and lane utilisation under the two key orders.

usage: python scripts/bidir_sched_sim.py [--config cfg4] [--side 128] [--budget 2]

The numpy reference of the walk (tests/bidir_ref.py) logs every ray's (lens, phase) sequence.  A wave of 64 consecutive
rays is then replayed as the kernel runs it: each round one key 2 lens + phase is picked among the lanes still
travelling -- the lowest key, or the key most lanes hold (ties: the lowest) -- and the lanes holding it advance one
segment.  Prints one JSON line: wave-segments (rounds) and active lanes per round for both orders, against the forward
chain's 2 lenses rounds per wave at budget 0.  The results of the rays do not depend on the order; this only counts."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
for p in (REPO / "cuda-bezier-triangle-raytracer_amd", REPO, REPO / "tests"):
    sys.path.insert(0, str(p))


def replay(keys, most):
    """keys: per lane the list of its segments' keys -> (rounds, lane-segments)."""
    pos = [0] * len(keys)
    rounds = lanes = 0
    while True:
        held = {}
        for i, k in enumerate(keys):
            if pos[i] < len(k):
                held.setdefault(k[pos[i]], []).append(i)
        if not held:
            return rounds, lanes
        key = max(sorted(held), key=lambda x: len(held[x])) if most else min(held)
        for i in held[key]:
            pos[i] += 1
        rounds += 1
        lanes += len(held[key])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--side", type=int, default=128)
    ap.add_argument("--budget", type=int, default=2)
    a = ap.parse_args()
    import bidir_ref
    import bzr_amd
    from bzr_amd.configs import CONFIGS, build_lens, grid_rays
    from oracle import pyoracle as orc

    cfg = CONFIGS[a.config]
    lenses = [build_lens(bzr_amd.TriMesh, l).bezier_patches() for l in cfg.lenses]
    nl = len(lenses)
    rows = [[1.3, 1.5, 1.8, 2.4], [1.5, 1.5168, 1.53, 1.62]]
    table = [rows[min(l, 1)] for l in range(nl)]
    gaps = np.ones((nl + 1, 4), np.float32)
    gaps[1:nl] = 1.56
    rays = grid_rays(cfg, side=a.side)
    n = rays.shape[1]
    channel = np.random.default_rng(7).integers(0, 4, n).astype(np.uint8)
    out = {"config": a.config, "rays": n, "max_bounces": a.budget}
    for budget in sorted({0, a.budget}):
        log = {}
        res = bidir_ref.chain(orc, lenses, table, gaps, None, None, rays, channel, None, None, budget, log=log)
        keys = [[2 * l + p for l, p in zip(ls, ps)] for ls, ps in zip(log["lenses"], log["phases"])]
        for name, most in (("lowest", False), ("most", True)):
            r = s = 0
            for w in range(0, n, 64):
                dr, ds = replay(keys[w:w + 64], most)
                r, s = r + dr, s + ds
            out[f"budget{budget}_{name}"] = {"rounds_per_wave": round(r / ((n + 63) // 64), 3),
                                            "lanes_per_round": round(s / max(r, 1), 2)}
        out[f"budget{budget}_reflected_share"] = round(float((res[4] > 0).mean()), 5)
        out[f"budget{budget}_back_share"] = round(float((res[2] == 4).mean()), 5)
        out[f"budget{budget}_segments_per_ray"] = round(float(res[3].mean()), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
