#!/usr/bin/env python3
"""bzr_trace_chain_ghost beside bzr_trace_chain_absorb, lone frames, device pointers: what the Fresnel roulette costs on
top of the absorbing chain -- the draw in every OUTSIDE tail, and the bounce segments of the rays it reflects.

usage: python scripts/ghost_ab.py [--config cfg4] [--side 0] [--rounds 5] [--steps 20] [--pipelines fused,staged]
                                  [--budget 2] [--seed 2024]

Per pipeline, runs alternating within each round, on the same table ([[1.3, 1.5, 1.8, 2.4], [1.5, 1.5168, 1.53, 1.62],
...]), the same gap table (1.56 between the lenses, vacuum outside), the same absorption tables, the same four channels
drawn per ray:
  absorb  bzr_trace_chain_absorb at the budget (the yardstick: the kernel the ghost mode was derived from)
  ghost0  bzr_trace_chain_ghost at budget 0 (its seven outputs are checked against bzr_trace_chain_absorb at budget 0
          first, bit for bit): no draw is taken; what the mode's code costs where it does nothing
  ghost   bzr_trace_chain_ghost at the budget: the draws, and the bounce segments of the reflected rays -- a few lanes of
          nearly every wave
Each subject has its own context, stream and output buffers; a round queues `steps` frames and waits for them.  The
subjects are created in this order, and the earlier scripts of this family recorded that a later-created subject can
run a per cent or so off an identical earlier one: read the ratios against the yardstick's own round spread.  absorb
and ghost0 run different budgets, so their ratio compares two workloads.  Prints one JSON line per subject and
pipeline (median / min / max ms per frame, the spread of the per-round values, segments per ray, the share of rays that
reflect) and one with the ratios to absorb of the medians and of each round."""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
PKG = REPO / "cuda-bezier-triangle-raytracer_amd"
sys.path.insert(0, str(PKG))
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "scripts"))

ROWS = [[1.3, 1.5, 1.8, 2.4], [1.5, 1.5168, 1.53, 1.62]]
CEMENT = 1.56
FIRST_RAY = (1 << 40) + 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--side", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pipelines", default="fused,staged")
    ap.add_argument("--budget", type=int, default=2)
    ap.add_argument("--seed", type=int, default=2024)
    a = ap.parse_args()
    import torch

    import bzr_amd
    from ab import bind
    from bzr_amd.configs import CONFIGS, build_lens, grid_rays

    cfg = CONFIGS[a.config]
    patches = [np.ascontiguousarray(build_lens(bzr_amd.TriMesh, l).bezier_patches(), np.float32) for l in cfg.lenses]
    nl = len(patches)
    rays = torch.from_numpy(grid_rays(cfg, side=a.side or None)).cuda()
    n = rays.shape[1]
    P = ctypes.c_void_p
    table = np.ascontiguousarray([ROWS[min(l, len(ROWS) - 1)] for l in range(nl)], np.float32)
    cement = np.ones((nl + 1, 4), np.float32)
    cement[1:nl] = CEMENT  # the joints between the lenses
    glass = np.ascontiguousarray([[0.0, 0.05, 0.7, 200.0]] * nl, np.float32)
    front = np.ascontiguousarray([[0.0, 0.02, 0.3, 0.0]] * nl, np.float32)
    drawn = torch.from_numpy(np.random.default_rng(7).integers(0, 4, n).astype(np.uint8)).cuda()
    h = bind(PKG / "lib" / "libbzr.so")

    def subject(name, ghost, mb, flags):
        stream = torch.cuda.Stream()
        ctx = P()
        assert h.bzr_ctx_create(0, ctypes.byref(ctx)) == 0, h.bzr_last_error()
        h.bzr_ctx_set_stream(ctx, P(stream.cuda_stream))
        meshes = []
        for p in patches:
            m = P()
            assert h.bzr_mesh_create(ctx, p.ctypes.data, len(p), 264, ctypes.byref(m)) == 0, h.bzr_last_error()
            meshes.append(m)
        s = dict(name=name, ctx=ctx, stream=stream, meshes=meshes, marr=(P * nl)(*[m.value for m in meshes]), budget=mb,
                 out=torch.empty((6, n), dtype=torch.float32, device="cuda"),
                 w=torch.empty(n, dtype=torch.float32, device="cuda"),
                 st=torch.empty(n, dtype=torch.int32, device="cuda"),
                 sg=torch.empty(n, dtype=torch.int32, device="cuda"),
                 bn=torch.zeros(n, dtype=torch.int32, device="cuda"),
                 op=torch.zeros(n, dtype=torch.float32, device="cuda"),
                 gl=torch.zeros(n, dtype=torch.float32, device="cuda"))
        head = (ctx, s["marr"], table.ctypes.data, cement.ctypes.data, glass.ctypes.data, front.ctypes.data, nl, 4,
                P(rays.data_ptr()), P(drawn.data_ptr()), None, None, n, mb)
        tail = (P(s["out"].data_ptr()), P(s["w"].data_ptr()), P(s["st"].data_ptr()), P(s["sg"].data_ptr()),
                P(s["bn"].data_ptr()), P(s["op"].data_ptr()), P(s["gl"].data_ptr()), flags)

        def step():
            if ghost:
                r = h.bzr_trace_chain_ghost(*head, a.seed, FIRST_RAY, *tail)
            else:
                r = h.bzr_trace_chain_absorb(*head, *tail)
            assert r == 0, h.bzr_last_error()

        s["step"] = step
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        return s

    def release(s):
        for m in s["meshes"]:
            h.bzr_mesh_destroy(m)
        h.bzr_ctx_destroy(s["ctx"])

    words = ("out", "w", "st", "sg", "bn", "op", "gl")
    for pipe in a.pipelines.split(","):
        flags = bzr_amd.DEVICE_PTRS | (bzr_amd.PIPELINE_FUSED if pipe == "fused" else bzr_amd.PIPELINE_STAGED)
        torch.cuda.synchronize()
        zero = subject("absorb0", False, 0, flags)  # the check's reference: not timed
        subjects = [subject("absorb", False, a.budget, flags), subject("ghost0", True, 0, flags),
                    subject("ghost", True, a.budget, flags)]
        ref, same, lit = subjects
        assert all(torch.equal(same[k].view(torch.int32), zero[k].view(torch.int32)) for k in words), \
            "ghost at budget 0 differs from absorb at budget 0"
        release(zero)
        row0 = lit["bn"] == 0  # the rays that never reflected keep absorb's geometry
        assert all(torch.equal(lit[k][..., row0].view(torch.int32), ref[k][..., row0].view(torch.int32))
                   for k in ("out", "st", "sg", "op", "gl")), "a ray that never reflected left absorb's path"
        times = {s["name"]: [] for s in subjects}
        for _ in range(a.rounds):
            for s in subjects:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    s["step"]()
                torch.cuda.synchronize()
                times[s["name"]].append((time.perf_counter() - t0) * 1e3 / a.steps)
        med = {}
        for s in subjects:
            t = times[s["name"]]
            segs = int(s["sg"].sum().item())
            med[s["name"]] = statistics.median(t)
            print(json.dumps({"subject": s["name"], "pipeline": pipe, "config": a.config, "rays": n,
                              "max_bounces": s["budget"], "ms_median": round(med[s["name"]], 4),
                              "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                              "round_spread": round((max(t) - min(t)) / med[s["name"]], 4),
                              "segments_per_ray": round(segs / n, 4),
                              "mrays_s": round(segs / med[s["name"]] / 1e3, 1),
                              "outside_share": round(float((s["st"] == 2).sum().item()) / n, 5),
                              "reflected_share": round(float((s["bn"] > 0).sum().item()) / n, 5),
                              "weight_sum_outside": round(float(s["w"][s["st"] == 2].double().sum().item()), 3)}),
                  flush=True)
        print(json.dumps({"pipeline": pipe, "max_bounces": a.budget,
                          "ghost0_over_absorb": round(med["ghost0"] / med["absorb"], 4),
                          "ghost0_over_absorb_rounds": [round(x / y, 4) for x, y in zip(times["ghost0"], times["absorb"])],
                          "ghost_over_absorb": round(med["ghost"] / med["absorb"], 4),
                          "ghost_over_absorb_rounds": [round(x / y, 4) for x, y in zip(times["ghost"], times["absorb"])],
                          "ghost0_same_bits_as_absorb0": True}), flush=True)
        for s in subjects:
            release(s)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
