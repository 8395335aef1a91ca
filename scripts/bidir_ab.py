#!/usr/bin/env python3
"""bzr_trace_chain_bidir beside bzr_trace_chain_absorb and bzr_trace_chain_ghost, lone frames, device pointers, the fused
kernel: what the per-lane schedule costs where it does nothing, and what the walk costs where it acts.

usage: python scripts/bidir_ab.py [--config cfg4] [--side 0] [--rounds 5] [--steps 20] [--budget 2] [--seed 2024]
                                  [--library PATH]

Runs alternating within each round, on ghost_ab.py's tables, gap table, absorption tables and channels:
  absorb0  bzr_trace_chain_absorb at budget 0 (the yardstick of bidir0)
  bidir0   bzr_trace_chain_bidir at budget 0 (its seven outputs are compared with absorb0's first: they may differ only on
           the few rim rays that meet a surface facing backward, at most 0.1 %; the count is printed): no draw, no
           reflection; the cost of the vote, the LDS word and the per-lane tables
  ghost    bzr_trace_chain_ghost at the budget (the yardstick of bidir)
  bidir    bzr_trace_chain_bidir at the budget: draws at every surface, rays walking back, waves split over keys
Each subject has its own context, stream and output buffers; a round queues `steps` frames and waits for them.
--library names another build of libbzr.so (the BZR_BIDIR_PICK=1 variant).  Prints one JSON line per
subject and one with the ratios."""
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
    ap.add_argument("--library", default=str(PKG / "lib" / "libbzr.so"))
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
    h = bind(a.library)
    axis = (ctypes.c_float * 3)(1.0, 0.0, 0.0)

    def subject(name, kind, mb, flags):
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
            if kind == "bidir":
                r = h.bzr_trace_chain_bidir(*head, a.seed, FIRST_RAY, axis, *tail)
            elif kind == "ghost":
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
    flags = bzr_amd.DEVICE_PTRS | bzr_amd.PIPELINE_FUSED
    torch.cuda.synchronize()
    subjects = [subject("absorb0", "absorb", 0, flags), subject("bidir0", "bidir", 0, flags),
                subject("ghost", "ghost", a.budget, flags), subject("bidir", "bidir", a.budget, flags)]
    zero, same, ghost, lit = subjects
    # a ray that meets a surface facing backward from inside glass has no counterpart in the forward chain (the side rule
    # takes the other gap's index); on a grid along the axis these are a few rim rays: counted, and bounded
    differ = torch.zeros(n, dtype=torch.bool, device="cuda")
    for k in words:
        d = same[k].view(torch.int32) != zero[k].view(torch.int32)
        differ |= d.any(dim=0) if d.dim() == 2 else d
    assert int(differ.sum().item()) <= n // 1000, "bidir at budget 0 differs from absorb at budget 0 on more than 0.1 % of the rays"
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
        print(json.dumps({"subject": s["name"], "config": a.config, "rays": n, "max_bounces": s["budget"],
                          "ms_median": round(med[s["name"]], 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                          "round_spread": round((max(t) - min(t)) / med[s["name"]], 4),
                          "segments_per_ray": round(segs / n, 4), "mrays_s": round(segs / med[s["name"]] / 1e3, 1),
                          "outside_share": round(float((s["st"] == 2).sum().item()) / n, 5),
                          "back_share": round(float((s["st"] == 4).sum().item()) / n, 5),
                          "reflected_share": round(float((s["bn"] > 0).sum().item()) / n, 5),
                          "weight_sum_outside": round(float(s["w"][s["st"] == 2].double().sum().item()), 3),
                          "weight_sum_back": round(float(s["w"][s["st"] == 4].double().sum().item()), 3)}), flush=True)
    print(json.dumps({"max_bounces": a.budget, "library": Path(a.library).parent.name,
                      "bidir0_over_absorb0": round(med["bidir0"] / med["absorb0"], 4),
                      "bidir0_over_absorb0_rounds": [round(x / y, 4) for x, y in zip(times["bidir0"], times["absorb0"])],
                      "bidir_over_ghost": round(med["bidir"] / med["ghost"], 4),
                      "bidir_over_ghost_rounds": [round(x / y, 4) for x, y in zip(times["bidir"], times["ghost"])],
                      "bidir0_rays_differing_from_absorb0": int(differ.sum().item()),
                      "bidir0_rays_back": int((same["st"] == 4).sum().item())}), flush=True)
    for s in subjects:
        release(s)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
