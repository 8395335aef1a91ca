#!/usr/bin/env python3
"""bzr_trace_chain_opl beside bzr_trace_chain_tir, lone frames and frames in flight, device pointers: what the optical
path's two accumulators cost on top of the reflecting chain.

usage: python scripts/opl_ab.py [--config cfg4] [--side 0] [--inflight 3] [--rounds 5] [--steps 20]
                                [--pipelines fused,staged] [--budgets 0,4]

Per pipeline and bounce budget, and for lone frames (one slot) and `inflight` frames in flight, runs alternating within
each round, on the same table ([[1.3, 1.5, 1.8, 2.4], [1.5, 1.5168, 1.53, 1.62], ...]), the same four channels drawn per
ray and the same budget:
  tir   bzr_trace_chain_tir (the yardstick: the kernel the optical-path mode was derived from)
  opl   bzr_trace_chain_opl with opl_in NULL and both output rows (its first five outputs are checked against tir's
        first, bit for bit)
Each subject has its own `inflight` contexts, streams and output buffers; a round queues `steps` frames round-robin over
the slots in use and waits for all of them.  Prints one JSON line per subject, pipeline, budget and frames in flight
(median / min / max ms per frame, the spread of the per-round values, segments per ray, the share of rays that reflect)
and one with the opl / tir ratio of the medians and of each round."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--side", type=int, default=0)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pipelines", default="fused,staged")
    ap.add_argument("--budgets", default="0,4")
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
    drawn = torch.from_numpy(np.random.default_rng(7).integers(0, 4, n).astype(np.uint8)).cuda()
    h = bind(PKG / "lib" / "libbzr.so")

    def subject(name, opl, max_bounces, flags):
        slots = []
        for _ in range(a.inflight):
            stream = torch.cuda.Stream()
            ctx = P()
            assert h.bzr_ctx_create(0, ctypes.byref(ctx)) == 0, h.bzr_last_error()
            h.bzr_ctx_set_stream(ctx, P(stream.cuda_stream))
            meshes = []
            for p in patches:
                m = P()
                assert h.bzr_mesh_create(ctx, p.ctypes.data, len(p), 264, ctypes.byref(m)) == 0, h.bzr_last_error()
                meshes.append(m)
            slots.append(dict(ctx=ctx, stream=stream, meshes=meshes, marr=(P * nl)(*[m.value for m in meshes]),
                              out=torch.empty((6, n), dtype=torch.float32, device="cuda"),
                              w=torch.empty(n, dtype=torch.float32, device="cuda"),
                              st=torch.empty(n, dtype=torch.int32, device="cuda"),
                              sg=torch.empty(n, dtype=torch.int32, device="cuda"),
                              bn=torch.zeros(n, dtype=torch.int32, device="cuda"),
                              op=torch.zeros(n, dtype=torch.float32, device="cuda"),
                              gl=torch.zeros(n, dtype=torch.float32, device="cuda")))

        def step(k, m):
            s = slots[k % m]
            if opl:
                r = h.bzr_trace_chain_opl(s["ctx"], s["marr"], table.ctypes.data, nl, 4, P(rays.data_ptr()),
                                          P(drawn.data_ptr()), None, None, n, max_bounces, P(s["out"].data_ptr()),
                                          P(s["w"].data_ptr()), P(s["st"].data_ptr()), P(s["sg"].data_ptr()),
                                          P(s["bn"].data_ptr()), P(s["op"].data_ptr()), P(s["gl"].data_ptr()), flags)
            else:
                r = h.bzr_trace_chain_tir(s["ctx"], s["marr"], table.ctypes.data, nl, 4, P(rays.data_ptr()),
                                          P(drawn.data_ptr()), None, n, max_bounces, P(s["out"].data_ptr()),
                                          P(s["w"].data_ptr()), P(s["st"].data_ptr()), P(s["sg"].data_ptr()),
                                          P(s["bn"].data_ptr()), flags)
            assert r == 0, h.bzr_last_error()

        for k in range(2 * a.inflight):
            step(k, a.inflight)
        torch.cuda.synchronize()
        return dict(name=name, step=step, slots=slots)

    def release(s):
        for slot in s["slots"]:
            for m in slot["meshes"]:
                h.bzr_mesh_destroy(m)
            h.bzr_ctx_destroy(slot["ctx"])
        s["slots"].clear()

    for pipe in a.pipelines.split(","):
        flags = bzr_amd.DEVICE_PTRS | (bzr_amd.PIPELINE_FUSED if pipe == "fused" else bzr_amd.PIPELINE_STAGED)
        for mb in [int(x) for x in a.budgets.split(",")]:
            torch.cuda.synchronize()
            subjects = [subject("tir", False, mb, flags), subject("opl", True, mb, flags)]
            ref = subjects[0]["slots"][0]
            for slot in subjects[1]["slots"]:
                assert all(torch.equal(slot[k].view(torch.int32), ref[k].view(torch.int32))
                           for k in ("out", "w", "st", "sg", "bn")), "opl's chain differs from tir's"
                assert bool(torch.isfinite(slot["op"]).all().item()) and bool((slot["gl"] <= slot["op"]).all().item())
            for m in sorted({1, a.inflight}):
                times = {s["name"]: [] for s in subjects}
                for _ in range(a.rounds):
                    for s in subjects:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for k in range(a.steps):
                            s["step"](k, m)
                        torch.cuda.synchronize()
                        times[s["name"]].append((time.perf_counter() - t0) * 1e3 / a.steps)
                med = {}
                for s in subjects:
                    t = times[s["name"]]
                    slot = s["slots"][0]
                    segs = int(slot["sg"].sum().item())
                    med[s["name"]] = statistics.median(t)
                    print(json.dumps({"subject": s["name"], "pipeline": pipe, "config": a.config, "rays": n,
                                      "max_bounces": mb, "inflight": m, "ms_median": round(med[s["name"]], 4),
                                      "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                                      "round_spread": round((max(t) - min(t)) / med[s["name"]], 4),
                                      "segments_per_ray": round(segs / n, 4),
                                      "mrays_s": round(segs / med[s["name"]] / 1e3, 1),
                                      "reflected_share": round(float((slot["bn"] > 0).sum().item()) / n, 5),
                                      "with_glass_share": round(float((slot["gl"] > 0).sum().item()) / n, 5)}), flush=True)
                per_round = [o / t for o, t in zip(times["opl"], times["tir"])]
                print(json.dumps({"pipeline": pipe, "max_bounces": mb, "inflight": m,
                                  "opl_over_tir": round(med["opl"] / med["tir"], 4),
                                  "opl_over_tir_rounds": [round(x, 4) for x in per_round],
                                  "chain_same_bits_as_tir": True}), flush=True)
            for s in subjects:
                release(s)
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
