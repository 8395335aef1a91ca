#!/usr/bin/env python3
"""bzr_trace_chain_tir beside bzr_trace_chain_spectral, lone frames and frames in flight, device pointers: what the
reflecting mode costs by itself, and what the reflections cost.

usage: python scripts/tir_ab.py [--config cfg4] [--side 0] [--inflight 3] [--rounds 5] [--steps 20]
                                [--pipelines fused,staged]

Per pipeline, and for lone frames (one slot) and `inflight` frames in flight, runs alternating within each round:
  spectral_uniform   bzr_trace_chain_spectral, every column of the table 1.3, four channels drawn per ray (the yardstick:
                     the kernel the reflecting mode was derived from)
  tir_zero           bzr_trace_chain_tir with max_bounces = 0 on the same table and channels: the cost of the mode itself
                     (its bits are checked against the spectral chain's first, and its bounce row must be zero)
  tir_four           bzr_trace_chain_tir with max_bounces = 4 and the table [[1.3, 1.5, 1.8, 2.4], [1.5, 1.5168, 1.53,
                     1.62], ...]: the cost of the physics (more segments per ray, and waves whose lanes wait)
Each subject has its own `inflight` contexts, streams and output buffers; a round queues `steps` frames round-robin over
the slots in use and waits for all of them.  Prints one JSON line per subject, pipeline and frames in flight (median /
min ms per frame, the spread of the per-round values, segments per ray, the share of rays that reflect and that exit)
and the ratios."""
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
    uniform = np.full((nl, 4), 1.3, np.float32)
    glass = np.ascontiguousarray([ROWS[min(l, len(ROWS) - 1)] for l in range(nl)], np.float32)
    drawn = torch.from_numpy(np.random.default_rng(7).integers(0, 4, n).astype(np.uint8)).cuda()
    h = bind(PKG / "lib" / "libbzr.so")

    def subject(name, table, max_bounces, flags):
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
                              bn=torch.zeros(n, dtype=torch.int32, device="cuda")))

        def step(k, m):
            s = slots[k % m]
            if max_bounces is None:
                r = h.bzr_trace_chain_spectral(s["ctx"], s["marr"], table.ctypes.data, nl, 4, P(rays.data_ptr()),
                                               P(drawn.data_ptr()), None, n, P(s["out"].data_ptr()),
                                               P(s["w"].data_ptr()), P(s["st"].data_ptr()), P(s["sg"].data_ptr()), flags)
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
        torch.cuda.synchronize()
        subjects = [subject("spectral_uniform", uniform, None, flags), subject("tir_zero", uniform, 0, flags),
                    subject("tir_four", glass, 4, flags)]
        ref = subjects[0]["slots"][0]
        for slot in subjects[1]["slots"]:
            assert torch.equal(slot["out"].view(torch.int32), ref["out"].view(torch.int32)) and \
                torch.equal(slot["w"].view(torch.int32), ref["w"].view(torch.int32)) and \
                torch.equal(slot["st"], ref["st"]) and torch.equal(slot["sg"], ref["sg"]) and \
                not bool(slot["bn"].any().item()), "tir_zero"
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
                print(json.dumps({"subject": s["name"], "pipeline": pipe, "config": a.config, "rays": n, "inflight": m,
                                  "ms_median": round(med[s["name"]], 4), "ms_min": round(min(t), 4),
                                  "ms_max": round(max(t), 4),
                                  "round_spread": round((max(t) - min(t)) / med[s["name"]], 4),
                                  "segments_per_ray": round(segs / n, 4),
                                  "mrays_s": round(segs / med[s["name"]] / 1e3, 1),
                                  "reflected_share": round(float((slot["bn"] > 0).sum().item()) / n, 5),
                                  "exited_share": round(float((slot["st"] == 2).sum().item()) / n, 5)}), flush=True)
            print(json.dumps({"pipeline": pipe, "inflight": m,
                              "zero_over_spectral": round(med["tir_zero"] / med["spectral_uniform"], 4),
                              "four_over_zero": round(med["tir_four"] / med["tir_zero"], 4),
                              "zero_same_bits_as_spectral": True}), flush=True)
        for s in subjects:
            release(s)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
