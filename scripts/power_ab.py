#!/usr/bin/env python3
"""bzr_trace_chain_power beside bzr_trace_chain, frames in flight, device pointers: what the weight costs.

usage: python scripts/power_ab.py [--config cfg4] [--side 0] [--inflight 3] [--rounds 7] [--steps 30] [--parent VARIANT]

Runs, alternating within each round, the plain chain and the power chain of lib/libbzr.so and -- with --parent, a
build of an earlier commit under lib/VARIANT/libbzr.so, loaded beside it as scripts/ab.py loads variants -- that
build's plain chain.  Each has its own `inflight` contexts, streams and output buffers; a round queues `steps` frames
round-robin over the slots and waits for all of them.  Prints one JSON line per subject (median / min ms per frame,
Mrays/s from the frame's segment count) and the ratios.  The power chain's rays, status and segments are checked
against the plain chain's bits first."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--side", type=int, default=0)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--parent", default="", help="lib/<variant>/libbzr.so of an earlier commit: its plain chain too")
    a = ap.parse_args()
    import torch

    import bzr_amd
    from ab import bind
    from bzr_amd.configs import CONFIGS, build_lens, grid_rays

    cfg = CONFIGS[a.config]
    patches = [np.ascontiguousarray(build_lens(bzr_amd.TriMesh, l).bezier_patches(), np.float32) for l in cfg.lenses]
    ris = (ctypes.c_float * len(patches))(*[l.ri for l in cfg.lenses])
    rays = torch.from_numpy(grid_rays(cfg, side=a.side or None)).cuda()
    n = rays.shape[1]
    flags = bzr_amd.DEVICE_PTRS | bzr_amd.PIPELINE_FUSED
    P = ctypes.c_void_p

    def subject(name, path, power):
        h = bind(path)
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
            slots.append(dict(ctx=ctx, stream=stream, marr=(P * len(meshes))(*[m.value for m in meshes]),
                              out=torch.empty((6, n), dtype=torch.float32, device="cuda"),
                              w=torch.empty(n, dtype=torch.float32, device="cuda"),
                              st=torch.empty(n, dtype=torch.int32, device="cuda"),
                              sg=torch.empty(n, dtype=torch.int32, device="cuda")))

        def step(k):
            s = slots[k % a.inflight]
            if power:
                r = h.bzr_trace_chain_power(s["ctx"], s["marr"], ris, len(patches), P(rays.data_ptr()), None, n,
                                            P(s["out"].data_ptr()), P(s["w"].data_ptr()), P(s["st"].data_ptr()),
                                            P(s["sg"].data_ptr()), flags)
            else:
                r = h.bzr_trace_chain(s["ctx"], s["marr"], ris, len(patches), P(rays.data_ptr()), n,
                                      P(s["out"].data_ptr()), P(s["st"].data_ptr()), P(s["sg"].data_ptr()), flags)
            assert r == 0, h.bzr_last_error()

        for k in range(3 * a.inflight):
            step(k)
        torch.cuda.synchronize()
        return dict(name=name, step=step, slots=slots, times=[])

    torch.cuda.synchronize()
    subjects = [subject("chain", PKG / "lib" / "libbzr.so", False), subject("chain_power", PKG / "lib" / "libbzr.so", True)]
    if a.parent:
        subjects.append(subject(f"{a.parent}:chain", PKG / "lib" / a.parent / "libbzr.so", False))
    ref = subjects[0]["slots"][0]
    for s in subjects[1:]:
        for slot in s["slots"]:
            assert torch.equal(slot["out"].view(torch.int32), ref["out"].view(torch.int32)) and \
                torch.equal(slot["st"], ref["st"]) and torch.equal(slot["sg"], ref["sg"]), s["name"]
    w = subjects[1]["slots"][0]["w"]
    exited = ref["st"] == 2
    segs = int(ref["sg"].sum().item())
    for _ in range(a.rounds):
        for s in subjects:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(a.steps):
                s["step"](k)
            torch.cuda.synchronize()
            s["times"].append((time.perf_counter() - t0) * 1e3 / a.steps)
    med = {}
    for s in subjects:
        med[s["name"]] = statistics.median(s["times"])
        print(json.dumps({"subject": s["name"], "config": a.config, "rays": n, "inflight": a.inflight,
                          "ms_median": round(med[s["name"]], 4), "ms_min": round(min(s["times"]), 4),
                          "mrays_s": round(segs / med[s["name"]] / 1e3, 1)}), flush=True)
    out = {"power_over_chain": round(med["chain_power"] / med["chain"], 4), "same_rays_status_segments": True,
           "exited": int(exited.sum().item()), "mean_exited_weight": round(float(w[exited].mean().item()), 5)}
    if a.parent:
        out["power_over_parent_chain"] = round(med["chain_power"] / med[f"{a.parent}:chain"], 4)
        out["chain_over_parent_chain"] = round(med["chain"] / med[f"{a.parent}:chain"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
