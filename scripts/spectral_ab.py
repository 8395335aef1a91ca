#!/usr/bin/env python3
"""bzr_trace_chain_spectral beside bzr_trace_chain_power, frames in flight, device pointers: what dispersion costs.

usage: python scripts/spectral_ab.py [--config cfg4] [--side 0] [--inflight 3] [--rounds 7] [--steps 30]

Runs, alternating within each round:
  chain_power        the power chain (the yardstick: the kernel the spectral mode was derived from)
  spectral_zero      the spectral chain with the channel row all zero and every column of the table the lens's own
                     index: the same rays, what the per-lane index costs by itself (its bits are checked against the
                     power chain's first)
  spectral_four      the spectral chain with four channels drawn per ray and the table [[1.290, 1.297, 1.304, 1.312]]
                     per lens: what mixed colours cost in a wave (the rays diverge after the first surface)
Each has its own `inflight` contexts, streams and output buffers; a round queues `steps` frames round-robin over the
slots and waits for all of them.  Prints one JSON line per subject (median / min ms per frame, the spread of the
per-round values, Mrays/s from the subject's own segment count, its Newton pass counters for one frame) and the
ratios."""
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

FOUR = [1.290, 1.297, 1.304, 1.312]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--side", type=int, default=0)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    import torch

    import bzr_amd
    from ab import bind
    from bzr_amd.configs import CONFIGS, build_lens, grid_rays

    cfg = CONFIGS[a.config]
    patches = [np.ascontiguousarray(build_lens(bzr_amd.TriMesh, l).bezier_patches(), np.float32) for l in cfg.lenses]
    nl = len(patches)
    ris = (ctypes.c_float * nl)(*[l.ri for l in cfg.lenses])
    rays = torch.from_numpy(grid_rays(cfg, side=a.side or None)).cuda()
    n = rays.shape[1]
    flags = bzr_amd.DEVICE_PTRS | bzr_amd.PIPELINE_FUSED
    P = ctypes.c_void_p
    own = np.ascontiguousarray([[l.ri] * 4 for l in cfg.lenses], np.float32)
    four = np.ascontiguousarray([FOUR] * nl, np.float32)
    zero = torch.zeros(n, dtype=torch.uint8, device="cuda")
    drawn = torch.from_numpy(np.random.default_rng(7).integers(0, 4, n).astype(np.uint8)).cuda()
    h = bind(PKG / "lib" / "libbzr.so")

    def subject(name, table, channel):
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
            slots.append(dict(ctx=ctx, stream=stream, marr=(P * nl)(*[m.value for m in meshes]),
                              out=torch.empty((6, n), dtype=torch.float32, device="cuda"),
                              w=torch.empty(n, dtype=torch.float32, device="cuda"),
                              st=torch.empty(n, dtype=torch.int32, device="cuda"),
                              sg=torch.empty(n, dtype=torch.int32, device="cuda")))

        def step(k):
            s = slots[k % a.inflight]
            if table is None:
                r = h.bzr_trace_chain_power(s["ctx"], s["marr"], ris, nl, P(rays.data_ptr()), None, n,
                                            P(s["out"].data_ptr()), P(s["w"].data_ptr()), P(s["st"].data_ptr()),
                                            P(s["sg"].data_ptr()), flags)
            else:
                r = h.bzr_trace_chain_spectral(s["ctx"], s["marr"], table.ctypes.data, nl, 4, P(rays.data_ptr()),
                                               P(channel.data_ptr()), None, n, P(s["out"].data_ptr()),
                                               P(s["w"].data_ptr()), P(s["st"].data_ptr()), P(s["sg"].data_ptr()), flags)
            assert r == 0, h.bzr_last_error()

        for k in range(3 * a.inflight):
            step(k)
        torch.cuda.synchronize()
        return dict(name=name, step=step, slots=slots, times=[])

    torch.cuda.synchronize()
    subjects = [subject("chain_power", None, None), subject("spectral_zero", own, zero),
                subject("spectral_four", four, drawn)]
    ref = subjects[0]["slots"][0]
    for slot in subjects[1]["slots"]:
        assert torch.equal(slot["out"].view(torch.int32), ref["out"].view(torch.int32)) and \
            torch.equal(slot["w"].view(torch.int32), ref["w"].view(torch.int32)) and \
            torch.equal(slot["st"], ref["st"]) and torch.equal(slot["sg"], ref["sg"]), "spectral_zero"
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
        # one counted frame on slot 0 (the counting kernels are other instantiations: after the timing)
        ctx = s["slots"][0]["ctx"]
        assert h.bzr_ctx_counters(ctx, 1) == 0
        report = np.zeros(len(bzr_amd.COUNTERS), np.uint64)
        assert h.bzr_ctx_counters_report(ctx, report.ctypes.data) == 0
        s["step"](0)
        assert h.bzr_ctx_counters_report(ctx, report.ctypes.data) == 0
        assert h.bzr_ctx_counters(ctx, 0) == 0
        counted = dict(zip(bzr_amd.COUNTERS, (int(x) for x in report)))
        segs = int(s["slots"][0]["sg"].sum().item())
        med[s["name"]] = statistics.median(s["times"])
        print(json.dumps({"subject": s["name"], "config": a.config, "rays": n, "inflight": a.inflight,
                          "ms_median": round(med[s["name"]], 4), "ms_min": round(min(s["times"]), 4),
                          "ms_max": round(max(s["times"]), 4),
                          "round_spread": round((max(s["times"]) - min(s["times"])) / med[s["name"]], 4),
                          "segments": segs, "mrays_s": round(segs / med[s["name"]] / 1e3, 1),
                          "exited": int((s["slots"][0]["st"] == 2).sum().item()),
                          "newton_rounds": counted["newton_rounds"], "short_passes": counted["short_passes"],
                          "pairs": counted["pairs"]}), flush=True)
    print(json.dumps({"zero_over_power": round(med["spectral_zero"] / med["chain_power"], 4),
                      "four_over_zero": round(med["spectral_four"] / med["spectral_zero"], 4),
                      "zero_same_bits_as_power": True}), flush=True)


if __name__ == "__main__":
    main()
