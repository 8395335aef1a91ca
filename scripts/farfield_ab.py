#!/usr/bin/env python3
"""A/B of k_land_far's wave combine (bzr_farfield_bin): how many leader-election rounds a wave runs before the lanes
left over issue their own atomics.  Same process, resident device inputs, warm, the settings interleaved.

Three cases of `rays` rays each (default 16 M), weights given, flux and count maps both kept:
  concentrated  a 5 degree cone about the pole into a 128 x 128 map (R = sqrt(2)): a collimator's far field
  diffuse       the uniform hemisphere into a 256 x 256 map
  pencil        a 0.5 degree cone into a 128 x 128 map: a handful of cells (beside the two cases that decide)
Settings: 0 rounds (plain per-lane atomics), 1, 2, 4, 8, 16 and 64 (unbounded), through bzr_debug_farfield_rounds.
Per sample `calls` calls are timed between two device events on the stream the kernels run on; `repeats` samples per
setting, the settings visited in rotating order.  The maps of every setting are compared with those of 0 rounds.
Prints one JSON line per case (milliseconds per call: median, min, max).

usage: farfield_ab.py [rays] [--calls 10] [--repeats 7] [--out FILE]
"""
import argparse
import ctypes
import json
import math
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "cuda-bezier-triangle-raytracer_amd"))
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

import bzr_amd  # noqa: E402

ROUNDS = (0, 1, 2, 4, 8, 16, 64)


def directions(n, cos_lo, seed):
    """[6, n] float32 on the device: zero starts, unit directions with the cosine to +x uniform in [cos_lo, 1)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    c = cos_lo + (1.0 - cos_lo) * torch.rand(n, device="cuda", generator=g, dtype=torch.float64)
    s = torch.sqrt(1.0 - c * c)
    turn = 2.0 * math.pi * torch.rand(n, device="cuda", generator=g, dtype=torch.float64)
    rays = torch.zeros((6, n), device="cuda", dtype=torch.float32)
    rays[3], rays[4], rays[5] = c.float(), (s * torch.cos(turn)).float(), (s * torch.sin(turn)).float()
    w = torch.rand(n, device="cuda", generator=g, dtype=torch.float32)
    return rays, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rays", nargs="?", type=int, default=1 << 24)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = bzr_amd.Context(0)
    ctx.use_torch_stream()
    lines = []
    for name, cos_lo, bins in (("concentrated: 5 degree cone, 128^2 map", math.cos(math.radians(5.0)), 128),
                               ("diffuse: uniform hemisphere, 256^2 map", 0.0, 256),
                               ("pencil: 0.5 degree cone, 128^2 map", math.cos(math.radians(0.5)), 128)):
        far = bzr_amd.FarField(axis_u=(0.0, 1.0, 0.0), axis_v=(0.0, 0.0, 1.0), extent=bzr_amd.SQRT2, bins_u=bins,
                               bins_v=bins)
        rays, w = directions(a.rays, cos_lo, 7)
        flux = torch.zeros((1, bins, bins), dtype=torch.int64, device="cuda")
        hist = torch.zeros((1, bins, bins), dtype=torch.int32, device="cuda")

        def call():
            L = bzr_amd.lib()
            st = L.bzr_farfield_bin(ctx.handle, ctypes.byref(far), rays.data_ptr(), w.data_ptr(), None, None, a.rays, 1,
                                    flux.data_ptr(), hist.data_ptr(), None, None, bzr_amd.DEVICE_PTRS)
            assert st == 0, L.bzr_last_error()

        base, same = None, {}
        for r in ROUNDS:  # warm-up and the maps' equality, one call per setting
            bzr_amd.debug_farfield_rounds(ctx, r)
            flux.zero_(), hist.zero_()
            call()
            torch.cuda.synchronize()
            if base is None:
                base = (flux.clone(), hist.clone())
            same[r] = bool(torch.equal(flux, base[0]) and torch.equal(hist, base[1]))
        ms = {r: [] for r in ROUNDS}
        for k in range(a.repeats):
            order = ROUNDS[k % len(ROUNDS):] + ROUNDS[:k % len(ROUNDS)]
            for r in order:
                bzr_amd.debug_farfield_rounds(ctx, r)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.calls):
                    call()
                t1.record()
                torch.cuda.synchronize()
                ms[r].append(t0.elapsed_time(t1) / a.calls)
        bzr_amd.debug_farfield_rounds(ctx, -1)
        binned = int(base[1].sum())
        line = {"workload": "farfield_bin, " + name, "rays": a.rays, "binned": binned,
                "cells_hit": int((base[1] != 0).sum()), "calls_per_sample": a.calls, "samples": a.repeats,
                "ms_per_call": {str(r): {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                                         "max": round(max(v), 4)} for r, v in ms.items()},
                "grays_per_s_median": {str(r): round(a.rays / statistics.median(v) / 1e6, 2) for r, v in ms.items()},
                "maps_equal_to_0_rounds": same}
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
        del rays, w, flux, hist
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
