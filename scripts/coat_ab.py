#!/usr/bin/env python3
"""bzr_trace_chain_coated beside bzr_trace_chain_bidir, lone frames, device pointers, the fused kernel: what the per-lane
choice between fresnel_t and the table lookup costs where no surface is coated, and what the lookup costs where every
surface is.

usage: python scripts/coat_ab.py [--config cfg4] [--side 0] [--rounds 5] [--steps 20] [--budget 2] [--seed 2024]
                                 [--library PATH]

Runs alternating within each round, on bidir_ab.py's tables, gap table, absorption tables and channels, each at budget 0
and at the budget:
  bidir   bzr_trace_chain_bidir (the yardstick)
  mask0   bzr_trace_chain_coated with no surface coated (its seven outputs are compared with bidir's first, bit for
          bit): k_trace<kModeCoat> with the table read voted away
  bare    every surface coated with bare-Fresnel rows (bzr_coating_reflectance, no layer): the same physics within the
          interpolation error, fresnel_t voted away, so the difference is the lookup
  mgf2    every surface coated with quarter-wave MgF2 rows (1.38, a quarter wave at 0.55 um; the channels at 0.45, 0.50,
          0.55 and 0.65 um): fewer reflections
Each subject has its own context, stream and output buffers; a round queues `steps` frames and waits for them.  Prints
one JSON line per subject and one with the ratios."""
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

    lam = (0.45, 0.50, 0.55, 0.65)

    def rows_of(layers):
        """[2 nl][4][129]: surface (l, side) lies between gap l + side and lens l's glass"""
        rows = np.zeros((2 * nl, 4, bzr_amd.COAT_SAMPLES), np.float32)
        for l in range(nl):
            for side in (0, 1):
                for c in range(4):
                    stack = ([1.38], [0.55 / (4 * 1.38)]) if layers else ((), ())
                    rows[2 * l + side, c] = bzr_amd.coating_reflectance(cement[l + side, c], table[l, c], *stack, lam[c])
        return rows

    every = (1 << (2 * nl)) - 1
    tables = {"mask0": (None, 0), "bare": (rows_of(False), every), "mgf2": (rows_of(True), every)}

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

        rows, mask = tables.get(kind, (None, 0))
        coat = bzr_amd._CoatingC(rows.ctypes.data if rows is not None else None, mask)
        s["coat"] = (rows, coat)  # (kept alive)

        def step():
            if kind == "bidir":
                r = h.bzr_trace_chain_bidir(*head, a.seed, FIRST_RAY, axis, *tail)
            else:
                r = h.bzr_trace_chain_coated(*head, a.seed, FIRST_RAY, axis, ctypes.byref(coat), *tail)
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
    kinds = ("bidir", "mask0", "bare", "mgf2")
    subjects = [subject(f"{kind}{mb}", kind, mb, flags) for mb in (0, a.budget) for kind in kinds]
    by = {s["name"]: s for s in subjects}
    for mb in (0, a.budget):  # no surface coated: bzr_trace_chain_bidir bit for bit
        for k in words:
            assert torch.equal(by[f"mask0{mb}"][k].view(torch.int32), by[f"bidir{mb}"][k].view(torch.int32)), (mb, k)
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
    ratios = {"library": Path(a.library).parent.name}
    for mb in (0, a.budget):
        for kind in kinds[1:]:
            x, y = times[f"{kind}{mb}"], times[f"bidir{mb}"]
            ratios[f"{kind}{mb}_over_bidir{mb}"] = round(med[f"{kind}{mb}"] / med[f"bidir{mb}"], 4)
            ratios[f"{kind}{mb}_over_bidir{mb}_rounds"] = [round(p / q, 4) for p, q in zip(x, y)]
    print(json.dumps(ratios), flush=True)
    for s in subjects:
        release(s)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
