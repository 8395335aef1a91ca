#!/usr/bin/env python3
"""Throughput of the illumination pipeline (bzr_illuminate: emit -> sphere cull -> chain -> target counts)
on the cfg2 lens, emitter just behind it (inside the lens's bounding sphere, so nothing is culled and
every ray is traced).  Prints one JSON line: emitted rays / s and the landed fraction.

usage: bench_illum.py [total_rays] [--power] [--tir [max_bounces]] [--media] [--farfield] [--ghost] [--bidir]
--power times bzr_illuminate_power (Lambert emitter, Fresnel surfaces: k_emit<true> -> chain with weights ->
k_land<true>, 64-bit flux cells) beside bzr_illuminate on the same rays, alternating, and prints one more JSON line
with both; the chain kernels' share comes from the context's event timing in a separate pass, the rest of a call is
its emit and landing kernels and the host's part.  Per-kernel durations of k_land<false> / k_land<true>: run this
under a kernel-trace profiler.
--tir [max_bounces] (default 4) prints one more JSON line: on a wide emitter 1 unit in front of the lens (inside its
sphere: nothing is culled) with the indices 1.3 / 1.5 / 1.8 / 2.4, bzr_illuminate_spectral, bzr_illuminate_tir at budget
0 and bzr_illuminate_tir at max_bounces on the same rays, alternating; the ratios are the cost of the reflecting chain's
plumbing (the per-batch row clear, k_land_tir's ledger) and of the bounce segments.
--media prints one more JSON line: on the same wide emitter, bzr_illuminate_tir and bzr_illuminate_media (an encapsulant
of index 1.41 / 1.333 / 1.2 / 1 in front of the lens, absorbing, and absorbing glass) at four reflections on the same
emitted rays, alternating.  The media change which rays refract and reflect, so the ratio compares two workloads;
whole-call times scatter by +- 15 % here.
--farfield prints one more JSON line: on the same wide emitter and media, bzr_illuminate_media and
bzr_illuminate_farfield (the same call plus a 256^2 far-field map at R = sqrt(2), axes the target's) on the same emitted rays, alternating, the far-field call without a target, and the far-field call with
k_land_far's wave combine forced to 0, 4 and 64 rounds; the ratio is the cost of k_land_far per batch and of the far
maps' staging.
--ghost prints one more JSON line: on the same wide emitter, media and far-field frame, bzr_illuminate_farfield (the
yardstick), bzr_illuminate_ghost at budget 0 (its stats and power checked equal to the yardstick's at budget 0) and
bzr_illuminate_ghost at four reflections on the same emitted rays, alternating and rotated; the ratio is the cost of the
roulette's draws and of the bounce segments of the rays it reflects, and the ledger shows where they went."""
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "cuda-bezier-triangle-raytracer_amd"))
sys.path.insert(0, str(REPO))

import bzr_amd  # noqa: E402
from bzr_amd.configs import CONFIGS, build_lens  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if a not in ("--power", "--media", "--farfield", "--ghost", "--bidir")]
    power, media, farfield = "--power" in sys.argv[1:], "--media" in sys.argv[1:], "--farfield" in sys.argv[1:]
    tir = None
    if "--tir" in args:
        k = args.index("--tir")
        tir = int(args[k + 1]) if k + 1 < len(args) and args[k + 1].isdigit() else 4
        del args[k:k + (2 if k + 1 < len(args) and args[k + 1].isdigit() else 1)]
    total = int(args[0]) if args else 1 << 24
    ctx = bzr_amd.Context(0)
    dm = bzr_amd.DeviceMesh(ctx, build_lens(bzr_amd.TriMesh, CONFIGS["cfg2"].lenses[0]).bezier_patches())
    em = bzr_amd.Emitter(origin=(0.0, -0.5, -0.5), edge_u=(0.0, 1.0, 0.0), edge_v=(0.0, 0.0, 1.0), parts_u=4,
                         parts_v=4, points_per_part=1024, rays_per_point=1024, belts=16, seed=1)
    tg = bzr_amd.Target(origin=(25.0, -12.0, -12.0), axis_u=(0.0, 1.0, 0.0), axis_v=(0.0, 0.0, 1.0), size_u=24.0,
                        size_v=24.0, bins_u=512, bins_v=512)
    bzr_amd.illuminate(ctx, [dm], [1.3], em, 1 << 20, tg)  # warm-up
    t0 = time.perf_counter()
    hist, stats = bzr_amd.illuminate(ctx, [dm], [1.3], em, total, tg)
    dt = time.perf_counter() - t0
    print(json.dumps({"workload": "illuminate cfg2 lens, emitter at x=0 (no cull), 512^2 target",
                      "rays": total, "seconds": round(dt, 4), "mrays_per_s": round(total / dt / 1e6, 1),
                      "stats": stats, "landed_fraction": round(stats["landed"] / total, 5)}))
    if tir is not None:
        bench_tir(ctx, dm, tg, total, tir)
    if media:
        bench_media(ctx, dm, tg, total)
    if farfield:
        bench_farfield(ctx, dm, tg, total)
    if "--ghost" in sys.argv[1:]:
        bench_ghost(ctx, dm, tg, total)
    if "--bidir" in sys.argv[1:]:
        bench_bidir(ctx, dm, tg, total)
    if not power:
        return

    def counts():
        return bzr_amd.illuminate(ctx, [dm], [1.3], em, total, tg)[1]

    def weighted():
        return bzr_amd.illuminate_power(ctx, [dm], [1.3], em, total, tg)[2:]

    bzr_amd.illuminate_power(ctx, [dm], [1.3], em, 1 << 20, tg)  # warm-up
    wall = {"illuminate": [], "illuminate_power": []}
    for _ in range(5):  # alternating, so drift hits both alike
        for name, call in (("illuminate", counts), ("illuminate_power", weighted)):
            t0 = time.perf_counter()
            out = call()
            wall[name].append(time.perf_counter() - t0)
    pstats, ppower = out
    chain = {}
    for name, call in (("illuminate", counts), ("illuminate_power", weighted)):  # event timing perturbs the wall time
        ctx.timing(True)
        ctx.timing_report()
        call()
        chain[name] = sum(v[0] for v in ctx.timing_report().values()) / 1e3
        ctx.timing(False)
    med = {k: statistics.median(v) for k, v in wall.items()}
    print(json.dumps({"workload": "illuminate_power (Lambert, Fresnel) beside illuminate, same rays, 512^2 target",
                      "rays": total,
                      "seconds": {k: round(v, 4) for k, v in med.items()},
                      "mrays_per_s": {k: round(total / v / 1e6, 1) for k, v in med.items()},
                      "chain_kernels_seconds": {k: round(v, 4) for k, v in chain.items()},
                      "emit_land_host_seconds": {k: round(med[k] - chain[k], 4) for k in med},
                      "power_over_counts": round(med["illuminate_power"] / med["illuminate"], 4),
                      "stats": pstats, "landed_power_fraction": round(ppower["landed"] / max(ppower["emitted"], 1), 5)}))


def bench_tir(ctx, dm, tg, total, max_bounces):
    row1 = [1.3, 1.5, 1.8, 2.4]
    em = bzr_amd.Emitter(origin=(8.0, -3.0, -1.5), edge_u=(0.0, 6.0, 0.0), edge_v=(0.0, 0.0, 3.0), parts_u=4, parts_v=4,
                         points_per_part=1024, rays_per_point=1024, belts=16, seed=1)
    calls = {"illuminate_spectral": lambda n: bzr_amd.illuminate_spectral(ctx, [dm], [row1], em, n, tg)[2:],
             "illuminate_tir_0": lambda n: bzr_amd.illuminate_tir(ctx, [dm], [row1], em, n, tg, max_bounces=0)[4:],
             f"illuminate_tir_{max_bounces}":
                 lambda n: bzr_amd.illuminate_tir(ctx, [dm], [row1], em, n, tg, max_bounces=max_bounces)[4:]}
    wall, out = {k: [] for k in calls}, {}
    for call in calls.values():
        call(1 << 20)  # warm-up
    names = list(calls)
    for r in range(6):  # alternating, so drift hits all three alike; rotated, so each call follows each other one
        for name in names[r % 3:] + names[:r % 3]:
            t0 = time.perf_counter()
            out[name] = calls[name](total)
            wall[name].append(time.perf_counter() - t0)
    chain = {}
    for name in names:  # the chain kernels' share, from the context's events (a pass of its own: it perturbs the wall time)
        ctx.timing(True)
        ctx.timing_report()
        calls[name](total)
        chain[name] = sum(v[0] for v in ctx.timing_report().values()) / 1e3
        ctx.timing(False)
    med = {k: statistics.median(v) for k, v in wall.items()}
    top = f"illuminate_tir_{max_bounces}"
    stats, _, ledger = out[top]
    count = ledger["count"].sum(axis=0)
    print(json.dumps({"workload": "illuminate_tir beside illuminate_spectral, cfg2 lens, emitter at x=8 (no cull), "
                                  "indices 1.3/1.5/1.8/2.4, 512^2 target",
                      "rays": total, "max_bounces": max_bounces,
                      "seconds": {k: round(v, 4) for k, v in med.items()},
                      "seconds_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in wall.items()},
                      "mrays_per_s": {k: round(total / v / 1e6, 1) for k, v in med.items()},
                      "chain_kernels_seconds": {k: round(v, 4) for k, v in chain.items()},
                      "emit_land_host_seconds": {k: round(med[k] - chain[k], 4) for k in med},
                      "tir_0_over_spectral": round(med["illuminate_tir_0"] / med["illuminate_spectral"], 4),
                      "tir_n_over_tir_0": round(med[top] / med["illuminate_tir_0"], 4),
                      "reflecting_fraction": round(int(count[1:, :2].sum()) / total, 5),
                      "landed": {"spectral": sum(s["landed"] for s in out["illuminate_spectral"][0]),
                                 "tir_0": sum(s["landed"] for s in out["illuminate_tir_0"][0]),
                                 top: sum(s["landed"] for s in stats), "reflected": int(count[1:, 2].sum())},
                      "ledger_rows_lost_exited_landed": count.tolist()}))


def bench_media(ctx, dm, tg, total, max_bounces=4):
    row1 = [1.3, 1.5, 1.8, 2.4]
    gaps, glass, front = [[1.41, 1.333, 1.2, 1.0], [1.0] * 4], [[0.05, 0.7, 0.4, 200.0]], [[0.3, 0.02, 0.0, 0.1]]
    em = bzr_amd.Emitter(origin=(8.0, -3.0, -1.5), edge_u=(0.0, 6.0, 0.0), edge_v=(0.0, 0.0, 3.0), parts_u=4, parts_v=4,
                         points_per_part=1024, rays_per_point=1024, belts=16, seed=1)
    calls = {"illuminate_tir": lambda n: bzr_amd.illuminate_tir(ctx, [dm], [row1], em, n, tg, max_bounces=max_bounces)[4:],
             "illuminate_media_vacuum": lambda n: bzr_amd.illuminate_media(ctx, [dm], [row1], None, None, None, em, n, tg,
                                                                          max_bounces=max_bounces)[4:],
             "illuminate_media": lambda n: bzr_amd.illuminate_media(ctx, [dm], [row1], gaps, glass, front, em, n, tg,
                                                                   max_bounces=max_bounces)[4:]}
    wall, out = {k: [] for k in calls}, {}
    for call in calls.values():
        call(1 << 20)  # warm-up
    names = list(calls)
    for r in range(6):  # alternating and rotated, as bench_tir
        for name in names[r % 3:] + names[:r % 3]:
            t0 = time.perf_counter()
            out[name] = calls[name](total)
            wall[name].append(time.perf_counter() - t0)
    chain = {}
    for name in names:
        ctx.timing(True)
        ctx.timing_report()
        calls[name](total)
        chain[name] = sum(v[0] for v in ctx.timing_report().values()) / 1e3
        ctx.timing(False)
    med = {k: statistics.median(v) for k, v in wall.items()}
    same = out["illuminate_tir"][0] == out["illuminate_media_vacuum"][0] and \
        out["illuminate_tir"][1] == out["illuminate_media_vacuum"][1]
    print(json.dumps({"workload": "illuminate_media beside illuminate_tir, cfg2 lens, emitter at x=8 (no cull), "
                                  "indices 1.3/1.5/1.8/2.4, 512^2 target",
                      "rays": total, "max_bounces": max_bounces,
                      "seconds": {k: round(v, 4) for k, v in med.items()},
                      "seconds_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in wall.items()},
                      "mrays_per_s": {k: round(total / v / 1e6, 1) for k, v in med.items()},
                      "chain_kernels_seconds": {k: round(v, 4) for k, v in chain.items()},
                      "media_vacuum_over_tir": round(med["illuminate_media_vacuum"] / med["illuminate_tir"], 4),
                      "media_over_tir": round(med["illuminate_media"] / med["illuminate_tir"], 4),
                      "vacuum_stats_and_power_same_as_tir": bool(same),
                      "landed": {k: sum(s["landed"] for s in v[0]) for k, v in out.items()},
                      "landed_power_fraction": {k: round(sum(p["landed"] for p in v[1]) /
                                                         max(sum(p["emitted"] for p in v[1]), 1), 5)
                                                for k, v in out.items()}}))


def bench_farfield(ctx, dm, tg, total, max_bounces=4):
    row1 = [1.3, 1.5, 1.8, 2.4]
    gaps, glass, front = [[1.41, 1.333, 1.2, 1.0], [1.0] * 4], [[0.05, 0.7, 0.4, 200.0]], [[0.3, 0.02, 0.0, 0.1]]
    em = bzr_amd.Emitter(origin=(8.0, -3.0, -1.5), edge_u=(0.0, 6.0, 0.0), edge_v=(0.0, 0.0, 3.0), parts_u=4, parts_v=4,
                         points_per_part=1024, rays_per_point=1024, belts=16, seed=1)
    far = bzr_amd.FarField(axis_u=(0.0, 1.0, 0.0), axis_v=(0.0, 0.0, 1.0), extent=bzr_amd.SQRT2, bins_u=256, bins_v=256)
    calls = {"illuminate_media": lambda n: bzr_amd.illuminate_media(ctx, [dm], [row1], gaps, glass, front, em, n, tg,
                                                                   max_bounces=max_bounces)[4:],
             "illuminate_farfield": lambda n: bzr_amd.illuminate_farfield(ctx, [dm], [row1], gaps, glass, front, em, n, tg,
                                                                         far, max_bounces=max_bounces)[4:],
             "illuminate_farfield_no_target": lambda n: bzr_amd.illuminate_farfield(ctx, [dm], [row1], gaps, glass, front,
                                                                                   em, n, None, far,
                                                                                   max_bounces=max_bounces)[4:]}

    def at_rounds(rounds):  # the far-field call with k_land_far's wave combine at `rounds` rounds (64: unbounded)
        def call(n):
            bzr_amd.debug_farfield_rounds(ctx, rounds)
            try:
                return calls["illuminate_farfield"](n)
            finally:
                bzr_amd.debug_farfield_rounds(ctx, -1)
        return call

    for rounds in (0, 4, 64):
        calls[f"illuminate_farfield_rounds_{rounds}"] = at_rounds(rounds)
    wall, out = {k: [] for k in calls}, {}
    for call in calls.values():
        call(1 << 20)  # warm-up
    names = list(calls)
    for r in range(6):  # alternating and rotated, as bench_tir
        for name in names[r % len(names):] + names[:r % len(names)]:
            t0 = time.perf_counter()
            out[name] = calls[name](total)
            wall[name].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in wall.items()}
    fo = out["illuminate_farfield"][3]
    same = out["illuminate_media"][:2] == out["illuminate_farfield"][:2]
    print(json.dumps({"workload": "illuminate_farfield beside illuminate_media, cfg2 lens, emitter at x=8 (no cull), "
                                  "indices 1.3/1.5/1.8/2.4, 512^2 target, 256^2 far-field map",
                      "rays": total, "max_bounces": max_bounces,
                      "seconds": {k: round(v, 4) for k, v in med.items()},
                      "seconds_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in wall.items()},
                      "mrays_per_s": {k: round(total / v / 1e6, 1) for k, v in med.items()},
                      "farfield_over_media": round(med["illuminate_farfield"] / med["illuminate_media"], 4),
                      "no_target_over_media": round(med["illuminate_farfield_no_target"] / med["illuminate_media"], 4),
                      "stats_and_power_same_as_media": bool(same),
                      "seen": sum(s["seen"] for s in fo["stats"]), "binned": sum(s["binned"] for s in fo["stats"]),
                      "exited": sum(s["exited"] for s in out["illuminate_farfield"][0]),
                      "binned_power_fraction": round(sum(p["binned"] for p in fo["power"]) /
                                                     max(sum(p["emitted"] for p in out["illuminate_farfield"][1]), 1), 5)}))


def bench_ghost(ctx, dm, tg, total, max_bounces=4, seed=2024):
    row1 = [1.3, 1.5, 1.8, 2.4]
    gaps, glass, front = [[1.41, 1.333, 1.2, 1.0], [1.0] * 4], [[0.05, 0.7, 0.4, 200.0]], [[0.3, 0.02, 0.0, 0.1]]
    em = bzr_amd.Emitter(origin=(8.0, -3.0, -1.5), edge_u=(0.0, 6.0, 0.0), edge_v=(0.0, 0.0, 3.0), parts_u=4, parts_v=4,
                         points_per_part=1024, rays_per_point=1024, belts=16, seed=1)
    far = bzr_amd.FarField(axis_u=(0.0, 1.0, 0.0), axis_v=(0.0, 0.0, 1.0), extent=bzr_amd.SQRT2, bins_u=256, bins_v=256)

    def farfield(n, budget=max_bounces):
        return bzr_amd.illuminate_farfield(ctx, [dm], [row1], gaps, glass, front, em, n, tg, far, max_bounces=budget)[4:]

    def ghost(n, budget=max_bounces):
        return bzr_amd.illuminate_ghost(ctx, [dm], [row1], gaps, glass, front, em, n, tg, far, max_bounces=budget,
                                        ghost_seed=seed)[4:]

    calls = {"illuminate_farfield": farfield, "illuminate_ghost_0": lambda n: ghost(n, 0), "illuminate_ghost": ghost}
    for call in calls.values():
        call(1 << 20)  # warm-up
    same = farfield(1 << 20, 0)[:2] == ghost(1 << 20, 0)[:2]
    wall, out = {k: [] for k in calls}, {}
    names = list(calls)
    for r in range(6):  # alternating and rotated, as bench_tir
        for name in names[r % 3:] + names[:r % 3]:
            t0 = time.perf_counter()
            out[name] = calls[name](total)
            wall[name].append(time.perf_counter() - t0)
    chain = {}
    for name in names:
        ctx.timing(True)
        ctx.timing_report()
        calls[name](total)
        chain[name] = sum(v[0] for v in ctx.timing_report().values()) / 1e3
        ctx.timing(False)
    med = {k: statistics.median(v) for k, v in wall.items()}
    count = {k: out[k][2]["count"].sum(axis=0) for k in ("illuminate_farfield", "illuminate_ghost")}
    print(json.dumps({"workload": "illuminate_ghost beside illuminate_farfield, cfg2 lens, emitter at x=8 (no cull), "
                                  "indices 1.3/1.5/1.8/2.4, 512^2 target, 256^2 far-field map",
                      "rays": total, "max_bounces": max_bounces, "ghost_seed": seed,
                      "seconds": {k: round(v, 4) for k, v in med.items()},
                      "seconds_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in wall.items()},
                      "mrays_per_s": {k: round(total / v / 1e6, 1) for k, v in med.items()},
                      "chain_kernels_seconds": {k: round(v, 4) for k, v in chain.items()},
                      "ghost_0_over_farfield": round(med["illuminate_ghost_0"] / med["illuminate_farfield"], 4),
                      "ghost_over_farfield": round(med["illuminate_ghost"] / med["illuminate_farfield"], 4),
                      "ghost_over_farfield_rounds": [round(x / y, 4) for x, y in
                                                     zip(wall["illuminate_ghost"], wall["illuminate_farfield"])],
                      "budget_0_stats_and_power_same_as_farfield": bool(same),
                      "reflecting_fraction": {k: round(int(v[1:, :2].sum()) / total, 5) for k, v in count.items()},
                      "landed_reflected": {k: int(v[1:, 2].sum()) for k, v in count.items()},
                      "landed_power_fraction": {k: round(sum(p["landed"] for p in out[k][1]) /
                                                         max(sum(p["emitted"] for p in out[k][1]), 1), 5) for k in count},
                      "ledger_rows_lost_exited_landed": {k: v.tolist() for k, v in count.items()}}))


def bench_bidir(ctx, dm, tg, total, max_bounces=4, seed=2024):
    """--bidir: on bench_ghost's emitter, media and far-field frame, bzr_illuminate_ghost (the yardstick) and
    bzr_illuminate_bidir at four reflections on the same emitted rays, alternating and rotated; one more JSON line."""
    row1 = [1.3, 1.5, 1.8, 2.4]
    gaps, glass, front = [[1.41, 1.333, 1.2, 1.0], [1.0] * 4], [[0.05, 0.7, 0.4, 200.0]], [[0.3, 0.02, 0.0, 0.1]]
    em = bzr_amd.Emitter(origin=(8.0, -3.0, -1.5), edge_u=(0.0, 6.0, 0.0), edge_v=(0.0, 0.0, 3.0), parts_u=4, parts_v=4,
                         points_per_part=1024, rays_per_point=1024, belts=16, seed=1)
    far = bzr_amd.FarField(axis_u=(0.0, 1.0, 0.0), axis_v=(0.0, 0.0, 1.0), extent=bzr_amd.SQRT2, bins_u=256, bins_v=256)

    def ghost(n):
        return bzr_amd.illuminate_ghost(ctx, [dm], [row1], gaps, glass, front, em, n, tg, far, max_bounces=max_bounces,
                                        ghost_seed=seed, mode=bzr_amd.PIPELINE_FUSED)[4:]

    def bidir(n):
        return bzr_amd.illuminate_bidir(ctx, [dm], [row1], gaps, glass, front, em, n, tg, far, max_bounces=max_bounces,
                                        ghost_seed=seed, axis=(1.0, 0.0, 0.0))[4:]

    calls = {"illuminate_ghost": ghost, "illuminate_bidir": bidir}
    for call in calls.values():
        call(1 << 20)  # warm-up
    wall, out = {k: [] for k in calls}, {}
    names = list(calls)
    for r in range(6):  # alternating and rotated
        for name in names[r % 2:] + names[:r % 2]:
            t0 = time.perf_counter()
            out[name] = calls[name](total)
            wall[name].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in wall.items()}
    led = out["illuminate_bidir"][2]
    emitted = sum(p["emitted"] for p in out["illuminate_bidir"][1])
    traced = sum(s["emitted"] - s["culled"] for s in out["illuminate_bidir"][0])
    print(json.dumps({"workload": "illuminate_bidir beside illuminate_ghost (fused), cfg2 lens, emitter at x=8 (no cull), "
                                  "indices 1.3/1.5/1.8/2.4, 512^2 target, 256^2 far-field map",
                      "rays": total, "max_bounces": max_bounces, "ghost_seed": seed,
                      "seconds": {k: round(v, 4) for k, v in med.items()},
                      "seconds_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in wall.items()},
                      "bidir_over_ghost": round(med["illuminate_bidir"] / med["illuminate_ghost"], 4),
                      "bidir_over_ghost_rounds": [round(x / y, 4) for x, y in
                                                  zip(wall["illuminate_bidir"], wall["illuminate_ghost"])],
                      "count_identity_holds": int(led["count"][:, :, :2].sum()) + int(led["back_count"].sum()) == traced,
                      "back_rays_by_row": led["back_count"].sum(axis=0).tolist(),
                      "back_power_fraction": round(int(led["back_power"].sum()) / max(emitted, 1), 5),
                      "landed_power_fraction": {k: round(sum(p["landed"] for p in out[k][1]) /
                                                         max(sum(p["emitted"] for p in out[k][1]), 1), 5) for k in calls}}))


if __name__ == "__main__":
    main()
