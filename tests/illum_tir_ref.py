"""Reference for illumination with total internal reflection (bzr_illuminate_tir), composed from what the project
already trusts.  Nothing here comes from the code under test.

  1. orc.emit gives the emitter's rays;
  2. tir_ref.chain over every ray (none is culled: the sphere cull only drops rays that end NONE after one segment
     without a bounce), ray i in channel i mod nchan, with its emitted weight;
  3. orc.land and power_ref.flux per (channel, ledger row) give the maps, power_ref.q32 the power sums.

Every figure is an integer, so every comparison against it is exact.
"""
from types import SimpleNamespace

import numpy as np

import power_ref
import tir_ref
from bzr_amd.configs import CONFIGS, build_lens

F = np.float32
ROW1 = [1.3, 1.5, 1.8, 2.4]        # lens 1's index per channel (tests/test_gpu_tir.py)
ROW2 = [1.5, 1.5168, 1.53, 1.62]   # cfg4's second lens
N_RAYS = 10_000                    # no multiple of 64; three batches at a chunk cap of 4 096
# The emitter's origin.  NEAR: 1 unit in front of the cfg2 lens, inside its bounding sphere (nothing is culled).
# FAR: further back and off to the side, so that over half of its rays miss the sphere (centre (9.92, 0.02, -1.89),
# radius 8.39: the rectangle at (4, -3, -1.5) still lies wholly inside it and loses no ray to the cull).
NEAR, FAR = (8.0, -3.0, -1.5), (4.0, -3.0, 4.5)
ROWS, FIELDS = 9, 3                # BZR_LEDGER_ROWS, BZR_LEDGER_FIELDS
LOST, EXITED, LANDED = 0, 1, 2     # BZR_LEDGER_*
MAX_BOUNCES = 8
RR_NONE, RR_OUTSIDE = 0, 2


def emitter(mod, origin):
    return mod.Emitter(origin=origin, edge_u=(0.0, 6.0, 0.0), edge_v=(0.0, 0.0, 3.0), parts_u=2, parts_v=2,
                       points_per_part=64, rays_per_point=128, belts=16, seed=7)


def target(mod):
    """tests/test_gpu_illumination.py's target()."""
    return mod.Target(origin=(25.0, -12.0, -12.0), axis_u=(0.0, 1.0, 0.0), axis_v=(0.0, 0.0, 1.0), size_u=24.0,
                      size_v=24.0, bins_u=48, bins_v=48)


def lenses_of(bzr, name):
    return [build_lens(bzr.TriMesh, lens).bezier_patches() for lens in CONFIGS[name].lenses]


def reference(orc, lenses, table, origin, max_bounces, n=N_RAYS, lambert=True):
    """What bzr_illuminate_tir must return for the emitter at `origin`, plus the per-ray rows it was made from."""
    table = np.asarray(table, F)
    nchan = table.shape[1]
    rays, _ = orc.emit(emitter(orc, origin), 0, n)
    channel = (np.arange(n) % nchan).astype(np.uint8)
    w0 = rays[3].copy() if lambert else np.ones(n, F)
    out, w, status, seg, bounces = tir_ref.chain(orc, lenses, table, rays, channel, w0, max_bounces)
    assert set(np.unique(status)) <= {RR_NONE, RR_OUTSIDE}
    tg = target(orc)
    shape = (nchan, tg.bins_v, tg.bins_u)
    q, q0 = power_ref.q32(w), power_ref.q32(w0)
    row = np.minimum(bounces, MAX_BOUNCES)
    flux, hist = np.zeros(shape, np.uint64), np.zeros(shape, np.uint32)
    rflux, rhist = np.zeros(shape, np.uint64), np.zeros(shape, np.uint32)
    count, power = np.zeros((nchan, ROWS, FIELDS), np.uint64), np.zeros((nchan, ROWS, FIELDS), np.uint64)
    for c in range(nchan):
        for r in range(ROWS):
            mine = (channel == c) & (row == r)
            if not mine.any():
                continue
            st = np.where(mine, status, 0).astype(np.uint32)
            h, exited, landed = orc.land(tg, out, st)
            f = power_ref.flux(orc, tg, out, st, w) if landed else np.zeros(shape[1:], np.uint64)
            assert exited == int((mine & (status == RR_OUTSIDE)).sum()) and landed == int(h.sum())
            flux[c] += f
            hist[c] += h
            if r > 0:
                rflux[c] += f
                rhist[c] += h
            # LOST here holds every ray that ended NONE, the ones the sphere cull drops included: see `uncut`
            count[c, r] = (int((mine & (status == RR_NONE)).sum()), exited, landed)
            power[c, r] = (int(q[mine & (status == RR_NONE)].sum()), int(q[mine & (status == RR_OUTSIDE)].sum()),
                           int(f.sum()))
    emitted = [int((channel == c).sum()) for c in range(nchan)]
    emitted_q = [int(q0[channel == c].sum()) for c in range(nchan)]
    for a in (rays, channel, w0, out, w, status, seg, bounces, flux, hist, rflux, rhist, count, power):
        a.setflags(write=False)
    return SimpleNamespace(nchan=nchan, rays=rays, channel=channel, w0=w0, out=out, w=w, status=status, seg=seg,
                           bounces=bounces, flux=flux, hist=hist, rflux=rflux, rhist=rhist, uncut_count=count,
                           uncut_power=power, emitted=emitted, emitted_q=emitted_q)


def ledger_for(ref, culled):
    """The ledger given which rays the sphere cull drops (`culled` [n] bool): the reference traces every ray uncut, a
    culled ray would have ended NONE without a bounce, so it leaves row 0's LOST and nothing else."""
    assert not (culled & ((ref.status != RR_NONE) | (ref.bounces != 0))).any()
    count, power = ref.uncut_count.copy(), ref.uncut_power.copy()
    q0 = power_ref.q32(ref.w0)
    for c in range(ref.nchan):
        mine = culled & (ref.channel == c)
        count[c, 0, LOST] -= np.uint64(int(mine.sum()))
        power[c, 0, LOST] -= np.uint64(int(q0[mine].sum()))
    return count, power


def reflected(ref):
    return ref.bounces > 0


def mixed_waves(ref):
    """Waves of 64 consecutive rays that hold both reflected and unreflected lanes."""
    b = reflected(ref)
    return sum(1 for k in range(0, len(b), 64) if b[k:k + 64].any() and not b[k:k + 64].all())
