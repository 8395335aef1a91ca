"""Reference for the far-field maps: the cell rule of include/bzr.h (bzr_farfield) in numpy float32, written from the
header's text.  Nothing here comes from the code under test.

Every numpy call below is one correctly rounded IEEE binary32 operation on float32 arrays, in the header's order (dot
products as x0 y0 + (x1 y1 + x2 y2)), so the cells agree with the device and with bzr_farfield_cell bit for bit.  The
rows the maps are made from come from what is already trusted (illum_tir_ref.reference, absorb_ref.illum_reference:
per-ray out, w, status, channel, bounces).  Everything compared is an integer, so every comparison is exact.
"""
from types import SimpleNamespace

import numpy as np

F = np.float32
RR_OUTSIDE = 2
SQRT2 = F(np.sqrt(2.0))  # 0x3FB504F3: the largest extent


def frame(axis_u, axis_v, extent, bins_u, bins_v):
    """The frame and what the rule derives from it: the pole n = axis_u x axis_v, normalised as illuminate() normalises
    the target's normal (z = x x + (y y + z z); each component / sqrt(z) when z > 0)."""
    au, av = np.asarray(axis_u, F), np.asarray(axis_v, F)
    n = np.array([au[1] * av[2] - au[2] * av[1], au[2] * av[0] - au[0] * av[2], au[0] * av[1] - au[1] * av[0]], F)
    z = F(n[0] * n[0] + F(n[1] * n[1] + n[2] * n[2]))
    if z > 0:
        n = (n / np.sqrt(z)).astype(F)
    R = F(extent)
    assert n.dtype == F and 0 < R <= SQRT2
    return SimpleNamespace(axis_u=au, axis_v=av, n=n, R=R, bins_u=int(bins_u), bins_v=int(bins_v),
                           cells=int(bins_u) * int(bins_v))


def struct(mod, fr):
    """The frame as mod.FarField (bzr_amd's ctypes structure)."""
    return mod.FarField(axis_u=tuple(float(x) for x in fr.axis_u), axis_v=tuple(float(x) for x in fr.axis_v),
                        extent=float(fr.R), bins_u=fr.bins_u, bins_v=fr.bins_v)


def _dot(d, a):
    return d[0] * a[0] + (d[1] * a[1] + d[2] * a[2])


def project(fr, d):
    """(X, Y, g) of directions d [3, n] float32."""
    d = np.asarray(d, F)
    with np.errstate(all="ignore"):
        mu, a, b = _dot(d, fr.n), _dot(d, fr.axis_u), _dot(d, fr.axis_v)
        g = F(1) + mu
        h = F(2) / g
        k = np.sqrt(h)
        X, Y = a * k, b * k
    assert X.dtype == F and Y.dtype == F and g.dtype == F
    return X, Y, g


def cell(fr, d):
    """int64 cell index iv * bins_u + iu per direction of d [3, n], -1 where it is not binned."""
    X, Y, g = project(fr, d)
    with np.errstate(all="ignore"):
        u, v, S = X + fr.R, Y + fr.R, fr.R + fr.R
        ok = (g > 0) & (u >= 0) & (u < S) & (v >= 0) & (v < S)
        cu, cv = S / F(fr.bins_u), S / F(fr.bins_v)
        assert u.dtype == F and isinstance(cu, F) and isinstance(S, F)
        iu = np.minimum(np.where(ok, u / cu, F(0)).astype(np.int64), fr.bins_u - 1)
        iv = np.minimum(np.where(ok, v / cv, F(0)).astype(np.int64), fr.bins_v - 1)
    return np.where(ok, iv * fr.bins_u + iu, -1)


def q32(w):
    """q(w) = trunc(w x 2^32) for w > 0, else 0 (NaN and negative weights carry nothing), as uint64."""
    w = np.asarray(w, F)
    pos = w > 0  # False for NaN
    return np.where(pos, np.floor(np.where(pos, w, F(0)).astype(np.float64) * 2.0 ** 32), 0.0).astype(np.uint64)


def bin_rays(fr, rays, weight=None, status=None, channel=None, nchan=1, bounces=None):
    """What bzr_farfield_bin adds for rays [6, n]: flux uint64 and hist uint32 [nchan, bins_v, bins_u], stats and power
    uint64 [nchan, 2] (SEEN, BINNED); with `bounces` also rflux, the flux of the rays with bounces > 0."""
    rays = np.asarray(rays, F)
    n = rays.shape[1]
    w = np.ones(n, F) if weight is None else np.asarray(weight, F)
    ch = np.zeros(n, np.int64) if channel is None else np.asarray(channel).astype(np.int64)
    seen = (np.ones(n, bool) if status is None else np.asarray(status) == RR_OUTSIDE) & (ch < nchan)
    c = cell(fr, rays[3:6])
    binned = seen & (c >= 0)
    q = q32(w)
    key = np.where(binned, ch * fr.cells + c, 0)
    flux, hist = np.zeros(nchan * fr.cells, np.uint64), np.zeros(nchan * fr.cells, np.uint32)
    np.add.at(flux, key[binned], q[binned])
    np.add.at(hist, key[binned], np.uint32(1))
    stats, power = np.zeros((nchan, 2), np.uint64), np.zeros((nchan, 2), np.uint64)
    for k in range(nchan):
        for col, m in enumerate((seen, binned)):
            stats[k, col] = int((m & (ch == k)).sum())
            power[k, col] = int(q[m & (ch == k)].sum(dtype=np.uint64))
    shape = (nchan, fr.bins_v, fr.bins_u)
    out = SimpleNamespace(flux=flux.reshape(shape), hist=hist.reshape(shape), stats=stats, power=power, cell=c,
                          binned=binned, seen=seen)
    if bounces is not None:
        r = binned & (np.asarray(bounces) > 0)
        rflux = np.zeros(nchan * fr.cells, np.uint64)
        np.add.at(rflux, key[r], q[r])
        out.rflux, out.reflected = rflux.reshape(shape), r
    return out


def of_illumination(fr, ref):
    """The far outputs of bzr_illuminate_farfield for the per-ray rows of an illumination reference (illum_tir_ref /
    absorb_ref: ref.out, ref.w, ref.status, ref.channel, ref.bounces, ref.nchan)."""
    return bin_rays(fr, ref.out, ref.w, ref.status, ref.channel, ref.nchan, ref.bounces)
