"""Reference for the optical-path tests: tir_ref's chain (the oracle composed segment by segment, the reflecting step
and the Fresnel term in numpy float32) plus the per-leg step of include/bzr.h bzr_trace_chain_opl.

Nothing here comes from the code under test.  The chain is tir_ref.chain_one's, statement for statement; every segment
that ends in a successful refraction or in a reflection adds its leg, from the segment's origin s (the ray the oracle
was given) to the winning hit's point p (rows 1-3 of the oracle's BezierMesh::intersect):

    e = p - s      z = e0 e0 + (e1 e1 + e2 e2)      len = sqrt(z)
    refract(INSIDE):   opl = opl + len
    refract(OUTSIDE):  glass = glass + len;  m = ri len;  opl = opl + m        (bounce segments included)

in np.float32 -- IEEE binary32, one correctly rounded operation per numpy call, the contract's order.  Two more sums
over the same legs serve the tests: `tsum`, the same accumulation with the hit's t (row 0) in place of len -- the form
the contract rejects -- and `opl64`, the legs' lengths and the sum in float64 from the same float32 points.
"""
import numpy as np

import power_ref
import tir_ref

F = np.float32
RR_NONE, RR_INSIDE, RR_OUTSIDE = 0, 1, 2
INTERSECT = 4


def leg(s, p):
    """len [m] of the legs from s [3, m] to p [3, m], float32 in the contract's order."""
    e = np.asarray(p, F) - np.asarray(s, F)
    sq = e * e
    z = sq[0] + (sq[1] + sq[2])
    out = np.sqrt(z)
    assert out.dtype == F
    return out


def leg64(s, p):
    e = np.asarray(p, F).astype(np.float64) - np.asarray(s, F).astype(np.float64)
    return np.sqrt((e * e).sum(axis=0))


def chain_one(orc, lenses, ris, rays, weight=None, opl=None, max_bounces=4, threads=16):
    """(rays [6, n], weight [n], status [n], segments [n], bounces [n], opl [n], glass [n], tsum [n], opl64 [n]) of the
    chain with one index per lens."""
    rays = np.ascontiguousarray(rays, F)
    n = rays.shape[1]
    out = rays.copy()
    w = np.ones(n, F) if weight is None else np.array(weight, F)
    path = np.zeros(n, F) if opl is None else np.array(opl, F)
    glass = np.zeros(n, F)
    tsum = path.copy()
    path64 = path.astype(np.float64)
    status = np.zeros(n, np.uint32)
    seg = np.zeros(n, np.uint32)
    bounces = np.zeros(n, np.uint32)
    alive = np.arange(n)
    for patches, ri in zip(lenses, ris):
        if alive.size == 0:
            break
        ri = F(ri)
        # refract(INSIDE): never reflects; the leg lies in air
        r = np.ascontiguousarray(out[:, alive])
        hit = orc.intersect(patches, r, threads)
        cs = hit[4]
        o, s = orc.refract(patches, float(ri), r, np.full(alive.size, RR_INSIDE, np.uint32), threads)
        seg[alive] += 1
        status[alive] = s
        ok = s != RR_NONE
        t, s2 = power_ref.fresnel_t(np.full(int(ok.sum()), F(1) / ri, F), cs[ok])
        assert (s2 < F(0.99)).all()
        w[alive[ok]] = w[alive[ok]] * t
        path[alive[ok]] = path[alive[ok]] + leg(r[0:3][:, ok], hit[1:4][:, ok])
        tsum[alive[ok]] = tsum[alive[ok]] + hit[0][ok]
        path64[alive[ok]] += leg64(r[0:3][:, ok], hit[1:4][:, ok])
        out[:, alive[ok]] = o[:, ok]
        pend = alive[ok]  # inside this lens
        left = []
        for b in range(max_bounces + 1):
            if pend.size == 0:
                break
            r = np.ascontiguousarray(out[:, pend])
            hit = orc.intersect(patches, r, threads)
            cs, what = hit[4], hit.view(np.uint32)[11]
            o, s = orc.refract(patches, float(ri), r, np.full(pend.size, RR_OUTSIDE, np.uint32), threads)
            seg[pend] += 1
            with np.errstate(invalid="ignore"):
                s2 = (ri * ri) * (F(1) - cs * cs)
                refl = (what == INTERSECT) & (cs >= F(0)) & (s2 >= F(1)) & (b < max_bounces)
            assert s2.dtype == F
            assert (s[refl] == RR_NONE).all()  # Snell's step gave these rays up
            out[0:3, pend[refl]] = hit[1:4][:, refl]
            out[3:6, pend[refl]] = tir_ref.reflect(r[3:6][:, refl], hit[8:11][:, refl], cs[refl])
            bounces[pend[refl]] += 1
            rest = ~refl
            status[pend[rest]] = s[rest]
            ok = rest & (s != RR_NONE)
            t, s2ok = power_ref.fresnel_t(np.full(int(ok.sum()), ri, F), cs[ok])
            assert (s2ok < F(0.99)).all()
            w[pend[ok]] = w[pend[ok]] * t
            out[:, pend[ok]] = o[:, ok]
            # the leg lies in glass, for the rays that left the lens and for the rays that were reflected alike
            went = ok | refl
            ln = leg(r[0:3][:, went], hit[1:4][:, went])
            glass[pend[went]] = glass[pend[went]] + ln
            m = ri * ln
            assert m.dtype == F
            path[pend[went]] = path[pend[went]] + m
            tsum[pend[went]] = tsum[pend[went]] + ri * hit[0][went]
            path64[pend[went]] += float(ri) * leg64(r[0:3][:, went], hit[1:4][:, went])
            left.append(pend[ok])
            pend = pend[refl]
        assert pend.size == 0  # the last OUTSIDE segment reflects nothing
        alive = np.sort(np.concatenate(left)) if left else np.zeros(0, np.int64)
    assert path.dtype == F and glass.dtype == F and tsum.dtype == F
    return out, w, status, seg, bounces, path, glass, tsum, path64


def chain(orc, lenses, ri_table, rays, channel=None, weight=None, opl=None, max_bounces=4, extra=None):
    """(rays, weight, status, segments, bounces, opl, glass) with ri_table[l][channel[i]] for ray i; channel None: channel
    0.  A ray whose channel is not below nchan is not traced: NONE, one segment, no bounce, ray, weight and opl as they
    were, glass 0.  `extra`, a dict, receives "tsum" and "opl64"."""
    table = np.asarray(ri_table, F)
    rays = np.ascontiguousarray(rays, F)
    n = rays.shape[1]
    channel = np.zeros(n, np.uint8) if channel is None else np.asarray(channel)
    assert table.ndim == 2 and table.shape[0] == len(lenses) and channel.shape == (n,)
    out = rays.copy()
    w = np.ones(n, F) if weight is None else np.array(weight, F)
    path = np.zeros(n, F) if opl is None else np.array(opl, F)
    glass = np.zeros(n, F)
    tsum, path64 = path.copy(), path.astype(np.float64)
    status = np.zeros(n, np.uint32)
    seg = np.ones(n, np.uint32)
    bounces = np.zeros(n, np.uint32)
    for c in range(table.shape[1]):
        idx = np.nonzero(channel == c)[0]
        if idx.size == 0:
            continue
        res = chain_one(orc, lenses, list(table[:, c]), rays[:, idx], w[idx], path[idx], max_bounces)
        out[:, idx], w[idx], status[idx], seg[idx], bounces[idx], path[idx], glass[idx], tsum[idx], path64[idx] = res
    if extra is not None:
        extra["tsum"], extra["opl64"] = tsum, path64
    return out, w, status, seg, bounces, path, glass
