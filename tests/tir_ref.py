"""Reference for the total-internal-reflection tests: the oracle composed segment by segment, Snell's s2, the
reflecting step and the Fresnel term in numpy float32.

Nothing here comes from the code under test.  It has the shape of power_ref.chain, run once per channel like
spectral_ref.chain.  Per lens the rays alive go through one refract(INSIDE) segment and then up to 1 + max_bounces
refract(OUTSIDE) segments.  The oracle's BezierLens::refract decides and performs every refraction; its
BezierMesh::intersect supplies the hit's cosine (row 4), point (rows 1-3), normal (rows 8-10) and kind (row 11).  A ray
of an OUTSIDE segment whose hit is an intersection with cs >= 0 and s2 = ri^2 (1 - cs^2) >= 1 is reflected while it has
bounce budget left in this lens: k = 2 cs, r = d - normal k, direction = normalized(r), origin = the hit's point
(include/bzr.h bzr_trace_chain_tir), evaluated in np.float32 -- IEEE binary32, one correctly rounded operation per
numpy call, the contract's order.  The oracle must have returned NONE for every ray reflected here (asserted).
"""
import numpy as np

import power_ref

F = np.float32
RR_NONE, RR_INSIDE, RR_OUTSIDE = 0, 1, 2
INTERSECT = 4


def reflect(d, normal, cs):
    """The reflecting step for float32 arrays d [3, m], normal [3, m], cs [m] -> direction [3, m]."""
    d, normal, cs = np.asarray(d, F), np.asarray(normal, F), np.asarray(cs, F)
    k = F(2) * cs
    r = d - normal * k
    sq = r * r
    z = sq[0] + (sq[1] + sq[2])
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = r / np.sqrt(z)
    out = np.where(z > F(0), unit, r)
    assert out.dtype == F
    return out


def chain_one(orc, lenses, ris, rays, weight=None, max_bounces=4, threads=16):
    """(rays [6, n], weight [n], status [n], segments [n], bounces [n]) of the chain with one index per lens."""
    rays = np.ascontiguousarray(rays, F)
    n = rays.shape[1]
    out = rays.copy()
    w = np.ones(n, F) if weight is None else np.array(weight, F)
    status = np.zeros(n, np.uint32)
    seg = np.zeros(n, np.uint32)
    bounces = np.zeros(n, np.uint32)
    alive = np.arange(n)
    for patches, ri in zip(lenses, ris):
        if alive.size == 0:
            break
        ri = F(ri)
        # refract(INSIDE): never reflects
        r = np.ascontiguousarray(out[:, alive])
        cs = orc.intersect(patches, r, threads)[4]
        o, s = orc.refract(patches, float(ri), r, np.full(alive.size, RR_INSIDE, np.uint32), threads)
        seg[alive] += 1
        status[alive] = s
        ok = s != RR_NONE
        t, s2 = power_ref.fresnel_t(np.full(int(ok.sum()), F(1) / ri, F), cs[ok])
        assert (s2 < F(0.99)).all()
        w[alive[ok]] = w[alive[ok]] * t
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
            out[3:6, pend[refl]] = reflect(r[3:6][:, refl], hit[8:11][:, refl], cs[refl])
            bounces[pend[refl]] += 1
            rest = ~refl
            status[pend[rest]] = s[rest]
            ok = rest & (s != RR_NONE)
            t, s2ok = power_ref.fresnel_t(np.full(int(ok.sum()), ri, F), cs[ok])
            assert (s2ok < F(0.99)).all()
            w[pend[ok]] = w[pend[ok]] * t
            out[:, pend[ok]] = o[:, ok]
            left.append(pend[ok])
            pend = pend[refl]
        assert pend.size == 0  # the last OUTSIDE segment reflects nothing
        alive = np.sort(np.concatenate(left)) if left else np.zeros(0, np.int64)
    return out, w, status, seg, bounces


def chain(orc, lenses, ri_table, rays, channel=None, weight=None, max_bounces=4):
    """(rays, weight, status, segments, bounces) with ri_table[l][channel[i]] for ray i; channel None: channel 0.  A
    ray whose channel is not below nchan is not traced: NONE, one segment, no bounce, ray and weight as they were."""
    table = np.asarray(ri_table, F)
    rays = np.ascontiguousarray(rays, F)
    n = rays.shape[1]
    channel = np.zeros(n, np.uint8) if channel is None else np.asarray(channel)
    assert table.ndim == 2 and table.shape[0] == len(lenses) and channel.shape == (n,)
    out = rays.copy()
    w = np.ones(n, F) if weight is None else np.array(weight, F)
    status = np.zeros(n, np.uint32)
    seg = np.ones(n, np.uint32)
    bounces = np.zeros(n, np.uint32)
    for c in range(table.shape[1]):
        idx = np.nonzero(channel == c)[0]
        if idx.size == 0:
            continue
        o, wc, s, g, b = chain_one(orc, lenses, list(table[:, c]), rays[:, idx], w[idx], max_bounces)
        out[:, idx], w[idx], status[idx], seg[idx], bounces[idx] = o, wc, s, g, b
    return out, w, status, seg, bounces
