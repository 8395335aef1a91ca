"""Reference for the ray-power tests: the oracle composed segment by segment, the Fresnel term in numpy float32.

Nothing here comes from the code under test.  For each lens and side the rays still alive go through the oracle's
BezierMesh::intersect (the hit's cosine is row 4) and BezierLens::refract; the transmittance of every refraction whose
status is not NONE is evaluated with the contract's formula (include/bzr.h bzr_trace_chain_power) in np.float32 --
IEEE binary32, one correctly rounded operation per numpy call, the contract's order -- and multiplied into the ray's
weight.  Power sums use the contract's fixed point q(w) = trunc(w x 2^32), exact in float64.
"""
import numpy as np

F = np.float32
RR_NONE, RR_INSIDE, RR_OUTSIDE = 0, 1, 2


def fresnel_t(eta, cs):
    """T for float32 arrays (eta, cs) with s2 = eta^2 (1 - cs^2); the value is meaningful where s2 < 0.99."""
    eta, cs = np.asarray(eta, F), np.asarray(cs, F)
    one, half = F(1), F(0.5)
    with np.errstate(invalid="ignore", divide="ignore"):
        s2 = (eta * eta) * (one - cs * cs)
        c1 = np.abs(cs)
        c2 = np.sqrt(one - s2)
        a = eta * c1
        rs = (a - c2) / (a + c2)
        b = eta * c2
        rp = (b - c1) / (b + c1)
        t = one - half * (rs * rs + rp * rp)
    assert t.dtype == F
    return t, s2


def chain(orc, lenses, ris, rays, weight=None, threads=16):
    """(rays [6, n], weight [n], status [n], segments [n]) of the refraction chain with ray power."""
    rays = np.ascontiguousarray(rays, F)
    n = rays.shape[1]
    out = rays.copy()
    w = np.ones(n, F) if weight is None else np.array(weight, F)
    status = np.zeros(n, np.uint32)
    seg = np.zeros(n, np.uint32)
    alive = np.arange(n)
    for patches, ri in zip(lenses, ris):
        for expected in (RR_INSIDE, RR_OUTSIDE):
            if alive.size == 0:
                break
            r = np.ascontiguousarray(out[:, alive])
            cs = orc.intersect(patches, r, threads)[4]
            o, s = orc.refract(patches, ri, r, np.full(alive.size, expected, np.uint32), threads)
            seg[alive] += 1
            status[alive] = s
            ok = s != RR_NONE
            eta = F(1) / F(ri) if expected == RR_INSIDE else F(ri)
            t, s2 = fresnel_t(np.full(int(ok.sum()), eta, F), cs[ok])
            assert (s2 < F(0.99)).all()  # a successful refraction, as Snell's step decided it
            w[alive[ok]] = w[alive[ok]] * t
            out[:, alive[ok]] = o[:, ok]
            alive = alive[ok]
    return out, w, status, seg


def q32(w):
    """q(w) = trunc(w x 2^32) as uint64 (exact: a float32 times 2^32 is a float64)."""
    return np.floor(np.asarray(w, F).astype(np.float64) * 2.0 ** 32).astype(np.uint64)


def flux(orc, tg, rays, status, w):
    """The weighted target histogram (uint64 [bins_v, bins_u], 32.32 fixed point): bit b of every ray's q lands on
    its own through the oracle's binning, sum over b of (count << b)."""
    q = q32(w)
    total = np.zeros((tg.bins_v, tg.bins_u), np.uint64)
    for b in range(33):
        st = np.where((q >> np.uint64(b)) & np.uint64(1), status, 0).astype(np.uint32)
        h, _, _ = orc.land(tg, rays, st)
        total += h.astype(np.uint64) << np.uint64(b)
    return total
