"""Reference for the absorption tests: media_ref's chain with the Beer-Lambert step of include/bzr.h
bzr_trace_chain_absorb, and the illumination reference composed over it.

Nothing here comes from the code under test.  `att` restates the header's recipe in np.float32, one numpy call per
rounded operation (IEEE binary32, no contraction).  The chain has media_ref.chain_one's shape; every leg that ends in a
refraction or a reflection first attenuates the weight and then, for a refraction, applies the Fresnel term:

    x = a len;  A = a > 0 ? att(x) : 1;  w = w A;  w = w T
    a = gap_absorb[l][c] on a refract(INSIDE) segment, glass_absorb[l][c] on a refract(OUTSIDE) one (bounces included)

tests/test_absorb_ref.py pins it: with both tables zero it is media_ref.chain bit for bit, and att lies within
2^-23 (1 + y) of binary64 exp(-x).
"""
from types import SimpleNamespace

import numpy as np

import illum_tir_ref as itr
import media_ref
import opl_ref
import power_ref
import tir_ref

F = np.float32
RR_NONE, RR_INSIDE, RR_OUTSIDE = 0, 1, 2
INTERSECT = 4
LOG2E = np.array([0x3FB8AA3B], np.uint32).view(F)[0]
# c_j = float32((-ln 2)^j / j!), j = 0 .. 7 (tests/test_absorb_ref.py recomputes them in binary64)
COEFF = np.array([0x3f800000, 0xbf317218, 0x3e75fdf0, 0xbd635847, 0x3c1d955b, 0xbaaec3ff, 0x39218489, 0xb77fe5fe],
                 np.uint32).view(F)


def att(x):
    """att(x) of include/bzr.h for x >= 0 (or NaN), elementwise, float32."""
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore", over="ignore"):
        y = x * LOG2E
        live = y < F(125)
        ys = np.where(live, y, F(0)).astype(F)
        k = np.rint(ys)
        f = ys - k
        p = np.full(x.shape, COEFF[7], F)
        for j in range(6, -1, -1):
            p = p * f
            p = p + COEFF[j]
        scale = ((np.uint32(127) - k.astype(np.uint32)) << np.uint32(23)).astype(np.uint32).view(F)
        r = p * scale
    assert y.dtype == F and k.dtype == F and f.dtype == F and p.dtype == F and r.dtype == F
    return np.where(live, r, F(0)).astype(F)


def attenuation(a, ln):
    """The leg's factor A for the coefficient a (a float32 scalar) and the lengths ln [m]."""
    a = F(a)
    ln = np.asarray(ln, F)
    if not a > F(0):
        return np.ones(ln.shape, F)
    x = a * ln
    assert x.dtype == F
    return att(x)


def chain_one(orc, lenses, ris, gaps, glass_abs, gap_abs, rays, weight=None, opl=None, max_bounces=4, threads=16):
    """media_ref.chain_one with one absorption coefficient per lens glass (glass_abs [nlens]) and per medium in front of
    a lens (gap_abs [nlens])."""
    assert len(gaps) == len(lenses) + 1 == len(ris) + 1 and len(glass_abs) == len(gap_abs) == len(lenses)
    rays = np.ascontiguousarray(rays, F)
    n = rays.shape[1]
    out = rays.copy()
    w = np.ones(n, F) if weight is None else np.array(weight, F)
    path = np.zeros(n, F) if opl is None else np.array(opl, F)
    glass = np.zeros(n, F)
    status = np.zeros(n, np.uint32)
    seg = np.zeros(n, np.uint32)
    bounces = np.zeros(n, np.uint32)
    alive = np.arange(n)
    for l, patches in enumerate(lenses):
        if alive.size == 0:
            break
        n0, n1, n2 = F(gaps[l]), F(ris[l]), F(gaps[l + 1])
        eta_in, eta_out = n0 / n1, n1 / n2
        assert type(eta_in) is F and type(eta_out) is F
        # refract(INSIDE): never reflects; the leg lies in the medium in front of the lens
        r = np.ascontiguousarray(out[:, alive])
        hit = orc.intersect(patches, r, threads)
        s, dirs = media_ref.step(np.full(alive.size, eta_in, F), r[3:6], hit, RR_INSIDE)
        seg[alive] += 1
        status[alive] = s
        ok = s != RR_NONE
        ln = opl_ref.leg(r[0:3][:, ok], hit[1:4][:, ok])
        w[alive[ok]] = w[alive[ok]] * attenuation(gap_abs[l], ln)  # first the leg ...
        t, s2 = power_ref.fresnel_t(np.full(int(ok.sum()), eta_in, F), hit[4][ok])
        assert (s2 < F(0.99)).all()
        w[alive[ok]] = w[alive[ok]] * t                            # ... then the surface
        m = n0 * ln
        assert m.dtype == F
        path[alive[ok]] = path[alive[ok]] + m
        out[0:3, alive[ok]] = hit[1:4][:, ok]
        out[3:6, alive[ok]] = dirs[:, ok]
        pend = alive[ok]  # inside this lens
        left = []
        for b in range(max_bounces + 1):
            if pend.size == 0:
                break
            r = np.ascontiguousarray(out[:, pend])
            hit = orc.intersect(patches, r, threads)
            cs, what = hit[4], hit.view(np.uint32)[11]
            s, dirs = media_ref.step(np.full(pend.size, eta_out, F), r[3:6], hit, RR_OUTSIDE)
            seg[pend] += 1
            with np.errstate(invalid="ignore"):
                s2 = (eta_out * eta_out) * (F(1) - cs * cs)
                refl = (what == INTERSECT) & (cs >= F(0)) & (s2 >= F(1)) & (b < max_bounces)
            assert s2.dtype == F
            assert (s[refl] == RR_NONE).all()  # Snell's step gave these rays up
            out[0:3, pend[refl]] = hit[1:4][:, refl]
            out[3:6, pend[refl]] = tir_ref.reflect(r[3:6][:, refl], hit[8:11][:, refl], cs[refl])
            bounces[pend[refl]] += 1
            rest = ~refl
            status[pend[rest]] = s[rest]
            ok = rest & (s != RR_NONE)
            # the leg lies in glass, for the rays that left the lens and for the rays that were reflected alike
            went = ok | refl
            ln = opl_ref.leg(r[0:3][:, went], hit[1:4][:, went])
            w[pend[went]] = w[pend[went]] * attenuation(glass_abs[l], ln)
            t, s2ok = power_ref.fresnel_t(np.full(int(ok.sum()), eta_out, F), cs[ok])
            assert (s2ok < F(0.99)).all()
            w[pend[ok]] = w[pend[ok]] * t
            out[0:3, pend[ok]] = hit[1:4][:, ok]
            out[3:6, pend[ok]] = dirs[:, ok]
            glass[pend[went]] = glass[pend[went]] + ln
            m = n1 * ln
            assert m.dtype == F
            path[pend[went]] = path[pend[went]] + m
            left.append(pend[ok])
            pend = pend[refl]
        assert pend.size == 0  # the last OUTSIDE segment reflects nothing
        alive = np.sort(np.concatenate(left)) if left else np.zeros(0, np.int64)
    assert path.dtype == F and glass.dtype == F and w.dtype == F
    return out, w, status, seg, bounces, path, glass


def chain(orc, lenses, ri_table, gap_table, glass_absorb, gap_absorb, rays, channel=None, weight=None, opl=None,
          max_bounces=4):
    """media_ref.chain with glass_absorb[l][channel[i]] and gap_absorb[l][channel[i]] for ray i; either table None: all
    zero.  A ray whose channel is not below nchan is not traced and keeps its weight."""
    table = np.asarray(ri_table, F)
    nl, nchan = len(lenses), table.shape[1]
    gaps = np.ones((nl + 1, nchan), F) if gap_table is None else np.asarray(gap_table, F)
    ga = np.zeros((nl, nchan), F) if glass_absorb is None else np.asarray(glass_absorb, F)
    pa = np.zeros((nl, nchan), F) if gap_absorb is None else np.asarray(gap_absorb, F)
    rays = np.ascontiguousarray(rays, F)
    n = rays.shape[1]
    channel = np.zeros(n, np.uint8) if channel is None else np.asarray(channel)
    assert table.ndim == 2 and table.shape[0] == nl and channel.shape == (n,)
    assert gaps.shape == (nl + 1, nchan) and ga.shape == pa.shape == (nl, nchan)
    out = rays.copy()
    w = np.ones(n, F) if weight is None else np.array(weight, F)
    path = np.zeros(n, F) if opl is None else np.array(opl, F)
    glass = np.zeros(n, F)
    status = np.zeros(n, np.uint32)
    seg = np.ones(n, np.uint32)
    bounces = np.zeros(n, np.uint32)
    for c in range(nchan):
        idx = np.nonzero(channel == c)[0]
        if idx.size == 0:
            continue
        res = chain_one(orc, lenses, list(table[:, c]), list(gaps[:, c]), list(ga[:, c]), list(pa[:, c]), rays[:, idx],
                        w[idx], path[idx], max_bounces)
        out[:, idx], w[idx], status[idx], seg[idx], bounces[idx], path[idx], glass[idx] = res
    return out, w, status, seg, bounces, path, glass


# ---------------------------------------------------------------------------------------------------- shared tables
# per channel: none, faint, strong, opaque (att returns 0 in glass: weight-0 rays are traced on) / clear in front
GLASS_ROW, GAP_ROW = [0.0, 0.05, 0.7, 200.0], [0.0, 0.02, 0.3, 0.0]
GLASS2, GAPA2 = [GLASS_ROW], [GAP_ROW]
GLASS4, GAPA4 = [GLASS_ROW, [0.01, 0.0, 150.0, 0.4]], [GAP_ROW, [0.6, 0.0, 0.05, 0.1]]
DOUBLET_GLASS, DOUBLET_GAPA = [[0.7], [0.05]], [[0.02], [0.3]]
# the illumination scenes: the emitter under an encapsulant (gap row 0), air behind the lens
ILLUM_GAPS = [[1.41, 1.333, 1.2, 1.0], [1.0, 1.0, 1.0, 1.0]]
ILLUM_GAPA = [[0.3, 0.02, 0.0, 0.1]]
ILLUM_GLASS = [[0.05, 0.7, 0.4, 200.0]]  # (every channel absorbs somewhere; channel 2 only in glass)


# ------------------------------------------------------------------------------------------ illumination reference
def illum_reference(orc, lenses, table, gaps, glass_absorb, gap_absorb, origin, max_bounces, n=itr.N_RAYS, lambert=True):
    """illum_tir_ref.reference over `chain`: what bzr_illuminate_media must return for the emitter at `origin`, with
    the same fields (illum_tir_ref.ledger_for applies to it)."""
    table = np.asarray(table, F)
    nchan = table.shape[1]
    rays, _ = orc.emit(itr.emitter(orc, origin), 0, n)
    channel = (np.arange(n) % nchan).astype(np.uint8)
    w0 = rays[3].copy() if lambert else np.ones(n, F)
    out, w, status, seg, bounces, _, _ = chain(orc, lenses, table, gaps, glass_absorb, gap_absorb, rays, channel, w0, None,
                                               max_bounces)
    assert set(np.unique(status)) <= {RR_NONE, RR_OUTSIDE}
    tg = itr.target(orc)
    shape = (nchan, tg.bins_v, tg.bins_u)
    q, q0 = power_ref.q32(w), power_ref.q32(w0)
    row = np.minimum(bounces, itr.MAX_BOUNCES)
    flux, hist = np.zeros(shape, np.uint64), np.zeros(shape, np.uint32)
    rflux, rhist = np.zeros(shape, np.uint64), np.zeros(shape, np.uint32)
    count = np.zeros((nchan, itr.ROWS, itr.FIELDS), np.uint64)
    power = np.zeros((nchan, itr.ROWS, itr.FIELDS), np.uint64)
    for c in range(nchan):
        for r in range(itr.ROWS):
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


def att_values(n=1 << 20):
    """[n] float32 >= 0 (or NaN): 0, denormals, every k boundary (k +- 1/2) / log2(e) with its float neighbours, the
    cut-off's neighbours, inf and NaN; the rest uniform in [0, 90) and log-uniform in [1e-12, 100)."""
    edge = [F(0), np.array([1, 2, 0x7FFFFF, 0x800000], np.uint32).view(F), F(np.inf), F(np.nan)]
    marks = np.concatenate([(np.arange(0, 127) + s) / np.log2(np.e) for s in (-0.5, 0.0, 0.5)])
    marks = marks[marks >= 0].astype(F)
    near = marks.copy()
    for _ in range(4):  # four floats to either side of every mark
        near = np.concatenate([near, np.nextafter(near, F(np.inf)), np.nextafter(near, F(0))])
    edge.append(np.unique(near))
    fixed = np.concatenate([np.atleast_1d(e).astype(F) for e in edge])
    rng = np.random.default_rng(1905)
    m = n - fixed.size
    assert m > n // 2
    body = np.concatenate([rng.random(m // 2) * 90.0, 10.0 ** (rng.random(m - m // 2) * 14.0 - 12.0)]).astype(F)
    x = np.concatenate([fixed, body])
    x.setflags(write=False)
    return x
