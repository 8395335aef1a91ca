"""Reference for the surrounding-media tests: the oracle's BezierMesh::intersect per segment, Snell's step restated in
numpy float32 with one eta per ray, tir_ref's reflecting step, power_ref's Fresnel term and opl_ref's leg.

Nothing here comes from the code under test.  The chain has opl_ref.chain_one's shape, run once per channel like
opl_ref.chain.  Lens l of channel c lies between the media n0 = gap[l][c] and n2 = gap[l + 1][c] and has n1 = ri[l][c]
(include/bzr.h bzr_trace_chain_media):

    refract(INSIDE):   eta = n0 / n1     m = n0 len;  opl = opl + m
    refract(OUTSIDE):  eta = n1 / n2     glass = glass + len;  m = n1 len;  opl = opl + m     (bounce segments included)
    reflection test of an OUTSIDE segment:  s2 = eta eta (1 - cs cs) >= 1 with that eta

The oracle's BezierLens::refract takes one index and derives eta from the side it finds (1 / ri or ri), so it cannot
be handed n0 / n1; `step` is orc_lens_refract's body after the intersection, statement for statement, on the hit rows
of the oracle's BezierMesh::intersect, in np.float32 -- IEEE binary32, one correctly rounded operation per numpy call,
its order -- with the normalisation written as in tir_ref.reflect.  tests/test_media_ref.py pins it: with every gap 1
the chain is opl_ref.chain's bit for bit (where the oracle's own refract decides every refraction), and with a
uniform eta it is the oracle's refract(OUTSIDE) with ri = eta.
"""
import numpy as np

import opl_ref
import power_ref
import tir_ref

F = np.float32
RR_NONE, RR_INSIDE, RR_OUTSIDE = 0, 1, 2
INTERSECT = 4


def step(eta, d, hit, expected):
    """Snell's step after the intersection: eta [m] float32, d [3, m] the rays' directions, hit [13, m] the oracle's
    intersect rows, expected INSIDE or OUTSIDE -> (status [m], direction [3, m]).  Where the status is not NONE the
    refracted ray starts at the hit's point (rows 1-3)."""
    eta, d = np.asarray(eta, F), np.asarray(d, F)
    cs, normal, what = hit[4], hit[8:11], hit.view(np.uint32)[11]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        side = np.where(cs < F(0), RR_INSIDE, RR_OUTSIDE)
        s2 = (eta * eta) * (F(1) - cs * cs)
        sgn = np.where(side == RR_INSIDE, F(1), F(-1)).astype(F)
        nn = normal * sgn
        c1 = np.abs(cs)
        c2 = np.sqrt(F(1) - s2)
        k = eta * c1 - c2
        v = d * eta + nn * k
        sq = v * v
        z = sq[0] + (sq[1] + sq[2])
        unit = np.where(z > F(0), v / np.sqrt(z), v)
        status = np.where((what == INTERSECT) & (s2 < F(0.99)) & (side == expected), side, RR_NONE).astype(np.uint32)
        out = np.where(s2 > F(1e-12), unit, d)
    assert s2.dtype == F and k.dtype == F and out.dtype == F
    return status, out


def chain_one(orc, lenses, ris, gaps, rays, weight=None, opl=None, max_bounces=4, threads=16):
    """(rays [6, n], weight [n], status [n], segments [n], bounces [n], opl [n], glass [n]) of the chain with one index
    per lens (ris [nlens]) and one per gap (gaps [nlens + 1])."""
    assert len(gaps) == len(lenses) + 1 == len(ris) + 1
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
        s, dirs = step(np.full(alive.size, eta_in, F), r[3:6], hit, RR_INSIDE)
        seg[alive] += 1
        status[alive] = s
        ok = s != RR_NONE
        t, s2 = power_ref.fresnel_t(np.full(int(ok.sum()), eta_in, F), hit[4][ok])
        assert (s2 < F(0.99)).all()
        w[alive[ok]] = w[alive[ok]] * t
        m = n0 * opl_ref.leg(r[0:3][:, ok], hit[1:4][:, ok])
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
            s, dirs = step(np.full(pend.size, eta_out, F), r[3:6], hit, RR_OUTSIDE)
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
            t, s2ok = power_ref.fresnel_t(np.full(int(ok.sum()), eta_out, F), cs[ok])
            assert (s2ok < F(0.99)).all()
            w[pend[ok]] = w[pend[ok]] * t
            out[0:3, pend[ok]] = hit[1:4][:, ok]
            out[3:6, pend[ok]] = dirs[:, ok]
            # the leg lies in glass, for the rays that left the lens and for the rays that were reflected alike
            went = ok | refl
            ln = opl_ref.leg(r[0:3][:, went], hit[1:4][:, went])
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


def chain(orc, lenses, ri_table, gap_table, rays, channel=None, weight=None, opl=None, max_bounces=4):
    """(rays, weight, status, segments, bounces, opl, glass) with ri_table[l][channel[i]] and gap_table[l][channel[i]] for
    ray i; channel None: channel 0; gap_table None: every entry 1.  A ray whose channel is not below nchan is not
    traced: NONE, one segment, no bounce, ray, weight and opl as they were, glass 0."""
    table = np.asarray(ri_table, F)
    gaps = np.ones((len(lenses) + 1, table.shape[1]), F) if gap_table is None else np.asarray(gap_table, F)
    rays = np.ascontiguousarray(rays, F)
    n = rays.shape[1]
    channel = np.zeros(n, np.uint8) if channel is None else np.asarray(channel)
    assert table.ndim == 2 and table.shape[0] == len(lenses) and channel.shape == (n,)
    assert gaps.shape == (len(lenses) + 1, table.shape[1])
    out = rays.copy()
    w = np.ones(n, F) if weight is None else np.array(weight, F)
    path = np.zeros(n, F) if opl is None else np.array(opl, F)
    glass = np.zeros(n, F)
    status = np.zeros(n, np.uint32)
    seg = np.ones(n, np.uint32)
    bounces = np.zeros(n, np.uint32)
    for c in range(table.shape[1]):
        idx = np.nonzero(channel == c)[0]
        if idx.size == 0:
            continue
        res = chain_one(orc, lenses, list(table[:, c]), list(gaps[:, c]), rays[:, idx], w[idx], path[idx], max_bounces)
        out[:, idx], w[idx], status[idx], seg[idx], bounces[idx], path[idx], glass[idx] = res
    return out, w, status, seg, bounces, path, glass


# ---------------------------------------------------------------------------------------------------- shared scenes
ROW1 = [1.3, 1.5, 1.8, 2.4]         # test_gpu_tir.py's cfg2 row
ROW2 = [1.5, 1.5168, 1.53, 1.62]    # and cfg4's second lens
GAPS2 = [[1.0, 1.333, 1.41, 1.0], [1.0, 1.333, 1.0, 1.56]]                       # cfg2: in front, behind
GAPS4 = [[1.0, 1.333, 1.0, 1.0], [1.56, 1.56, 1.56, 1.56], [1.0, 1.0, 1.333, 1.0]]  # cfg4: the middle row is cement
GAPS_FRONT = [[1.333, 1.41, 1.2, 1.56], [1.0, 1.0, 1.0, 1.0]]                     # cfg2 immersed in front, air behind
DOUBLET_RI = [[1.5168], [1.62]]     # two (1, 4, 2) ellipsoids, apexes 0.01 apart
DOUBLET_CEMENT = [[1.0], [1.56], [1.0]]
DOUBLET_AIR = [[1.0], [1.0], [1.0]]


def doublet_lenses(builder_cls):
    """The doublet's two lens meshes: cfg2's ellipsoid at x = 10 and the same at x = 12.01."""
    from bzr_amd.configs import CONFIGS, Lens, build_lens
    first = CONFIGS["cfg2"].lenses[0]
    second = Lens("ellipsoid", first.sectors, first.belts, first.size, (12.01, 0.0, 0.0))
    return [build_lens(builder_cls, first).bezier_patches(), build_lens(builder_cls, second).bezier_patches()]
