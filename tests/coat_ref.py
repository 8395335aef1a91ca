"""Reference for the coated-chain tests: the walk of include/bzr.h bzr_trace_chain_bidir with the coating of
bzr_coating, in numpy float32 / uint64, built from the header's text alone.

Nothing here comes from the code under test.  `chain_one` is bidir_ref.chain_one's structure over the oracle's
BezierMesh::intersect with two differences, both the header's: the side rule `back` is evaluated in open segments as
well, and T is chosen per ray between power_ref.fresnel_t and `coat_t`, the header's lookup restated in numpy.  The
older references' pieces (media_ref.step, tir_ref.reflect, opl_ref.leg, absorb_ref.attenuation, bidir_ref.uniform) are
imported, not edited.

A coating is (table, mask): table [2 nlens, nchan, 129] float32, mask bit 2 l + side.  `chain` returns the seven outputs
and, when `log` is a dict, fills bidir_ref's per-ray lists; log["draws"][i] holds one tuple per draw of ray i:
    (segment q - 1, surface 2 l + side, coated?, T, u, glass segment?)

`reflectance64` is the binary64 restatement of the characteristic-matrix formula for the host helper's test, written
with numpy's complex128 and 2 x 2 matrix products from the gap side, another operation order than the library's.
"""
import numpy as np

import bidir_ref
import ghost_ref
import media_ref
import opl_ref
import power_ref
import tir_ref
from bidir_ref import AXIS, FIRST_RAY, INTERSECT, RR_BACK, RR_INSIDE, RR_NONE, RR_OUTSIDE, SEED, _att, new_log, uniform

F = np.float32
U64 = np.uint64
SAMPLES = 129


def coat_t(rows, mu):
    """The header's lookup: rows [m, 129] (or [129]) float32, mu [m] float32 -> T [m], every operation in binary32."""
    rows, mu = np.asarray(rows, F), np.atleast_1d(np.asarray(mu, F))
    if rows.ndim == 1:
        rows = np.broadcast_to(rows, (mu.size, SAMPLES))
    assert rows.shape == (mu.size, SAMPLES)
    mu = np.minimum(mu, F(1))
    x = mu * F(128)
    i = np.minimum(x.astype(np.int32), 127)
    f = x - i.astype(F)
    k = np.arange(mu.size)
    r0, r1 = rows[k, i], rows[k, i + 1]
    d = r1 - r0
    p = f * d
    r = r0 + p
    t = F(1) - r
    assert t.dtype == F and f.dtype == F
    return t


def surface_t(eta, cs, s2, gl, sf, rows, mask):
    """T per ray of one segment: coat_t on the surfaces the mask names, power_ref.fresnel_t on the others.
    gl: a glass segment; sf [m] the surfaces; rows [2 nlens, 129] this channel's rows (None with mask 0)."""
    m = eta.size
    t = np.ones(m, F)
    coated = ((mask >> sf) & 1).astype(bool)
    if (~coated).any():
        t[~coated], _ = power_ref.fresnel_t(eta[~coated], cs[~coated])
    if coated.any():
        mu = np.sqrt(F(1) - s2[coated]) if gl else np.abs(cs[coated])
        assert mu.dtype == F
        t[coated] = coat_t(rows[sf[coated]], mu)
    return t, coated


def chain_one(orc, lenses, ris, gaps, glass_abs, gap_abs, rays, jnum, seed, axis, rows, mask, weight=None, opl=None,
              max_bounces=4, lossless=False, log=None, threads=16):
    """bidir_ref.chain_one with the coating: rows [2 nlens, 129] this channel's rows (or None), mask the coated
    surfaces."""
    nl = len(lenses)
    assert len(gaps) == nl + 1 == len(ris) + 1 and len(glass_abs) == len(gap_abs) == nl
    assert 0 <= mask < (1 << (2 * nl)) and (mask == 0 or rows is not None)
    ris, gaps = np.asarray(ris, F), np.asarray(gaps, F)
    glass_abs, gap_abs = np.asarray(glass_abs, F), np.asarray(gap_abs, F)
    rows = None if rows is None else np.asarray(rows, F)
    a = np.asarray(axis, F)
    assert a.shape == (3,) and np.isfinite(a).all() and (a != 0).any()
    rays = np.ascontiguousarray(rays, F)
    n = rays.shape[1]
    jnum = np.asarray(jnum, U64)
    assert jnum.shape == (n,) and nl <= 8 and max_bounces <= 8
    out = rays.copy()
    w = np.ones(n, F) if weight is None else np.array(weight, F)
    path = np.zeros(n, F) if opl is None else np.array(opl, F)
    glass = np.zeros(n, F)
    status = np.zeros(n, np.uint32)
    q = np.zeros(n, np.uint32)
    k = np.zeros(n, np.uint32)
    g = np.zeros(n, np.int64)
    fwd = np.ones(n, bool)
    inside = np.zeros(n, bool)
    lens = np.zeros(n, np.int64)
    live = np.ones(n, bool)
    while True:
        opn = live & ~inside
        end = opn & fwd & (g == nl)
        status[end] = RR_OUTSIDE
        live[end] = False
        end = opn & ~fwd & (g == 0)
        status[end] = RR_BACK
        live[end] = False
        if not live.any():
            break
        heading = np.where(inside, lens, np.where(fwd, g, g - 1))
        key = np.where(live, 2 * heading + inside, 1 << 30)
        kmin = int(key.min())
        idx = np.nonzero(key == kmin)[0]
        l, gl = kmin >> 1, bool(kmin & 1)
        r = np.ascontiguousarray(out[:, idx])
        hit = orc.intersect(lenses[l], r, threads)
        cs, what, normal = hit[4], hit.view(np.uint32)[11], hit[8:11]
        seg = q[idx].copy()
        q[idx] += 1
        with np.errstate(invalid="ignore"):
            pr = normal * a[:, None]
            back = (pr[0] + (pr[1] + pr[2])) >= F(0)  # the side rule, in open segments too
            assert pr.dtype == F
            sf = 2 * l + back.astype(np.int64)
            if gl:
                gi = np.where(back, l + 1, l)
                eta = ris[l] / gaps[gi]
                side = cs >= F(0)
                expected, nm, coeff = RR_OUTSIDE, np.full(idx.size, ris[l], F), np.full(idx.size, glass_abs[l], F)
            else:
                gi = g[idx]
                assert (gi <= nl - 1).all() and (gi >= 0).all()
                eta = gaps[gi] / ris[l]
                side = cs < F(0)
                expected, nm, coeff = RR_INSIDE, gaps[gi], gap_abs[gi]
            assert eta.dtype == F
            s, dirs = media_ref.step(eta, r[3:6], hit, expected)
            s2 = (eta * eta) * (F(1) - cs * cs)
            assert s2.dtype == F
            may = (what == INTERSECT) & side & (k[idx] < max_bounces)
            total = may & (s2 >= F(1))
            drawn = may & (s2 < F(0.99)) & (not lossless)
        assert (s[total] == RR_NONE).all() and (s[drawn] == expected).all()
        ghost = np.zeros(idx.size, bool)
        if drawn.any():
            t_d, coated = surface_t(eta[drawn], cs[drawn], s2[drawn], gl, sf[drawn], rows, mask)
            u = uniform(seed, jnum[idx[drawn]], seg[drawn])
            assert t_d.dtype == F and u.dtype == F
            ghost[drawn] = u >= t_d
            if log is not None:
                for i, e, f, c, t, uu in zip(idx[drawn], seg[drawn], sf[drawn], coated, t_d, u):
                    log["draws"][i].append((int(e), int(f), bool(c), t, uu, gl))
        refl = total | ghost
        ok = ~refl & (s != RR_NONE)
        lost = ~refl & (s == RR_NONE)
        went = ok | refl
        ln = opl_ref.leg(r[0:3][:, went], hit[1:4][:, went])
        w[idx[went]] = w[idx[went]] * _att(coeff[went], ln)
        paying = ok & ~drawn  # the budget is spent: no draw, the surface takes its share
        if not lossless and paying.any():
            assert (s2[paying] < F(0.99)).all()
            t, _ = surface_t(eta[paying], cs[paying], s2[paying], gl, sf[paying], rows, mask)
            w[idx[paying]] = w[idx[paying]] * t
        m = nm[went] * ln
        assert m.dtype == F
        path[idx[went]] = path[idx[went]] + m
        if gl:
            glass[idx[went]] = glass[idx[went]] + ln
        out[0:3, idx[went]] = hit[1:4][:, went]
        out[3:6, idx[refl]] = tir_ref.reflect(r[3:6][:, refl], normal[:, refl], cs[refl])
        out[3:6, idx[ok]] = dirs[:, ok]
        k[idx[refl]] += 1
        status[idx[lost]] = RR_NONE
        live[idx[lost]] = False
        if gl:
            g[idx[ok]] = gi[ok]
            fwd[idx[ok]] = back[ok]
            inside[idx[ok]] = False
        else:
            fwd[idx[refl]] = ~fwd[idx[refl]]
            inside[idx[ok]] = True
            lens[idx[ok]] = l
        if log is not None:
            for j, i in enumerate(idx):
                log["lenses"][i].append(l)
                log["phases"][i].append(int(gl))
                log["events"][i].append("r" if refl[j] else "x" if lost[j] else "o" if gl else "i")
                if gl and what[j] == INTERSECT and cs[j] >= F(0) and not back[j]:
                    log["all_back"][i] = False
    assert path.dtype == F and glass.dtype == F and w.dtype == F
    assert (q <= bidir_ref.segment_bound(nl, max_bounces)).all() and (k <= max_bounces).all()
    return out, w, status, q, k, path, glass


def chain(orc, lenses, ri_table, gap_table, glass_absorb, gap_absorb, rays, channel=None, weight=None, opl=None,
          max_bounces=4, seed=SEED, first_ray=FIRST_RAY, axis=AXIS, coat=None, lossless=False, log=None):
    """(rays, weight, status, segments, bounces, opl, glass) of bzr_trace_chain_coated; coat: None or (table, mask).
    A ray whose channel is not below nchan is not traced: NONE, one segment, everything else as it came."""
    table = np.asarray(ri_table, F)
    nl, nchan = len(lenses), table.shape[1]
    gaps = np.ones((nl + 1, nchan), F) if gap_table is None else np.asarray(gap_table, F)
    ga = np.zeros((nl, nchan), F) if glass_absorb is None else np.asarray(glass_absorb, F)
    pa = np.zeros((nl, nchan), F) if gap_absorb is None else np.asarray(gap_absorb, F)
    ctab, mask = (None, 0) if coat is None else coat
    if lossless:
        mask = 0  # the header: a lossless call ignores the coating
    if mask:
        ctab = np.asarray(ctab, F)
        assert ctab.shape == (2 * nl, nchan, SAMPLES)
    rays = np.ascontiguousarray(rays, F)
    n = rays.shape[1]
    channel = np.zeros(n, np.uint8) if channel is None else np.asarray(channel)
    assert table.ndim == 2 and table.shape[0] == nl and channel.shape == (n,)
    jnum = ghost_ref.ray_numbers(first_ray, n)
    out = rays.copy()
    w = np.ones(n, F) if weight is None else np.array(weight, F)
    path = np.zeros(n, F) if opl is None else np.array(opl, F)
    glass = np.zeros(n, F)
    status = np.zeros(n, np.uint32)
    seg = np.ones(n, np.uint32)
    bounces = np.zeros(n, np.uint32)
    if log is not None:
        log.update(new_log(n))
    for c in range(nchan):
        idx = np.nonzero(channel == c)[0]
        if idx.size == 0:
            continue
        sub = new_log(idx.size) if log is not None else None
        res = chain_one(orc, lenses, table[:, c], gaps[:, c], ga[:, c], pa[:, c], rays[:, idx], jnum[idx], seed, axis,
                        ctab[:, c] if mask else None, mask, w[idx], path[idx], max_bounces, lossless, sub)
        out[:, idx], w[idx], status[idx], seg[idx], bounces[idx], path[idx], glass[idx] = res
        if log is not None:
            for name in log:
                for j, i in enumerate(idx):
                    log[name][i] = sub[name][j]
    return out, w, status, seg, bounces, path, glass


def draw_stats(log, coated_only=True):
    """Over the log's (coated) draws: their number, the reflections among them, sum of 1 - T and of T (1 - T) in
    binary64."""
    t = np.array([d[3] for ds in log["draws"] for d in ds if d[2] or not coated_only], np.float64)
    u = np.array([d[4] for ds in log["draws"] for d in ds if d[2] or not coated_only], np.float64)
    return t.size, int((u >= t).sum()), float((1.0 - t).sum()), float((t * (1.0 - t)).sum())


def draw_kinds(log, nlens, mask):
    """The three counts tests/test_coat_ref.py establishes: draws at a coated surface from an open segment, draws at a
    coated surface from a glass segment, draws at an uncoated surface from a glass segment of a lens that also has a
    coated face."""
    lens_coated = [bool((mask >> (2 * l)) & 3) for l in range(nlens)]
    a = b = c = 0
    for ds in log["draws"]:
        for _, sf, coated, _, _, gl in ds:
            a += coated and not gl
            b += coated and gl
            c += (not coated) and gl and lens_coated[sf >> 1]
    return int(a), int(b), int(c)


# --------------------------------------------------------------------------------- the characteristic-matrix restatement
def reflectance64(n_gap, n_glass, layer_index=(), layer_thickness_um=(), wavelength_um=0.55):
    """The unpolarised reflectance (R_s + R_p) / 2 of a lossless stack at mu_i = i / 128 in binary64 -> [129] float64;
    entry 0 is 1 by definition.  M = M_1 M_2 ... M_k as 2 x 2 complex matrices from the gap side, (B, C) = M (1, y_glass),
    Y = C / B, r = (y_gap - Y) / (y_gap + Y)."""
    out = np.ones(SAMPLES, np.float64)
    for i in range(1, SAMPLES):
        mu = i / 128.0
        sin2 = 1.0 - mu * mu

        def cosine(nj):
            return np.sqrt(complex(1.0 - (n_gap / nj) ** 2 * sin2))  # the root with a non-negative imaginary part

        cg = cosine(n_glass)
        if cg.real == 0.0:  # the glass is at or beyond its critical angle
            out[i] = 1.0
            continue
        total = 0.0
        for pol in ("s", "p"):
            def adm(nj, cj):
                return nj * cj if pol == "s" else nj / cj

            m = np.eye(2, dtype=np.complex128)
            for nj, tj in zip(layer_index, layer_thickness_um):
                cj = cosine(nj)
                delta = 2.0 * np.pi * nj * tj * cj / wavelength_um
                y = adm(nj, cj)
                m = m @ np.array([[np.cos(delta), -1j * np.sin(delta) / y], [-1j * y * np.sin(delta), np.cos(delta)]])
            bc = m @ np.array([1.0, adm(n_glass, cg)], np.complex128)
            big_y = bc[1] / bc[0]
            y0 = adm(n_gap, complex(mu))
            r = (y0 - big_y) / (y0 + big_y)
            total += abs(r) ** 2
        out[i] = min(0.5 * total, 1.0)
    return out


# ------------------------------------------------------------------------------------------------- the tests' coatings
MGF2_INDEX, MGF2_DESIGN_UM = 1.38, 0.55
WAVELENGTHS_UM = (0.45, 0.50, 0.55, 0.65)  # the four channels' wavelengths (the doublet's one channel: 0.55)


def mgf2_rows(bzr, s):
    """Quarter-wave MgF2 rows (1.38, a quarter wave at 0.55 um) for every surface and channel of ghost_ref.scene `s`,
    built by the library's host helper: [2 nlens, nchan, 129] float32.  Surface (l, side) lies between gap l + side and
    lens l's glass."""
    table, gaps = np.asarray(s["table"], np.float64), np.asarray(s["gaps"], np.float64)
    nl, nchan = table.shape
    lam = WAVELENGTHS_UM if nchan == 4 else (0.55,)
    rows = np.zeros((2 * nl, nchan, SAMPLES), F)
    for l in range(nl):
        for side in (0, 1):
            for c in range(nchan):
                rows[2 * l + side, c] = bzr.coating_reflectance(gaps[l + side, c], table[l, c], [MGF2_INDEX],
                                                                [MGF2_DESIGN_UM / (4 * MGF2_INDEX)], lam[c])
    rows.setflags(write=False)
    return rows


def mixed(bzr, s):
    """The "mixed" coating: the front of lens 0 and the back of the last lens carry the MgF2 rows, the rest is bare."""
    nl = len(s["lenses"])
    return mgf2_rows(bzr, s), 1 | (1 << (2 * nl - 1))


def all_coated(bzr, s, mirror=None):
    """Every surface coated with the MgF2 rows; `mirror`: one surface number whose rows are all ones."""
    nl = len(s["lenses"])
    rows = mgf2_rows(bzr, s).copy()
    if mirror is not None:
        rows[mirror] = F(1)
    rows.setflags(write=False)
    return rows, (1 << (2 * nl)) - 1


# ------------------------------------------------------------------------------------------ illumination reference
def illum_reference(orc, lenses, table, gaps, glass_absorb, gap_absorb, origin, max_bounces, coat, n=None, lambert=True,
                    seed=SEED, axis=AXIS, lossless=False, log=None):
    """bidir_ref.illum_reference over this module's `chain`: what bzr_illuminate_coated must return."""
    saved = bidir_ref.chain

    def coated_chain(*args, **kw):
        # bidir_ref.illum_reference's call: the fourteen arguments up to axis, then lossless and log, all positional
        assert len(args) == 16 and not kw and isinstance(args[14], bool) and np.shape(args[13]) == (3,), len(args)
        return chain(*args[:14], coat, *args[14:])

    bidir_ref.chain = coated_chain  # (bidir_ref.illum_reference calls its module's `chain` positionally)
    try:
        return bidir_ref.illum_reference(orc, lenses, table, gaps, glass_absorb, gap_absorb, origin, max_bounces, n,
                                         lambert, seed, axis, lossless, log)
    finally:
        bidir_ref.chain = saved
