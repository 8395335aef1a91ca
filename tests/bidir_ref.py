"""Reference for the bidirectional-chain tests: the walk of include/bzr.h bzr_trace_chain_bidir in numpy, built from the
header's text alone.

Nothing here comes from the code under test.  The walk runs over the oracle's BezierMesh::intersect (pyoracle),
media_ref.step (Snell's step with one eta per ray), power_ref.fresnel_t, tir_ref.reflect (the mirror step),
opl_ref.leg, absorb_ref.attenuation and ghost_ref.uniform at e = 256 + q - 1.  Per ray it keeps the header's state
(g, fwd, k, q) and, while inside a lens, that lens; rays are advanced event by event, grouped by the (lens, phase) they
need next -- a ray's results depend on its own inputs alone, so the grouping is only a way to batch the oracle's calls.

`chain` returns the seven outputs and, when `log` is a dict, fills it per ray of the call:
    log["draws"][i]    the (q - 1, T, u) triples of the ray's draws, in order
    log["lenses"][i]   the lens of every segment, in order: the ray's q-th segment met log["lenses"][i][q - 1]
    log["phases"][i]   0 for an open segment, 1 for a glass segment, beside it
    log["events"][i]   'i' refracted in, 'o' refracted out, 'r' reflected, 'x' ended NONE, beside them
    log["all_back"][i] whether every surface the ray met from inside glass faced forward (a back-side exit, or the attempt
                       at one: the side rule took the gap behind the lens for eta every time)
tests/test_bidir_ref.py pins it: at budget 0 it is absorb_ref.chain bit for bit on every ray whose exits all faced
forward.
"""
import numpy as np

import ghost_ref
import media_ref
import opl_ref
import power_ref
import tir_ref
from absorb_ref import attenuation

F = np.float32
U64 = np.uint64
RR_NONE, RR_INSIDE, RR_OUTSIDE, RR_BACK = 0, 1, 2, 4
INTERSECT = 4
DRAW_OFFSET = 256
SEED, FIRST_RAY = ghost_ref.SEED, ghost_ref.FIRST_RAY
AXIS = (1.0, 0.0, 0.0)


def segment_bound(nlens, max_bounces):
    """The header's bound on out_segments."""
    return (max_bounces + 1) * (2 * nlens + 1)


def uniform(seed, jnum, seg):
    """G(seed, j, 256 + seg) per ray: jnum [m] uint64, seg [m] the segments' ordinals from 0."""
    jnum, seg = np.asarray(jnum, U64), np.asarray(seg)
    u = np.zeros(jnum.shape, F)
    for e in np.unique(seg):
        m = seg == e
        u[m] = ghost_ref.uniform(seed, jnum[m], DRAW_OFFSET + int(e))
    return u


def _att(coeff, ln):
    """The legs' factors A for one coefficient per ray (coeff [m]) and the lengths ln [m]."""
    coeff, ln = np.asarray(coeff, F), np.asarray(ln, F)
    a = np.ones(ln.shape, F)
    for v in np.unique(coeff):
        m = coeff == v
        a[m] = attenuation(v, ln[m])
    return a


def chain_one(orc, lenses, ris, gaps, glass_abs, gap_abs, rays, jnum, seed, axis, weight=None, opl=None, max_bounces=4,
              lossless=False, log=None, threads=16):
    """The walk for the rays of one channel: ris [nlens], gaps [nlens + 1], glass_abs and gap_abs [nlens]; jnum [n] the
    rays' 64-bit numbers.  log: None, or a dict of per-ray lists (see the module's text) indexed like `rays`."""
    nl = len(lenses)
    assert len(gaps) == nl + 1 == len(ris) + 1 and len(glass_abs) == len(gap_abs) == nl
    ris, gaps = np.asarray(ris, F), np.asarray(gaps, F)
    glass_abs, gap_abs = np.asarray(glass_abs, F), np.asarray(gap_abs, F)
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
    inside = np.zeros(n, bool)      # in glass, of lens `lens`
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
        seg = q[idx].copy()  # the segment's ordinal from 0: q - 1 after the increment
        q[idx] += 1
        with np.errstate(invalid="ignore"):
            if gl:
                pr = normal * a[:, None]
                back = (pr[0] + (pr[1] + pr[2])) >= F(0)
                assert pr.dtype == F
                gi = np.where(back, l + 1, l)
                eta = ris[l] / gaps[gi]
                side = cs >= F(0)
                expected, nm, coeff = RR_OUTSIDE, np.full(idx.size, ris[l], F), np.full(idx.size, glass_abs[l], F)
            else:
                back = np.zeros(idx.size, bool)
                gi = g[idx]
                assert (gi <= nl - 1).all() and (gi >= 0).all()  # the header's argument: no open leg lies behind the last lens
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
            t_d, _ = power_ref.fresnel_t(eta[drawn], cs[drawn])
            u = uniform(seed, jnum[idx[drawn]], seg[drawn])
            assert t_d.dtype == F and u.dtype == F
            ghost[drawn] = u >= t_d
            if log is not None:
                for i, e, t, uu in zip(idx[drawn], seg[drawn], t_d, u):
                    log["draws"][i].append((int(e), t, uu))
        refl = total | ghost
        ok = ~refl & (s != RR_NONE)
        lost = ~refl & (s == RR_NONE)
        went = ok | refl
        ln = opl_ref.leg(r[0:3][:, went], hit[1:4][:, went])
        w[idx[went]] = w[idx[went]] * _att(coeff[went], ln)
        paying = ok & ~drawn  # the budget is spent (or the surface lossless): no draw, the surface takes its share
        if not lossless:
            t, s2ok = power_ref.fresnel_t(eta[paying], cs[paying])
            assert (s2ok < F(0.99)).all()
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
                    log["all_back"][i] = False  # (whatever became of the ray there: eta was the front gap's)
    assert path.dtype == F and glass.dtype == F and w.dtype == F
    assert (q <= segment_bound(nl, max_bounces)).all() and (k <= max_bounces).all()
    return out, w, status, q, k, path, glass


def new_log(n):
    return dict(draws=[[] for _ in range(n)], lenses=[[] for _ in range(n)], phases=[[] for _ in range(n)],
                events=[[] for _ in range(n)], all_back=[True] * n)


def chain(orc, lenses, ri_table, gap_table, glass_absorb, gap_absorb, rays, channel=None, weight=None, opl=None,
          max_bounces=4, seed=SEED, first_ray=FIRST_RAY, axis=AXIS, lossless=False, log=None):
    """(rays, weight, status, segments, bounces, opl, glass) of bzr_trace_chain_bidir: ray i has the number first_ray + i.
    A ray whose channel is not below nchan is not traced: NONE, one segment, everything else as it came.  log: None or
    an empty dict, filled as the module's text says."""
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
                        w[idx], path[idx], max_bounces, lossless, sub)
        out[:, idx], w[idx], status[idx], seg[idx], bounces[idx], path[idx], glass[idx] = res
        if log is not None:
            for name in log:
                for j, i in enumerate(idx):
                    log[name][i] = sub[name][j]
    return out, w, status, seg, bounces, path, glass


def kinds(status, log):
    """The path kinds of tests/test_bidir_ref.py as boolean rows over the rays:
    a: ends BACK after a front-surface reflection at lens 0 (its first segment reflects);
    b: reflects at lens 1's front surface (an open segment at lens 1), re-enters lens 0 and ends BACK;
    c: the two-element ghost: reflects at lens 1 (either surface), later reflects again at or inside lens 0, and leaves
       OUTSIDE through lens 1."""
    n = len(log["lenses"])
    a, b, c = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    for i in range(n):
        ln, ph, ev = log["lenses"][i], log["phases"][i], log["events"][i]
        if not ev:
            continue
        a[i] = status[i] == RR_BACK and ev[0] == "r" and ln[0] == 0 and ph[0] == 0
        at1 = [j for j in range(len(ev)) if ev[j] == "r" and ln[j] == 1]
        if at1:
            first = at1[0]
            front = [j for j in at1 if ph[j] == 0]
            if status[i] == RR_BACK and front:
                b[i] = any(ev[j] == "i" and ln[j] == 0 for j in range(front[0] + 1, len(ev)))
            if status[i] == RR_OUTSIDE:
                again = [j for j in range(first + 1, len(ev)) if ev[j] == "r" and ln[j] == 0]
                c[i] = bool(again) and ev[-1] == "o" and ln[-1] == 1
    return a, b, c


# ------------------------------------------------------------------------------------------ illumination reference
def illum_reference(orc, lenses, table, gaps, glass_absorb, gap_absorb, origin, max_bounces, n=None, lambert=True,
                    seed=SEED, axis=AXIS, lossless=False, log=None):
    """ghost_ref.illum_reference over `chain`: what bzr_illuminate_bidir must return near the target for the emitter at
    `origin` (emitter ray j draws with ray number j); the same fields, and back_count / back_power [nchan, ROWS]: the
    BACK rays by min(bounces, 8) and their q(w).  A BACK ray is in no other field and lands nowhere."""
    from types import SimpleNamespace

    import illum_tir_ref as itr
    n = itr.N_RAYS if n is None else n
    table = np.asarray(table, F)
    nchan = table.shape[1]
    rays, _ = orc.emit(itr.emitter(orc, origin), 0, n)
    channel = (np.arange(n) % nchan).astype(np.uint8)
    w0 = rays[3].copy() if lambert else np.ones(n, F)
    out, w, status, seg, bounces, _, _ = chain(orc, lenses, table, gaps, glass_absorb, gap_absorb, rays, channel, w0, None,
                                               max_bounces, seed, 0, axis, lossless, log)
    assert set(np.unique(status)) <= {RR_NONE, RR_OUTSIDE, RR_BACK}
    tg = itr.target(orc)
    shape = (nchan, tg.bins_v, tg.bins_u)
    q, q0 = power_ref.q32(w), power_ref.q32(w0)
    row = np.minimum(bounces, itr.MAX_BOUNCES)
    flux, hist = np.zeros(shape, np.uint64), np.zeros(shape, np.uint32)
    rflux, rhist = np.zeros(shape, np.uint64), np.zeros(shape, np.uint32)
    count = np.zeros((nchan, itr.ROWS, itr.FIELDS), np.uint64)
    power = np.zeros((nchan, itr.ROWS, itr.FIELDS), np.uint64)
    back_count, back_power = np.zeros((nchan, itr.ROWS), np.uint64), np.zeros((nchan, itr.ROWS), np.uint64)
    for c in range(nchan):
        for r in range(itr.ROWS):
            mine = (channel == c) & (row == r)
            if not mine.any():
                continue
            st = np.where(mine & (status == RR_OUTSIDE), RR_OUTSIDE, RR_NONE).astype(np.uint32)  # only OUTSIDE rays land
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
            back_count[c, r] = int((mine & (status == RR_BACK)).sum())
            back_power[c, r] = int(q[mine & (status == RR_BACK)].sum())
    emitted = [int((channel == c).sum()) for c in range(nchan)]
    emitted_q = [int(q0[channel == c].sum()) for c in range(nchan)]
    for a in (rays, channel, w0, out, w, status, seg, bounces, flux, hist, rflux, rhist, count, power, back_count, back_power):
        a.setflags(write=False)
    return SimpleNamespace(nchan=nchan, rays=rays, channel=channel, w0=w0, out=out, w=w, status=status, seg=seg,
                           bounces=bounces, flux=flux, hist=hist, rflux=rflux, rhist=rhist, uncut_count=count,
                           uncut_power=power, emitted=emitted, emitted_q=emitted_q, back_count=back_count,
                           back_power=back_power)
