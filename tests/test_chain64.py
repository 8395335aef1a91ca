"""tests/chain64.py (bzr_trace_chain_opl in binary64) against the float32 statements of the same steps, on the CPU.

tests/test_gpu_fast_chain64.py judges BZR_MODE_FAST's chain outputs by the oracle's own error against chain64, so
chain64 has to be right and the comparison has to mean something.  Asserted here, from the reference side alone:

Steps.  Each binary64 step equals its float32 statement (tir_ref.reflect, opl_ref.leg, power_ref.fresnel_t, Snell's
direction restated from the oracle's line in numpy float32) on 2^16 random float32 operands, within a tolerance that
counts the float32 statement's roundings: (roundings on the longest path to a result) x (the largest magnitude an
intermediate reaches) x (the largest factor by which a later operation amplifies an earlier error) x 2^-24.  Operands
are restricted to 1 - s2 >= 1/2 where sqrt(1 - s2) would amplify, as tests/test_fresnel_host.py does.

    step      roundings                                                    magnitude   amplification   tolerance
    reflect   2 (normal k, d - .) + 7 (3 squares, 2 adds, sqrt, divide) = 9    3            1           27 x 2^-24
    leg       1 (e) + 1 (square) + 2 (adds) + 1 (sqrt) = 5                relative     1 (sqrt: 1/2)    5 x 2^-24
    Snell     4 (s2) + 2 (c2) + 2 (eta c1 - c2) + 3 (d eta, n ., add) + 6 (normalize: square, 2 adds, sqrt, divide,
              counted on one component's path) = 17                        eta^2       1 (c2 >= 0.7)   17 eta^2 x 2^-24
    Fresnel   4 (s2) + 2 (c2) + 1 (eta c1) + 3 (rs) + 2 (squares' sum) + 1 (1 - .) = 13 on the longer path
                                                                           eta^2       2 / c2 <= 2.83  13 x 2.83 eta^2 x 2^-24

(rs = N / D with |rs| <= 1 and D >= c2 >= 0.7: an error in eta c1 or c2 enters N and D alike, so 2 / c2.)  With
eta <= 2.4 these are 1.6e-6, 3.0e-7 relative, 5.8e-6 and 1.3e-5; a negated normal or a leg taken as t |d| is off by
1e-3 to 1 on most operands.  The whole step as the chain wires it (step64) is then run on the oracle's own float32
hits of every segment of a real chain and compared with what the oracle's refract, tir_ref.reflect, opl_ref.leg and
power_ref.fresnel_t make of the same words, with the same tolerances.

Scenes.  The populations the GPU test relies on (floors on the well-conditioned rays, on the oracle's share of them
with chain64's structure, on the bounced and on the unbounced OUTSIDE class), and which error quantiles can carry a
bar of 2: a quantile of the oracle's error must not itself differ by more than 1.5 x between random halves of its
class.  The bounced class's 99th percentiles and its weight do (1.6 to 4.8 x, printed), so they are not asserted
there; the Newton stage on bounce segments is held at the 99th percentile per segment instead.
"""
import numpy as np
import pytest

import chain64
import opl_ref
import power_ref
import ref64
import tir_ref

F = np.float32
U = 2.0 ** -24
N_OPERANDS = 1 << 16
ETA32 = np.array([F(1) / F(1.3), F(1.3), F(1) / F(1.5), F(1.5), F(1) / F(2.4), F(2.4)], F)
ETA2_MAX = float(ETA32.max()) ** 2
TOL_REFLECT = 9 * 3 * U
TOL_LEG = 5 * U                       # relative
TOL_SNELL = 17 * ETA2_MAX * U
TOL_FRESNEL = 13 * 2.83 * ETA2_MAX * U

WELL_MIN, SHARE_MIN, BOUNCED_MIN, UNBOUNCED_MIN = 18_000, 0.995, 900, 6_000
MEASURED = {"cfg2": (24_010, 23_949, 1_242, 11_143), "cfg4": (19_867, 19_804, 1_068, 7_046)}
HALVES_MAX, HALVES_SEEDS = 1.5, 20
SEGMENT_WELL_MIN, SEGMENT_SHARE_MIN = 4_000, 0.995
SEGMENTS_MEASURED = {"inside": (16_347, 8_202), "outside": (11_160, 8_461), "bounce": (7_682, 5_140)}


def unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def operands(seed):
    """(d [n, 3], normal [n, 3], cs [n], eta [n]) float32: unit vectors, cs their product rounded once, eta from the
    chain tests' indices, the side by the sign of cs as the chain has it (eta < 1 going in, > 1 going out)."""
    rng = np.random.default_rng(seed)
    d, normal = unit_vectors(rng, N_OPERANDS), unit_vectors(rng, N_OPERANDS)
    cs = (d.astype(np.float64) * normal).sum(axis=1).astype(F)
    ri = np.array([1.3, 1.5, 2.4], F)[rng.integers(0, 3, N_OPERANDS)]
    eta = np.where(cs < 0, F(1) / ri, ri).astype(F)
    return d, normal, cs, eta


def snell32(d, normal, cs, eta):
    """Snell's direction as the oracle's line states it, one rounded float32 operation per numpy call."""
    d, normal, cs, eta = (np.asarray(a, F) for a in (d, normal, cs, eta))
    s2 = (eta * eta) * (F(1) - cs * cs)
    n = normal * np.where(cs < 0, F(1), F(-1)).astype(F)[:, None]
    c1 = np.abs(cs)
    with np.errstate(invalid="ignore"):
        c2 = np.sqrt(F(1) - s2)
        v = d * eta[:, None] + n * (eta * c1 - c2)[:, None]
        sq = v * v
        z = sq[:, 0] + (sq[:, 1] + sq[:, 2])
        out = np.where((s2 > F(1e-12))[:, None], v / np.sqrt(z)[:, None], d)
    assert out.dtype == F
    return out, s2


# ------------------------------------------------------------------ steps, on random operands
def test_reflect_step():
    d, normal, cs, _ = operands(1)
    got = chain64.reflect(d.astype(np.float64), normal.astype(np.float64), cs.astype(np.float64))
    want = tir_ref.reflect(d.T, normal.T, cs).T
    err = np.abs(got - want).max()
    print(f"reflect: binary64 vs float32 on {N_OPERANDS} operands, max {err:.2e} (tolerance {TOL_REFLECT:.2e})")
    assert err <= TOL_REFLECT
    # the step is a mirror: the normal component of d changes sign, the rest stays
    n64, d64 = normal.astype(np.float64), d.astype(np.float64)
    n64 /= np.linalg.norm(n64, axis=1, keepdims=True)
    along = (got * n64).sum(axis=1) + (d64 * n64).sum(axis=1)
    assert np.abs(along).max() < 1e-6


def test_leg_step():
    rng = np.random.default_rng(2)
    s = rng.uniform(-20, 20, (N_OPERANDS, 3)).astype(F)
    p = (s + rng.normal(size=(N_OPERANDS, 3)) * rng.choice([1e-3, 0.1, 3.0, 30.0], (N_OPERANDS, 1))).astype(F)
    got = chain64.leg(s.astype(np.float64), p.astype(np.float64))
    want = opl_ref.leg(s.T, p.T)
    rel = np.abs(got - want) / got
    print(f"leg: max relative {rel.max():.2e} (tolerance {TOL_LEG:.2e})")
    assert (got > 0).all() and rel.max() <= TOL_LEG
    assert np.array_equal(want, opl_ref.leg(p.T, s.T))  # a distance: symmetric, bit for bit


def test_fresnel_step():
    _, _, cs, eta = operands(3)
    t32, s2 = power_ref.fresnel_t(eta, cs)
    keep = (F(1) - s2) >= F(0.5)
    assert keep.sum() >= N_OPERANDS // 4
    for e in ETA32:
        assert (keep & (eta == e)).sum() > 400, e
    got = chain64.fresnel_t(eta.astype(np.float64)[keep], cs.astype(np.float64)[keep])
    err = np.abs(got - t32[keep]).max()
    print(f"Fresnel T: {int(keep.sum())} operands with 1 - s2 >= 1/2, max {err:.2e} (tolerance {TOL_FRESNEL:.2e})")
    assert err <= TOL_FRESNEL
    assert (got > 0).all() and (got <= 1).all()


def test_snell_step():
    d, normal, cs, eta = operands(4)
    want, s2 = snell32(d, normal, cs, eta)
    keep = (F(1) - s2) >= F(0.5)
    assert keep.sum() >= N_OPERANDS // 4 and (keep & (cs < 0)).sum() > 5000 and (keep & (cs > 0)).sum() > 2000
    f = lambda a: a.astype(np.float64)[keep]  # noqa: E731
    got = chain64.snell(f(d), f(normal), f(cs), f(eta), cs[keep] < 0)
    err = np.abs(got - want[keep]).max()
    print(f"Snell: {int(keep.sum())} operands with 1 - s2 >= 1/2, max {err:.2e} (tolerance {TOL_SNELL:.2e})")
    assert err <= TOL_SNELL
    # Snell's law itself: the tangential part scales by eta, and the ray keeps going through the surface
    n64 = f(normal) / np.linalg.norm(f(normal), axis=1, keepdims=True)
    tang = lambda v: v - n64 * (v * n64).sum(axis=1, keepdims=True)  # noqa: E731
    assert np.abs(tang(got) - tang(f(d)) * f(eta)[:, None]).max() < 1e-5
    assert (np.sign((got * n64).sum(axis=1)) == np.sign(f(cs))).all()
    # s2 <= 1e-12: the direction is kept
    head_on = chain64.snell(f(d)[:4], f(d)[:4], np.ones(4), f(eta)[:4], np.zeros(4, bool))
    assert np.array_equal(head_on, f(d)[:4])


def test_binary64_rays_pass_unrounded(orc):
    """ref64 takes binary64 rays as they are and float32 rays through their float32 values, as before."""
    patches, ox, yz = ref64.lens_set(orc)["cfg2"]
    idx, limit, rays = ref64.aimed_triples(patches, ox, yz, 22, n=256)
    a = ref64.patch_intersect64(patches, idx, limit, rays)
    b = ref64.patch_intersect64(patches, idx, limit, rays.astype(np.float64))
    assert np.array_equal(a.t, b.t) and np.array_equal(a.point, b.point)
    moved = rays.astype(np.float64)
    moved[1] += 1e-9  # far below a float32 ulp of the origins
    assert np.array_equal(moved.astype(F), rays)
    c = ref64.patch_intersect64(patches, idx, limit, moved)
    hit = a.what == ref64.INTERSECT
    assert hit.sum() > 50 and (c.point[hit, 1] != a.point[hit, 1]).mean() > 0.9
    assert np.abs(c.point[hit] - a.point[hit]).max() < 1e-6


# ------------------------------------------------------------------ the step as the chain wires it
@pytest.fixture(scope="module")
def recorded(orc):
    return chain64.recorded(orc)


def hit_namespace(hits):
    """A float32 hit's rows [13, m] as step64 takes them, in binary64."""
    h = np.asarray(hits, F).astype(np.float64)
    return chain64.SimpleNamespace(what=np.asarray(hits, F).view(np.uint32)[11].astype(np.int64), t=h[0],
                                   cs=h[4], point=h[1:4].T, normal=h[8:11].T)


def test_chain_step_on_the_oracles_own_hits(recorded):
    """step64 over every logged segment, fed the oracle's float32 hit words: the status is the oracle's wherever s2
    keeps S2_WELL from its thresholds, the reflected rays are the ones tir_ref reflects, and the continued ray, the
    Fresnel term and the leg equal the float32 statements on the same words within the steps' tolerances."""
    rec, _ = recorded
    kinds = rec.kinds()
    seen = dict.fromkeys(chain64.KINDS, 0)
    worst = dict.fromkeys(("snell", "reflect", "fresnel", "leg", "origin"), 0.0)
    budget, b = 4, 0  # chain64.recorded's max_bounces; b counts the reflections before the segment
    for e, kind in zip(rec.log, kinds):
        b = 0 if kind in ("inside", "outside") else b + 1
        may_reflect = kind != "inside" and b < budget
        rays64 = e.rays.astype(np.float64)
        g = chain64.step64(rays64, hit_namespace(e.hits), e.expected, e.ri, may_reflect)
        cs = e.hits[4]
        what = e.hits.view(np.uint32)[11]
        clear = chain64.s2_margin(g.s2, e.expected) | ~g.decides
        seen[kind] += int(clear.sum())
        assert np.array_equal(g.status[clear], e.status[clear]), kind
        with np.errstate(invalid="ignore"):
            s2_32 = (e.ri * e.ri) * (F(1) - cs * cs)
            refl32 = (what == ref64.INTERSECT) & (cs >= F(0)) & (s2_32 >= F(1)) & may_reflect & (e.expected == chain64.RR_OUTSIDE)
        assert np.array_equal(g.refl[clear], refl32[clear]), kind
        ok = clear & (g.status != chain64.RR_NONE)
        # the refracted ray: the oracle's own
        worst["origin"] = max(worst["origin"], float(np.abs(g.rays[0:3, ok] - e.out_rays[0:3, ok]).max(initial=0)))
        eta = np.where(cs < 0, F(1) / e.ri, e.ri).astype(F)
        t32, s2f = power_ref.fresnel_t(eta, cs)
        flat = ok & ((F(1) - s2f) >= F(0.5))
        worst["snell"] = max(worst["snell"], float(np.abs(g.rays[3:6, flat] - e.out_rays[3:6, flat]).max(initial=0)))
        worst["fresnel"] = max(worst["fresnel"], float(np.abs(g.t[flat] - t32[flat]).max(initial=0)))
        r = clear & g.refl
        want = tir_ref.reflect(e.rays[3:6][:, r], e.hits[8:11][:, r], cs[r])
        worst["reflect"] = max(worst["reflect"], float(np.abs(g.rays[3:6, r] - want).max(initial=0)))
        worst["origin"] = max(worst["origin"], float(np.abs(g.rays[0:3, r] - e.hits[1:4][:, r]).max(initial=0)))
        went = ok | r
        l32 = opl_ref.leg(e.rays[0:3][:, went], e.hits[1:4][:, went])
        worst["leg"] = max(worst["leg"], float((np.abs(g.length[went] - l32) / g.length[went]).max(initial=0)))
        stay = clear & ~went
        assert np.array_equal(g.rays[:, stay], rays64[:, stay]) and not g.length[stay].any() and (g.t[stay] == 1).all()
    print("step64 on the oracle's hits:", seen, {k: f"{v:.2e}" for k, v in worst.items()})
    assert min(seen.values()) >= 5000
    assert worst["origin"] == 0.0  # the hit's point, unchanged
    assert worst["snell"] <= TOL_SNELL and worst["reflect"] <= TOL_REFLECT
    assert worst["fresnel"] <= TOL_FRESNEL and worst["leg"] <= TOL_LEG


# ------------------------------------------------------------------ scenes
@pytest.fixture(scope="module", params=["cfg2", "cfg4"])
def case(request, orc):
    return request.param, chain64.reference(orc, request.param)


def selections(c):
    sel = c.ref.well & chain64.same_structure(c.oracle, c.ref)
    return sel, chain64.classes(c.ref, sel)


def test_populations(case):
    name, c = case
    n = c.rays.shape[1]
    assert n == 192 * 192 - 37 == 36_827 and n % 64 != 0
    sel, cl = selections(c)
    counts = (int(c.ref.well.sum()), int(sel.sum()), int(cl["bounced"].sum()), int(cl["unbounced"].sum()))
    print(f"{name}: well {counts[0]}, with the oracle's structure {counts[1]} ({counts[1] / counts[0]:.4f}), of those "
          f"bounced {counts[2]}, unbounced and OUTSIDE {counts[3]}; measured when written {MEASURED[name]}")
    assert counts[0] >= WELL_MIN and counts[1] >= SHARE_MIN * counts[0]
    assert counts[2] >= BOUNCED_MIN and counts[3] >= UNBOUNCED_MIN
    # weight 1 and opl 0 going in: what chain64 returns is physical
    r = c.ref
    assert (r.weight > 0).all() and (r.weight <= 1).all() and (r.opl >= r.glass).all() and (r.glass >= 0).all()
    assert np.array_equal(r.glass > 0, (r.status == chain64.RR_OUTSIDE) | (r.bounces > 0) | (r.segments > r.bounces + 2))
    assert np.abs(np.linalg.norm(r.rays[3:6], axis=0) - 1).max() < 1e-6


def test_which_quantiles_carry_a_bar(case):
    """The oracle's error quantiles between random halves of each class, 20 seeds: the asserted ones within 1.5 x."""
    name, c = case
    _, cl = selections(c)
    for cls, sel in cl.items():
        err = chain64.chain_errors(c.oracle, c.ref, sel, c.span)
        m = int(sel.sum())
        worst = {(k, w): 1.0 for k in chain64.ERRORS for w in ("median", "p99")}
        for seed in range(HALVES_SEEDS):
            half = np.random.default_rng(seed).permutation(m) < m // 2
            qa = ref64.quantiles({k: v[half] for k, v in err.items()})
            qb = ref64.quantiles({k: v[~half] for k, v in err.items()})
            for k in chain64.ERRORS:
                for j, w in enumerate(("median", "p99")):
                    lo, hi = sorted((qa[k][j], qb[k][j]))
                    worst[k, w] = max(worst[k, w], chain64.ratio(hi, lo))
        print(f"{name} {cls} ({m} rays): largest ratio between halves: "
              + ", ".join(f"{k} {w} {v:.2f}{'' if chain64.asserted(name, cls, w, k) else ' (printed)'}"
                          for (k, w), v in worst.items()))
        for (k, w), v in worst.items():
            if chain64.asserted(name, cls, w, k):
                assert v <= HALVES_MAX, (name, cls, k, w, v)


def test_segment_populations(orc, recorded):
    """The three kinds of segment on lens 0 of cfg2 at 128^2 - 37 rays, as the float32 chain meets them."""
    rec, lens = recorded
    span = ref64.mesh_span(lens)
    assert span > 0
    for kind, (rays, hits) in rec.segments(lens).items():
        ref = ref64.intersect64(lens, rays, orc.planar_gate(lens, rays, threads=16))
        u = hits.view(np.uint32)
        well = ref.well
        same = (u[11, well] == ref64.INTERSECT) & (u[12, well] == ref.patch[well])
        print(f"{kind}: {rays.shape[1]} rays, {int(well.sum())} well, the oracle's same-hit share {same.mean():.5f}; "
              f"measured when written {SEGMENTS_MEASURED[kind]}")
        assert well.sum() >= SEGMENT_WELL_MIN and same.mean() >= SEGMENT_SHARE_MIN
        if kind == "bounce":  # origins on the surface: the hit's point of the segment before
            t = hits[0, u[11] == ref64.INTERSECT]
            assert (t > 1e-3 * span).all()  # no accepted self-hit at t ~ 0
