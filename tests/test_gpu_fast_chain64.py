"""BZR_MODE_FAST's chain outputs -- exit ray, weight, optical path, glass path, with reflections -- judged against a
binary64 chain (tests/chain64.py), the way tests/test_gpu_fast_ref64.py judges the Newton stage.

Snell's step, the Fresnel term, the reflecting step and the per-leg step are exact binary32 in both modes, so the only
difference between FAST and the float32 oracle that reaches the chain's outputs is the Newton stage's hit, and to
first order both propagate their hit's error through the same smooth map.  FAST and the oracle (opl_ref.chain) are
therefore measured against chain64 on the same well-conditioned rays, and FAST may have BAR = 2 x the oracle's error
and CLASS_ALLOW = 0.005 less of its class agreement (both imported from test_gpu_fast_ref64.py).

(a) The Newton stage on the rays chain segments really see: the float32 rays of every refract(INSIDE), first
    refract(OUTSIDE) and after-a-reflection segment on lens 0 of cfg2 (128^2 - 37 rays in, four channels, four
    reflections allowed), recorded from the oracle's chain.  Parity equals the oracle's logged hits bit for bit; FAST
    gets test_gpu_fast_ref64.py's checks against ref64.intersect64: the same-hit share, and the median and the 99th
    percentile of t, point, barycentric and normal.  The third kind is the new ground: origins on the surface the
    ray must not hit again, inside the glass, at oblique incidence.
(b) trace_chain_opl in FAST end to end on cfg2 and cfg4 at 192^2 - 37 rays, weight 1 and opl 0 going in.  On the
    `well` rays FAST's share with chain64's status, segments and bounces is at least the oracle's - CLASS_ALLOW; on
    those where both have it, FAST's quantile of an error is at most BAR x the oracle's for
        unbounced and OUTSIDE, both scenes:  the median of direction, origin, weight, opl, glass
        unbounced and OUTSIDE, cfg2:         the 99th percentile of direction, origin, opl, glass
        bounced (any end), both scenes:      the median of direction, origin, opl, glass
    The bounced class is held at the median only, and its weight not at all: the oracle's own error in a reflected
    ray is heavy-tailed (each reflection multiplies the direction error by the surface's curvature times the leg),
    so between two random halves of the class its 99th percentiles differ by up to 4.8 x and its median weight error
    by 1.6 x, and no bar of 2 can sit on that (tests/test_chain64.py asserts the listed quantiles stable within
    1.5 x).  The tails of the bounce segments are what (a) holds at the 99th percentile, per segment.  Every other
    quantile is printed as FAST / oracle.
(c) The per-leg step is exact in FAST: a ray that comes back NONE after two segments of a budget-0 chain stands on
    its first hit's point and nothing else was added, so out_opl = opl_in + leg(input origin, output origin) in
    numpy float32 bit for bit and out_glass = 0.  A contracted or approximated leg fails here.

Measured on an MI355X (fused and staged give the same figures unless two are shown):
  (a) FAST / oracle (median, p99) and same-hit share oracle / FAST on the `well` rays
      inside   8 202 well of 16 347: t 0.68 0.70, point 0.71 0.66, bary 0.74 0.58, normal 0.86 0.57; 0.99988 / 0.99927
      outside  8 461 well of 11 160: t 0.68 0.62, point 0.69 0.71, bary 0.68 0.59, normal 0.87 0.76; 1.00000 / 1.00000
      bounce   5 140 well of  7 682: t 0.70 0.67, point 0.71 0.58, bary 0.72 0.66, normal 0.87 0.59; 0.99981 / 0.99981
  (b) share of the `well` rays with chain64's structure, oracle / FAST: cfg2 0.99746 / 0.99796 of 24 010, cfg4
      0.99683 / 0.99738 of 19 867.  FAST / oracle (median, p99; * = asserted):
      cfg2 unbounced 11 143: direction 0.87* 0.94*, origin 0.80* 0.73*, weight 0.87* 0.93, opl 0.74* 0.75*, glass 0.71* 0.74*
      cfg2 bounced    1 234: direction 0.80* 1.03, origin 0.80* 0.74, weight 0.66 1.38, opl 0.75* 0.98, glass 0.75* 1.13
      cfg4 unbounced  7 046: direction 0.88* 0.85, origin 0.87* 0.85, weight 0.87* 0.95, opl 0.77* 0.76, glass 0.70* 0.84
      cfg4 bounced    1 059: direction 0.77* 1.09, origin 0.81* 0.72, weight 0.72 1.79, opl 0.73* 0.77, glass 0.80* 1.17
      (the oracle's own errors, median / p99: unbounced direction 8.8e-6 / 1.1e-4, opl 1.2e-6 / 1.1e-5; bounced
      direction 1.0e-4 / 1.5e-2, opl 4.5e-6 / 7.9e-4 on cfg2)
  (c) 2 816 of 16 347 rays come back NONE after two segments on either pipeline; every one bit-exact.
  FAST with contraction is closer to the truth than the oracle in every asserted quantile.
"""
import numpy as np
import pytest

import chain64
import opl_ref
import ref64
from test_gpu_fast_ref64 import BAR, CLASS_ALLOW, PIPES, assert_bars, pipe_of
from test_gpu_power import bits

pytestmark = pytest.mark.gpu

F = np.float32
BOUNCED_MIN, UNBOUNCED_MIN = 900, 6_000   # tests/test_chain64.py's floors
LEG_RAYS_MIN = 2_000


# ------------------------------------------------------------------ (a) the Newton stage per segment kind
@pytest.fixture(scope="module")
def segments(orc):
    """kind -> (float32 rays, the oracle's logged hits, gate matrix, intersect64's namespace), and lens 0."""
    rec, lens = chain64.recorded(orc)
    out = {}
    for kind, (rays, hits) in rec.segments(lens).items():
        gate = orc.planar_gate(lens, rays, threads=16)
        out[kind] = (rays, hits, gate, ref64.intersect64(lens, rays, gate))
        for a in (rays, hits, gate):
            a.setflags(write=False)
    return out, lens


@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("kind", chain64.KINDS)
def test_newton_stage_on_chain_segments(bzr, ctx, segments, kind, pipe):
    by_kind, lens = segments
    rays, want, gate, ref = by_kind[kind]
    span = ref64.mesh_span(lens)
    dm = bzr.DeviceMesh(ctx, lens)
    mode = pipe_of(bzr, pipe)
    wu = bits(want)
    par = bits(bzr.intersect(ctx, dm, rays, mode=mode))
    assert np.array_equal(par, wu), f"{kind} {pipe}: parity differs on {int((par != wu).any(axis=0).sum())} rays"
    fast = bzr.intersect(ctx, dm, rays, mode=mode | bzr.MODE_FAST)
    fu = bits(fast)
    # exact: finite t on every INTERSECT row, and a hit lies on a gate candidate or on the neighbour a candidate names
    neigh = np.ascontiguousarray(lens).view(np.uint32)[:, 16:19]
    hit = np.nonzero(fu[11] == bzr.WHAT_INTERSECT)[0]
    assert len(hit) > 4000
    assert np.isfinite(fast[0, hit]).all(), f"{kind} {pipe}: INTERSECT with a non-finite t"
    p = fu[12, hit].astype(np.int64)
    assert (p < len(lens)).all()
    direct = gate[hit, p]
    named = np.zeros(len(hit), bool)
    for j in np.nonzero(~direct)[0]:
        named[j] = bool((neigh[gate[hit[j]]] == p[j]).any())
    assert (direct | named).all(), f"{kind} {pipe}: {int((~(direct | named)).sum())} hits outside the candidate set"
    none = ~gate.any(axis=1)
    assert np.array_equal(fu[:, none], wu[:, none])
    # against binary64, on the well-conditioned rays
    well = ref.well
    assert well.sum() >= 4000
    same = lambda u: (u[11, well] == bzr.WHAT_INTERSECT) & (u[12, well] == ref.patch[well])  # noqa: E731
    oracle_share, fast_share = float(same(wu).mean()), float(same(fu).mean())
    print(f"{kind} {pipe}: {rays.shape[1]} rays, {int(well.sum())} well; same hit as float64: oracle {oracle_share:.5f}, "
          f"FAST {fast_share:.5f}")
    assert fast_share >= oracle_share - CLASS_ALLOW
    both = well.copy()
    both[well] = same(wu) & same(fu)
    assert_bars(f"segments {kind} {pipe}", fast, want, ref, both, span)


# ------------------------------------------------------------------ (b) the chain end to end
@pytest.fixture(scope="module")
def cases(orc):
    return {name: chain64.reference(orc, name) for name in ("cfg2", "cfg4")}


@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("name", ["cfg2", "cfg4"])
def test_fast_chain_against_float64(bzr, ctx, cases, name, pipe):
    c = cases[name]
    ref, want = c.ref, c.oracle
    dms = [bzr.DeviceMesh(ctx, p) for p in c.lenses]
    got = bzr.trace_chain_opl(ctx, dms, c.table, c.rays, c.channel, max_bounces=4, mode=pipe_of(bzr, pipe) | bzr.MODE_FAST)
    got = tuple(np.asarray(a) for a in got)
    assert all(np.isfinite(a).all() for a in (got[0], got[1], got[5], got[6]))
    well = ref.well
    same_o, same_f = chain64.same_structure(want, ref), chain64.same_structure(got, ref)
    oracle_share, fast_share = float(same_o[well].mean()), float(same_f[well].mean())
    print(f"{name} {pipe}: {int(well.sum())} well rays of {len(well)}; chain64's status, segments and bounces: oracle "
          f"{oracle_share:.5f}, FAST {fast_share:.5f}")
    assert fast_share >= oracle_share - CLASS_ALLOW
    failures = []
    for cls, sel in chain64.classes(ref, well & same_o & same_f).items():
        m = int(sel.sum())
        assert m >= (BOUNCED_MIN if cls == "bounced" else UNBOUNCED_MIN), (cls, m)
        qf = ref64.quantiles(chain64.chain_errors(got, ref, sel, c.span))
        qo = ref64.quantiles(chain64.chain_errors(want, ref, sel, c.span))
        print(f"{name} {pipe} {cls}: {m} rays; FAST / oracle error ratio (median, p99; * = asserted): "
              + ", ".join(f"{k} " + " ".join(f"{chain64.ratio(f, o):.2f}{'*' if chain64.asserted(name, cls, w, k) else ''}"
                                             for w, f, o in zip(("median", "p99"), qf[k], qo[k])) for k in qf)
              + "; oracle median / p99: " + ", ".join(f"{k} {a:.2e} / {b:.2e}" for k, (a, b) in qo.items()))
        for k in qf:
            for w, f, o in zip(("median", "p99"), qf[k], qo[k]):
                if chain64.asserted(name, cls, w, k) and not f <= BAR * o:
                    failures.append(f"{cls}: FAST's {w} {k} error {f:.3e} exceeds {BAR} x the oracle's {o:.3e}")
    assert not failures, f"{name} {pipe}: " + "; ".join(failures)


# ------------------------------------------------------------------ (c) the per-leg step
@pytest.mark.parametrize("pipe", PIPES)
def test_fast_leg_is_exact(bzr, orc, ctx, pipe):
    lenses, table, rays, channel = chain64.scene(orc, "cfg2", 128)
    n = rays.shape[1]
    p_in = (np.random.default_rng(43).random(n, dtype=F) * F(8)).astype(F)
    dms = [bzr.DeviceMesh(ctx, p) for p in lenses]
    got = bzr.trace_chain_opl(ctx, dms, table, rays, channel, opl=p_in, max_bounces=0,
                              mode=pipe_of(bzr, pipe) | bzr.MODE_FAST)
    o, _, st, seg, b, opl, glass = (np.asarray(a) for a in got)
    assert not b.any()
    k = (st == bzr.RR_NONE) & (seg == 2)
    print(f"{pipe}: {int(k.sum())} of {n} rays NONE after two segments")
    assert int(k.sum()) >= LEG_RAYS_MIN, int(k.sum())
    want = p_in[k] + opl_ref.leg(rays[0:3][:, k], o[0:3][:, k])
    assert want.dtype == F
    bad = bits(opl[k]) != bits(want)
    assert not bad.any(), (f"{pipe}: out_opl of {int(bad.sum())} of {int(k.sum())} rays is not opl_in + the float32 leg; "
                           f"got {opl[k][bad][:4]} want {want[bad][:4]}")
    assert not bits(glass[k]).any()
    assert (bits(o[3:6][:, k]) != bits(rays[3:6][:, k])).any(axis=0).sum() > 0.9 * k.sum()  # they were refracted once
    # a ray that met nothing keeps its path, and a ray that left the lens has glass
    miss = seg == 1
    assert miss.sum() > 1000 and np.array_equal(bits(opl[miss]), bits(p_in[miss])) and not bits(glass[miss]).any()
    assert (glass[st == bzr.RR_OUTSIDE] > 0).all()
