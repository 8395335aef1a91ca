"""bzr_trace_chain_opl in binary64, for judging float32 chains (the oracle's and BZR_MODE_FAST's) against one truth.

A plain helper module like ref64.py (no fixtures, no plugin).  The chain steps are written from include/bzr.h's text:
Snell's step (s2 = eta^2 (1 - cs^2); a refraction when s2 < 0.99, the direction kept when s2 <= 1e-12, the normal's
sign by the side), the Fresnel T of bzr_trace_chain_power, the reflecting step of bzr_trace_chain_tir and the per-leg
step of bzr_trace_chain_opl.  eta and ri are taken at their float32 values -- eta = float32(1) / float32(ri) going
in, ri going out, as the device has them -- and the constants 0.99f and 1e-12f at theirs; everything computed from
them is binary64.

chain64            the chain, carrying binary64 rays from segment to segment.  Each segment's candidate set is the
                   oracle's planar gate of the float32-rounded rays, its winner ref64.intersect64's
Recorder           a proxy around the oracle module that logs every BezierMesh::intersect tir_ref / opl_ref make,
                   with the side the following refract expects, so the segments can be sorted by kind
scene              the inputs the CPU and the GPU tests share (test_gpu_tir.py's scenes at a denser grid)
chain_errors       the five errors of a float32 chain result against chain64's
"""
from types import SimpleNamespace

import numpy as np

import ref64

F = np.float32
RR_NONE, RR_INSIDE, RR_OUTSIDE = 0, 1, 2
S2_REFRACT = float(F(0.99))
S2_KEEP = float(F(1e-12))
S2_WELL = 1e-3          # |s2 - 0.99| and, on OUTSIDE segments, |s2 - 1|
KINDS = ("inside", "outside", "bounce")   # refract(INSIDE); the first refract(OUTSIDE); OUTSIDE after a reflection
ERRORS = ("direction", "origin", "weight", "opl", "glass")


def _dot(a, b):
    return (a * b).sum(axis=-1)


# ------------------------------------------------------------------ the steps, arrays over rays: vectors [m, 3]
def s2_of(eta, cs):
    return eta * eta * (1.0 - cs * cs)


def snell(d, normal, cs, eta, inside):
    """Snell's step's direction for the rays it refracts (s2 < 0.99): normalized(d eta + n (eta c1 - c2)) with
    n = normal on an INSIDE hit and -normal on an OUTSIDE one, c1 = |cs|, c2 = sqrt(1 - s2); d itself when
    s2 <= 1e-12."""
    s2 = s2_of(eta, cs)
    n = normal * np.where(inside, 1.0, -1.0)[:, None]
    c1 = np.abs(cs)
    with np.errstate(invalid="ignore"):
        c2 = np.sqrt(1.0 - s2)
    v = d * np.asarray(eta)[..., None] + n * (eta * c1 - c2)[:, None]
    return np.where((s2 > S2_KEEP)[:, None], ref64._unit(v), d)


def fresnel_t(eta, cs):
    s2 = s2_of(eta, cs)
    c1 = np.abs(cs)
    with np.errstate(invalid="ignore", divide="ignore"):
        c2 = np.sqrt(1.0 - s2)
        rs = (eta * c1 - c2) / (eta * c1 + c2)
        rp = (eta * c2 - c1) / (eta * c2 + c1)
    return 1.0 - 0.5 * (rs * rs + rp * rp)


def reflect(d, normal, cs):
    """k = 2 cs, r = d - normal k, direction = r / sqrt(r.r) (r itself if r.r is not > 0)."""
    k = 2.0 * cs
    return ref64._unit(d - normal * k[:, None])


def leg(s, p):
    """The distance from the segment's origin s to the hit's point p."""
    e = p - s
    return np.sqrt(_dot(e, e))


# ------------------------------------------------------------------ the chain
def step64(rays, hit, expected, ri32, may_reflect):
    """The chain step of one refract(expected) segment, given its winning hits: rays [6, m] binary64, hit a namespace
    with what, cs, point [m, 3], normal [m, 3] (intersect64's, or a float32 hit's words in binary64).  Returns a
    namespace: status [m] (expected or NONE), refl [m] (the ray is reflected), rays [6, m] (what the chain continues
    with where status != NONE or refl; the input elsewhere), t (the Fresnel term where status != NONE, else 1),
    length (the leg where the chain continues, else 0), s2, and decides [m]: s2 decided the ray's fate."""
    m = rays.shape[1]
    d = rays[3:6].T
    isect = hit.what == ref64.INTERSECT
    inside = hit.cs < 0.0
    side = np.where(inside, RR_INSIDE, RR_OUTSIDE)
    eta = np.where(inside, float(F(1) / F(ri32)), float(F(ri32)))
    s2 = s2_of(eta, hit.cs)
    mine = isect & (side == expected)
    with np.errstate(invalid="ignore"):
        refr = mine & (s2 < S2_REFRACT)
        refl = mine & (expected == RR_OUTSIDE) & (s2 >= 1.0) & bool(may_reflect)
    out = np.array(rays, np.float64)
    go = refr | refl
    out[0:3, go] = hit.point[go].T
    out[3:6, refr] = snell(d[refr], hit.normal[refr], hit.cs[refr], eta[refr], inside[refr]).T
    out[3:6, refl] = reflect(d[refl], hit.normal[refl], hit.cs[refl]).T
    t = np.ones(m)
    t[refr] = fresnel_t(eta[refr], hit.cs[refr])
    length = np.zeros(m)
    length[go] = leg(rays[0:3, go].T, hit.point[go])
    return SimpleNamespace(status=np.where(refr, expected, RR_NONE).astype(np.uint32), refl=refl, rays=out, t=t,
                           length=length, s2=s2, decides=mine)


def s2_margin(s2, expected):
    """|s2 - 0.99| and, on an OUTSIDE segment, |s2 - 1| exceed S2_WELL."""
    with np.errstate(invalid="ignore"):
        ok = np.abs(s2 - S2_REFRACT) > S2_WELL
        return ok & (np.abs(s2 - 1.0) > S2_WELL) if expected == RR_OUTSIDE else ok


def _segment(orc, patches, rays, expected, ri32, may_reflect, threads):
    """step64 on intersect64's winners over the planar gate of the float32-rounded rays, with `well` [m]."""
    hit = ref64.intersect64(patches, rays, orc.planar_gate(patches, rays.astype(F), threads))
    g = step64(rays, hit, expected, ri32, may_reflect)
    # a miss is intersect64's: no candidate pair is an INTERSECT with a finite t; it carries no margin of its own
    g.well = np.where(hit.what == ref64.INTERSECT, hit.well & (s2_margin(g.s2, expected) | ~g.decides), True)
    return g


def chain64_one(orc, lenses, ris, rays, max_bounces=4, threads=16):
    """The chain with one index per lens; rays [6, n] float32 or binary64.  Weight starts at 1 and opl at 0."""
    out = np.array(rays, np.float64)
    n = out.shape[1]
    w, opl, glass = np.ones(n), np.zeros(n), np.zeros(n)
    status = np.zeros(n, np.uint32)
    seg = np.zeros(n, np.uint32)
    bounces = np.zeros(n, np.uint32)
    well = np.ones(n, bool)
    alive = np.arange(n)
    for patches, ri in zip(lenses, ris):
        if alive.size == 0:
            break
        ri32 = F(ri)
        g = _segment(orc, patches, out[:, alive], RR_INSIDE, ri32, False, threads)
        seg[alive] += 1
        status[alive] = g.status
        well[alive] &= g.well
        ok = g.status != RR_NONE
        pend = alive[ok]
        w[pend] *= g.t[ok]
        opl[pend] += g.length[ok]   # the leg lies in air
        out[:, pend] = g.rays[:, ok]
        left = []
        for b in range(max_bounces + 1):
            if pend.size == 0:
                break
            g = _segment(orc, patches, out[:, pend], RR_OUTSIDE, ri32, b < max_bounces, threads)
            seg[pend] += 1
            well[pend] &= g.well
            rest = ~g.refl
            status[pend[rest]] = g.status[rest]
            bounces[pend[g.refl]] += 1
            ok = g.status != RR_NONE
            went = ok | g.refl      # the leg lies in glass, refracted out or reflected alike
            w[pend[ok]] *= g.t[ok]
            glass[pend[went]] += g.length[went]
            opl[pend[went]] += float(ri32) * g.length[went]
            out[:, pend[went]] = g.rays[:, went]
            left.append(pend[ok])
            pend = pend[g.refl]
        assert pend.size == 0
        alive = np.sort(np.concatenate(left)) if left else np.zeros(0, np.int64)
    return out, w, status, seg, bounces, opl, glass, well


def chain64(orc, lenses, ri_table, rays, channel=None, max_bounces=4):
    """bzr_trace_chain_opl in binary64 with ri_table[l][channel[i]] for ray i, run per channel as tir_ref.chain is.
    Returns a namespace: rays [6, n], weight, status, segments, bounces, opl, glass, and well: every decision on the
    ray's way was taken with a margin -- each winner is intersect64's `well`, a miss is a segment on which no
    candidate is an INTERSECT with a finite t (intersect64's miss), and |s2 - 0.99| and (OUTSIDE segments) |s2 - 1| exceed S2_WELL where s2 decides."""
    table = np.asarray(ri_table, F)
    n = np.shape(rays)[1]
    channel = np.zeros(n, np.uint8) if channel is None else np.asarray(channel)
    assert table.ndim == 2 and table.shape[0] == len(lenses) and channel.shape == (n,) and (channel < table.shape[1]).all()
    r = SimpleNamespace(rays=np.array(rays, np.float64), weight=np.ones(n), status=np.zeros(n, np.uint32),
                        segments=np.ones(n, np.uint32), bounces=np.zeros(n, np.uint32), opl=np.zeros(n),
                        glass=np.zeros(n), well=np.zeros(n, bool))
    for c in range(table.shape[1]):
        idx = np.nonzero(channel == c)[0]
        if idx.size == 0:
            continue
        res = chain64_one(orc, lenses, list(table[:, c]), np.asarray(rays)[:, idx], max_bounces)
        (r.rays[:, idx], r.weight[idx], r.status[idx], r.segments[idx], r.bounces[idx], r.opl[idx], r.glass[idx],
         r.well[idx]) = res
    return r


# ------------------------------------------------------------------ the segments a float32 chain sees
class Recorder:
    """The oracle module with a log: hand it to tir_ref.chain or opl_ref.chain in the oracle's place.  intersect and
    refract are forwarded.  Every intersect call is logged as a namespace (lens, rays: float32, hits: the oracle's
    rows); the refract call on the same rays that follows it adds expected, ri, out_rays and status."""

    def __init__(self, orc):
        self._orc = orc
        self.log = []

    def __getattr__(self, name):
        return getattr(self._orc, name)

    def intersect(self, patches, rays, threads=0, L=None):
        hits = self._orc.intersect(patches, rays, threads, L)
        self.log.append(SimpleNamespace(lens=patches, rays=np.array(rays, F), hits=hits, expected=None))
        return hits

    def refract(self, patches, ri, rays, expected, threads=0):
        e = self.log[-1]
        assert e.lens is patches and e.expected is None
        assert np.array_equal(e.rays.view(np.uint32), np.asarray(rays, F).view(np.uint32))
        exp = np.unique(expected)
        assert exp.size == 1
        e.expected, e.ri = int(exp[0]), F(ri)
        e.out_rays, e.status = self._orc.refract(patches, ri, rays, expected, threads)
        return e.out_rays, e.status

    def kinds(self):
        """The kind of every logged segment.  A chain's calls on one lens run INSIDE, OUTSIDE, then OUTSIDE once more
        per reflection: an OUTSIDE segment that follows an OUTSIDE segment holds reflected rays, which start on the
        surface they must not hit again."""
        out, before = [], None
        for e in self.log:
            assert e.expected in (RR_INSIDE, RR_OUTSIDE)
            out.append("inside" if e.expected == RR_INSIDE else "outside" if before == RR_INSIDE else "bounce")
            before = e.expected
        return out

    def segments(self, patches):
        """kind -> (float32 rays [6, m], oracle hits [13, m]) over the logged segments on the lens `patches`."""
        got = {k: ([], []) for k in KINDS}
        for e, kind in zip(self.log, self.kinds()):
            if e.lens is patches:
                got[kind][0].append(e.rays)
                got[kind][1].append(e.hits)
        return {k: (np.ascontiguousarray(np.concatenate(r, axis=1)), np.ascontiguousarray(np.concatenate(h, axis=1)))
                for k, (r, h) in got.items()}


# ------------------------------------------------------------------ inputs the CPU and the GPU tests share
def scene(orc, name, side):
    """(lens patch arrays, table, rays [6, n], channel [n]): test_gpu_tir.py's scene at another grid, n = side^2 - 37
    (the last wave is ragged), the lenses built with the oracle's Mesh."""
    from bzr_amd.configs import CONFIGS, build_lens, grid_rays
    from test_gpu_tir import DROP, NCHAN, TABLES

    cfg = CONFIGS[name]
    lenses = [build_lens(orc.OMesh, lens).bezier_patches() for lens in cfg.lenses]
    rays = grid_rays(cfg, side=side)
    n = rays.shape[1] - DROP
    rays = np.ascontiguousarray(rays[:, :n])
    channel = np.random.default_rng(7).integers(0, NCHAN, side * side)[:n].astype(np.uint8)
    for a in lenses + [rays, channel]:
        a.setflags(write=False)
    return lenses, TABLES[name], rays, channel


def same_structure(res, ref):
    """res, a float32 chain's (rays, weight, status, segments, bounces, ...), has chain64's status, segments, bounces."""
    return (np.asarray(res[2]) == ref.status) & (np.asarray(res[3]) == ref.segments) & (np.asarray(res[4]) == ref.bounces)


def chain_errors(res, ref, sel, span):
    """Per selected ray of the float32 result `res` (rays, weight, status, segments, bounces, opl, glass) against
    chain64's namespace: exit direction (max component), exit origin / span, weight, opl and glass relative."""
    r = np.asarray(res[0], np.float64)[:, sel]
    rel = lambda got, want: np.abs(np.asarray(got, np.float64)[sel] - want[sel]) / np.abs(want[sel])  # noqa: E731
    with np.errstate(all="ignore"):
        return {
            "direction": np.abs(r[3:6] - ref.rays[3:6, sel]).max(axis=0),
            "origin": np.abs(r[0:3] - ref.rays[0:3, sel]).max(axis=0) / span,
            "weight": rel(res[1], ref.weight),
            "opl": rel(res[5], ref.opl),
            "glass": rel(res[6], ref.glass),
        }


def classes(ref, sel):
    """name -> the rays of `sel` in the class: unbounced and OUTSIDE; bounced (at least one reflection, any end)."""
    return {"unbounced": sel & (ref.bounces == 0) & (ref.status == RR_OUTSIDE), "bounced": sel & (ref.bounces > 0)}


def reference(orc, name, side=192, max_bounces=4):
    """The scene with its two chains, weight and opl starting at 1 and 0: a namespace with lenses, table, rays,
    channel, span, ref (chain64's namespace) and oracle (opl_ref.chain's tuple)."""
    import opl_ref

    lenses, table, rays, channel = scene(orc, name, side)
    ref = chain64(orc, lenses, table, rays, channel, max_bounces)
    oracle = opl_ref.chain(orc, lenses, table, rays, channel, None, None, max_bounces)
    for a in tuple(vars(ref).values()) + tuple(oracle):
        a.setflags(write=False)
    return SimpleNamespace(lenses=lenses, table=table, rays=rays, channel=channel, ref=ref, oracle=oracle,
                           span=max(ref64.mesh_span(p) for p in lenses))


def recorded(orc, name="cfg2", side=128, max_bounces=4):
    """The Recorder after tir_ref.chain over the scene, and the scene's first lens."""
    import tir_ref

    lenses, table, rays, channel = scene(orc, name, side)
    rec = Recorder(orc)
    tir_ref.chain(rec, lenses, table, rays, channel, None, max_bounces)
    return rec, lenses[0]


def ratio(a, b):
    return a / b if b > 0 else (0.0 if a == 0 else float("inf"))


def asserted(scene_name, cls, which, field):
    """Whether FAST's quantile is held to BAR x the oracle's: the quantiles that are stable between random halves of
    the class (tests/test_chain64.py asserts it); the others, heavy-tailed in the oracle itself, are only printed."""
    if cls == "unbounced":
        return which == "median" or (scene_name == "cfg2" and field != "weight")
    return which == "median" and field != "weight"
