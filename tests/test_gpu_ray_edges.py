"""Ray inputs at the edges of the batch calls' input space, against the oracle bit for bit.

tiers    origins with |s|inf exactly at, one ulp inside and one ulp beyond the near tier's radius s_near and the
         tree's validity radius s_max (the wave walks the near tree only when no active lane has !(|s|inf <= s_near);
         a lane with !(|s|inf <= s_max) takes the in-order scan), class by class and with all seven classes in every wave.
garbage  NaN, infinite, huge, zero, denormal and scaled directions and origins beside ordinary rays (the grid, an
         oblique parallel beam and incoherent rays): every word equals the oracle's, and the ordinary rays' words do
         not depend on what their wave's other lanes hold.
scaled   directions of length 0.99 .. 1.01 from close to the lens, where they still hit.
expected BezierLens::refract with a per-ray `expected` of 0..3.

The lenses are tests/test_gpu_long_chains.py's (432 patches each at x = 10, 13, 16).  s_max and s_near are read from
the product (bzr_debug_gate_boxes_tier), 1100.5068 and 88.04054 for lens 0.  Every population a test relies on is
computed from the oracle's output and asserted.
"""
import numpy as np
import pytest

from test_culling_conservative import gate_boxes
from test_gpu_long_chains import MODES, bits, chain_rays, lens_patches, mode_of

pytestmark = pytest.mark.gpu

N_CLASS = 2048
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
OPS = ("intersect", "chain1", "chain3")
RI3 = [1.3, 1.3, 1.3]


# ------------------------------------------------------------------ recipes (also used by test_gpu_variants.py's worker)
def tier_radii(bzr, patches):
    """(s_near, s_max) as bzr_mesh_create takes them: the far tier's radius, and the smaller of the two tiers'."""
    _, s_far = gate_boxes(bzr, patches, 0)
    _, s_near = gate_boxes(bzr, patches, 1)
    return np.float32(min(s_near, s_far)), np.float32(s_far)


def tier_classes(s_near, s_max):
    f, inf = np.float32, np.float32(np.inf)
    return [f(s_near), np.nextafter(f(s_near), -inf), np.nextafter(f(s_near), inf),
            f(s_max), np.nextafter(f(s_max), -inf), np.nextafter(f(s_max), inf), f(s_near) / f(2)]


def aimed_rays(patches, radius, seed, n=N_CLASS):
    """n rays from the surface of the cube |s|inf = radius (uniform inside, one coordinate moved to +-radius exactly),
    each aimed at a random control point of the lens pulled 10 % towards its centre (10, 0, 0)."""
    rng = np.random.default_rng(seed)
    r = np.float32(radius)
    o = rng.uniform(-float(r), float(r), (3, n)).astype(np.float32)
    o[rng.integers(0, 3, n), np.arange(n)] = np.where(rng.random(n) < 0.5, r, -r)
    assert (np.abs(o).max(axis=0) == r).all()
    cp = patches[:, 19:49].reshape(-1, 3).astype(np.float64)
    tgt = 0.9 * cp[rng.integers(0, len(cp), n)] + np.array([1.0, 0.0, 0.0])
    d = tgt.T - o.astype(np.float64)
    d /= np.linalg.norm(d, axis=0, keepdims=True)
    return np.ascontiguousarray(np.concatenate([o, d.astype(np.float32)]))


def tier_batches(patches, classes):
    """(per-class batches, the interleaved batch, its class per ray): lane j of every wave holds class j mod 7."""
    per = [aimed_rays(patches, r, 100 + k) for k, r in enumerate(classes)]
    waves = N_CLASS // 10                                   # class 0 takes 10 lanes of a wave, the others 9
    cls = np.tile(np.arange(64) % len(classes), waves)
    mix = np.empty((6, len(cls)), np.float32)
    for k, b in enumerate(per):
        mix[:, cls == k] = b[:, :int((cls == k).sum())]
    return per, mix, cls


def poisons():
    """name -> function(ray [6] float32 copy) -> poisoned ray."""
    f = np.float32
    out = {}

    def setter(row, val):
        def fn(r):
            r[row] = val
            return r
        return fn

    for name, row in (("ox", 0), ("oy", 1), ("dx", 3), ("dz", 5)):
        out[f"nan_{name}"] = setter(row, QNAN)
    for name, row in (("ox", 0), ("oy", 1), ("dx", 3), ("dy", 4)):
        out[f"+inf_{name}"] = setter(row, f(np.inf))
        out[f"-inf_{name}"] = setter(row, f(-np.inf))
    out["ox_-3e38"] = setter(0, f(-3e38))
    out["dx_3e38"] = setter(3, f(3e38))
    out["d_zero"] = setter(slice(3, 6), f(0.0))
    out["d_negzero"] = setter(slice(3, 6), f(-0.0))
    out["dx_1e-40"] = setter(3, f(1e-40))
    out["dy_1e-40"] = setter(4, f(1e-40))
    for k in (-30, -10, 10, 21, 25, 60, 120):
        def scaled(r, k=k):
            r[3:] = r[3:] * f(2.0) ** f(k)
            return r
        out[f"d_x2^{k}"] = scaled
    return out


PATTERNS = ("lane0", "lane17", "lane63", "third", "waves", "allbut1")


def poison_mask(pattern, n):
    lane, wave = np.arange(n) % 64, np.arange(n) // 64
    if pattern.startswith("lane"):
        return lane == int(pattern[4:])
    return {"third": np.arange(n) % 3 == 0, "waves": wave % 4 == 1, "allbut1": lane != 31}[pattern]


def poisoned(clean, pattern):
    """(batch, mask): `clean` with the pattern's lanes poisoned, every poison cycling over them."""
    mask = poison_mask(pattern, clean.shape[1])
    fns = list(poisons().values())
    out = np.array(clean, dtype=np.float32, copy=True)
    for j, i in enumerate(np.nonzero(mask)[0]):
        out[:, i] = fns[j % len(fns)](out[:, i].copy())
    return np.ascontiguousarray(out), mask


def oblique_rays():
    """The grid's 4 096 points moved onto the lens's plane x = 10, each met by a ray of one oblique direction from 12
    back: a parallel beam, so its waves take the bundle walk like the grid's, but with no axis of the bundle's
    direction box straddling zero.  Only then does a wrong bound on one axis (a NaN lane's, say) empty the bundle's
    time interval against another axis's and drop a box its other lanes meet; with the grid's +x directions the y
    and z axes bound nothing."""
    d = np.array([1.0, 0.45, 0.3])
    d /= np.linalg.norm(d)
    p = chain_rays()[:3].astype(np.float64)
    p[0] = 10.0
    o = p - 12.0 * d[:, None]
    return np.ascontiguousarray(np.concatenate([o, np.repeat(d[:, None], o.shape[1], axis=1)]).astype(np.float32))


def clean_batch(patches, s_near):
    """The 4 096 grid rays and 4 096 oblique parallel rays (coherent waves: the bundle walk), and 2 048 incoherent rays
    (wide bundles: the per-lane walk)."""
    return np.ascontiguousarray(np.concatenate([chain_rays(), aimed_rays(patches, np.float32(s_near) / np.float32(2), 106),
                                                oblique_rays()], axis=1))


def run_orc(orc, lenses, op, rays):
    """The oracle's words for one op as a list of uint32 arrays, and its work counters."""
    orc.counters_reset()
    if op == "intersect":
        res = [bits(orc.intersect(lenses[0], rays))]
    else:
        k = 1 if op == "chain1" else 3
        res = [bits(a) for a in orc.trace_chain(lenses[:k], RI3[:k], rays)]
    return res, orc.counters()


def run_gpu(bzr, ctx, dms, op, rays, mode):
    if op == "intersect":
        return [bits(bzr.intersect(ctx, dms[0], rays, mode=mode))]
    k = 1 if op == "chain1" else 3
    return [bits(a) for a in bzr.trace_chain(ctx, dms[:k], RI3[:k], rays, mode=mode)]


def differing(got, want):
    bad = np.zeros(got[0].shape[-1], bool)
    for g, w in zip(got, want):
        bad |= (g != w) if g.ndim == 1 else (g != w).any(axis=0)
    return bad


def assert_same(got, want, label, names=None):
    bad = differing(got, want)
    if bad.any():
        idx = np.nonzero(bad)[0]
        who = "" if names is None else f", kinds {sorted(set(names[i] for i in idx))[:12]}"
        i = idx[0]
        raise AssertionError(f"{label}: {len(idx)} of {len(bad)} rays differ, first {idx[:8]}{who}; ray {i}: got "
                             f"{[hex(int(x)) for g in got for x in np.atleast_1d(g[..., i])]} want "
                             f"{[hex(int(x)) for w in want for x in np.atleast_1d(w[..., i])]}")


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def lenses(orc):
    out = [lens_patches(orc, k) for k in range(3)]
    for p in out:
        p.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def dms(bzr, ctx, lenses):
    return [bzr.DeviceMesh(ctx, p) for p in lenses]


@pytest.fixture(scope="module")
def radii(bzr, lenses):
    s_near, s_max = tier_radii(bzr, lenses[0])
    print("s_near", s_near, "s_max", s_max)
    assert 0 < s_near < s_max < 1e6
    return s_near, s_max


@pytest.fixture(scope="module")
def tiers(orc, lenses, radii):
    """Per-class and interleaved batches with the oracle's words for the three ops."""
    classes = tier_classes(*radii)
    per, mix, cls = tier_batches(lenses[0], classes)
    batches = {f"class{k}": b for k, b in enumerate(per)}
    batches["mixed"] = mix
    want = {(name, op): run_orc(orc, lenses, op, b)[0] for name, b in batches.items() for op in OPS}
    return classes, batches, cls, want


@pytest.fixture(scope="module")
def garbage(orc, lenses, radii):
    """The clean batch, its poisoned versions, and the oracle's words and counters for each."""
    clean = clean_batch(lenses[0], radii[0])
    clean.setflags(write=False)
    names = list(poisons())
    out = {"clean": (clean, None, None, {op: run_orc(orc, lenses, op, clean) for op in OPS})}
    for pat in PATTERNS:
        batch, mask = poisoned(clean, pat)
        kind = np.full(batch.shape[1], "clean", dtype=object)
        kind[mask] = [names[j % len(names)] for j in range(int(mask.sum()))]
        out[pat] = (batch, mask, kind, {op: run_orc(orc, lenses, op, batch) for op in OPS})
    return out


@pytest.fixture(scope="module")
def clean_gpu(bzr, ctx, dms, garbage):
    """The unpoisoned batch on the GPU, per (op, mode): what the clean lanes of every poisoned run must reproduce."""
    clean = garbage["clean"][0]
    return {(op, m): run_gpu(bzr, ctx, dms, op, clean, mode_of(bzr, m)) for op in OPS for m in MODES}


# ------------------------------------------------------------------ B1: tier boundaries
def test_tier_batches_sit_on_the_boundaries(bzr, tiers, radii):
    """Non-vacuity: every class starts exactly on its cube and mostly hits; the mixed waves hold all three tiers."""
    classes, batches, cls, want = tiers
    s_near, s_max = radii
    assert len(set(float(c) for c in classes)) == 7
    for k, r in enumerate(classes):
        b = batches[f"class{k}"]
        assert (np.abs(b[:3]).max(axis=0) == r).all()
        hit = want[(f"class{k}", "intersect")][0][11] == bzr.WHAT_INTERSECT
        two = want[(f"class{k}", "chain1")][2] == 2
        print(f"class {k} R = {r!r}: {int(hit.sum())} hits, {int(two.sum())} two-segment rays of {N_CLASS}")
        assert hit.mean() > 0.9 and two.mean() > 0.5
    amax = np.abs(batches["mixed"][:3]).max(axis=0).reshape(-1, 64)
    assert ((amax <= s_near).any(1) & ((amax > s_near) & (amax <= s_max)).any(1) & (amax > s_max).any(1)).all()
    assert (want[("mixed", "intersect")][0][11] == bzr.WHAT_INTERSECT).mean() > 0.9
    assert (want[("mixed", "chain3")][2] == 6).sum() > 100


@pytest.mark.parametrize("m", MODES)
@pytest.mark.parametrize("op", OPS)
def test_tier_boundary_origins_equal_oracle(bzr, ctx, dms, tiers, op, m):
    classes, batches, cls, want = tiers
    for name, b in batches.items():
        assert_same(run_gpu(bzr, ctx, dms, op, b, mode_of(bzr, m)), want[(name, op)], f"{name} {op} {m}")


@pytest.mark.parametrize("m", ["fused", "staged"])
def test_only_origins_beyond_s_max_take_the_full_scan(bzr, ctx, dms, tiers, radii, m):
    """The inclusive boundary: a ray at |s|inf == s_max walks the tree, one an ulp beyond is counted as overflowed."""
    classes, batches, cls, want = tiers
    s_max = radii[1]
    seen = {}
    for name, b in batches.items():
        ctx.counters(True)
        ctx.counters_report()
        got = run_gpu(bzr, ctx, dms, "intersect", b, mode_of(bzr, m))
        rep = ctx.counters_report()
        ctx.counters(False)
        assert_same(got, want[(name, "intersect")], f"{name} {m}")
        beyond = int((np.abs(b[:3]).max(axis=0) > s_max).sum())
        seen[name] = (rep["overflow_rays"], beyond)
    print(m, "overflow rays (counted, beyond s_max):", seen)
    assert seen["class3"][1] == 0 and seen["class5"][1] == N_CLASS and seen["mixed"][1] > 1000
    for name, (counted, beyond) in seen.items():
        assert counted == beyond, (name, m, seen)


@pytest.mark.parametrize("m", ["fused", "staged"])
def test_a_wave_at_s_near_exactly_walks_the_near_tree(bzr, orc, ctx, dms, lenses, tiers, radii, m):
    """Which tree a wave walks does not reach the output (both are conservative), so the inclusive near boundary is
    pinned through the gate-test counter (per ray: leaf boxes its own box test hit).  Batch X: every origin at
    |s|inf == s_near exactly, lane 0 of each wave a ray that points away from the lens (it hits no box of either
    tier, checked below with the float32 slab replica).  Batch Y: X with lane 0's origin one ulp farther out, which
    sends its whole wave to the far tree.  The other 63 lanes are the same rays in both; the near tier's boxes lie
    inside the far tier's (tests/test_culling_conservative.py), so X can only evaluate fewer gates than Y, and
    strictly fewer here because these rays hit fewer near boxes than far boxes (asserted).  Equal counts mean that X
    walked the far tree: `<` for `<=` at s_near."""
    from test_culling_conservative import slab_f32

    s_near, _ = radii
    x = np.array(tiers[1]["class0"], copy=True)
    x[:, ::64] = np.array([-s_near, 0.0, 0.0, -1.0, 0.0, 0.0], np.float32)[:, None]
    y = x.copy()
    y[0, ::64] = -np.nextafter(s_near, np.float32(np.inf))
    assert (np.abs(x[:3]).max(axis=0) == s_near).all() and (np.abs(y[:3]).max(axis=0) > s_near).reshape(-1, 64).any(1).all()
    far_boxes, _ = gate_boxes(bzr, lenses[0], 0)
    near_boxes, _ = gate_boxes(bzr, lenses[0], 1)
    assert not slab_f32(far_boxes, y[:, ::64]).any() and not slab_f32(near_boxes, x[:, ::64]).any()
    n_near, n_far = int(slab_f32(near_boxes, x).sum()), int(slab_f32(far_boxes, x).sum())
    assert n_near < n_far
    want = bits(orc.intersect(lenses[0], x))
    gates = {}
    for name, b in (("x", x), ("y", y)):
        ctx.counters(True)
        ctx.counters_report()
        got = bits(bzr.intersect(ctx, dms[0], b, mode=mode_of(bzr, m)))
        rep = ctx.counters_report()
        ctx.counters(False)
        keep = np.arange(b.shape[1]) % 64 != 0
        assert np.array_equal(got[:, keep], want[:, keep]) and (got[11, ~keep] == bzr.WHAT_NONE).all()
        assert rep["overflow_rays"] == 0
        gates[name] = rep["gate_tests"]
    print(m, "gate tests at s_near", gates, "slab replica: near", n_near, "far", n_far)
    assert 0 < gates["x"] < gates["y"], (m, gates)


# ------------------------------------------------------------------ B2: garbage lanes
def test_garbage_batches_are_what_they_claim(bzr, garbage):
    """Non-vacuity, from the oracle: no ray with a non-finite component hits, the chain passes it through unchanged at
    segment 1, and the clean rays' oracle words do not depend on their neighbours."""
    clean, _, _, clean_want = garbage["clean"]
    assert (clean_want["intersect"][0][0][11] == bzr.WHAT_INTERSECT).mean() > 0.5
    for pat in PATTERNS:
        batch, mask, kind, want = garbage[pat]
        assert np.array_equal(bits(batch)[:, ~mask], bits(clean)[:, ~mask]) and mask.any() and not mask.all()
        if pat in ("third", "waves", "allbut1"):
            assert set(kind[mask]) == set(poisons())
        bad = ~np.isfinite(batch).all(axis=0)
        assert bad.sum() >= 0.4 * mask.sum() and not bad[~mask].any()
        assert not (want["intersect"][0][0][11][bad] == bzr.WHAT_INTERSECT).any()
        for op in ("chain1", "chain3"):
            o, st, sg = want[op][0]
            assert (sg[bad] == 1).all() and (st[bad] == bzr.RR_NONE).all()
            assert np.array_equal(o[:, bad], bits(batch)[:, bad])
        for op in OPS:
            for w, c in zip(want[op][0], clean_want[op][0]):
                assert np.array_equal(w[..., ~mask], c[..., ~mask])
        # the finite poisons are not all dead weight: the denormal-dy rays are ordinary rays
        alive = np.array([k == "dy_1e-40" for k in kind])
        if pat in ("third", "waves", "allbut1"):
            assert (want["intersect"][0][0][11][alive] == bzr.WHAT_INTERSECT).any()


@pytest.mark.parametrize("m", MODES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_garbage_lanes_leave_their_neighbours_alone(bzr, ctx, dms, garbage, clean_gpu, pattern, m):
    batch, mask, kind, want = garbage[pattern]
    for op in OPS:
        got = run_gpu(bzr, ctx, dms, op, batch, mode_of(bzr, m))
        # (b) first, the statement that needs no oracle: the clean lanes' words are those of the unpoisoned run
        assert_same([g[..., ~mask] for g in got], [c[..., ~mask] for c in clean_gpu[(op, m)]],
                    f"{pattern} {op} {m}: clean lanes vs the unpoisoned run")
        # (a) every word of every ray, poisoned or not, is the oracle's
        assert_same(got, want[op][0], f"{pattern} {op} {m}: vs the oracle", kind)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_garbage_lanes_do_the_oracles_work(bzr, ctx, dms, garbage, pattern):
    """Most scaled rays miss, so the counters show that their candidates and Newton passes were the reference's."""
    batch, mask, kind, want = garbage[pattern]
    for op in ("intersect", "chain3"):
        ctx.counters(True)
        ctx.counters_report()
        got = run_gpu(bzr, ctx, dms, op, batch, bzr.PIPELINE_FUSED)
        rep = ctx.counters_report()
        ctx.counters(False)
        work = want[op][1]
        print(pattern, op, rep, "oracle", work)
        assert_same(got, want[op][0], f"{pattern} {op}", kind)
        assert rep["segments"] == work["segments"]
        assert rep["pairs"] == work["newton"] and rep["follows"] == work["follow"]


# ------------------------------------------------------------------ B3: scaled directions that still hit
SCALES = (0.99, 0.999, 1.001, 1.01)


def scaled_batch():
    r = chain_rays()
    r[0] = np.float32(8.9)
    lane = np.arange(r.shape[1])
    odd = lane % 2 == 1
    r[3, odd] = np.array(SCALES, np.float32)[(lane[odd] // 2) % 4]
    return np.ascontiguousarray(r), odd


@pytest.mark.parametrize("m", MODES)
def test_scaled_directions_equal_oracle(bzr, orc, ctx, dms, lenses, m):
    batch, odd = scaled_batch()
    for s in SCALES:
        assert (batch[3] == np.float32(s)).sum() == batch.shape[1] // 8
    for op in OPS:
        want, _ = run_orc(orc, lenses, op, batch)
        if op == "intersect":
            hit = want[0][11] == bzr.WHAT_INTERSECT
            assert hit[odd].mean() >= 0.25 and hit[~odd].mean() >= 0.25
        assert_same(run_gpu(bzr, ctx, dms, op, batch, mode_of(bzr, m)), want, f"scaled {op} {m}")


# ------------------------------------------------------------------ B4: per-ray expected
@pytest.mark.parametrize("m", MODES)
def test_refract_with_per_ray_expected(bzr, orc, ctx, dms, lenses, m):
    """expected 0..3 mixed lane by lane; the grid meets the front surface, its first-refraction outputs the back."""
    front = chain_rays()
    back, st1 = orc.refract(lenses[0], 1.3, front, np.full(front.shape[1], bzr.RR_INSIDE, np.uint32))
    assert (st1 == bzr.RR_INSIDE).sum() > 1000
    exp = np.random.default_rng(9).integers(0, 4, front.shape[1]).astype(np.uint32)
    assert all((exp.reshape(-1, 64) == e).any(1).all() for e in range(4))  # every wave holds all four values
    for label, rays in (("front", front), ("back", back)):
        w_rays, w_st = orc.refract(lenses[0], 1.3, rays, exp)
        print(label, "status by expected:", {e: np.bincount(w_st[exp == e], minlength=3).tolist() for e in range(4)})
        assert len(np.unique(w_st)) >= 2
        g_rays, g_st = bzr.refract(ctx, dms[0], 1.3, rays, exp, mode=mode_of(bzr, m))
        assert_same([bits(g_rays), bits(g_st)], [bits(w_rays), bits(w_st)], f"refract {label} {m}")
