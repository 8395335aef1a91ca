"""illum64 (the binary64 emitter and landing step, written from include/bzr.h's text) pinned on the CPU: against the
oracle's orc.emit / orc.land, which the device equals bit for bit in the older illumination tests' one geometry, and
against the distribution the header claims.  The inputs are the ones tests/test_gpu_illum64.py runs on the device, so
what is asserted about them here (patch_near's share, the unsure share, K) holds there.

K: illum64.K_MARGIN = 32 passes test_landing_bounds_hold_the_oracle as it stands (it was not raised).
"""
import numpy as np
import pytest

import illum64
from illum64 import BELTS, FIRSTS, N_RAYS, TARGETS
from illum_tir_ref import lenses_of

F = np.float32


# ------------------------------------------------------------------ (a), (b): the emitter
@pytest.mark.parametrize("x", (illum64.OBLIQUE_X, illum64.FAR_X))
@pytest.mark.parametrize("belts", BELTS)
@pytest.mark.parametrize("first", FIRSTS)
def test_oracle_emit_is_emit64(orc, x, belts, first):
    em = illum64.emitter(orc, x, belts)
    rays, patch = orc.emit(em, first, N_RAYS)
    m = illum64.check_emit(em, first, rays, patch)
    print(f"x {x} belts {belts} first {first}: {m}")
    assert m["near"] <= 0.002


def test_emit64_ranges_are_independent():
    em = illum64.emitter(illum64.PLAIN)
    for first in FIRSTS[1:]:
        whole, part = illum64.emit64(em, first - 37, 300), illum64.emit64(em, first, 100)
        assert np.array_equal(whole.d[:, 37:137], part.d) and np.array_equal(whole.o[:, 37:137], part.o)
        assert np.array_equal(whole.patch[37:137], part.patch)
    # the 64-bit ray number matters: 2^32 apart is another ray
    a, b = illum64.emit64(em, 5, 64), illum64.emit64(em, 5 + 2 ** 32, 64)
    assert not np.array_equal(a.ci, b.ci) and not np.array_equal(a.a, b.a)


def test_stream_known_answers():
    """The splitmix64 finaliser's published test vector: the generator seeded with 0 returns mix64(k x golden) as its
    k-th output; the first three are fixed in the literature (Vigna's splitmix64.c)."""
    z = illum64.GOLDEN * np.arange(1, 4, dtype=np.uint64)
    assert [int(v) for v in illum64.mix64(z)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    # U(key, stream) with seed 0 hashes golden x (2 key + stream + 1): key 0, stream 0 is output 1, key 0 stream 1 is 2
    u, v = illum64.uniform2(0, np.array([0], np.uint64), 0)
    assert u[0] == (0xE220A8397B1DCDAF >> 40) / 2 ** 24 and v[0] == ((0xE220A8397B1DCDAF >> 16) & 0xFFFFFF) / 2 ** 24
    u, _ = illum64.uniform2(0, np.array([0, 1], np.uint64), 1)
    assert u[0] == (0x6E789E6AA1B965F4 >> 40) / 2 ** 24


# ------------------------------------------------------------------ (c): the distribution
def chi2(counts, expected):
    return float(((counts - expected) ** 2 / expected).sum())


def bar(dof):
    return dof + 6.0 * np.sqrt(2.0 * dof)


def table(x, y, k=8):
    ix, iy = np.minimum((x * k).astype(int), k - 1), np.minimum((y * k).astype(int), k - 1)
    return np.bincount(ix * k + iy, minlength=k * k)


@pytest.mark.parametrize("source", ("emit64", "oracle"))
@pytest.mark.parametrize("seed", (12345, 7, 2 ** 63 + 11))
def test_stream_is_the_claimed_distribution(orc, source, seed):
    n = 1 << 18
    em = illum64.emitter(orc, belts=16, seed=seed)
    ref = illum64.emit64(em, 0, n)
    if source == "emit64":
        ci, tf, a, b, patch = ref.ci, ref.tf, ref.a, ref.b, ref.patch
    else:  # read back from the oracle's float32 rays
        rays, patch = orc.emit(em, 0, n)
        r = rays.astype(np.float64)
        ci, tf = r[3], np.mod(np.arctan2(r[5], r[4]) / (2.0 * np.pi), 1.0)
        a, b = illum64.solve_ab(em, r[:3])
        assert np.abs(ci - ref.ci).max() < 1e-6
    assert (ci >= 0).all() and (ci < 1).all() and (tf >= 0).all() and (tf < 1).all()
    stats = {
        "ci": (chi2(np.bincount((ci * 64).astype(int), minlength=64), n / 64), 63),
        "tf": (chi2(np.bincount(np.minimum((tf * 64).astype(int), 63), minlength=64), n / 64), 63),
        "ci x tf": (chi2(table(ci, tf), n / 64), 63),
        "ci[j] x ci[j+1]": (chi2(table(ci[:-1], ci[1:]), (n - 1) / 64), 63),
    }
    # a point's (u, v) within its part, one sample per point
    firsts = np.arange(0, n, em.rays_per_point)
    u = np.clip(a[firsts] * em.parts_u - ref.pu[firsts], 0.0, 1.0 - 1e-12)
    v = np.clip(b[firsts] * em.parts_v - ref.pv[firsts], 0.0, 1.0 - 1e-12)
    stats["point (a, b)"] = (chi2(table(u, v), len(firsts) / 64), 63)
    print(source, seed, {k: round(s, 1) for k, (s, _) in stats.items()})
    for name, (s, dof) in stats.items():
        assert s <= bar(dof), (name, s, bar(dof))
    count = int(illum64.belt_counts(16)[0].sum())
    assert count == orc.Hemisphere(16).patch_count
    hist = np.bincount(np.asarray(patch).astype(np.int64), minlength=count)
    assert len(hist) == count and hist.min() > 0.5 * n / count and hist.max() < 1.6 * n / count


def test_belt_counts_are_the_reference_tables(orc):
    for belts in BELTS + (16, 4096):
        assert int(illum64.belt_counts(belts)[0].sum()) == orc.Hemisphere(belts).patch_count


# ------------------------------------------------------------------ (d), (e): landing
@pytest.fixture(scope="module")
def scene(bzr, orc):
    """The oblique emitter's rays through the cfg2 lens by the oracle's chain, once."""
    lens = lenses_of(bzr, "cfg2")
    rays, _ = orc.emit(illum64.emitter(orc), 0, N_RAYS)
    out, status, _ = orc.trace_chain(lens, [1.3], rays, threads=16)
    out.setflags(write=False), status.setflags(write=False)
    return out, status


def oracle_cells(orc, tg, rays, status):
    """orc.land's cell per ray (-1: not landed), one ray at a time."""
    cols = np.ascontiguousarray(rays.T)
    cell = np.full(rays.shape[1], -1, np.int64)
    hist = np.zeros((tg.bins_v, tg.bins_u), np.uint32)
    flat = hist.reshape(-1)
    two = np.array([2], np.uint32)
    for i in np.flatnonzero(status == 2):
        _, _, landed = orc.land(tg, cols[i].reshape(6, 1), two, hist)
        if landed:
            cell[i] = int(flat.argmax())
            flat[cell[i]] = 0
    return cell


@pytest.mark.parametrize("name", TARGETS)
def test_landing_bounds_hold_the_oracle(orc, scene, name):
    out, status = scene
    tg = illum64.target(orc, name)
    hist, exited, landed = orc.land(tg, out, status)
    b = illum64.bounds(tg, out, status)
    ld = b.landing
    assert exited == int(ld.exited.sum()) >= 5000
    share = b.unsure / exited
    print(f"{name}: exited {exited} landed {landed} unsure {b.unsure} ({100 * share:.3f} %), "
          f"sum(hi - lo) {int((b.hi - b.lo).sum())}")
    assert share <= 0.01
    assert (b.lo <= hist).all() and (hist <= b.hi).all()
    assert b.landed_lo <= landed <= b.landed_hi
    if name == "behind":
        assert landed == 0 and not b.hi.any()
        return
    assert landed >= 1000
    cell = oracle_cells(orc, tg, out, status)
    assert np.array_equal(np.bincount(cell[cell >= 0], minlength=hist.size).reshape(hist.shape), hist)
    on = cell >= 0
    assert (ld.cand[on] == cell[on, None]).any(axis=1).all()       # every oracle-landed ray is in a candidate cell
    assert ld.may_miss[ld.exited & ~on].all()                      # and every ray it drops may miss
    assert np.array_equal(cell[~ld.unsure], ld.cell[~ld.unsure])   # a sure ray is where binary64 puts it


def test_land64_against_hand_placed_rays():
    """Rays aimed in binary64 at chosen (a, b) of the tilted target land in the chosen cells: the u / v order, the map's
    row-major layout and the half-open edges."""
    tg = illum64.target(illum64.PLAIN, "tilted")
    org, au, av = (np.array(v, np.float64) for v in (tg.origin, tg.axis_u, tg.axis_v))
    ab = np.array([(0.3, 0.7), (21.9, 0.1), (0.1, 29.9), (11.2, 14.9), (-0.2, 5.0), (5.0, 30.2), (22.3, 1.0)])
    hits = org[None] + ab[:, :1] * au[None] + ab[:, 1:] * av[None]
    start = np.array([10.0, 1.0, -2.0])
    d = hits - start
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    rays = np.concatenate([np.repeat(start[:, None], len(ab), axis=1), d.T]).astype(F)
    ld = illum64.land64(tg, rays, np.full(len(ab), 2))
    cu, cv = 22.0 / 40, 30.0 / 24
    want = [int(b // cv) * 40 + int(a // cu) if 0 <= a < 22 and 0 <= b < 30 else -1 for a, b in ab]
    assert ld.cell.tolist() == want and not ld.unsure.any()
    back = rays.copy()
    back[3:] = -back[3:]
    assert (illum64.land64(tg, back, np.full(len(ab), 2)).cell == -1).all()   # t < 0
    assert (illum64.land64(tg, rays, np.zeros(len(ab))).cell == -1).all()      # not OUTSIDE


def swapped_is_transposed(orc, out, status, name):
    h, _, la = orc.land(illum64.target(orc, name), out, status)
    hs, _, ls = orc.land(illum64.target(orc, name + "_swapped"), out, status)
    assert hs.shape == h.shape[::-1] and la == ls >= 1000
    assert np.array_equal(hs, h.T)


def block_sums(a):
    return a.reshape(a.shape[:-2] + (a.shape[-2] // 2, 2, a.shape[-1] // 2, 2)).sum(axis=(-3, -1))


def test_exact_identities_on_the_oracle(orc, scene):
    out, status = scene
    for name in ("plain", "coarse", "tilted"):
        swapped_is_transposed(orc, out, status, name)
    for fine, coarse in (("plain", "coarse"), ("tilted20", "tilted20_coarse")):
        hf, _, lf = orc.land(illum64.target(orc, fine), out, status)
        hc, _, lc = orc.land(illum64.target(orc, coarse), out, status)
        assert lf == lc >= 1000 and np.array_equal(block_sums(hf), hc)


def test_bounds_per_key_and_flux(orc, scene):
    """bounds' bookkeeping: keys split the scalar maps, q = 2^32 turns counts into flux, landed_hi counts an unsure ray
    once."""
    out, status = scene
    tg = illum64.target(orc, "tilted")
    one = illum64.bounds(tg, out, status)
    key = np.arange(N_RAYS) % 3
    per = illum64.bounds(tg, out, status, key=key, nkey=3, landing=one.landing)
    assert np.array_equal(per.lo.sum(axis=0), one.lo) and np.array_equal(per.hi.sum(axis=0), one.hi)
    assert int(per.landed_lo.sum()) == one.landed_lo and int(per.landed_hi.sum()) == one.landed_hi
    w = np.ones(N_RAYS, F)
    fl = illum64.bounds(tg, out, status, q=illum64.q32(w), landing=one.landing)
    assert np.array_equal(fl.lo, one.lo << np.uint64(32)) and np.array_equal(fl.hi, one.hi << np.uint64(32))
    assert one.landed_hi - one.landed_lo <= one.unsure and int((one.hi - one.lo).sum()) <= 4 * one.unsure
    assert illum64.q32(np.array([0.0, 1.0, 0.5, 2.0 ** -32, 1.0 - 2.0 ** -24], F)).tolist() == \
        [0, 2 ** 32, 2 ** 31, 1, 2 ** 32 - 256]
