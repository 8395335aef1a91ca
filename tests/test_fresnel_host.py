"""The Fresnel transmittance text the kernels run, evaluated on the host (bzr_debug_fresnel; no device).

The hook runs csrc/device/patch_math_body.inc's fresnel_t -- the text k_trace, k_finish, the brute-force scan and the
host single-ray path all compile -- for (eta, cos) pairs, with Snell's step's own s2 = eta^2 (1 - cos^2), and writes 0
where s2 >= 0.99 (no refraction).  The reference is the contract's formula in numpy float32 (tests/power_ref.py).
"""
import ctypes
import re

import numpy as np

import power_ref
from conftest import REPO

F = np.float32
ETA32 = np.array([F(1) / F(1.3), F(1.3), F(1) / F(1.5), F(1.5), F(1) / F(2.4), F(2.4)], F)


def want(eta, cs):
    t, s2 = power_ref.fresnel_t(eta, cs)
    return np.where(s2 < F(0.99), t, F(0)).astype(F), s2


def ulps(got32, want64):
    """|got - want| in units of the float32 spacing at want."""
    w = np.asarray(want64, np.float64)
    return np.abs(np.asarray(got32, np.float64) - w) / np.spacing(w.astype(F)).astype(np.float64)


def t64(eta, cs):
    """The closed form in float64."""
    eta, cs = np.asarray(eta, np.float64), np.asarray(cs, np.float64)
    c1 = np.abs(cs)
    c2 = np.sqrt(1.0 - eta * eta * (1.0 - cs * cs))
    rs = (eta * c1 - c2) / (eta * c1 + c2)
    rp = (eta * c2 - c1) / (eta * c2 + c1)
    return 1.0 - 0.5 * (rs * rs + rp * rp), c2


def edge_pairs():
    """cs = +-1 and its float32 neighbours (s2 = 0 and the smallest s2 > 0 float32 reaches, ~1.2e-7 eta^2: the two
    sides of 1e-12), and for eta > 1 the float32 cosines around s2 = 0.99."""
    eta, cs = [], []
    below = np.nextafter(F(1), F(0))
    for e in ETA32:
        for c in (F(1), F(-1), below, -below, np.nextafter(below, F(0))):
            eta.append(e)
            cs.append(c)
        if e > 1:
            c0 = F(np.sqrt(1.0 - 0.99 / float(e) ** 2))
            c = np.nextafter(c0, F(0))
            for _ in range(8):
                c = np.nextafter(c, F(0))
            for _ in range(33):  # 16 float32 neighbours on each side of the threshold's cosine
                for sign in (F(1), F(-1)):
                    eta.append(e)
                    cs.append(sign * c)
                c = np.nextafter(c, F(1))
    return np.array(eta, F), np.array(cs, F)


def test_hook_equals_the_float32_formula_bit_for_bit(bzr):
    rng = np.random.default_rng(20261019)
    n = 1 << 20
    eta = ETA32[rng.integers(0, len(ETA32), n)]
    cs = rng.uniform(-1.0, 1.0, n).astype(F)
    e_eta, e_cs = edge_pairs()
    eta, cs = np.concatenate([eta, e_eta]), np.concatenate([cs, e_cs])
    got = bzr.debug_fresnel(eta, cs)
    ref, s2 = want(eta, cs)
    bad = got.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), (int(bad.sum()), eta[bad][:4], cs[bad][:4], got[bad][:4], ref[bad][:4])
    # both sides of each threshold are in the sample, and the hook writes 0 exactly where Snell's step refuses
    e_s2 = s2[n:]
    assert (e_s2 >= F(0.99)).sum() > 20 and ((e_s2 < F(0.99)) & (e_s2 > F(0.98))).sum() > 20
    assert (e_s2 <= F(1e-12)).sum() >= 12 and ((e_s2 > F(1e-12)) & (e_s2 < F(1e-5))).sum() >= 12
    assert np.array_equal(got == 0, s2 >= F(0.99))
    assert (s2 >= F(0.99)).sum() > 1000  # eta > 1 at grazing incidence: the random sample reaches the refusal too
    # every transmittance of a refraction lies in (0, 1]
    t = got[s2 < F(0.99)]
    assert (t > 0).all() and (t <= 1).all()


def test_normal_incidence_is_the_closed_form(bzr):
    eta = np.repeat(ETA32, 2)
    cs = np.tile(np.array([1, -1], F), len(ETA32))
    got = bzr.debug_fresnel(eta, cs)
    e = eta.astype(np.float64)
    u = ulps(got, 4.0 * e / (1.0 + e) ** 2)
    print("normal incidence, ulp:", u)
    assert (u <= 2).all(), u
    # n = 1.3: the value the chain tests' maximum weight is the square of
    assert abs(float(got[2]) - 4 * 1.3 / 2.3 ** 2) < 1e-6


def test_reciprocity(bzr):
    """A path entering at cos(theta1) (eta = 1/n) and the same path reversed, leaving at cos(theta2) (eta = n),
    transmit the same fraction.  Each float32 value agrees with the float64 closed form of its own float32 inputs to
    8 ulp, and the two closed forms agree with each other (same n in float64) to 1e-12.

    The cases are the paths with 1 - s2 >= 1/2 in both directions, cos(theta1) in [0.72, 1]: there every intermediate
    is of order 1 with no cancellation worse than a factor 2 (|d c2| <= |d s2| / (2 c2), c2 >= 0.7), so a dozen
    correctly rounded float32 operations stay within 8 ulp of T >= 1/2.  Towards grazing angles 1 - s2 cancels (down
    to 0.01) and the float32 value legitimately moves away from the float64 one by tens of ulp (up to 97 leaving at
    n = 2.4, and far more entering near cos = 0, where T itself goes to 0), whatever evaluates the contract's operation
    order; the bit-for-bit test above covers those."""
    rng = np.random.default_rng(7)
    m = 100_000
    for n32 in (F(1.3), F(1.5), F(2.4)):
        c1 = rng.uniform(0.72, 1.0, m).astype(F)
        eta_in = np.full(m, F(1) / n32, F)
        fwd = bzr.debug_fresnel(eta_in, c1)
        fwd64, c2_64 = t64(eta_in, c1)
        c2 = c2_64.astype(F)
        eta_out = np.full(m, n32, F)
        rev = bzr.debug_fresnel(eta_out, c2)
        rev64, _ = t64(eta_out, c2)
        uf, ur = ulps(fwd, fwd64), ulps(rev, rev64)
        print(f"n = {float(n32):.1f}: forward max {uf.max():.2f} ulp, reversed max {ur.max():.2f} ulp")
        assert (fwd >= 0.5).all() and (rev >= 0.5).all()
        assert uf.max() <= 8 and ur.max() <= 8
        # physical reciprocity of the closed form itself: one n, both directions, in float64
        n64 = float(n32)
        a, c2x = t64(np.full(m, 1.0 / n64), c1)
        b, _ = t64(np.full(m, n64), c2x)
        assert np.abs(a - b).max() < 1e-12


def test_symbols_are_exported_and_bound(bzr):
    lib = ctypes.CDLL(str(bzr.LIB_PATH))
    for name in ("bzr_trace_chain_power", "bzr_illuminate_power", "bzr_debug_fresnel"):
        assert hasattr(lib, name), name
        assert name in bzr.exported_symbols(), name
    header = (REPO / "include" / "bzr.h").read_text()
    assert re.search(r"#define BZR_ABI_VERSION 2\b", header)
    assert (bzr.EMISSION_UNIFORM, bzr.EMISSION_LAMBERT, bzr.SURFACE_LOSSLESS, bzr.SURFACE_FRESNEL) == (0, 1, 0, 1)
    assert ctypes.sizeof(bzr.Radiometry) == 8
    # arguments are checked before any output is touched (no device needed)
    L = bzr.lib()
    assert L.bzr_illuminate_power(None, None, None, 1, None, 0, None, None, None, None, None, None, 0) == 1
    assert b"radiometry" in L.bzr_last_error()
    assert L.bzr_trace_chain_power(None, None, None, 1, None, None, 0, None, None, None, None, 1 << 7) == 1
    assert b"unknown flag" in L.bzr_last_error()
    assert L.bzr_debug_fresnel(None, None, 1, None) == 1
    assert bzr.flux_to_float(np.array([1 << 32, 1 << 31], np.uint64)).tolist() == [1.0, 0.5]
