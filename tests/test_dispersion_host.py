"""bzr_dispersion_index: refractive index from the Cauchy and Sellmeier formulas, on the host (no context, no device).

The contract: evaluated in binary64 and rounded once to float.  The reference is the same formula in numpy float64; the
N-BK7 coefficients and catalogue indices at the F, d and C lines are Schott's published ones.
"""
import ctypes
import re

import numpy as np
import pytest

from conftest import REPO

F = np.float32
BK7_B = (1.03961212, 0.231792344, 1.01046945)
BK7_C = (0.00600069867, 0.0200179144, 103.560653)
BK7 = [x for pair in zip(BK7_B, BK7_C) for x in pair]  # B1, C1, B2, C2, B3, C3
LINES = {"F": (0.4861327, 1.52237629, 1.52238), "d": (0.5875618, 1.51680003, 1.51680), "C": (0.6562725, 1.51432235, 1.51432)}


def sellmeier64(coeff, lam):
    lam = np.asarray(lam, np.float64)
    l2 = lam * lam
    n2 = np.ones_like(l2)
    for b, c in zip(coeff[0::2], coeff[1::2]):
        n2 = n2 + b * l2 / (l2 - c)
    return np.sqrt(n2)


def ulps(got32, want64):
    w = np.asarray(want64, np.float64)
    return np.abs(np.asarray(got32, np.float64) - w) / np.spacing(w.astype(F)).astype(np.float64)


def test_symbols_are_exported_and_bound(bzr):
    lib = ctypes.CDLL(str(bzr.LIB_PATH))
    for name in ("bzr_trace_chain_spectral", "bzr_illuminate_spectral", "bzr_dispersion_index"):
        assert hasattr(lib, name), name
        assert name in bzr.exported_symbols(), name
    header = (REPO / "include" / "bzr.h").read_text()
    assert re.search(r"#define BZR_ABI_VERSION 2\b", header)
    assert re.search(r"#define BZR_MAX_CHANNELS 64\b", header)
    assert (bzr.DISPERSION_CAUCHY, bzr.DISPERSION_SELLMEIER, bzr.MAX_CHANNELS) == (0, 1, 64)
    # arguments are checked before any output is touched (no device needed)
    L = bzr.lib()
    assert L.bzr_trace_chain_spectral(None, None, None, 1, 4, None, None, None, 0, None, None, None, None, 0) == 1
    assert b"context" in L.bzr_last_error()
    assert L.bzr_illuminate_spectral(None, None, None, 1, 4, None, 0, None, None, None, None, None, None, 0) == 1
    assert b"radiometry" in L.bzr_last_error()


def test_sellmeier_bk7(bzr):
    lam = np.array([v[0] for v in LINES.values()])
    got = bzr.dispersion_index(bzr.DISPERSION_SELLMEIER, BK7, lam)
    want = sellmeier64(BK7, lam)
    assert got.dtype == F and got.shape == lam.shape
    assert np.allclose(want, [v[1] for v in LINES.values()], rtol=0, atol=5e-9)  # the float64 values quoted above
    assert (ulps(got, want) <= 1.0).all(), (got, want)
    assert (np.abs(got.astype(np.float64) - [v[2] for v in LINES.values()]) < 5e-5).all()
    assert got[0] > got[1] > got[2]  # normal dispersion: blue bends more
    for terms in (1, 2):  # ncoeff 2 and 4
        got = bzr.dispersion_index(bzr.DISPERSION_SELLMEIER, BK7[:2 * terms], lam)
        assert (ulps(got, sellmeier64(BK7[:2 * terms], lam)) <= 1.0).all()


def test_cauchy_against_numpy(bzr):
    lam = np.linspace(0.38, 1.6, 123)
    a, b, c = 1.5046, 0.00420, 1.3e-5  # BK7-like Cauchy coefficients
    got = bzr.dispersion_index(bzr.DISPERSION_CAUCHY, [a, b, c], lam)
    want = a + b / lam ** 2 + c / lam ** 4
    assert (ulps(got, want) <= 1.0).all()
    got = bzr.dispersion_index(bzr.DISPERSION_CAUCHY, [a, b], lam.reshape(3, 41))
    assert got.shape == (3, 41) and (ulps(got, (a + b / lam ** 2).reshape(3, 41)) <= 1.0).all()
    assert bzr.dispersion_index(bzr.DISPERSION_CAUCHY, [a, b], np.zeros(0)).shape == (0,)


@pytest.mark.parametrize("model, coeff, lam, msg", [
    (2, [1.5, 0.004], [0.5], "model"),
    (-1, [1.5, 0.004], [0.5], "model"),
    (0, [1.5], [0.5], "ncoeff"),
    (0, [1.5, 0.004, 0.0, 0.0], [0.5], "ncoeff"),
    (1, BK7[:3], [0.5], "ncoeff"),
    (1, BK7 + [1.0, 2.0], [0.5], "ncoeff"),
    (0, [1.5, 0.004], [0.5, 0.0], "wavelength"),
    (0, [1.5, 0.004], [0.5, -0.6], "wavelength"),
    (1, BK7, [0.5, np.nan], "wavelength"),
    (1, BK7, [np.inf, 0.5], "wavelength"),
    (0, [1.5, 1e300], [0.5, 1e-160], "finite"),            # B / l^2 overflows binary64
    (0, [1e39, 0.004], [0.5], "finite"),                   # finite in binary64, not in binary32
    (1, [1.0, 0.25], [0.4, 0.5], "Sellmeier|finite"),      # l^2 = C1: a pole
    (1, [1.0, 0.36], [0.5], "Sellmeier"),                  # n^2 = 1 + 0.25 / (0.25 - 0.36) < 0
    (1, [-1.0, 0.0], [0.5], "Sellmeier"),                  # n^2 = 0
])
def test_rejections_leave_the_output_untouched(bzr, model, coeff, lam, msg):
    c = np.asarray(coeff, np.float64)
    w = np.asarray(lam, np.float64)
    out = np.full(w.shape, 7.0, F)
    assert bzr.lib().bzr_dispersion_index(model, c.ctypes.data, c.size, w.ctypes.data, w.size, out.ctypes.data) == 1
    assert re.search(msg, bzr.lib().bzr_last_error().decode())
    assert (out == 7).all()
    with pytest.raises(bzr.BzrError, match=msg):
        bzr.dispersion_index(model, coeff, lam)
