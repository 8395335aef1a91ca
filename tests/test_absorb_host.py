"""Absorption, the parts that need no GPU: the entry points' declaration, export and binding, the Beer-Lambert text on
the host against its numpy restatement, the argument checks and the transmittance helper.
"""
import ctypes
import math
import re

import numpy as np
import pytest

import absorb_ref
from conftest import REPO

F = np.float32
SYMBOLS = ("bzr_trace_chain_absorb", "bzr_illuminate_media", "bzr_absorption_from_transmittance", "bzr_debug_attenuation")


def test_symbols_are_declared_exported_and_bound(bzr):
    lib = ctypes.CDLL(str(bzr.LIB_PATH))
    header = (REPO / "include" / "bzr.h").read_text() + (REPO / "include" / "bzr_debug.h").read_text()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in bzr.exported_symbols(), name
        assert re.search(name + r"\(", header), name
    assert re.search(r"#define BZR_ABI_VERSION 2\b", header)
    assert re.search(r"bzr_status bzr_trace_chain_absorb\(bzr_ctx \*ctx, const bzr_mesh \*const \*lenses, "
                     r"const float \*ri_table,\s+const float \*gap_table, const float \*glass_absorb, "
                     r"const float \*gap_absorb,\s+uint32_t nlens, uint32_t nchan,", header)
    assert re.search(r"int32_t bzr_debug_attenuation\(void \*ctx, const float \*x, uint32_t n, float \*out\);", header)
    assert re.search(r"traceChainAbsorb\(", (REPO / "include" / "bzr" / "bzr.hpp").read_text())
    for f in (bzr.trace_chain_absorb, bzr.illuminate_media, bzr.absorption_from_transmittance, bzr.debug_attenuation):
        assert callable(f)
    assert bzr.lib().bzr_abi_version() == 2


def test_host_attenuation_is_the_restatement(bzr):
    x = absorb_ref.att_values()
    assert x.size == 1 << 20 and np.isnan(x).any() and np.isinf(x).any() and (x == 0).any()
    got = bzr.debug_attenuation(x)
    want = absorb_ref.att(x)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[x == 0][0] == 1 and (got[np.isnan(x) | np.isinf(x)] == 0).all()
    assert np.unique(got).size > 1 << 18


def test_arguments_are_checked_without_a_device(bzr):
    L = bzr.lib()
    table, gaps = np.full((1, 4), 1.3, F), np.full((2, 4), 1.333, F)
    o = np.full((6, 4), 7.0, F)
    w, p, q = np.full(4, 7.0, F), np.full(4, 7.0, F), np.full(4, 7.0, F)
    s = np.full(4, 7, np.uint32)
    rays = np.zeros((6, 4), F)

    def call(glass=None, gap=None, out_opl=p.ctypes.data, max_bounces=4):
        return L.bzr_trace_chain_absorb(None, None, table.ctypes.data, gaps.ctypes.data,
                                        glass.ctypes.data if glass is not None else None,
                                        gap.ctypes.data if gap is not None else None, 1, 4, rays.ctypes.data, None, None,
                                        None, 4, max_bounces, o.ctypes.data, w.ctypes.data, s.ctypes.data, None, None,
                                        out_opl, q.ctypes.data, 0)

    good = np.array([[0.0, 0.5, 2.0, 200.0]], F)
    assert call(good, good) == 1 and b"null context" in L.bzr_last_error()
    assert call(out_opl=None) == 1 and b"out_opl" in L.bzr_last_error()
    assert call(max_bounces=9) == 1 and b"max_bounces" in L.bzr_last_error()
    for bad in (-1e-3, np.inf, np.nan, -0.5):
        t = good.copy()
        t[0, 2] = bad
        assert call(t, good) == 1 and b"glass_absorb" in L.bzr_last_error(), bad
        assert call(good, t) == 1 and b"gap_absorb" in L.bzr_last_error(), bad
        assert call(None, t) == 1 and b"gap_absorb" in L.bzr_last_error(), bad
    assert (o == 7).all() and (w == 7).all() and (s == 7).all() and (p == 7).all() and (q == 7).all()
    assert L.bzr_debug_attenuation(None, None, 4, None) == 1


class _NoContext:
    handle = None


class _NoMesh:
    handle = None


@pytest.mark.parametrize("which", ("gap_table", "glass_absorb", "gap_absorb"))
@pytest.mark.parametrize("shape", [(3, 4), (1, 3), (4,)])
def test_wrappers_refuse_tables_of_the_wrong_shape(bzr, which, shape):
    rays = np.zeros((6, 4), F)
    tables = {"gap_table": np.ones((2, 4), F), "glass_absorb": np.zeros((1, 4), F), "gap_absorb": np.zeros((1, 4), F)}
    tables[which] = np.ones(shape, F)
    with pytest.raises(bzr.BzrError, match=which + " must be"):
        bzr.trace_chain_absorb(_NoContext(), [_NoMesh()], np.full((1, 4), 1.3, F), tables["gap_table"],
                               tables["glass_absorb"], tables["gap_absorb"], rays)
    with pytest.raises(bzr.BzrError, match=which + " must be"):
        bzr.illuminate_media(_NoContext(), [_NoMesh()], np.full((1, 4), 1.3, F), tables["gap_table"],
                             tables["glass_absorb"], tables["gap_absorb"], None, 64, None)


def test_absorption_from_transmittance(bzr):
    t = np.array([1.0, 0.999, 0.98, 0.5, 0.01, 1e-300], np.float64)
    for d in (10.0, 25.0, 0.3):
        got = bzr.absorption_from_transmittance(t, d)
        want = np.array([-math.log(v) / d for v in t], np.float64).astype(F)
        assert got.dtype == F and np.array_equal(got, want)
        assert got[0] == 0 and (got[1:] > 0).all()
    out = np.full(3, 7.0, F)

    def raw(ts, d):
        a = np.array(ts, np.float64)
        return bzr.lib().bzr_absorption_from_transmittance(a.ctypes.data, a.size, ctypes.c_double(d), out.ctypes.data)

    for ts, d in (([0.9, 0.0, 0.5], 10.0), ([0.9, -0.1, 0.5], 10.0), ([0.9, 1.0000001, 0.5], 10.0),
                  ([0.9, np.nan, 0.5], 10.0), ([0.9, 0.8, 0.5], 0.0), ([0.9, 0.8, 0.5], -1.0),
                  ([0.9, 0.8, 0.5], np.inf), ([0.9, 0.8, 0.5], np.nan), ([0.9, 1e-300, 0.5], 1e-40)):
        assert raw(ts, d) == 1, (ts, d)
        assert (out == 7).all(), (ts, d)
    assert raw([0.9, 0.8, 0.5], 10.0) == 0 and (out != 7).all()
    with pytest.raises(bzr.BzrError):
        bzr.absorption_from_transmittance([0.5, 2.0], 10.0)
