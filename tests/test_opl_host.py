"""Optical path length, the parts that need no GPU: the reference itself (tests/opl_ref.py) against tir_ref's chain,
against the straight-line distance and against a float64 sum of its own legs, and the entry point's declaration,
export and argument checks.
"""
import ctypes
import re

import numpy as np
import pytest

import opl_ref
import tir_ref
from bzr_amd.configs import CONFIGS, build_lens, grid_rays
from conftest import REPO
from test_gpu_tir import NCHAN, SIDE, TABLES

F = np.float32
RR_OUTSIDE = 2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def scenes(bzr, orc):
    """name -> (patches, rays [6, 64^2], channel): computed once, never changed."""
    out = {}
    for name in TABLES:
        cfg = CONFIGS[name]
        lenses = [build_lens(bzr.TriMesh, lens).bezier_patches() for lens in cfg.lenses]
        rays = grid_rays(cfg, side=SIDE)
        channel = np.random.default_rng(7).integers(0, NCHAN, SIDE * SIDE).astype(np.uint8)
        rays.setflags(write=False)
        channel.setflags(write=False)
        out[name] = (lenses, rays, channel)
    return out


@pytest.mark.parametrize("max_bounces", (0, 4))
@pytest.mark.parametrize("name", list(TABLES))
def test_same_chain_as_tir_ref(orc, scenes, name, max_bounces):
    """The path adds to the chain and changes nothing in it: the first five outputs are tir_ref.chain's bit for bit."""
    lenses, rays, channel = scenes[name]
    w_in = np.random.default_rng(41).random(rays.shape[1], dtype=F)
    want = tir_ref.chain(orc, lenses, TABLES[name], rays, channel, w_in, max_bounces)
    got = opl_ref.chain(orc, lenses, TABLES[name], rays, channel, w_in, None, max_bounces)
    assert int((want[2] == RR_OUTSIDE).sum()) > 1500
    for k in range(5):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert got[5].dtype == F and got[6].dtype == F
    assert (got[6] <= got[5]).all()  # every index is above 1: the glass legs count at least once in opl
    assert (got[3][got[6] > 0] >= 2).all() and (got[6][got[2] == RR_OUTSIDE] > 0).all()  # glass: a second segment


@pytest.mark.parametrize("name", list(TABLES))
def test_straight_line_anchor(orc, scenes, name):
    """With every index 1.0 a ray goes straight, so its polyline's length is the distance between its input and output
    origins.  Over the rays that end OUTSIDE the reference is within 1e-5 relative of that distance in float64 (the
    polyline through the hit points: measured 1.3e-6 on cfg2, 3.2e-6 on cfg4; the reference implementation states 3e-6
    typical accuracy), while the same sum built from the hits' t is off by more than 1e-4 on some ray (measured up to
    1.1e-3 and 1.5e-3): t is BezierIntersection's value from before the last Newton step.  That is why the contract
    is not a sum of t."""
    lenses, rays, _ = scenes[name]
    extra = {}
    got = opl_ref.chain(orc, lenses, [[1.0]] * len(lenses), rays, None, None, None, 0, extra=extra)
    out = got[2] == RR_OUTSIDE
    assert int(out.sum()) >= 2700
    a, b = rays[0:3][:, out].astype(np.float64), got[0][0:3][:, out].astype(np.float64)
    dist = np.sqrt(((b - a) ** 2).sum(axis=0))
    assert (dist > 0).all()
    rel = np.abs(got[5][out].astype(np.float64) - dist) / dist
    rel_t = np.abs(extra["tsum"][out].astype(np.float64) - dist) / dist
    print(f"{name}: {int(out.sum())} rays OUTSIDE; polyline vs distance max {rel.max():.3g}, median {np.median(rel):.3g}; "
          f"sum of t vs distance max {rel_t.max():.3g}, median {np.median(rel_t):.3g}")
    assert rel.max() <= 1e-5
    assert rel_t.max() > 1e-4
    # with index 1 glass and air count alike: opl is the whole polyline, glass a proper part of it
    assert (got[6][out] > 0).all() and (got[6][out] < got[5][out]).all()


@pytest.mark.parametrize("name", list(TABLES))
def test_float32_accumulation(orc, scenes, name):
    """out_opl against the same legs measured and summed in float64 from the same float32 points: within
    8 segments 2^-24 relative.  Per leg the float32 form rounds: three subtractions (together at most one rounding's
    worth of relative error in the length), three products and two additions under the square root (at most three, halved
    by the root: 1.5), the square root (1), the product with the index (1) and the addition to the accumulator (1, of a
    sum of positive terms): under 6 roundings of 2^-24 per leg, and a ray has at most `segments` legs.  Measured:
    1.48e-7 at up to 9 segments."""
    lenses, rays, channel = scenes[name]
    extra = {}
    opl_in = (np.random.default_rng(13).random(rays.shape[1], dtype=F) * F(4)).astype(F)
    got = opl_ref.chain(orc, lenses, TABLES[name], rays, channel, None, opl_in, 4, extra=extra)
    moved = got[5] != opl_in
    assert int(moved.sum()) >= 2700 and int(got[3].max()) >= 6
    want = extra["opl64"]
    rel = np.abs(got[5].astype(np.float64) - want) / want
    bound = 8.0 * got[3].astype(np.float64) * 2.0 ** -24
    print(f"{name}: float32 vs float64 accumulation, max relative {rel[moved].max():.3g} at up to {int(got[3].max())} segments")
    assert (rel <= bound).all()
    assert np.array_equal(bits(got[5][~moved]), bits(opl_in[~moved])) and not got[6][~moved].any()


def test_symbol_is_declared_exported_and_bound(bzr):
    lib = ctypes.CDLL(str(bzr.LIB_PATH))
    assert hasattr(lib, "bzr_trace_chain_opl")
    assert "bzr_trace_chain_opl" in bzr.exported_symbols()
    header = (REPO / "include" / "bzr.h").read_text()
    assert re.search(r"#define BZR_ABI_VERSION 2\b", header)
    assert re.search(r"bzr_status bzr_trace_chain_opl\(", header)
    assert re.search(r"traceChainOpl\(", (REPO / "include" / "bzr" / "bzr.hpp").read_text())
    assert callable(bzr.trace_chain_opl)
    assert bzr.lib().bzr_abi_version() == 2


def test_arguments_are_checked_without_a_device(bzr):
    """A null context, a NULL out_opl and a budget above the maximum are rejected before anything is touched (no device
    needed: the last two are refused ahead of the context check, as the error text shows)."""
    L = bzr.lib()
    table = np.full((1, 4), 1.3, F)
    o = np.full((6, 4), 7.0, F)
    w, p, q = np.full(4, 7.0, F), np.full(4, 7.0, F), np.full(4, 7.0, F)
    s = np.full(4, 7, np.uint32)
    rays = np.zeros((6, 4), F)

    def call(out_opl, max_bounces):
        return L.bzr_trace_chain_opl(None, None, table.ctypes.data, 1, 4, rays.ctypes.data, None, None, None, 4,
                                     max_bounces, o.ctypes.data, w.ctypes.data, s.ctypes.data, None, None, out_opl,
                                     q.ctypes.data, 0)

    assert call(p.ctypes.data, 4) == 1 and b"null context" in L.bzr_last_error()
    assert call(None, 4) == 1 and b"out_opl" in L.bzr_last_error()
    assert call(p.ctypes.data, 9) == 1 and b"max_bounces" in L.bzr_last_error()
    assert (o == 7).all() and (w == 7).all() and (s == 7).all() and (p == 7).all() and (q == 7).all()
