"""Surrounding media, the parts that need no GPU: the entry point's declaration, export and binding, its argument checks
and the Python wrapper's gap_table shape check.  (The reference itself is pinned in tests/test_media_ref.py.)
"""
import ctypes
import re

import numpy as np
import pytest

from conftest import REPO

F = np.float32


def test_symbol_is_declared_exported_and_bound(bzr):
    lib = ctypes.CDLL(str(bzr.LIB_PATH))
    assert hasattr(lib, "bzr_trace_chain_media")
    assert "bzr_trace_chain_media" in bzr.exported_symbols()
    header = (REPO / "include" / "bzr.h").read_text()
    assert re.search(r"#define BZR_ABI_VERSION 2\b", header)
    assert re.search(r"bzr_status bzr_trace_chain_media\(bzr_ctx \*ctx, const bzr_mesh \*const \*lenses, "
                     r"const float \*ri_table,\s+const float \*gap_table, uint32_t nlens, uint32_t nchan,", header)
    assert re.search(r"traceChainMedia\(", (REPO / "include" / "bzr" / "bzr.hpp").read_text())
    assert callable(bzr.trace_chain_media)
    assert bzr.lib().bzr_abi_version() == 2


def test_arguments_are_checked_without_a_device(bzr):
    """A null context, a NULL out_opl and a budget above the maximum are rejected before anything is touched (no device
    needed: the last two are refused ahead of the context check, as the error text shows)."""
    L = bzr.lib()
    table, gaps = np.full((1, 4), 1.3, F), np.full((2, 4), 1.333, F)
    o = np.full((6, 4), 7.0, F)
    w, p, q = np.full(4, 7.0, F), np.full(4, 7.0, F), np.full(4, 7.0, F)
    s = np.full(4, 7, np.uint32)
    rays = np.zeros((6, 4), F)

    def call(out_opl, max_bounces):
        return L.bzr_trace_chain_media(None, None, table.ctypes.data, gaps.ctypes.data, 1, 4, rays.ctypes.data, None, None,
                                       None, 4, max_bounces, o.ctypes.data, w.ctypes.data, s.ctypes.data, None, None,
                                       out_opl, q.ctypes.data, 0)

    assert call(p.ctypes.data, 4) == 1 and b"null context" in L.bzr_last_error()
    assert call(None, 4) == 1 and b"out_opl" in L.bzr_last_error()
    assert call(p.ctypes.data, 9) == 1 and b"max_bounces" in L.bzr_last_error()
    assert (o == 7).all() and (w == 7).all() and (s == 7).all() and (p == 7).all() and (q == 7).all()


class _NoContext:
    handle = None


class _NoMesh:
    handle = None


@pytest.mark.parametrize("shape", [(1, 4), (3, 4), (2, 3), (8,)])
def test_wrapper_refuses_a_gap_table_of_the_wrong_shape(bzr, shape):
    """gap_table must be [nlens + 1, nchan]: refused in Python, before the library is called."""
    rays = np.zeros((6, 4), F)
    with pytest.raises(bzr.BzrError, match="gap_table must be"):
        bzr.trace_chain_media(_NoContext(), [_NoMesh()], np.full((1, 4), 1.3, F), np.ones(shape, F), rays)
