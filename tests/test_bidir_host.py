"""bzr_bidir_uniform, the bidirectional walk's draw on the host (no GPU): against ghost_ref.uniform(seed, j, 256 +
segment) bit for bit, off bzr_ghost_uniform's draws, and the argument checks."""
import ctypes

import numpy as np
import pytest

import bidir_ref
import ghost_ref

F = np.float32
SEEDS = (0, 2024, 2 ** 64 - 1)
RAYS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5, 2 ** 64 - 1)
BOUND = (8 + 1) * (2 * 8 + 1)


def test_host_uniform_is_the_restatement(bzr):
    assert BOUND == 153 == bidir_ref.segment_bound(8, 8) and bidir_ref.DRAW_OFFSET == 256
    for seed in SEEDS:
        for ray in RAYS:
            for segment in range(BOUND + 1):
                got = bzr.bidir_uniform(seed, ray, segment)
                want = ghost_ref.uniform(seed, [ray], 256 + segment)[0]
                assert isinstance(got, F) and 0.0 <= got < 1.0
                assert got.view(np.uint32) == want.view(np.uint32), (seed, ray, segment)
                assert bidir_ref.uniform(seed, [ray], [segment])[0].view(np.uint32) == want.view(np.uint32)


def test_off_the_ghost_chains_draws(bzr):
    """The offset 256 lies above every e = 16 lens + reflections <= 135 of bzr_trace_chain_ghost, and segment 0 is not
    that call's draw 0."""
    assert 16 * 7 + 8 < 256
    same = sum(bzr.bidir_uniform(2024, j, 0) == bzr.ghost_uniform(2024, j, 0, 0) for j in range(512))
    assert same <= 1


def test_bad_arguments(bzr):
    u = ctypes.c_float(7.0)
    for segment in (BOUND + 1, 1000, 2 ** 31, 2 ** 32 - 1):
        assert bzr.lib().bzr_bidir_uniform(1, 2, segment, ctypes.byref(u)) == 1
        assert u.value == 7.0
    assert bzr.lib().bzr_bidir_uniform(1, 2, 0, None) == 1
    assert bzr.lib().bzr_bidir_uniform(1, 2, BOUND, ctypes.byref(u)) == 0 and u.value != 7.0
    with pytest.raises(bzr.BzrError):
        bzr.bidir_uniform(0, 0, BOUND + 1)
    assert bzr.RR_BACK == 4
