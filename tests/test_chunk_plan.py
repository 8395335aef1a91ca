"""The staged path's chunking rule (trace.hip chunk_for, exported as bzr_debug_chunk_plan) against a restatement.

The rule (DESIGN.md "Data layout"): the cap is what a quarter of the device's free memory holds at the workspace's
bytes per ray, in whole waves, at least one wave and at most 2^23 rays (free memory unknown, passed as 0: 2^23); a batch
that fits the cap is one chunk, a larger one is split into ceil(n / cap) equal chunks rounded up to whole waves, never
above the cap, the last one ragged.  Pure host arithmetic: no device is needed.
"""
import ctypes

import pytest

WAVE = 64
CEILING = 1 << 23                                       # trace.hip kChunk (kChunkLog2 = 23)
MAX_CAND = 40                                           # trace.hip kMaxCand
RAY_BYTES = MAX_CAND * (4 + 4 + 48 + 8 + 4) + (4 + 8 + 4)  # trace.hip kWorkBytesPerRay: per list slot cand, rank, slot,
#                                                         pair, fol; per ray count, key, ovf


def exactly(cap):
    """The fewest free bytes that give `cap`."""
    return 4 * RAY_BYTES * cap


FREE = sorted({0, 1, exactly(CEILING) * 2, exactly(CEILING) + 12345}
              | {exactly(c) + d for c in (64, 128, 192, 4096) for d in (0, -RAY_BYTES, RAY_BYTES, -1, 4 * RAY_BYTES)})


def cap_rule(free):
    if free == 0:
        return CEILING
    return min(CEILING, max(free // 4 // RAY_BYTES // WAVE * WAVE, WAVE))


def chunk_rule(n, cap):
    if n <= cap:
        return n
    pieces = -(-n // cap)
    return min(cap, -(-(-(-n // pieces)) // WAVE) * WAVE)


def n_values(cap):
    return sorted({1, 63, 64, 65, cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1, 10007 * cap + 5, 2 ** 32 - 1, 2 ** 40})


def plan(bzr, free, n):
    cap, chunk = ctypes.c_uint32(0), ctypes.c_uint32(0)
    assert bzr.lib().bzr_debug_chunk_plan(free, n, ctypes.byref(cap), ctypes.byref(chunk)) == 0
    return cap.value, chunk.value


def test_the_free_byte_values_give_the_caps_they_claim():
    for c in (64, 128, 192, 4096):
        assert cap_rule(exactly(c)) == c and cap_rule(exactly(c) - 1) == max(c - WAVE, WAVE)
        assert cap_rule(exactly(c) - RAY_BYTES) == max(c - WAVE, WAVE) and cap_rule(exactly(c) + RAY_BYTES) == c
    assert cap_rule(0) == cap_rule(FREE[-1]) == CEILING and cap_rule(1) == WAVE
    assert len({cap_rule(f) for f in FREE}) >= 6


@pytest.mark.parametrize("free", FREE)
def test_chunk_plan_follows_the_rule(bzr, free):
    want_cap = cap_rule(free)
    for n in n_values(want_cap):
        cap, chunk = plan(bzr, free, n)
        label = f"free {free}, n {n}: cap {cap}, chunk {chunk}"
        assert cap == want_cap and chunk == chunk_rule(n, cap), label
        assert cap % WAVE == 0 and cap >= WAVE, label
        assert 0 < chunk <= cap, label
        count = -(-n // chunk)
        assert count * chunk >= n, label
        assert n - (count - 1) * chunk > 0, label           # the last chunk is not empty
        if n <= cap:
            assert count == 1 and chunk == n, label
        else:
            assert chunk % WAVE == 0, label
            assert count == -(-n // cap), label             # no more chunks than the cap forces
            assert chunk - WAVE < n / count, label          # equal chunks: within a wave of n / count


def test_chunk_plan_rejects_null_outputs(bzr):
    c = ctypes.c_uint32(0)
    assert bzr.lib().bzr_debug_chunk_plan(1 << 30, 1000, None, ctypes.byref(c)) == 1
    assert bzr.lib().bzr_debug_chunk_plan(1 << 30, 1000, ctypes.byref(c), None) == 1
