"""k_trace's near-first pass order on the device: bzr_debug_pass_order (include/bzr_debug.h) feeds one wave per key
sequence through batch_append -- the insertion trace_segment runs while it collects a batch of leaves -- and returns
the batch in the order its passes would run, each entry with the patch index and the gate ballot it was collected with.

That order must be numpy.argsort(kind="stable") of the keys: ascending, ties in collection order.  The key sets: every
length from 1 to 16, all keys equal, strictly descending, two equal pairs, keys that differ only in the last bit, and
256 random sequences (fixed seed; half of them drawn from 4 values, so ties are common).  One launch for all of them.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENTRIES = 16
BALLOT = 0x9E3779B97F4A7C15  # the hook's ballot of entry e: BALLOT * (e + 1) mod 2^64
ONE = 0x3F800000             # 1.0f: the keys are the raw bits of positive floats


def key_sets():
    rng = np.random.default_rng(20241)
    sets = []
    for n in range(1, ENTRIES + 1):  # every length, distinct keys in random order
        sets.append(("len%d" % n, rng.permutation(np.arange(ONE, ONE + n, dtype=np.uint32))))
    for n in (2, 5, 16):
        sets.append(("equal%d" % n, np.full(n, ONE, np.uint32)))
        sets.append(("descending%d" % n, np.arange(ONE + n, ONE, -1, dtype=np.uint32)))
    sets.append(("two_pairs", np.array([ONE + 9, ONE + 3, ONE + 9, ONE + 5, ONE + 3, ONE + 1], np.uint32)))
    sets.append(("two_pairs16", np.array([40, 7, 39, 38, 7, 37, 36, 35, 34, 40, 33, 32, 31, 30, 29, 28], np.uint32) + ONE))
    sets.append(("last_bit", np.array([ONE + 1, ONE, ONE + 1, ONE, ONE, ONE + 1, ONE + 1, ONE], np.uint32)))
    sets.append(("last_bit_high", np.array([0x7F800000, 0x7F7FFFFF, 0x7F800000, 0x7F7FFFFE, 1, 0], np.uint32)))
    for k in range(256):
        n = int(rng.integers(1, ENTRIES + 1))
        if k % 2:
            sets.append(("random%d" % k, rng.integers(ONE, ONE + 4, n).astype(np.uint32)))
        else:
            sets.append(("random%d" % k, rng.integers(1, 0x7F800000, n).astype(np.uint32)))
    return sets


def test_order_is_the_stable_argsort(bzr, ctx):
    torch = pytest.importorskip("torch")
    sets = key_sets()
    n = len(sets)
    keys = np.full((n, ENTRIES), 0xDEADBEEF, np.uint32)  # (past a sequence's length: never read as a key)
    lens = np.zeros(n, np.uint32)
    for w, (_, k) in enumerate(sets):
        keys[w, :len(k)] = k
        lens[w] = len(k)
    assert set(lens.tolist()) == set(range(1, ENTRIES + 1))
    d_keys = torch.from_numpy(keys.view(np.int32)).cuda()
    d_lens = torch.from_numpy(lens.view(np.int32)).cuda()
    d_out = torch.zeros((n, ENTRIES, 3), dtype=torch.int32, device="cuda")
    L = bzr.lib()
    ctx.use_torch_stream()
    assert L.bzr_debug_pass_order(ctx.handle, ctypes.c_void_p(d_keys.data_ptr()), ctypes.c_void_p(d_lens.data_ptr()), n,
                                  ctypes.c_void_p(d_out.data_ptr())) == 0, L.bzr_last_error()
    ctx.sync()
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    for w, (name, k) in enumerate(sets):
        want = np.argsort(k, kind="stable").astype(np.uint32)
        got = out[w, :len(k), 0]
        assert np.array_equal(got, want), f"{name}: keys {k} -> order {got}, want {want}"
        ballot = (want.astype(object) + 1) * BALLOT % (1 << 64)
        got_ballot = out[w, :len(k), 1].astype(object) | (out[w, :len(k), 2].astype(object) << 32)
        assert list(got_ballot) == list(ballot), f"{name}: the entries' ballots did not travel with them"
        assert (out[w, len(k):] == 0xFFFFFFFF).all(), f"{name}: places past the length"
