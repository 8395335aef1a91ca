"""The trace kernels' per-segment bundle setup (trace.hip bundle_setup_swap: a reduce-scatter on half-wave swaps)
returns, bit for bit, the 22 bundle words and the spread that the wave's rays define: per component the min / max
over the active, non-NaN lanes under the order-preserving integer map, the finite flag, the clamped and correctly
rounded reciprocals of the direction bounds and the mixed flags.  Called through the C-ABI test hook
bzr_debug_bundle_setup (include/bzr_debug.h) on about 40 waves: coherent and wide ones, single lanes, partial and
empty waves, NaN, +-inf, signed zeros, the clamps' and the finite flag's thresholds.

A second reference writes out the earlier kernel's semantics -- twelve independent reductions, each with its own
identity, then one lane's scalar code -- and must agree with the first on every wave, so the expectations do not
encode the kernel's own structure."""
import ctypes

import numpy as np
import pytest

F = np.float32
INT_MAX, INT_MIN = np.int32(0x7FFFFFFF), np.int32(-0x80000000)
TINY = F(1e-20)
BIG = F(1e30)


def _order(x):
    """float -> int32 with the floats' order (sign-magnitude to two's complement); its own inverse"""
    b = np.asarray(x, dtype=F).view(np.int32)
    return b ^ ((b >> 31) & INT_MAX)


def _unorder(v):
    v = np.asarray(v, dtype=np.int32)
    return (v ^ ((v >> 31) & INT_MAX)).view(F)


# ------------------------------------------------------------------ the waves
def _coherent(rng, jitter=0.01):
    s = (rng.normal(size=(3, 64)) * 0.1 + rng.normal(size=(3, 1))).astype(F)
    d = np.array([[0.0], [0.0], [1.0]]) + rng.normal(size=(3, 64)) * jitter
    d = (d / np.linalg.norm(d, axis=0)).astype(F)
    return np.concatenate([s, d]).astype(F)


def _waves():
    rng = np.random.default_rng(20261)
    out = []

    def add(name, rays, act=None):
        act = np.ones(64, np.uint8) if act is None else np.asarray(act, np.uint8)
        out.append((name, np.ascontiguousarray(rays, dtype=F), act))

    for k in range(6):  # random coherent waves, some lanes idle in half of them
        act = (rng.random(64) > 0.25) if k % 2 else np.ones(64, bool)
        add(f"coherent{k}", _coherent(rng), act)
    for lane in (0, 15, 16, 31, 32, 63):  # one active lane
        act = np.zeros(64, np.uint8)
        act[lane] = 1
        add(f"lane{lane}", _coherent(rng), act)
    lanes = np.arange(64)
    add("upper_half", _coherent(rng), lanes >= 32)
    add("row3", _coherent(rng), lanes >= 48)
    add("even_lanes", _coherent(rng), lanes % 2 == 0)
    add("odd_lanes", _coherent(rng), lanes % 2 == 1)
    add("empty", _coherent(rng), np.zeros(64))
    # NaN: whole components, every active lane of a partial wave, single lanes
    r = _coherent(rng); r[0] = np.nan; add("nan_sx", r)
    r = _coherent(rng); r[4] = np.nan; add("nan_dy", r)
    r = _coherent(rng); r[2] = np.nan; r[3] = np.nan; add("nan_partial", r, lanes % 3 == 0)
    for comp, lane in ((0, 0), (1, 17), (3, 40), (5, 63)):
        r = _coherent(rng); r[comp, lane] = np.nan; add(f"nan_c{comp}_l{lane}", r)
    r = _coherent(rng); r[5, 9] = np.nan; r[5, 10] = -3.0; add("nan_idle_lane", r, lanes != 9)
    # +-inf
    r = _coherent(rng); r[1, 5] = np.inf; r[2, 50] = -np.inf; add("inf_origin", r)
    r = _coherent(rng); r[3, 33] = np.inf; r[5] = -np.inf; add("inf_direction", r)
    # signed zeros in one component
    r = _coherent(rng); r[0] = np.where(lanes % 2 == 0, 0.0, -0.0); add("zeros_sx", r)
    r = _coherent(rng); r[4] = 0.0; r[4, 37] = -0.0; add("one_negzero_dy", r)
    r = _coherent(rng); r[4] = -0.0; r[4, 18] = 0.0; add("one_poszero_dy", r)
    r = _coherent(rng); r[3] = -0.0; add("all_negzero_dx", r)
    # direction components below 1e-20 of either sign (the clamps), and at the thresholds
    r = _coherent(rng); r[3] = rng.uniform(1e-26, 1e-24, 64); add("tiny_pos_dx", r)
    r = _coherent(rng); r[4] = -rng.uniform(1e-26, 1e-24, 64); add("tiny_neg_dy", r)
    r = _coherent(rng); r[3] = rng.uniform(-1e-30, 1e-30, 64); r[4] = 1e-40; r[5] = -1e-40; add("tiny_both", r)
    r = _coherent(rng); r[3] = TINY; r[4] = -TINY; r[5] = np.nextafter(TINY, F(1)); add("clamp_edges", r)
    r = _coherent(rng); r[3] = np.nextafter(TINY, F(0)); r[4] = np.nextafter(-TINY, F(-1)); add("clamp_edges2", r)
    # a component that straddles zero (the mixed flag); one of each sign beside it
    r = _coherent(rng); r[3] = rng.uniform(-0.3, 0.3, 64); r[4] = rng.uniform(0.1, 0.2, 64)
    r[5] = -rng.uniform(0.1, 0.2, 64); add("straddle_dx", r)
    r = _coherent(rng); r[5] = rng.uniform(-0.01, 0.01, 64); add("straddle_dz", r, lanes % 5 != 0)
    # magnitudes above 1e30 (finite flag 0), the threshold itself, and a huge idle lane
    r = _coherent(rng); r[2, 44] = 2e30; add("huge_sz", r)
    r = _coherent(rng); r[3, 3] = -1e38; add("huge_dx", r)
    r = _coherent(rng); r[1, 20] = BIG; r[4, 21] = -BIG; add("at_1e30", r)
    r = _coherent(rng); r[1, 20] = np.nextafter(BIG, F(np.inf)); add("above_1e30", r)
    r = _coherent(rng); r[0, 7] = 3e35; add("huge_idle_lane", r, lanes != 7)
    # wide bundles
    for k in range(2):
        r = _coherent(rng); r[3:] = rng.normal(size=(3, 64)); add(f"wide{k}", r)
    return out


WAVES = _waves()


# ------------------------------------------------------------------ reference 1: what the words mean
def _reference(rays, act):
    """min / max over the active, non-NaN lanes under the integer order; an idle lane stands for +inf (min) or
    -inf (max), a NaN lane for INT_MAX (min) or INT_MIN (max)"""
    act = act.astype(bool)
    w = np.zeros(23, F)
    for c in range(6):
        x = rays[c]
        ok = act & ~np.isnan(x)
        lo, hi = [_order(x[ok])], [_order(x[ok])]
        if (~act).any():
            lo.append(_order([np.inf])); hi.append(_order([-np.inf]))
        if (act & np.isnan(x)).any():
            lo.append(np.array([INT_MAX])); hi.append(np.array([INT_MIN]))
        base = 0 if c < 3 else 6
        w[base + c % 3] = _unorder(np.concatenate(lo).min())
        w[base + 3 + c % 3] = _unorder(np.concatenate(hi).max())
    b = w[:12]
    with np.errstate(all="ignore"):
        w[12] = 0.0 if (np.abs(b[~np.isnan(b)]) > BIG).any() else 1.0
        for a in range(3):
            dl, dh = w[6 + a], w[9 + a]
            lo = dl if dl > TINY else (-TINY if np.isnan(dl) else min(dl, -TINY))
            hi = dh if dh < -TINY else (TINY if np.isnan(dh) else max(dh, TINY))
            w[13 + a] = F(1.0) / F(lo)
            w[16 + a] = F(1.0) / F(hi)
            w[19 + a] = 1.0 if (lo < 0 and hi > 0) else 0.0
        w[22] = np.fmax(np.fmax(w[9] - w[6], w[10] - w[7]), w[11] - w[8])
    return w


# ------------------------------------------------------------------ reference 2: the earlier kernel, written out
def _reference_twelve(rays, act):
    """twelve independent reductions (each value selected by `act`, tested for NaN, mapped, reduced with its own
    identity, mapped back), then the code one lane ran: an fmaxf chain for the finite flag, the clamps, six
    divisions, the flags"""
    act = act.astype(bool)
    inf = F(np.inf)
    s, d = rays[:3], rays[3:]
    x = [np.where(act, s[0], inf), np.where(act, s[1], inf), np.where(act, s[2], inf),
         np.where(act, s[0], -inf), np.where(act, s[1], -inf), np.where(act, s[2], -inf),
         np.where(act, d[0], inf), np.where(act, d[1], inf), np.where(act, d[2], inf),
         np.where(act, d[0], -inf), np.where(act, d[1], -inf), np.where(act, d[2], -inf)]
    r = np.zeros(12, F)
    for i in range(12):
        mx = (0xE38 >> i) & 1
        v = np.where(x[i] == x[i], _order(x[i]), INT_MIN if mx else INT_MAX).astype(np.int32)
        acc = INT_MIN if mx else INT_MAX
        for lane in range(64):
            acc = max(acc, v[lane]) if mx else min(acc, v[lane])
        r[i] = _unorder(acc)
    w = np.zeros(23, F)
    with np.errstate(all="ignore"):
        m = F(0.0)
        for k in range(12):
            w[k] = r[k]
            m = np.fmax(m, np.abs(r[k]))
        w[12] = 1.0 if m <= BIG else 0.0
        for a in range(3):
            dl, dh = r[6 + a], r[9 + a]
            lo = dl if dl > TINY else np.fmin(dl, -TINY)
            hi = dh if dh < -TINY else np.fmax(dh, TINY)
            w[13 + a] = F(1.0) / lo
            w[16 + a] = F(1.0) / hi
            w[19 + a] = 1.0 if (lo < 0.0 and hi > 0.0) else 0.0
        w[22] = np.fmax(np.fmax(r[9] - r[6], r[10] - r[7]), r[11] - r[8])
    return w


REFERENCE = np.stack([_reference(r, a) for _, r, a in WAVES])


def _report(got, want):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    return [(WAVES[w][0], int(k), hex(got.view(np.uint32)[w, k]), hex(want.view(np.uint32)[w, k])) for w, k in bad[:12]]


def test_waves_cover_the_cases():
    assert 36 <= len(WAVES) <= 48
    ref = REFERENCE
    assert not np.isnan(ref[:, 22]).any()  # (a NaN spread's payload is the one thing the formats leave open)
    assert (ref[:, 12] == 0).any() and (ref[:, 12] == 1).any()
    assert (ref[:, 19:22] == 1).any() and (ref[:, 19:22] == 0).any()
    assert np.isnan(ref[:, :12]).any() and np.isinf(ref[:, :12]).any()
    assert (ref[:, 22] > 0.5).any() and (ref[:, 22] <= 0.5).any()  # both sides of the walk choice


def test_the_two_references_agree():
    twelve = np.stack([_reference_twelve(r, a) for _, r, a in WAVES])
    assert np.array_equal(twelve.view(np.uint32), REFERENCE.view(np.uint32)), _report(twelve, REFERENCE)


@pytest.mark.gpu
def test_bundle_words_are_bit_exact(bzr, ctx):
    torch = pytest.importorskip("torch")
    L = bzr.lib()
    ctx.use_torch_stream()
    n = 64 * len(WAVES)
    rays = torch.from_numpy(np.concatenate([r for _, r, _ in WAVES], axis=1).copy()).cuda().contiguous()
    act = torch.from_numpy(np.concatenate([a for _, _, a in WAVES])).cuda().contiguous()
    assert rays.shape == (6, n) and act.shape == (n,)
    out = torch.full((len(WAVES), 23), -7.0, device="cuda")
    assert L.bzr_debug_bundle_setup(ctx.handle, ctypes.c_void_p(rays.data_ptr()), ctypes.c_void_p(act.data_ptr()), n,
                                    ctypes.c_void_p(out.data_ptr())) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), REFERENCE.view(np.uint32)), _report(got, REFERENCE)
