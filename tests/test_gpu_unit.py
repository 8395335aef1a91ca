"""The exact normalized() (Eigen `a / sqrt(a.a)`, reference/3dGeomUtil.h via bezierTriangle.cpp:164,233)
with one square root and a shared reciprocal (patch_math.hpp `unit`) returns the same bits as one
correctly rounded division per component, and as numpy's IEEE float32 arithmetic, over vectors whose
components span the whole float range (the guard's fallback included).  Called through the C-ABI test
hook bzr_debug_unit (include/bzr_debug.h)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _vectors(torch, n, gen, kind):
    if kind == "unitish":  # what the Newton site normalizes: tangent crosses, hit - plane point
        mag = torch.exp2(torch.empty(n, 1, device="cuda").uniform_(-40.0, 20.0, generator=gen))
        return (torch.randn(n, 3, device="cuda", generator=gen) * mag).T.contiguous()
    if kind == "wide":  # every exponent, both signs, per component
        e = torch.randint(-150, 128, (3, n), device="cuda", generator=gen).float()
        m = torch.empty(3, n, device="cuda").uniform_(1.0, 2.0, generator=gen)
        s = torch.randint(0, 2, (3, n), device="cuda", generator=gen).float() * 2 - 1
        return (s * m * torch.exp2(e)).float().contiguous()
    if kind == "zeros":  # axis-aligned and signed-zero components
        v = torch.randn(3, n, device="cuda", generator=gen)
        z = torch.randint(0, 4, (3, n), device="cuda", generator=gen)
        v = torch.where(z == 0, torch.zeros_like(v), v)
        v = torch.where(z == 1, -torch.zeros_like(v), v)
        return v.contiguous()
    # guard edges: |a_k| near 2^-100, z near 2^-96 and 2^40
    base = torch.randn(3, n, device="cuda", generator=gen)
    pick = torch.randint(0, 4, (1, n), device="cuda", generator=gen).float()
    scale = torch.where(pick == 0, 2.0 ** -100, torch.where(pick == 1, 2.0 ** -48, torch.where(pick == 2, 2.0 ** 20, 2.0 ** -101)))
    jitter = torch.exp2(torch.empty(3, n, device="cuda").uniform_(-2.0, 2.0, generator=gen))
    return (base * scale * jitter).float().contiguous()


def _numpy_unit(a):
    x, y, z = a.astype(np.float32)
    with np.errstate(all="ignore"):
        zz = x * x + (y * y + z * z)
        s = np.sqrt(zz)
        out = np.stack([x / s, y / s, z / s])
    keep = ~(zz > 0)
    out[:, keep] = a[:, keep]
    return out


@pytest.mark.parametrize("kind", ["unitish", "wide", "zeros", "edges"])
def test_shared_reciprocal_unit_is_bit_exact(bzr, ctx, kind):
    torch = pytest.importorskip("torch")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234 + len(kind))
    L = bzr.lib()
    n = 1 << 22
    ctx.use_torch_stream()
    for rep in range(4):
        a = _vectors(torch, n, gen, kind)
        out = torch.empty(6, n, device="cuda")
        assert L.bzr_debug_unit(ctx.handle, ctypes.c_void_p(a.data_ptr()), n, ctypes.c_void_p(out.data_ptr())) == 0
        torch.cuda.synchronize()
        got, ref = out[:3].view(torch.int32), out[3:].view(torch.int32)
        bad = (got != ref).any(dim=0)
        assert int(bad.sum()) == 0, (kind, rep, a[:, bad][:, :4].cpu().numpy(), out[:, bad][:, :4].cpu().numpy())
        if rep == 0:  # IEEE float32 on the CPU: the oracle's arithmetic
            k = 1 << 16
            host = a[:, :k].cpu().numpy()
            want = _numpy_unit(host)
            gotk = out[:3, :k].cpu().numpy()
            same = (gotk.view(np.uint32) == want.view(np.uint32)) | (np.isnan(gotk) & np.isnan(want))
            assert same.all(), (kind, host[:, ~same.all(axis=0)][:, :4])


def _heights(torch, n, gen, kind):
    """(hIn, hOut, cos) rows: the dome heights are record constants, cos a lane's plane cosine."""
    if kind == "lens":  # what the Newton site sees: heights ~1e-3..1, |cos| in [1e-5, 1]
        h = torch.exp2(torch.empty(2, n, device="cuda").uniform_(-12.0, 0.0, generator=gen))
        h = h * (torch.randint(0, 2, (2, n), device="cuda", generator=gen).float() * 2 - 1)
        c = torch.exp2(torch.empty(1, n, device="cuda").uniform_(-16.6, 0.0, generator=gen))
        c = c * (torch.randint(0, 2, (1, n), device="cuda", generator=gen).float() * 2 - 1)
        return torch.cat([h, c]).contiguous()
    if kind == "edge":  # the whole proven range and its edges, every lane inside it (see _in_fast_range)
        pick = torch.randint(0, 4, (3, n), device="cuda", generator=gen)
        m = torch.empty(3, n, device="cuda").uniform_(1.0, 2.0, generator=gen).clamp_(max=2.0 - 2.0 ** -23)
        m = torch.where(pick == 0, torch.ones_like(m), m)
        m = torch.where(pick == 1, torch.full_like(m, 1.0 + 2.0 ** -23), m)
        m = torch.where(pick == 2, torch.full_like(m, 2.0 - 2.0 ** -23), m)
        e = torch.cat([torch.randint(-40, 41, (2, n), device="cuda", generator=gen),
                       torch.randint(-20, 21, (1, n), device="cuda", generator=gen)])
        m[2] = torch.where(e[2] == 20, torch.ones_like(m[2]), m[2])  # |cos| <= 2^20: that exponent holds 2^20 alone
        s = torch.randint(0, 2, (3, n), device="cuda", generator=gen).float() * 2 - 1
        v = torch.ldexp(s * m, e).float()
        # a fixed block pairs the extremes: |h| just below 2^41 over 2^-20, and 2^-40 over 2^20 (both signs)
        big, tiny = (2.0 - 2.0 ** -23) * 2.0 ** 40, 2.0 ** -40
        sign = torch.tensor([1.0, -1.0], device="cuda").repeat(64)
        sign2 = torch.tensor([1.0, 1.0, -1.0, -1.0], device="cuda").repeat(32)
        v[0, 0:128], v[1, 0:128], v[2, 0:128] = big * sign, -big, 2.0 ** -20 * sign2
        v[0, 128:256], v[1, 128:256], v[2, 128:256] = tiny * sign, -tiny, 2.0 ** 20 * sign2
        v[0, 256:384], v[1, 256:384], v[2, 256:384] = big * sign, tiny, -(2.0 ** -20)
        v[0, 384:512], v[1, 384:512], v[2, 384:512] = tiny, big * sign, 2.0 ** 20
        return v.contiguous()
    # every exponent (the guard's fallback), zeros of both signs
    e = torch.randint(-150, 128, (3, n), device="cuda", generator=gen).float()
    m = torch.empty(3, n, device="cuda").uniform_(1.0, 2.0, generator=gen)
    s = torch.randint(0, 2, (3, n), device="cuda", generator=gen).float() * 2 - 1
    v = (s * m * torch.exp2(e)).float()
    z = torch.randint(0, 16, (3, n), device="cuda", generator=gen)
    v = torch.where(z == 0, torch.zeros_like(v), torch.where(z == 1, -torch.zeros_like(v), v))
    return v.contiguous()


def _in_fast_range(torch, a):
    """div_heights' test for the shared-reciprocal chain, per element, as patch_math.hpp states it: both heights'
    biased exponents in 87..167 (2^-40 <= |h| < 2^41) and 2^-20 <= |cos| <= 2^20."""
    e = (a[:2].view(torch.int32) >> 23) & 0xFF
    c = a[2].abs()
    return ((e - (127 - 40) >= 0) & (e - (127 - 40) <= 80)).all(dim=0) & (c >= 2.0 ** -20) & (c <= 2.0 ** 20)


@pytest.mark.parametrize("kind", ["lens", "wide", "edge"])
def test_shared_reciprocal_heights_are_bit_exact(bzr, ctx, kind):
    """newton_tail's din = hIn / cos, dout = hOut / cos (reference/bezierTriangle.cpp:132-133) with one shared
    reciprocal (patch_math.hpp div_heights) == one correctly rounded division each == numpy float32.  The chain
    runs only when a whole wave is in its proven range: "wide" almost never gives such a wave and "lens" stays far
    from the range's edges, so "edge" puts every lane inside it (asserted before the launch: every wave takes the
    chain), exponents uniform over the whole range, the mantissas 1, 1 + 2^-23, 2 - 2^-23 and random, the exact
    bounds 2^-20 and 2^20 of |cos| and a block of lanes with the extreme quotients."""
    torch = pytest.importorskip("torch")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4321 + len(kind))
    L = bzr.lib()
    n = 1 << 22
    ctx.use_torch_stream()
    for rep in range(4):
        a = _heights(torch, n, gen, kind)
        if kind == "edge":
            assert bool(_in_fast_range(torch, a).all()) and not bool((a == 0).any())
            assert bool((a[2].abs() == 2.0 ** -20).any()) and bool((a[2].abs() == 2.0 ** 20).any())
            assert bool((a < 0).any(dim=1).all()) and bool((a > 0).any(dim=1).all())
        out = torch.empty(4, n, device="cuda")
        assert L.bzr_debug_div_heights(ctx.handle, ctypes.c_void_p(a.data_ptr()), n, ctypes.c_void_p(out.data_ptr())) == 0
        torch.cuda.synchronize()
        got, ref = out[:2].view(torch.int32), out[2:].view(torch.int32)
        bad = (got != ref).any(dim=0) & ~(torch.isnan(out[:2]).any(dim=0) & torch.isnan(out[2:]).any(dim=0))
        assert int(bad.sum()) == 0, (kind, rep, a[:, bad][:, :4].cpu().numpy())
        if rep == 0:
            k = 1 << 16
            host = a[:, :k].cpu().numpy()
            with np.errstate(all="ignore"):
                want = np.stack([host[0] / host[2], host[1] / host[2]]).astype(np.float32)
            gotk = out[:2, :k].cpu().numpy()
            same = (gotk.view(np.uint32) == want.view(np.uint32)) | (np.isnan(gotk) & np.isnan(want))
            assert same.all(), (kind, host[:, ~same.all(axis=0)][:, :4])


# ------------------------------------------------------------------ BZR_MODE_FAST's primitives
U = 2.0 ** -23
FAST_DIV_REL = 1.5 * U    # v_rcp_f32's 1 ulp, then one rounded product
FAST_SQRT_REL = U         # v_sqrt_f32's 1 ulp
FAST_UNIT_REL = 2.5 * U   # v_rsq_f32's 1 ulp, one rounded product, half of z's three roundings (0.75 U)


def _fast_unit(bzr, ctx, torch, a):
    n = a.shape[1]
    out = torch.empty(5, n, device="cuda")
    assert bzr.lib().bzr_debug_fast_unit(ctx.handle, ctypes.c_void_p(a.data_ptr()), n, ctypes.c_void_p(out.data_ptr())) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _fast_operands(torch, n, gen, kind):
    """[3, n] operands with every result of its kind in the normal range."""
    sign = lambda *shape: torch.randint(0, 2, shape, device="cuda", generator=gen).float() * 2 - 1  # noqa: E731
    mant = lambda *shape: torch.empty(*shape, device="cuda").uniform_(1.0, 2.0, generator=gen).clamp_(max=2.0 - U)  # noqa: E731
    if kind == "div_wide":  # every divisor exponent with a normal reciprocal, quotients over 2^-121 .. 2^121
        eb = torch.randint(-125, 126, (n,), device="cuda", generator=gen)
        ea = (eb + torch.randint(-120, 121, (n,), device="cuda", generator=gen)).clamp_(-125, 126)
        a = torch.ldexp(sign(n) * mant(n), ea)
        b = torch.ldexp(sign(n) * mant(n), eb)
        return torch.stack([a, b, torch.ones_like(a)]).float().contiguous()
    if kind == "sqrt_wide":  # every normal exponent
        a = torch.ldexp(sign(n) * mant(n), torch.randint(-126, 128, (n,), device="cuda", generator=gen))
        return torch.stack([a, torch.ones_like(a), torch.ones_like(a)]).float().contiguous()
    if kind == "unit_wide":  # a common exponent in -58 .. 58, Gaussian components (the test keeps the normal z = a.a)
        e = torch.randint(-58, 59, (1, n), device="cuda", generator=gen)
        return torch.ldexp(torch.randn(3, n, device="cuda", generator=gen), e).float().contiguous()
    # lens-like: what the Newton site divides and normalizes, magnitudes 2^-12 .. 2^4
    return (sign(3, n) * torch.exp2(torch.empty(3, n, device="cuda").uniform_(-12.0, 4.0, generator=gen))).float().contiguous()


@pytest.mark.parametrize("kind", ["div_wide", "sqrt_wide", "unit_wide", "lens"])
def test_fast_primitives_against_float64(bzr, ctx, kind):
    """fast::div_rn, fast::sqrt_rn and fast::normalized (patch_math.hpp; v_rcp_f32, v_sqrt_f32, v_rsq_f32 at the
    documented 1 ulp) against numpy float64, 2^22 operands per kind with every result in the normal range.  A bound
    exceeded here is a finding about the documented 1 ulp: the message names the operand."""
    torch = pytest.importorskip("torch")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(977 + len(kind))
    n = 1 << 22
    ctx.use_torch_stream()
    a = _fast_operands(torch, n, gen, kind)
    got = _fast_unit(bzr, ctx, torch, a).astype(np.float64)
    h = a.cpu().numpy().astype(np.float64)
    tiny = float(np.finfo(np.float32).tiny)

    def check(label, g, ref, bound, ops):
        g, ref = np.atleast_2d(g), np.atleast_2d(ref)
        assert (np.abs(ref) >= tiny).all() and (np.abs(ref) <= 3.4e38).all(), label
        rel = np.abs(g - ref) / np.abs(ref)
        rel[~np.isfinite(g)] = np.inf
        k = int(np.argmax(rel.max(axis=0)))
        print(f"{kind} {label}: max relative error {rel.max() / U:.3f} x 2^-23 (bound {bound / U} x 2^-23) at operand "
              f"{ops[:, k]!r}")
        assert rel.max() <= bound, (label, ops[:, k], g[:, k], ref[:, k])

    if kind in ("div_wide", "lens"):
        check("div", got[0], h[0] / h[1], FAST_DIV_REL, h)
    if kind in ("sqrt_wide", "lens"):
        check("sqrt", got[1], np.sqrt(np.abs(h[0])), FAST_SQRT_REL, h)
    if kind in ("unit_wide", "lens"):
        z = (h * h).sum(axis=0)
        ref = h / np.sqrt(z)
        # the normal range: z (v_rsq_f32 takes a denormal z for 0 and returns inf) and every component of the result
        keep = (z >= 2.0 * tiny) & (z <= 1e38) & (np.abs(ref) >= tiny).all(axis=0)
        assert keep.mean() > 0.999
        check("unit", got[2:5][:, keep], ref[:, keep], FAST_UNIT_REL, h[:, keep])


def test_fast_unit_or_self_keeps_a_without_a_positive_z(bzr, ctx):
    """fast::unit_or_self returns `a` unchanged when z = a.a is 0 or NaN (Eigen's normalized()).  The operands outside
    the normal range (a denormal or overflowing z, a divisor below 2^-126 or above 2^126) are printed, not asserted:
    DESIGN.md (a) records what the hardware returns."""
    torch = pytest.importorskip("torch")
    ctx.use_torch_stream()
    nan = float("nan")
    keep = np.array([[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [nan, 1.0, 2.0], [1.0, nan, -2.0], [3.0, 4.0, nan],
                     [nan, nan, nan]], np.float32).T
    got = _fast_unit(bzr, ctx, torch, torch.from_numpy(np.ascontiguousarray(keep)).cuda())
    assert np.array_equal(got[2:5].view(np.uint32), keep.view(np.uint32))
    f = np.float32
    outside = {
        "z denormal (|a| = 2^-70 x (1, 1, 1))": [f(2.0) ** -70] * 3,
        "z underflows to 0 (|a| = 2^-80 x (3, 4, 12))": [f(3 * 2.0 ** -80), f(4 * 2.0 ** -80), f(12 * 2.0 ** -80)],
        "z overflows (|a| = 2^64 x (3, 4, 12))": [f(3 * 2.0 ** 64), f(4 * 2.0 ** 64), f(12 * 2.0 ** 64)],
        "divisor 2^-127 (denormal)": [f(1.0), f(2.0) ** -127, f(1.0)],
        "divisor 2^-140 (denormal)": [f(1.0), f(2.0) ** -140, f(1.0)],
        "divisor 2^127 under 1": [f(1.0), f(2.0) ** 127, f(1.0)],
        "divisor 2^127 under 2^100": [f(2.0) ** 100, f(2.0) ** 127, f(1.0)],
        "divisor 1.5 x 2^126 under 3": [f(3.0), f(1.5 * 2.0 ** 126), f(1.0)],
    }
    ops = np.ascontiguousarray(np.array(list(outside.values()), np.float32).T)
    res = _fast_unit(bzr, ctx, torch, torch.from_numpy(ops).cuda())
    for k, name in enumerate(outside):
        print(f"{name}: a = {ops[:, k]!r} -> div {res[0, k]!r}, sqrt {res[1, k]!r}, unit {res[2:5, k]!r}")
