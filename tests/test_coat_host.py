"""The coating's two host functions (no GPU): bzr_coat_transmittance against coat_ref.coat_t bit for bit, and
bzr_coating_reflectance against coat_ref.reflectance64, known answers and every refusal.

The bare row (nlayers = 0) looked up through coat_t against 1 - fresnel_t in binary64 over mu in [0, 1], for 1.5168 in
air with BZR_COAT_SAMPLES = 129, measured and printed by test_bare_row_interpolation_error (not asserted against a
number chosen in advance): the maximum error is 2.9e-4 over all of [0, 1], 2.7e-4 for mu >= 1/128 and 1.4e-4 for
mu >= 0.1.
"""
import ctypes

import numpy as np
import pytest

import coat_ref

F = np.float32
QW = 0.55 / (4 * 1.38)  # a quarter wave of MgF2 at 0.55 um


def special_mu():
    grid = (np.arange(129) / 128.0).astype(F)
    below = np.nextafter(grid[1:], F(0))
    return np.concatenate([[F(0), F(1)], grid, below, [F(1) + F(2.0 ** -23)]]).astype(F)


def test_symbols(bzr):
    for name in ("bzr_trace_chain_coated", "bzr_illuminate_coated", "bzr_coat_transmittance", "bzr_coating_reflectance"):
        assert name in bzr.exported_symbols(), name
        assert hasattr(bzr.lib(), name), name
    assert bzr.COAT_SAMPLES == 129 == coat_ref.SAMPLES
    assert bzr.lib().bzr_abi_version() == 2


def test_transmittance_is_the_restatement(bzr):
    rng = np.random.default_rng(11)
    mu = np.concatenate([rng.random(2 ** 16, dtype=F), special_mu()])
    rows = [rng.random(129, dtype=F), np.zeros(129, F), np.ones(129, F), (np.arange(129) % 2).astype(F)]
    rows[0][rng.integers(0, 129, 8)] = F(1)
    rows[0][rng.integers(0, 129, 8)] = F(0)
    for row in rows:
        got = bzr.coat_transmittance(row, mu)
        want = coat_ref.coat_t(row, mu)
        assert got.dtype == F and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert (got >= 0).all() and (got <= 1).all()  # no clamp in the lookup: the header's argument
    assert (bzr.coat_transmittance(rows[1], mu) == 1).all() and (bzr.coat_transmittance(rows[2], mu) == 0).all()
    assert isinstance(bzr.coat_transmittance(rows[0], 0.5), F)
    # the one-cosine entry point and the batched one are the same compilation
    for m in special_mu():
        assert bzr.coat_transmittance(rows[0], float(m)).view(np.uint32) == coat_ref.coat_t(rows[0], [m])[0].view(np.uint32)
    out = np.full(3, 7.0, F)
    batch = bzr.lib().bzr_debug_coat_transmittance
    for bad in (np.array([0.5, np.nan, 0.2], F), np.array([0.5, 0.1, -0.2], F)):
        assert batch(rows[0].ctypes.data, bad.ctypes.data, 3, out.ctypes.data) == 1 and (out == 7).all()
    assert batch(None, out.ctypes.data, 3, out.ctypes.data) == 1 and batch(rows[0].ctypes.data, None, 3, out.ctypes.data) == 1
    assert batch(rows[0].ctypes.data, out.ctypes.data, 3, None) == 1 and batch(None, None, 0, None) == 0


STACKS = [
    (1.0, 1.5168, [], [], 0.55),
    (1.0, 1.5168, [1.38], [QW], 0.55),
    (1.0, 1.5168, [1.38], [QW], 0.45),
    (1.333, 1.8, [1.38], [QW], 0.65),
    (1.0, 1.62, [1.38, 2.1, 1.63], [QW, 0.55 / (2 * 2.1), 0.55 / (4 * 1.63)], 0.55),
    (1.56, 1.5, [1.38], [QW], 0.55),          # a gap denser than the glass: R = 1 beyond the critical cosine
    (1.56, 1.62, [1.38], [0.05], 0.55),       # the layer evanescent over part of the row, frustrated by its thinness
    (1.0, 2.4, [1.38, 1.7, 1.38, 1.7, 1.38, 1.7, 1.38, 1.7], [0.1] * 8, 0.5),
]


@pytest.mark.parametrize("stack", STACKS)
def test_reflectance_is_the_restatement(bzr, stack):
    n0, ns, idx, th, lam = stack
    got = bzr.coating_reflectance(n0, ns, idx, th, lam)
    want = coat_ref.reflectance64(n0, ns, idx, th, lam)
    assert got.dtype == F and got.shape == (129,) and got[0] == 1
    assert (got >= 0).all() and (got <= 1).all()
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= 2.0 ** -23 * want + 1e-12).all(), float(err.max())


def test_known_answers(bzr):
    n = 1.5168
    bare = bzr.coating_reflectance(1.0, n)
    assert bare[0] == 1 and abs(float(bare[128]) - 0.0421646) < 1e-7
    assert abs(float(bare[128]) - ((n - 1) / (n + 1)) ** 2) < 2.0 ** -23 * 0.05
    qw = bzr.coating_reflectance(1.0, n, [1.38], [QW], 0.55)
    assert qw[0] == 1 and abs(float(qw[128]) - 0.0128354) < 1e-7
    assert abs(float(qw[128]) - ((n - 1.38 ** 2) / (n + 1.38 ** 2)) ** 2) < 2.0 ** -23 * 0.02
    nc = np.sqrt(n)
    ideal = bzr.coating_reflectance(1.0, n, [nc], [0.55 / (4 * nc)], 0.55)
    assert 0 <= float(ideal[128]) < 1e-12 and ideal[0] == 1


def test_same_reflectance_from_either_side(bzr):
    """A lossless stack: evaluated from the glass side (media swapped, layers reversed) at the Snell-linked cosine it
    gives the same R.  Through the library alone: for samples a < b the index ratio n_glass / n_gap =
    sqrt((1 - (a/128)^2) / (1 - (b/128)^2)) links the gap-side sample a to the glass-side sample b, so both values are
    entries of rows the library filled -- one pair of samples per ratio, oblique on both sides, the layers in between
    propagating or evanescent as their indices fall.  Over a whole row the glass side comes from the restatement's formula
    at the linked cosine (reflectance_at), which is no sample in general."""
    lam = 0.55
    for a, b, layers in ((64, 96, ([1.38, 2.1], [QW, 0.07])), (16, 112, ([1.38], [QW])), (100, 120, ([1.7, 1.2], [0.08, 0.3])),
                         (8, 127, ([1.05, 2.3], [0.2, 0.05])), (32, 64, ([], []))):
        n0 = 1.0
        ns = np.sqrt((1.0 - (a / 128.0) ** 2) / (1.0 - (b / 128.0) ** 2))
        idx, th = layers
        front = bzr.coating_reflectance(n0, ns, idx, th, lam).astype(np.float64)
        back = bzr.coating_reflectance(ns, n0, idx[::-1], th[::-1], lam).astype(np.float64)
        # (two float roundings of half an ulp each; the link holds to a rounding of ns in binary64, inside the 1e-12)
        assert abs(back[b] - front[a]) <= 2.0 ** -23 * front[a] + 1e-12, (a, b, back[b], front[a])
        assert 0.0 < front[a] < 1.0
    n0, ns = 1.0, 1.5168
    idx, th = [1.38, 2.1], [QW, 0.07]
    front = bzr.coating_reflectance(n0, ns, idx, th, lam).astype(np.float64)
    for i in (16, 64, 100, 128):
        mu = i / 128.0
        linked = np.sqrt(1.0 - (n0 / ns) ** 2 * (1.0 - mu * mu))
        back = reflectance_at(ns, n0, idx[::-1], th[::-1], lam, linked)
        assert abs(back - front[i]) <= 2.0 ** -23 * front[i] + 1e-12, (i, back, front[i])
    back_row = bzr.coating_reflectance(ns, n0, idx[::-1], th[::-1], lam).astype(np.float64)
    assert abs(back_row[128] - front[128]) <= 2.0 ** -23 * front[128] + 1e-12


def test_thick_evanescent_layer_and_a_layer_at_its_critical_angle(bzr):
    """Physically valid inputs the helper must answer, not refuse.  A layer far thicker than the evanescent decay length
    (cosh and sinh of its phase overflow binary64) frustrates nothing: R is 1 to rounding wherever the layer is
    evanescent, and the row is the thin-layer restatement's elsewhere.  A layer exactly at its critical angle (its cosine
    exactly 0 in binary64 at one sample) takes the value the restatement gives a hair to either side."""
    n0, ns = 1.56, 1.62
    row = bzr.coating_reflectance(n0, ns, [1.2], [5000.0], 0.55)
    mu = np.arange(129) / 128.0
    evan = 1.0 - (n0 / 1.2) ** 2 * (1.0 - mu * mu) < -1e-3
    assert int(evan.sum()) > 60 and np.isfinite(row).all()
    assert (row[evan] >= 1.0 - 2.0 ** -23).all() and (row <= 1).all()
    thin = bzr.coating_reflectance(n0, ns, [1.2], [0.05], 0.55)
    assert (thin[evan][1:] < 1).all()  # (thin, the same layer does frustrate)
    # exactly at the critical angle: layer indices for which 1 - q / (nj nj) == 0.0 in binary64 at a sample, found by
    # trying nj = sqrt(q) and its neighbours; the helper's branch for a zero cosine runs there, in both polarisations
    reached = 0
    for n0, ns, i in ((1.3, 1.7, 51), (1.6, 1.5, 64), (1.0, 1.62, 90), (1.45, 2.0, 17)):
        m = i / 128.0
        q = n0 * n0 * (1.0 - m * m)
        exact = [nj for nj in (np.nextafter(np.sqrt(q), 0.0), np.sqrt(q), np.nextafter(np.sqrt(q), 9.0))
                 if 1.0 - q / (nj * nj) == 0.0]
        for nj in exact:
            reached += 1
            row = bzr.coating_reflectance(n0, ns, [nj], [0.2], 0.55).astype(np.float64)
            assert np.isfinite(row).all()
            if 1.0 - q / (ns * ns) <= 0.0:  # (the glass beyond its own critical angle there: 1 by definition)
                assert row[i] == 1.0
                continue
            # the restatement a hair to either side of the singular index: R is continuous there
            near = [coat_ref.reflectance64(n0, ns, [nj * (1 + e)], [0.2], 0.55)[i] for e in (-1e-9, 1e-9)]
            assert abs(near[0] - near[1]) < 1e-6 and abs(row[i] - near[0]) < 1e-6, (n0, ns, i, row[i], near)
    assert reached >= 2  # (the first case is one: n_gap 1.3, sample 51, nj = 1.192354131130277)


def reflectance_at(n_gap, n_glass, idx, th, lam, mu):
    """coat_ref.reflectance64's formula at one cosine (binary64)."""
    sin2 = 1.0 - mu * mu
    total = 0.0
    for pol in "sp":
        def cosine(nj):
            return np.sqrt(complex(1.0 - (n_gap / nj) ** 2 * sin2))

        def adm(nj, cj):
            return nj * cj if pol == "s" else nj / cj

        m = np.eye(2, dtype=np.complex128)
        for nj, tj in zip(idx, th):
            cj = cosine(nj)
            d = 2.0 * np.pi * nj * tj * cj / lam
            y = adm(nj, cj)
            m = m @ np.array([[np.cos(d), -1j * np.sin(d) / y], [-1j * y * np.sin(d), np.cos(d)]])
        bc = m @ np.array([1.0, adm(n_glass, cosine(n_glass))], np.complex128)
        y0 = adm(n_gap, complex(mu))
        r = (y0 - bc[1] / bc[0]) / (y0 + bc[1] / bc[0])
        total += abs(r) ** 2
    return 0.5 * total


def test_denser_gap_reflects_totally(bzr):
    n0, ns = 1.56, 1.5
    mu_c = np.sqrt(1.0 - (ns / n0) ** 2)  # beyond the critical angle: mu below this
    for idx, th in (([], []), ([1.38], [QW]), ([2.1, 1.38], [0.05, 0.1])):
        row = bzr.coating_reflectance(n0, ns, idx, th, 0.55)
        mu = np.arange(129) / 128.0
        assert (row[mu <= mu_c] == 1).all() and int((mu <= mu_c).sum()) > 30
        assert (row[mu > mu_c + 1 / 128] < 1).all()


def test_bare_row_interpolation_error(bzr):
    """The reason for BZR_COAT_SAMPLES: measured, printed, recorded in the module's text and in DESIGN.md."""
    n = 1.5168
    row = bzr.coating_reflectance(1.0, n)
    mu = np.linspace(0.0, 1.0, 128 * 64 + 1)
    looked = bzr.coat_transmittance(row, mu.astype(F)).astype(np.float64)
    mu = mu.astype(F).astype(np.float64)
    c2 = np.sqrt(1.0 - (1.0 - mu * mu) / n ** 2)
    rs = (mu - n * c2) / (mu + n * c2)
    rp = (n * mu - c2) / (n * mu + c2)
    exact = 1.0 - 0.5 * (rs * rs + rp * rp)
    err = np.abs(looked - exact)
    for lo in (0.0, 1 / 128, 0.1):
        print(f"bare 1.5168, 129 samples: max |coat_t - (1 - fresnel)| for mu >= {lo:.4f}: {err[mu >= lo].max():.3e}")
    assert np.isfinite(err).all()


def test_refusals(bzr):
    lib = bzr.lib()
    out = np.full(129, 7.0, F)
    idx, th = (ctypes.c_double * 9)(*[1.38] * 9), (ctypes.c_double * 9)(*[0.1] * 9)
    call = lib.bzr_coating_reflectance
    bad = [
        (1.0, 1.5, idx, th, 9, 0.55), (1.0, 1.5, None, th, 1, 0.55), (1.0, 1.5, idx, None, 1, 0.55),
        (0.0, 1.5, idx, th, 1, 0.55), (-1.0, 1.5, idx, th, 1, 0.55), (float("nan"), 1.5, idx, th, 1, 0.55),
        (1.0, 0.0, idx, th, 1, 0.55), (1.0, float("inf"), idx, th, 1, 0.55),
        (1.0, 1.5, idx, th, 1, 0.0), (1.0, 1.5, idx, th, 1, -0.5), (1.0, 1.5, idx, th, 1, float("nan")),
        (1.0, 1.5, idx, th, 1, float("inf")),
    ]
    for a in bad:
        assert call(*a, out.ctypes.data) == 1, a
        assert (out == 7).all()
    assert call(1.0, 1.5, idx, th, 1, 0.55, None) == 1
    for k, v in ((0, 0.0), (0, -1.38), (0, float("nan")), (1, float("inf"))):
        for arr in (idx, th):
            keep = arr[k]
            arr[k] = v
            assert call(1.0, 1.5, idx, th, 2, 0.55, out.ctypes.data) == 1 and (out == 7).all()
            arr[k] = keep
    assert call(1.0, 1.5, idx, th, 8, 0.55, out.ctypes.data) == 0 and out[0] == 1 and (out != 7).all()
    assert call(1.0, 1.5, None, None, 0, 0.55, out.ctypes.data) == 0
    t = ctypes.c_float(7.0)
    row = np.zeros(129, F)
    f = lib.bzr_coat_transmittance
    assert f(None, 0.5, ctypes.byref(t)) == 1 and f(row.ctypes.data, 0.5, None) == 1
    assert f(row.ctypes.data, float("nan"), ctypes.byref(t)) == 1 and f(row.ctypes.data, -0.5, ctypes.byref(t)) == 1
    assert t.value == 7.0
    assert f(row.ctypes.data, 0.5, ctypes.byref(t)) == 0 and t.value == 1.0
    with pytest.raises(bzr.BzrError):
        bzr.coating_reflectance(1.0, 1.5, [1.38], [0.1, 0.2])
    with pytest.raises(bzr.BzrError):
        bzr.coat_transmittance(np.zeros(128, F), 0.5)


def test_coating_class(bzr):
    rows = np.random.default_rng(3).random((4, 129), dtype=F)
    c = bzr.Coating({(0, 0): rows, (1, 1): rows}, nlens=2)
    assert c.mask == 0b1001 and c.table.shape == (4, 4, 129)
    assert np.array_equal(c.table[0], rows) and np.array_equal(c.table[3], rows) and not c.table[1:3].any()
    assert bzr.Coating(c.table, 5).mask == 5 and bzr.Coating(None, 0).table is None
    for bad in ({(2, 0): rows}, {(0, 2): rows}):
        with pytest.raises(bzr.BzrError):
            bzr.Coating(bad, nlens=2)
    with pytest.raises(bzr.BzrError):
        bzr.Coating({(0, 0): rows[:, :100]}, nlens=2)
