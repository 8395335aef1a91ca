"""Far-field maps, the parts that need no GPU: the entry points' declaration, export and binding; bzr_farfield_cell
against the numpy restatement (farfield_ref) bit for bit; the inverse helper's round trip; the intensity helper; the
argument checks; and the restatement's own equal-area property on the oracle's uniform hemisphere.
"""
import ctypes
import re

import numpy as np
import pytest

import farfield_ref as ffr
import illum_tir_ref as itr
from conftest import REPO

F = np.float32
SYMBOLS = ("bzr_farfield_bin", "bzr_illuminate_farfield", "bzr_farfield_cell", "bzr_farfield_directions",
           "bzr_farfield_intensity", "bzr_debug_farfield_rounds", "bzr_debug_farfield_cells")
X_POLE = ((0.0, 1.0, 0.0), (0.0, 0.0, 1.0))  # axis_u x axis_v = +x, the emitter's axis


def tilted():
    """Unit, orthogonal axes that are no coordinate axes (to rounding, as a caller would make them)."""
    u = np.array([0.36, 0.48, 0.8], np.float64)
    v = np.array([0.8, -0.6, 0.0], np.float64)
    return tuple(F(u)), tuple(F(v))


def test_symbols_are_declared_exported_and_bound(bzr):
    lib = ctypes.CDLL(str(bzr.LIB_PATH))
    header = (REPO / "include" / "bzr.h").read_text() + (REPO / "include" / "bzr_debug.h").read_text()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in bzr.exported_symbols(), name
        assert re.search(name + r"\(", header), name
    assert re.search(r"#define BZR_ABI_VERSION 2\b", header)
    assert re.search(r"typedef struct bzr_farfield \{\s+float axis_u\[3\], axis_v\[3\];\s+float extent;\s+"
                     r"uint32_t bins_u, bins_v;\s+\} bzr_farfield;", header)
    assert re.search(r"bzr_status bzr_farfield_bin\(bzr_ctx \*ctx, const bzr_farfield \*far, const float \*rays_soa, "
                     r"const float \*weight,\s+const uint32_t \*status, const uint8_t \*channel, uint32_t n, "
                     r"uint32_t nchan,\s+uint64_t \*far_flux_q32, uint32_t \*far_hist,\s+uint64_t \*far_stats, "
                     r"uint64_t \*far_power_q32, uint32_t flags\);", header)
    assert re.search(r"enum \{ BZR_FAR_SEEN = 0, BZR_FAR_BINNED = 1 \};", header)
    assert re.search(r"farfieldBin\(", (REPO / "include" / "bzr" / "bzr.hpp").read_text())
    for f in (bzr.farfield_bin, bzr.illuminate_farfield, bzr.farfield_cell, bzr.farfield_directions,
              bzr.farfield_intensity):
        assert callable(f)
    assert ctypes.sizeof(bzr.FarField) == 36
    assert bzr.lib().bzr_abi_version() == 2
    assert F(bzr.SQRT2).view(np.uint32) == 0x3FB504F3


def directions(fr, n=1 << 20, seed=11):
    """[3, n] float32: random unit and non-unit directions, then the special ones -- the pole, its opposite (mu = -1)
    and directions just off it, NaN and inf components, zero, and points on the map's and the cells' edges."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((3, n))
    d /= np.linalg.norm(d, axis=0)
    d[:, : n // 8] *= rng.uniform(0.5, 1.5, n // 8)       # directions are used as given
    d = d.astype(F)
    n64, u64, v64 = (np.asarray(a, np.float64) for a in (fr.n, fr.axis_u, fr.axis_v))
    k = n // 4
    special = [n64, -n64, -n64 + 1e-7 * u64, -n64 + 3e-4 * v64, -n64 * (1 - 2.0 ** -24), u64, -v64, np.zeros(3),
               np.array([np.nan, 0, 0]), np.array([0, np.inf, 0]), np.array([-np.inf, 1, 0]), np.array([1, 1, np.nan])]
    for s in special:
        d[:, k] = np.asarray(s, np.float64).astype(F)
        k += 1
    # edges: the inverse map at (X, Y) on cell boundaries and on the map's rim, in binary64, rounded to binary32
    R = float(fr.R)
    gx = -R + 2 * R * np.arange(fr.bins_u + 1) / fr.bins_u
    gy = -R + 2 * R * np.arange(fr.bins_v + 1) / fr.bins_v
    X, Y = np.meshgrid(gx, rng.uniform(-R, R, 64))
    X2, Y2 = np.meshgrid(rng.uniform(-R, R, 64), gy)
    X, Y = np.concatenate([X.ravel(), X2.ravel()]), np.concatenate([Y.ravel(), Y2.ravel()])
    rho2 = X * X + Y * Y
    keep = rho2 < 4.0
    X, Y, rho2 = X[keep], Y[keep], rho2[keep]
    w = np.sqrt(1 - rho2 / 4)
    e = (X * w)[None] * u64[:, None] + (Y * w)[None] * v64[:, None] + (1 - rho2 / 2)[None] * n64[:, None]
    d[:, k:k + e.shape[1]] = e.astype(F)
    return d, k + e.shape[1]


@pytest.mark.parametrize("axes,extent,bins", [(X_POLE, ffr.SQRT2, (48, 48)), (tilted(), ffr.SQRT2, (24, 40)),
                                              (tilted(), 0.5, (7, 3)), (X_POLE, 1.0, (1, 1))])
def test_farfield_cell_is_the_restatement(bzr, axes, extent, bins):
    fr = ffr.frame(axes[0], axes[1], extent, *bins)
    d, used = directions(fr)
    assert d.shape == (3, 1 << 20) and np.isnan(d).any() and np.isinf(d).any() and used > (1 << 18)
    want = ffr.cell(fr, d)
    got = bzr.farfield_cell(ffr.struct(bzr, fr), np.ascontiguousarray(d.T))
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert (want >= 0).sum() > 1000 and want.max() < fr.cells
    if fr.cells > 1:
        assert np.unique(want).size == fr.cells + 1  # every cell and -1
    bad = np.isnan(d).any(axis=0) | np.isinf(d).any(axis=0)
    assert (want[bad] == -1).all()
    k = (1 << 20) // 4
    assert want[k] == ffr.cell(fr, fr.n[:, None])[0] >= 0   # the pole: the cell that holds (X, Y) = (0, 0)
    if axes is X_POLE:
        assert want[k + 1] == -1                            # mu = -1 exactly: g = 0
    one = bzr.farfield_cell(ffr.struct(bzr, fr), d[:, 5])
    assert int(one) == want[5]
    c = ctypes.c_int32(7)
    v = (ctypes.c_float * 3)(*[float(x) for x in d[:, 9]])
    assert bzr.lib().bzr_farfield_cell(ctypes.byref(ffr.struct(bzr, fr)), v, ctypes.byref(c)) == 0 and c.value == want[9]


@pytest.mark.parametrize("extent", (ffr.SQRT2, 0.5))
def test_directions_round_trip(bzr, extent):
    fr = ffr.frame(*tilted(), extent, 24, 40)
    far = ffr.struct(bzr, fr)
    d, polar, azimuth = bzr.farfield_directions(far)
    assert d.shape == (40, 24, 3) and polar.shape == (40, 24) and d.dtype == np.float64
    assert np.allclose(np.linalg.norm(d, axis=2), 1.0, atol=1e-6)
    flat = d.reshape(-1, 3)
    assert np.array_equal(bzr.farfield_cell(far, flat.astype(F)), np.arange(24 * 40))
    assert np.array_equal(ffr.cell(fr, flat.T.astype(F)), np.arange(24 * 40))
    n64 = np.asarray(fr.n, np.float64)
    assert np.allclose(np.cos(polar.ravel()), flat @ n64, atol=1e-6)
    R = float(fr.R)
    X = -R + 2 * R * (np.arange(24) + 0.5) / 24
    Y = -R + 2 * R * (np.arange(40) + 0.5) / 40
    assert np.allclose(azimuth, np.arctan2(Y[:, None], X[None, :]))
    assert np.allclose(2 * np.sin(polar / 2), np.hypot(X[None, :], Y[:, None]), atol=1e-6)  # rho = 2 sin(theta / 2)


def test_intensity_sums_to_the_binned_power(bzr):
    fr = ffr.frame(*X_POLE, 1.0, 24, 40)
    far = ffr.struct(bzr, fr)
    rng = np.random.default_rng(3)
    flux = rng.integers(0, 1 << 40, (3, 40, 24), dtype=np.uint64)
    omega = (2.0 / 24) * (2.0 / 40)
    got = bzr.farfield_intensity(far, flux, 0.25)
    assert got.shape == flux.shape and got.dtype == np.float64
    for c in range(3):
        assert np.isclose(got[c].sum() * omega, 0.25 * float(flux[c].sum()) / 2.0 ** 32, rtol=1e-12)
    assert np.allclose(got, 0.25 * flux.astype(np.float64) / 2.0 ** 32 / omega, rtol=1e-15)
    with pytest.raises(bzr.BzrError, match="flux must be"):
        bzr.farfield_intensity(far, flux[:, :, :5])


def test_arguments_are_checked_without_a_device(bzr):
    L = bzr.lib()
    rays = np.zeros((6, 4), F)
    flux, hist = np.full((2, 5, 3), 7, np.uint64), np.full((2, 5, 3), 7, np.uint32)
    stats, power = np.full((2, 2), 7, np.uint64), np.full((2, 2), 7, np.uint64)

    def call(far=None, nchan=2, f=flux, h=hist, flags=0, n=4, **kw):
        if far is None:
            far = bzr.FarField(axis_u=(0, 1, 0), axis_v=(0, 0, 1), extent=kw.get("extent", 1.0), bins_u=kw.get("bu", 3),
                               bins_v=kw.get("bv", 5))
        return L.bzr_farfield_bin(None, ctypes.byref(far) if far else None, rays.ctypes.data, None, None, None, n, nchan,
                                  f.ctypes.data if f is not None else None, h.ctypes.data if h is not None else None,
                                  stats.ctypes.data, power.ctypes.data, flags)

    assert call() == 1 and b"null context" in L.bzr_last_error()  # everything else is fine
    assert call(n=0) == 0                                          # nothing to do, nothing touched
    assert call(far=False) == 1 and b"null far-field frame" in L.bzr_last_error()
    for kw in ({"bu": 0}, {"bv": 0}):
        assert call(**kw) == 1 and b"bins" in L.bzr_last_error()
    for extent in (0.0, -1.0, 1.5, float(np.nextafter(ffr.SQRT2, F(2))), np.nan, np.inf):
        assert call(extent=extent) == 1 and b"extent" in L.bzr_last_error(), extent
    assert call(extent=float(ffr.SQRT2)) == 1 and b"null context" in L.bzr_last_error()
    assert call(bu=1 << 16, bv=1 << 15) == 1 and b"2^32" in L.bzr_last_error()        # 2 x 2^31 cells
    assert call(bu=1 << 16, bv=1 << 16, nchan=1) == 1 and b"2^32" in L.bzr_last_error()
    for nchan in (0, 65):
        assert call(nchan=nchan) == 1 and b"nchan" in L.bzr_last_error()
    assert call(f=None, h=None) == 1 and b"far_flux_q32 and far_hist" in L.bzr_last_error()
    assert call(flags=1 << 7) == 1 and b"unknown flag" in L.bzr_last_error()
    assert call(flags=bzr.RAYS_AOS) == 1 and b"BZR_RAYS_AOS" in L.bzr_last_error()
    for flags in (bzr.PIPELINE_FUSED, bzr.PIPELINE_STAGED, bzr.MODE_FAST, bzr.DEVICE_PTRS):
        assert call(flags=flags) == 1 and b"null context" in L.bzr_last_error()
    assert (flux == 7).all() and (hist == 7).all() and (stats == 7).all() and (power == 7).all()
    # the host helpers refuse the same frames
    bad = bzr.FarField(axis_u=(0, 1, 0), axis_v=(0, 0, 1), extent=1.5, bins_u=3, bins_v=5)
    with pytest.raises(bzr.BzrError, match="extent"):
        bzr.farfield_cell(bad, np.zeros((1, 3), F))
    with pytest.raises(bzr.BzrError, match="extent"):
        bzr.farfield_directions(bad)
    with pytest.raises(bzr.BzrError, match="extent"):
        bzr.farfield_intensity(bad, np.zeros((5, 3), np.uint64))
    assert L.bzr_debug_farfield_rounds(None, 4) == 1


class _NoContext:
    handle = None


class _NoMesh:
    handle = None


def test_illuminate_farfield_is_checked_without_a_device(bzr):
    em, tg = itr.emitter(bzr, itr.NEAR), itr.target(bzr)
    table = np.full((1, 4), 1.3, F)
    good = bzr.FarField(axis_u=(0, 1, 0), axis_v=(0, 0, 1), extent=1.0, bins_u=4, bins_v=4)
    far_flux = np.full((4, 4, 4), 7, np.uint64)
    for kw, msg in (({"extent": 0.0}, "extent"), ({"extent": 1.5}, "extent"), ({"extent": float("nan")}, "extent"),
                    ({"bins_u": 0}, "bins")):
        far = bzr.FarField(axis_u=(0, 1, 0), axis_v=(0, 0, 1), **{"extent": 1.0, "bins_u": 4, "bins_v": 4, **kw})
        with pytest.raises(bzr.BzrError, match=msg):
            bzr.illuminate_farfield(_NoContext(), [_NoMesh()], table, None, None, None, em, 64, tg, far, far_flux=far_flux)
    with pytest.raises(bzr.BzrError, match="without a target"):
        bzr.illuminate_farfield(_NoContext(), [_NoMesh()], table, None, None, None, em, 64, None, good,
                                flux=np.zeros((4, 48, 48), np.uint64), far_flux=far_flux)
    with pytest.raises(bzr.BzrError, match="null context"):
        bzr.illuminate_farfield(_NoContext(), [_NoMesh()], table, None, None, None, em, 64, None, good, far_flux=far_flux)
    assert (far_flux == 7).all()


# ------------------------------------------------------------------ the independent binary64 check
def test_restatement_and_host_lie_within_the_binary64_bounds(bzr):
    """farfield64 computes the cells from arccos and arctan2 in binary64; the restatement's and the host's counts lie
    between its per-cell bounds on a tilted, non-square map, and the margin leaves few rays open."""
    import farfield64

    fr = ffr.frame(*tilted(), 1.25, 24, 40)
    rng = np.random.default_rng(51)
    d = rng.standard_normal((3, 100_000))
    d = (d / np.linalg.norm(d, axis=0)).astype(F)
    # (towards the direction opposite the pole the margin grows without bound; the map's corners lie at mu = -0.56)
    d = np.ascontiguousarray(d[:, np.asarray(fr.n, np.float64) @ d > -0.9])
    lower, upper, unsure = farfield64.bounds(fr, d)
    assert unsure < 100 and lower.sum() > 30_000
    for c in (ffr.cell(fr, d), bzr.farfield_cell(ffr.struct(bzr, fr), np.ascontiguousarray(d.T))):
        hist = np.bincount(c[c >= 0], minlength=fr.cells).reshape(40, 24)
        assert (hist >= lower).all() and (hist <= upper).all()
    # the check can fail: a map one part in 10 000 larger moves a few dozen rays across cell edges
    c = ffr.cell(ffr.frame(*tilted(), 1.25 * 1.0001, 24, 40), d)
    hist = np.bincount(c[c >= 0], minlength=fr.cells).reshape(40, 24)
    assert not ((hist >= lower).all() and (hist <= upper).all())


# ------------------------------------------------------------------ equal area: a condition on the reference
def test_restatement_is_equal_area_on_the_uniform_hemisphere(orc):
    """orc.emit's directions have cos(incidence) uniform in [0, 1): uniform over the hemisphere about +x.  Under the
    projection about +x, rho^2 = 2 (1 - cos), so the share of rays with rho < r0 is r0^2 / 2."""
    n = 200_000
    rays, _ = orc.emit(itr.emitter(orc, itr.NEAR), 0, n)
    fr = ffr.frame(*X_POLE, ffr.SQRT2, 48, 48)
    X, Y, g = ffr.project(fr, rays[3:6])
    assert (g > 0).all()
    rho = np.hypot(X.astype(np.float64), Y.astype(np.float64))
    assert rho.max() <= np.sqrt(2.0) * (1 + 1e-6)
    for r0 in (0.4, 0.9, 1.3):
        p = r0 * r0 / 2
        sigma = np.sqrt(n * p * (1 - p))
        assert abs(int((rho < r0).sum()) - n * p) <= 6 * sigma, r0
    # and binned: every ray lands in the map, the inscribed disc's cells fill evenly (chi-square over the cells that
    # lie wholly inside it, 6 sigma of its own distribution)
    c = ffr.cell(fr, rays[3:6])
    assert (c >= 0).all()
    iu, iv = np.meshgrid(np.arange(48), np.arange(48))
    R = float(fr.R)
    far_corner = np.hypot(np.maximum(np.abs(-R + 2 * R * iu / 48), np.abs(-R + 2 * R * (iu + 1) / 48)),
                          np.maximum(np.abs(-R + 2 * R * iv / 48), np.abs(-R + 2 * R * (iv + 1) / 48)))
    inside = (far_corner < np.sqrt(2.0) * 0.999).ravel()
    counts = np.bincount(c, minlength=48 * 48)[inside]
    expect = n * (2 * R / 48) ** 2 / (2 * np.pi)
    k = int(inside.sum())
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    assert k > 1000 and abs(chi2 - k) <= 6 * np.sqrt(2 * k), (chi2, k)
