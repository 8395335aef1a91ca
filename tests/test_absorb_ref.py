"""Absorption, the reference pinned (no GPU): tests/absorb_ref.py against media_ref.chain with zero tables, and its att
against binary64 exp(-x).

Scene: cfg2, 64^2 - 37 = 4 059 rays, channels from default_rng(7), as in test_media_ref.py.
"""
import math

import numpy as np
import pytest

import absorb_ref
import media_ref
from bzr_amd.configs import CONFIGS, build_lens, grid_rays
from test_gpu_tir import DROP, NCHAN, SIDE
from test_media_ref import differ

F = np.float32


@pytest.fixture(scope="module")
def cfg2(bzr):
    cfg = CONFIGS["cfg2"]
    lenses = [build_lens(bzr.TriMesh, lens).bezier_patches() for lens in cfg.lenses]
    rays = grid_rays(cfg, side=SIDE)
    n = rays.shape[1] - DROP
    rays = np.ascontiguousarray(rays[:, :n])
    channel = np.random.default_rng(7).integers(0, NCHAN, SIDE * SIDE)[:n].astype(np.uint8)
    return lenses, rays, channel


def test_zero_tables_are_media_ref(orc, cfg2):
    lenses, rays, channel = cfg2
    n = rays.shape[1]
    w_in = np.random.default_rng(41).random(n, dtype=F)
    p_in = (np.random.default_rng(43).random(n, dtype=F) * F(8)).astype(F)
    want = media_ref.chain(orc, lenses, [media_ref.ROW1], media_ref.GAPS2, rays, channel, w_in, p_in, 4)
    zeros = np.zeros((1, NCHAN), F)
    for ga, pa in ((zeros, zeros), (None, None), (zeros, None)):
        got = absorb_ref.chain(orc, lenses, [media_ref.ROW1], media_ref.GAPS2, ga, pa, rays, channel, w_in, p_in, 4)
        assert not differ(got, want).any()
    assert int((want[4] > 0).sum()) >= 100
    # and non-zero tables move the weight alone
    got = absorb_ref.chain(orc, lenses, [media_ref.ROW1], media_ref.GAPS2, absorb_ref.GLASS2, absorb_ref.GAPA2, rays,
                           channel, w_in, p_in, 4)
    for k in (0, 2, 3, 4, 5, 6):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32))
    changed = got[1].view(np.uint32) != want[1].view(np.uint32)
    assert not changed[channel == 0].any() and int(changed.sum()) >= 1500
    assert ((got[1] >= 0) & (got[1] <= want[1])).all()


def test_coefficients():
    c = [np.float32((-math.log(2.0)) ** j / math.factorial(j)) for j in range(8)]
    assert np.array_equal(np.array(c, F).view(np.uint32), absorb_ref.COEFF.view(np.uint32))
    assert absorb_ref.COEFF[0] == 1 and absorb_ref.LOG2E == np.float32(math.log2(math.e))


def test_att_against_exp():
    """Relative error at most 2^-23 (1 + y), y = x log2(e), wherever exp(-x) > 1e-37; att(0) = 1; every result in
    [0, 1]; 0 from the first x with x log2(e) >= 125."""
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.random(1 << 21) * 87.0, 10.0 ** (rng.random(1 << 21) * 14.0 - 12.0),
                        absorb_ref.att_values()]).astype(F)
    x = x[np.isfinite(x)]
    a = absorb_ref.att(x)
    assert a.dtype == F
    want = np.exp(-x.astype(np.float64))
    keep = want > 1e-37
    y = x.astype(np.float64) * math.log2(math.e)
    rel = np.abs(a[keep].astype(np.float64) - want[keep]) / want[keep]
    worst = float((rel / (1.0 + y[keep])).max())
    print(f"att: {int(keep.sum())} points, max relative error {float(rel.max()):.3g}, max error / (1 + y) = "
          f"{worst / 2.0 ** -24:.3f} x 2^-24")
    assert (rel <= 2.0 ** -23 * (1.0 + y[keep])).all()
    assert ((a >= 0) & (a <= 1)).all()
    assert absorb_ref.att(np.zeros(1, F))[0] == 1
    nz = a[a > 0]
    assert nz.min() >= np.finfo(F).tiny
    # the cut-off: the first float whose product with log2(e) reaches 125, and everything above it
    cut = F(125.0) / absorb_ref.LOG2E
    near = [cut]
    for _ in range(8):
        near = near + [np.nextafter(near[0], F(0))] + [np.nextafter(near[-1], F(np.inf))]
        near.sort()
    near = np.array(near, F)
    dead = near * absorb_ref.LOG2E >= F(125)
    assert dead.any() and not dead.all()
    got = absorb_ref.att(near)
    assert (got[dead] == 0).all() and (got[~dead] > 0).all()
    assert (absorb_ref.att(np.array([90.0, 1e30, np.inf, np.nan], F)) == 0).all()
