"""Surrounding media, the reference and its populations (no GPU): tests/media_ref.py against opl_ref.chain in vacuum and
against the oracle's own refract with a uniform eta, and what the media do to the scenes the GPU tests use.

Scenes: 64^2 - 37 = 4 059 rays (a ragged last wave), channels from default_rng(7), as in test_gpu_tir.py.
"""
import numpy as np
import pytest

import media_ref
import opl_ref
from bzr_amd.configs import CONFIGS, build_lens, grid_rays
from test_gpu_tir import DROP, NCHAN, SIDE, TABLES

F = np.float32
RR_NONE, RR_INSIDE, RR_OUTSIDE = 0, 1, 2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def differ(a, b):
    """[n] bool: ray i differs in any word of the seven outputs."""
    bad = (bits(a[0]) != bits(b[0])).any(axis=0)
    for k in range(1, 7):
        bad |= bits(a[k]) != bits(b[k])
    return bad


@pytest.fixture(scope="module")
def scenes(bzr, orc):
    """name -> (patches, rays [6, 4 059], channel): computed once, never changed."""
    out = {}
    for name in TABLES:
        cfg = CONFIGS[name]
        lenses = [build_lens(bzr.TriMesh, lens).bezier_patches() for lens in cfg.lenses]
        rays = grid_rays(cfg, side=SIDE)
        n = rays.shape[1] - DROP
        rays = np.ascontiguousarray(rays[:, :n])
        channel = np.random.default_rng(7).integers(0, NCHAN, SIDE * SIDE)[:n].astype(np.uint8)
        rays.setflags(write=False)
        channel.setflags(write=False)
        out[name] = (lenses, rays, channel)
    return out


@pytest.mark.parametrize("max_bounces", (0, 4))
@pytest.mark.parametrize("name", list(TABLES))
def test_vacuum_is_opl_ref(orc, scenes, name, max_bounces):
    """With every gap 1 the restated step decides what the oracle's refract decided: all seven outputs bit for bit."""
    lenses, rays, channel = scenes[name]
    n = rays.shape[1]
    assert n == 4059 and n % 64 != 0
    w_in = np.random.default_rng(41).random(n, dtype=F)
    p_in = (np.random.default_rng(43).random(n, dtype=F) * F(8)).astype(F)
    want = opl_ref.chain(orc, lenses, TABLES[name], rays, channel, w_in, p_in, max_bounces)
    ones = np.ones((len(lenses) + 1, NCHAN), F)
    for gaps in (ones, None):
        got = media_ref.chain(orc, lenses, TABLES[name], gaps, rays, channel, w_in, p_in, max_bounces)
        assert not differ(got, want).any()
    refracted = int((want[3] >= 2).sum())  # the first segment refracted: the ray went on to a second one
    print(f"{name}, max_bounces {max_bounces}: {refracted} rays refract")
    assert refracted >= 2700


def test_step_against_the_oracle(orc, scenes):
    """The step with a uniform eta and expected OUTSIDE is the oracle's refract(OUTSIDE) with ri = eta, on the rays of
    cfg2's OUTSIDE segment (the oracle's eta on that side is ri itself)."""
    lenses, rays, _ = scenes["cfg2"]
    patches = lenses[0]
    n = rays.shape[1]
    o, s = orc.refract(patches, 1.3, rays, np.full(n, RR_INSIDE, np.uint32), 16)
    r = np.ascontiguousarray(o[:, s == RR_INSIDE])
    m = r.shape[1]
    assert m >= 2700
    eta = F(F(1.5) / F(1.333))
    want_o, want_s = orc.refract(patches, float(eta), r, np.full(m, RR_OUTSIDE, np.uint32), 16)
    hit = orc.intersect(patches, r, 16)
    got_s, dirs = media_ref.step(np.full(m, eta, F), r[3:6], hit, RR_OUTSIDE)
    assert np.array_equal(got_s, want_s)
    ok = got_s != RR_NONE
    assert int(ok.sum()) >= 2000 and int((~ok).sum()) >= 1
    got_o = r.copy()
    got_o[0:3, ok] = hit[1:4][:, ok]
    got_o[3:6, ok] = dirs[:, ok]
    assert np.array_equal(bits(got_o), bits(want_o))


def test_cfg2_with_media_per_channel(orc, scenes):
    lenses, rays, channel = scenes["cfg2"]
    vac = media_ref.chain(orc, lenses, [media_ref.ROW1], None, rays, channel, None, None, 4)
    med = media_ref.chain(orc, lenses, [media_ref.ROW1], media_ref.GAPS2, rays, channel, None, None, 4)
    bad = differ(med, vac)
    assert not bad[channel == 0].any()  # channel 0 lies in vacuum on both sides
    changed = [int(bad[channel == c].sum()) for c in (1, 2, 3)]
    refl_med = [int((med[4][channel == c] > 0).sum()) for c in range(NCHAN)]
    refl_vac = [int((vac[4][channel == c] > 0).sum()) for c in range(NCHAN)]
    none_path = int(((med[2] == RR_NONE) & (med[5] > 0)).sum())
    print(f"cfg2 with media: rays unlike vacuum per channel 1-3 {changed}; reflecting per channel {refl_med} (vacuum "
          f"{refl_vac}); NONE with a path {none_path}")
    assert min(changed) >= 600
    assert refl_med[1] == 0 and refl_vac[1] > 0  # 1.5 in water: eta 1.125 where vacuum has 1.5 (vacuum: 88 reflect)
    assert refl_med[2] >= 100 and refl_med[3] >= 100
    assert none_path >= 90


def test_index_matched_lens(orc, scenes):
    """Every index 1.5: eta = 1 on both sides, nothing reflects and no ray is bent.  max |d_out - d_in| <= 2.4e-7, 4 ulp
    of 1: each of the two steps scales d by 1, adds n (c1 - c2) with c2 = sqrt(1 - (1 - cs^2)) within an ulp or two of
    c1, and normalises."""
    lenses, rays, channel = scenes["cfg2"]
    got = media_ref.chain(orc, lenses, [[1.5] * NCHAN], [[1.5] * NCHAN] * 2, rays, channel, None, None, 4)
    entered = got[3] >= 2
    out = got[2] == RR_OUTSIDE
    dev = np.abs(got[0][3:6][:, out] - rays[3:6][:, out]).max()
    print(f"index-matched: {int(entered.sum())} rays enter the lens, {int(out.sum())} end OUTSIDE, max |d_out - d_in| {dev:.3g}")
    assert int(out.sum()) >= 2750
    # a ray that entered and did not leave met the back surface inside the grazing limit (0.99 <= s2 < 1, NONE after
    # its second segment): none was reflected and none needed a third segment
    assert not got[4].any()
    assert (got[3][entered & ~out] == 2).all() and (got[2][entered & ~out] == RR_NONE).all()
    assert dev <= 2.4e-7


def test_doublet_cement_against_air(bzr, orc, scenes):
    lenses = media_ref.doublet_lenses(bzr.TriMesh)
    _, rays, _ = scenes["cfg2"]
    res = {}
    for what, gaps in (("cement", media_ref.DOUBLET_CEMENT), ("air", media_ref.DOUBLET_AIR)):
        got = media_ref.chain(orc, lenses, media_ref.DOUBLET_RI, gaps, rays, None, None, None, 4)
        res[what] = (int((got[2] == RR_OUTSIDE).sum()), int((got[4] > 0).sum()))
    print(f"doublet (OUTSIDE, reflecting): {res}")
    assert res["cement"][0] >= 2750 and res["cement"][1] <= 10
    assert res["air"][0] <= 2420 and res["air"][1] >= 350


def test_denser_front_never_reflects(orc, scenes):
    """1.6 in front of 1.3: an INSIDE segment with s2 >= 0.99 is NONE after one segment (measured: 102 more than in
    vacuum)."""
    lenses, rays, _ = scenes["cfg2"]
    vac = media_ref.chain(orc, lenses, [[1.3]], None, rays, None, None, None, 4)
    med = media_ref.chain(orc, lenses, [[1.3]], [[1.6], [1.0]], rays, None, None, None, 4)
    one = [int(((g[2] == RR_NONE) & (g[3] == 1)).sum()) for g in (vac, med)]
    print(f"NONE after one segment: vacuum {one[0]}, 1.6 in front {one[1]}")
    assert one[1] - one[0] >= 80
    assert not (med[4][med[3] == 1] > 0).any()
