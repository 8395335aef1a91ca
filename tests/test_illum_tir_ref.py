"""The populations tests/test_gpu_illum_tir.py relies on, asserted from the reference alone (no GPU): rays that
reflect, reflected rays that land, every ledger row 1..4 with an exit, waves that mix reflected and unreflected lanes,
and the reference's zero-budget form against the spectral reference."""
import numpy as np
import pytest

import illum_tir_ref as itr
import spectral_ref


@pytest.fixture(scope="module")
def cfg2(bzr):
    return itr.lenses_of(bzr, "cfg2")


def test_near_scene_budget_four(orc, cfg2):
    ref = itr.reference(orc, cfg2, [itr.ROW1], itr.NEAR, 4)
    refl = itr.reflected(ref)
    landed = int(ref.rhist.sum())
    print(f"near, budget 4: {int(refl.sum())} reflect, {landed} of them land, per channel "
          f"{[int(ref.rhist[c].sum()) for c in range(4)]}; ledger rows 1..4 (LOST, EXITED, LANDED) "
          f"{ref.uncut_count[:, 1:5].sum(axis=0).tolist()}; {itr.mixed_waves(ref)} mixed waves of "
          f"{-(-itr.N_RAYS // 64)}")
    assert int(refl.sum()) >= 300
    assert landed >= 100
    for r in range(1, 5):
        assert int(ref.uncut_count[:, r, itr.EXITED].sum()) >= 1, r
    assert itr.mixed_waves(ref) >= 100
    # odd bounce counts leave through the front surface and never land
    assert int(ref.uncut_count[:, 1::2, itr.LANDED].sum()) == 0
    # the reference's own identities: the rows partition the rays, the reflected maps are rows >= 1
    assert int(ref.uncut_count[:, :, :2].sum()) == itr.N_RAYS
    assert int(ref.uncut_count[:, :, itr.LANDED].sum()) == int(ref.hist.sum())
    assert int(ref.uncut_power[:, 1:, itr.LANDED].sum()) == int(ref.rflux.sum())


def test_far_scene(orc, cfg2):
    ref = itr.reference(orc, cfg2, [itr.ROW1], itr.FAR, 4)
    print(f"far, budget 4: {int(itr.reflected(ref).sum())} reflect, {int(ref.rhist.sum())} of them land")
    assert int(itr.reflected(ref).sum()) >= 80


def test_near_scene_three_channels(orc, cfg2):
    ref = itr.reference(orc, cfg2, [itr.ROW1[:3]], itr.NEAR, 4)
    print(f"near, three channels: {int(itr.reflected(ref).sum())} reflect, {int(ref.rhist.sum())} of them land")
    assert int(itr.reflected(ref).sum()) >= 100


def test_zero_budget_is_the_spectral_reference(orc, cfg2):
    ref = itr.reference(orc, cfg2, [itr.ROW1], itr.NEAR, 0)
    want = spectral_ref.chain(orc, cfg2, [itr.ROW1], ref.rays, ref.channel, ref.w0)
    for got, exp in zip((ref.out, ref.w), want[:2]):
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(exp).view(np.uint32))
    assert np.array_equal(ref.status, want[2]) and np.array_equal(ref.seg, want[3])
    assert not ref.bounces.any() and not ref.rhist.any() and not ref.uncut_count[:, 1:].any()
