"""bzr_ghost_uniform, the roulette's draw on the host (no GPU): against the numpy restatement of include/bzr.h in
tests/ghost_ref.py bit for bit, as a distribution, and against the emitter's stream."""
import ctypes

import numpy as np
import pytest

import ghost_ref
import illum64
from test_illum64 import bar, chi2, table

F = np.float32
SEEDS = (0, 2024, 2 ** 64 - 1)
RAYS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5, 2 ** 64 - 1)


def test_host_uniform_is_the_restatement(bzr):
    for seed in SEEDS:
        for ray in RAYS:
            for lens in range(8):
                for k in range(9):
                    got = bzr.ghost_uniform(seed, ray, lens, k)
                    want = ghost_ref.uniform(seed, [ray], 16 * lens + k)[0]
                    assert isinstance(got, F) and 0.0 <= got < 1.0
                    assert got.view(np.uint32) == want.view(np.uint32), (seed, ray, lens, k)
                    assert float(got) * 2 ** 24 == int(float(got) * 2 ** 24)  # a 24-bit uniform


def test_bad_arguments(bzr):
    u = ctypes.c_float(7.0)
    for lens, k in ((8, 0), (0, 9), (2 ** 31, 0)):
        assert bzr.lib().bzr_ghost_uniform(1, 2, lens, k, ctypes.byref(u)) == 1
        assert u.value == 7.0
    assert bzr.lib().bzr_ghost_uniform(1, 2, 0, 0, None) == 1
    with pytest.raises(bzr.BzrError):
        bzr.ghost_uniform(0, 0, 8, 0)


def test_restatement_known_answers():
    """mix64 is the published splitmix64 finaliser (Vigna's splitmix64.c, seed 0: the first output)."""
    assert int(ghost_ref.mix64(np.array([0x9E3779B97F4A7C15], np.uint64))[0]) == 0xE220A8397B1DCDAF


@pytest.mark.parametrize("seed", SEEDS)
def test_uniform_is_uniform(bzr, seed):
    """Chi-square over 2^20 draws, as tests/test_illum64.py tests the emitter's stream: u alone, u against the next
    ray's u, and u against the same ray's next draw (e + 1)."""
    n = 1 << 20
    j = ghost_ref.ray_numbers(2 ** 40 + 5, n)
    u0, u1 = ghost_ref.uniform(seed, j, 0).astype(np.float64), ghost_ref.uniform(seed, j, 1).astype(np.float64)
    spot = np.arange(0, n, 4099)
    for k in spot:  # the numpy stream is the library's
        assert bzr.ghost_uniform(seed, int(j[k]), 0, 0) == F(u0[k]) and bzr.ghost_uniform(seed, int(j[k]), 0, 1) == F(u1[k])
    assert (u0 >= 0).all() and (u0 < 1).all()
    stats = {
        "u": (chi2(np.bincount((u0 * 256).astype(int), minlength=256), n / 256), 255),
        "u[j] x u[j+1]": (chi2(table(u0[:-1], u0[1:]), (n - 1) / 64), 63),
        "u[e] x u[e+1]": (chi2(table(u0, u1), n / 64), 63),
    }
    print(seed, {k: round(s, 1) for k, (s, _) in stats.items()})
    for name, (s, dof) in stats.items():
        assert s <= bar(dof), (name, s, bar(dof))


@pytest.mark.parametrize("seed", (0, 2024, 12345))
def test_off_the_emitters_stream(bzr, seed):
    """G(seed, j, 0, 0) is not the emitter's U(j, 0) for the same seed: no ray's first draw repeats its cos(incidence),
    and the two are independent."""
    n = 1 << 16
    em = illum64.emitter(illum64.PLAIN)
    em.seed = seed
    ci = illum64.emit64(em, 0, n).ci
    u = ghost_ref.uniform(seed, np.arange(n, dtype=np.uint64), 0).astype(np.float64)
    assert bzr.ghost_uniform(seed, 5, 0, 0) == F(u[5])
    assert int((np.abs(u - ci) < 2.0 ** -24).sum()) <= 2
    assert chi2(table(u, ci), n / 64) <= bar(63)
