"""The Fresnel roulette, the reference pinned (no GPU): tests/ghost_ref.py against absorb_ref.chain at budget 0, and
what its draws do on the test scenes -- how many rays the roulette reflects against the expectation sum (1 - T), and
the floors the GPU tests rely on (enough ghosts, enough double bounces, few draws near T).

Scenes: cfg2 and cfg4 of test_gpu_absorb.py, ghost_seed 2024, first_ray 2^40 + 5.
"""
import math

import numpy as np
import pytest

import absorb_ref
import ghost_ref
from test_media_ref import differ

F = np.float32
BUDGETS = (1, 4, 8)
FLOOR = {"cfg2": 100, "cfg4": 150}  # roulette reflections at every budget >= 1


@pytest.fixture(scope="module")
def scenes(bzr):
    return {name: ghost_ref.scene(bzr, name) for name in ("cfg2", "cfg4")}


@pytest.fixture(scope="module")
def runs(orc, scenes):
    """(name, budget, weights) -> (outputs, draw log); weights: "rand" (the random rows) or "one" (no rows, no
    absorption).  Computed once."""
    out = {}
    for name, s in scenes.items():
        for mb in BUDGETS:
            log = []
            res = ghost_ref.chain(orc, s["lenses"], s["table"], s["gaps"], s["glass"], s["gapa"], s["rays"], s["channel"],
                                  s["w_in"], s["p_in"], mb, log=log)
            out[name, mb, "rand"] = (res, log)
            log = []
            res = ghost_ref.chain(orc, s["lenses"], s["table"], s["gaps"], None, None, s["rays"], s["channel"], None, None,
                                  mb, log=log)
            out[name, mb, "one"] = (res, log)
    return out


@pytest.mark.parametrize("name", ("cfg2", "cfg4"))
def test_budget_0_is_absorb_ref(orc, scenes, name):
    s = scenes[name]
    args = (orc, s["lenses"], s["table"], s["gaps"], s["glass"], s["gapa"], s["rays"], s["channel"], s["w_in"], s["p_in"], 0)
    log = []
    got = ghost_ref.chain(*args, log=log)
    want = absorb_ref.chain(*args)
    assert not differ(got, want).any()
    assert log == [] and int((want[2] == 2).sum()) > 1500


@pytest.mark.parametrize("name", ("cfg2", "cfg4"))
@pytest.mark.parametrize("max_bounces", BUDGETS)
@pytest.mark.parametrize("rows", ("rand", "one"))
def test_reflections_against_expectation(runs, name, max_bounces, rows):
    """Each draw reflects with probability 1 - T: the count lies within 4 standard deviations of sum (1 - T)."""
    res, log = runs[name, max_bounces, rows]
    draws, refl, expect, var, close = ghost_ref.draw_stats(log)
    z = (refl - expect) / math.sqrt(var)
    print(f"{name} budget {max_bounces} {rows}: {refl} of {draws} draws reflect, expected {expect:.1f}, z = {z:+.2f}; "
          f"{close.size} rays with a draw within 1e-3 of T")
    assert abs(refl - expect) <= 4.0 * math.sqrt(var)
    assert refl >= FLOOR[name]
    assert close.size <= 0.01 * res[0].shape[1]


def test_geometry_does_not_depend_on_the_rows(runs):
    """The draws read T and the ray number alone: random weight and path rows change neither rays nor counts."""
    for name in ("cfg2", "cfg4"):
        a, b = runs[name, 4, "rand"][0], runs[name, 4, "one"][0]
        for k in (0, 2, 3, 4, 6):
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (name, k)


def test_double_bounce_ghosts(runs, scenes):
    """cfg2 at budget 4: at least 50 rays leave the lens with exactly two reflections (the classic ghost path)."""
    res, _ = runs["cfg2", 4, "rand"]
    twice = int(((res[4] == 2) & (res[2] == 2)).sum())
    print("cfg2 budget 4: rays that left with exactly two reflections:", twice)
    assert twice >= 50


def test_weights_of_unreflected_rays(orc, runs, scenes):
    """Row-0 invariant on the reference: a ray that never reflected has absorb_ref's geometry, and a weight at or
    above absorb_ref's (its exits did not pay T)."""
    for name in ("cfg2", "cfg4"):
        s = scenes[name]
        got = runs[name, 4, "rand"][0]
        want = absorb_ref.chain(orc, s["lenses"], s["table"], s["gaps"], s["glass"], s["gapa"], s["rays"], s["channel"],
                                s["w_in"], s["p_in"], 4)
        z = got[4] == 0
        assert int(z.sum()) > 3000
        for k in (0, 2, 3, 5, 6):
            assert np.array_equal(got[k][..., z].view(np.uint32), want[k][..., z].view(np.uint32)), (name, k)
        assert (want[1][z] <= got[1][z]).all()
        assert int((want[1][z] < got[1][z]).sum()) > 1000
