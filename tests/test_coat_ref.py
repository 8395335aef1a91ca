"""The coated chain, the reference pinned (no GPU): tests/coat_ref.py against bidir_ref.chain with no surface coated, the
header's consequences on the reference itself, and the floors the GPU tests rely on.

Scenes: ghost_ref.scene's cfg2, cfg4 and the doublet (4 059 rays along +x, four channels; the doublet one), axis
(1, 0, 0), ghost_seed 2024, first_ray 2^40 + 5.  The MgF2 rows come from the library's host helper, which
tests/test_coat_host.py checks against coat_ref.reflectance64.

Floors for the "mixed" coating (front of lens 0 and back of the last lens coated, the rest bare), draws counted over
the 4 059 rays at side 64 with their four channels -- no scene needed a larger side.  (open-coated, glass-coated,
glass-uncoated of a lens with a coated face) at budgets 1 / 4 / 8, printed by the test:
    cfg2     (2781, 2386, 0) / (2781, 2643, 0) / (2781, 2754, 0)
    cfg4     (2781, 2505, 2586) / (2781, 2596, 2688) / (2781, 2615, 2756)
    doublet  (2781, 2722, 2728) / (2781, 2744, 2760) / (2781, 2744, 2760)
cfg2 has one lens, and the mixed coating covers both of its faces: a draw at an uncoated surface of that lens does not
exist, whatever the side or the channels.  Its third count is therefore established on a coating of its own, "front"
(the front of lens 0 alone), which the GPU tests run on cfg2 beside the mixed one: (2781, 0, 2386) /
(2781, 200, 2456) / (2781, 207, 2539).
"""
import numpy as np
import pytest

import bidir_ref
import coat_ref
import ghost_ref
from test_media_ref import differ

F = np.float32
NAMES = ("cfg2", "cfg4", "doublet")
FLOOR = 200


@pytest.fixture(scope="module")
def scenes(bzr):
    return {name: ghost_ref.scene(bzr, name) for name in NAMES}


def args_of(orc, s, rows=True, absorb=True):
    return (orc, s["lenses"], s["table"], s["gaps"], s["glass"] if absorb else None, s["gapa"] if absorb else None,
            s["rays"], s["channel"], s["w_in"] if rows else None, s["p_in"] if rows else None)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("max_bounces", (0, 1, 4, 8))
def test_mask_0_is_bidir_ref(orc, bzr, scenes, name, max_bounces):
    s = scenes[name]
    want = bidir_ref.chain(*args_of(orc, s), max_bounces)
    assert not differ(coat_ref.chain(*args_of(orc, s), max_bounces), want).any()
    rows = coat_ref.mgf2_rows(bzr, s)
    assert not differ(coat_ref.chain(*args_of(orc, s), max_bounces, coat=(rows, 0)), want).any()
    assert int((want[2] == 2).sum()) > 1200


@pytest.mark.parametrize("name", NAMES)
def test_rows_of_zeros_never_mirror(orc, scenes, name):
    """A perfect anti-reflection coating on every surface: no draw mirrors, and without absorption every ray that never
    reflected (total reflection aside) keeps its weight bit for bit, budget spent or not."""
    s = scenes[name]
    nl, nchan = np.asarray(s["table"]).shape
    coat = (np.zeros((2 * nl, nchan, 129), F), (1 << (2 * nl)) - 1)
    for max_bounces in (0, 4):
        log = {}
        out, w, status, seg, bounces, _, _ = coat_ref.chain(*args_of(orc, s, absorb=False), max_bounces, coat=coat, log=log)
        draws = [d for ds in log["draws"] for d in ds]
        assert all(d[2] and d[3] == F(1) and d[4] < d[3] for d in draws) and (max_bounces == 0 or len(draws) > 5000)
        none = bounces == 0
        assert int(none.sum()) > 3000
        assert np.array_equal(w[none].view(np.uint32), s["w_in"][none].view(np.uint32))
        # what reflected did so by total reflection alone
        for i in np.nonzero(bounces > 0)[0]:
            assert "r" in log["events"][i]


def test_mirror_on_the_back_of_cfg2(orc, scenes):
    """cfg2's back surface a mirror, budget 1: whatever leaves behind the lens had its budget spent and weight 0; the
    rays the mirror sends back leave in front with one bounce."""
    s = scenes["cfg2"]
    nchan = np.asarray(s["table"]).shape[1]
    coat = (np.ones((2, nchan, 129), F), 2)
    out, w, status, seg, bounces, _, _ = coat_ref.chain(*args_of(orc, s), 1, coat=coat)
    outside = status == coat_ref.RR_OUTSIDE
    back1 = (status == coat_ref.RR_BACK) & (bounces == 1)
    print(f"cfg2 mirror: {int(outside.sum())} OUTSIDE rays, {int(back1.sum())} BACK rays with one bounce")
    assert (w[outside].view(np.uint32) == 0).all()
    assert int(back1.sum()) >= 1000


@pytest.mark.parametrize("name", NAMES)
def test_mgf2_reflects_fewer_rays(orc, bzr, scenes, name):
    s = scenes[name]
    bare = coat_ref.chain(*args_of(orc, s), 4)
    coated = coat_ref.chain(*args_of(orc, s), 4, coat=coat_ref.all_coated(bzr, s))
    nb, nc = int((bare[4] > 0).sum()), int((coated[4] > 0).sum())
    print(f"{name} budget 4: {nb} rays reflect on bare glass, {nc} with every surface MgF2-coated")
    assert nc < nb


@pytest.mark.parametrize("name", NAMES)
def test_draw_stats(orc, bzr, scenes, name):
    """Over the coated draws the reflections lie within 5 sigma of sum (1 - T)."""
    s = scenes[name]
    log = {}
    coat_ref.chain(*args_of(orc, s), 4, coat=coat_ref.all_coated(bzr, s), log=log)
    n, refl, mean, var = coat_ref.draw_stats(log)
    print(f"{name}: {n} coated draws, {refl} reflections, expected {mean:.1f} +- {np.sqrt(var):.1f}")
    assert n > 5000 and abs(refl - mean) <= 5.0 * np.sqrt(var)
    assert all(d[2] for ds in log["draws"] for d in ds)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("max_bounces", (1, 4, 8))
def test_floors_of_the_mixed_coating(orc, bzr, scenes, name, max_bounces):
    s = scenes[name]
    nl = len(s["lenses"])
    coat = coat_ref.mixed(bzr, s)
    log = {}
    coat_ref.chain(*args_of(orc, s), max_bounces, coat=coat, log=log)
    a, b, c = coat_ref.draw_kinds(log, nl, coat[1])
    print(f"{name} side 64, budget {max_bounces}, mixed: open-coated {a}, glass-coated {b}, glass-uncoated {c}")
    assert a >= FLOOR and b >= FLOOR
    if nl > 1:
        assert c >= FLOOR
        return
    # one lens: the mixed coating covers both faces (the module's text); the front-only coating takes the third count
    assert c == 0 and coat[1] == 3
    log = {}
    coat_ref.chain(*args_of(orc, s), max_bounces, coat=(coat[0], 1), log=log)
    a, b, c = coat_ref.draw_kinds(log, nl, 1)
    print(f"{name} side 64, budget {max_bounces}, front: open-coated {a}, glass-coated {b}, glass-uncoated {c}")
    assert a >= FLOOR and c >= FLOOR


def test_coat_t_is_the_headers_lookup():
    """coat_t on a ramp: exact at the samples, linear between them, clamped above 1."""
    row = (np.arange(129) / 128.0).astype(F)
    mu = np.array([0.0, 1.0, 0.5, 0.25 + 2.0 ** -10, 1.0 + 2.0 ** -23], F)
    assert np.array_equal(coat_ref.coat_t(row, mu), F(1) - np.minimum(mu, F(1)))
