"""The bidirectional chain, the reference pinned (no GPU): tests/bidir_ref.py against absorb_ref.chain at budget 0, the
path kinds the GPU tests rely on, and the header's consequences on the reference itself.

Scenes: ghost_ref.scene's cfg2, cfg4 and the doublet (4 059 rays along +x, four channels), axis (1, 0, 0), ghost_seed
2024, first_ray 2^40 + 5.

Budget 0: every traced ray of the three scenes leaves glass through surfaces that face forward only (0 rays do not), so
the comparison with absorb_ref.chain covers every ray.

Path kinds at budget 4 (bidir_ref.kinds).  On the 64^2 scenes kind (a) is plentiful (cfg2 140, cfg4 193, doublet 130
rays) but (b) is absent and (c) short (cfg4 2, doublet 14): the second lens of both two-lens scenes sits in cement of
index 1.56 against glass of 1.50 to 1.62, so its front surface reflects about 4 in 10 000 rays.  Following the issue,
`side` is raised and one channel is used for all rays until the reference alone meets the count: channel 0, side 512
for cfg4 (side 320 gave b = 6) and side 320 for the doublet.  The counts measured there, printed by the test:
(a, b, c) = cfg4 (3 881, 14, 94) and doublet (3 460, 13, 467).
"""
import numpy as np
import pytest

import absorb_ref
import bidir_ref
import ghost_ref
from bzr_amd.configs import CONFIGS, grid_rays
from test_media_ref import differ

F = np.float32
NAMES = ("cfg2", "cfg4", "doublet")
KIND_SIDE, KIND_CHANNEL, KIND_FLOOR = {"cfg4": 512, "doublet": 320}, 0, 8


@pytest.fixture(scope="module")
def scenes(bzr):
    return {name: ghost_ref.scene(bzr, name) for name in NAMES}


def args_of(orc, s, rows=True):
    return (orc, s["lenses"], s["table"], s["gaps"], s["glass"], s["gapa"], s["rays"], s["channel"],
            s["w_in"] if rows else None, s["p_in"] if rows else None)


@pytest.mark.parametrize("name", NAMES)
def test_budget_0_is_absorb_ref(orc, scenes, name):
    s = scenes[name]
    log = {}
    got = bidir_ref.chain(*args_of(orc, s), 0, log=log)
    want = absorb_ref.chain(*args_of(orc, s), 0)
    all_back = np.array(log["all_back"])
    print(f"{name}: {int((~all_back).sum())} of {all_back.size} rays left glass through a surface facing backward")
    assert all_back.all()  # every traced ray of these scenes: the comparison below covers them all
    assert not differ(got, want)[all_back].any()
    assert not any(log["draws"]) and int((want[2] == 2).sum()) > 1200
    assert set(np.unique(got[2])) <= {bidir_ref.RR_NONE, bidir_ref.RR_OUTSIDE}


@pytest.mark.parametrize("name", NAMES)
def test_path_kinds(orc, scenes, name):
    s = scenes[name]
    log = {}
    got = bidir_ref.chain(*args_of(orc, s), 4, log=log)
    a, b, c = bidir_ref.kinds(got[2], log)
    print(f"{name} side 64, four channels: kinds a {int(a.sum())}, b {int(b.sum())}, c {int(c.sum())}")
    assert int(a.sum()) >= KIND_FLOOR
    if name == "cfg2":
        assert not b.any() and not c.any()  # one lens: no neighbour to come back from
        return
    cfg = CONFIGS["cfg2" if name == "doublet" else name]
    rays = grid_rays(cfg, side=KIND_SIDE[name])
    n = rays.shape[1]
    log = {}
    got = bidir_ref.chain(orc, s["lenses"], s["table"], s["gaps"], s["glass"], s["gapa"], rays,
                          np.full(n, KIND_CHANNEL, np.uint8), None, None, 4, log=log)
    a, b, c = bidir_ref.kinds(got[2], log)
    print(f"{name} side {KIND_SIDE[name]}, channel {KIND_CHANNEL}: kinds a {int(a.sum())}, b {int(b.sum())}, c {int(c.sum())}")
    assert min(int(a.sum()), int(b.sum()), int(c.sum())) >= KIND_FLOOR
    # a kind-(b) ray met lens 1 and then lens 0 again; a kind-(c) ray met lens 1 twice with lens 0 in between
    i = int(np.nonzero(b)[0][0])
    assert 1 in log["lenses"][i] and log["lenses"][i][-1] == 0 and got[2][i] == bidir_ref.RR_BACK
    i = int(np.nonzero(c)[0][0])
    assert log["lenses"][i][-1] == 1 and got[4][i] >= 2 and got[2][i] == bidir_ref.RR_OUTSIDE


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("max_bounces", (1, 4, 8))
def test_consequences(orc, scenes, name, max_bounces):
    """Without absorption and with weight 1: a ray that ends with budget left kept its weight bit for bit, no weight
    grew, the segments stay within the bound, the statuses are NONE, OUTSIDE or BACK, and the draws sit at the
    segments' ordinals."""
    s = scenes[name]
    log = {}
    args = (orc, s["lenses"], s["table"], s["gaps"], None, None, s["rays"], s["channel"], s["w_in"], None)
    out, w, status, seg, bounces, path, glass = bidir_ref.chain(*args, max_bounces, log=log)
    assert set(np.unique(status)) <= {0, 2, 4} and int((status == 4).sum()) >= 100
    left = bounces < max_bounces
    assert np.array_equal(w[left].view(np.uint32), s["w_in"][left].view(np.uint32)) and int(left.sum()) > 3000
    assert (w <= s["w_in"]).all()
    assert (seg <= bidir_ref.segment_bound(len(s["lenses"]), max_bounces)).all() and (bounces <= max_bounces).all()
    for i, draws in enumerate(log["draws"]):
        assert all(0 <= e < seg[i] for e, _, _ in draws)
        assert len(log["lenses"][i]) == seg[i] or status[i] == 0 and seg[i] == 1


def test_rows_do_not_steer_the_walk(orc, scenes):
    """The draws read T and the ray number alone: random weight and path rows change neither rays nor counts."""
    s = scenes["cfg4"]
    a = bidir_ref.chain(*args_of(orc, s), 4)
    b = bidir_ref.chain(*args_of(orc, s, rows=False), 4)
    for k in (0, 2, 3, 4, 6):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
