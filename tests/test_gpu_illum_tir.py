"""bzr_illuminate_tir on the GPU: illumination through the chain that reflects, its stray-light maps and its bounce
ledger, against tests/illum_tir_ref.py bit for bit (everything compared is an integer).

The scenes are the cfg2 lens with ROW1's four indices and 10 000 rays of a wide emitter: `near` (1 unit in front of
the lens, inside its bounding sphere: nothing is culled, 394 rays reflect) and `far` (further back and off to the side:
over half of the rays miss the sphere and are culled, so culled and reflecting rays share batches and waves).  tests/test_illum_tir_ref.py asserts the populations.
"""
import ctypes
import itertools

import numpy as np
import pytest

import illum_tir_ref as itr
import power_ref
from test_gpu_power import culled_by_sphere, set_cap

pytestmark = pytest.mark.gpu

F = np.float32
N = itr.N_RAYS
TABLE, TABLE3, TABLE_CFG4 = [itr.ROW1], [itr.ROW1[:3]], [itr.ROW1, itr.ROW2]
OUTPUTS = ("flux", "hist", "rflux", "rhist", "stats", "power", "lcount", "lpower")
KEYS = ("emitted", "culled", "exited", "landed")


@pytest.fixture(scope="module")
def world(bzr, orc, ctx):
    """The lenses, their device meshes on the session context and the references, each computed once and frozen."""
    lenses = {"cfg2": itr.lenses_of(bzr, "cfg2"), "cfg4": itr.lenses_of(bzr, "cfg4")}
    dms = {k: [bzr.DeviceMesh(ctx, p) for p in v] for k, v in lenses.items()}
    tables = {"cfg2": TABLE, "cfg2x3": TABLE3, "cfg4": TABLE_CFG4}
    cache = {}

    def ref(name, origin, budget):
        key = (name, origin, budget)
        if key not in cache:
            cache[key] = itr.reference(orc, lenses[name.split("x")[0]], tables[name], origin, budget)
        return cache[key]

    return lenses, dms, ref


def run(bzr, ctx, dms, table, origin, budget, mode, **kw):
    return bzr.illuminate_tir(ctx, dms, table, itr.emitter(bzr, origin), N, itr.target(bzr), max_bounces=budget, mode=mode,
                              **kw)


def identities(got, added_rflux, label, lossless=False):
    """include/bzr.h, bzr_illuminate_tir: what holds by construction.  LOST + EXITED partition the traced rays; the
    ledger's power is what the rays ended with, so against the emitted power that line is an equality only where no
    surface takes power (a Fresnel transmittance is at most 1, and q is monotone: never more than was emitted)."""
    _, _, _, _, stats, power, ledger = got
    for c in range(len(stats)):
        for led, tot in ((ledger["count"], stats), (ledger["power"], power)):
            assert int(led[c, :, itr.EXITED].sum()) == tot[c]["exited"], (label, c)
            assert int(led[c, :, itr.LANDED].sum()) == tot[c]["landed"], (label, c)
        assert int(ledger["count"][c, :, :2].sum()) == stats[c]["emitted"] - stats[c]["culled"], (label, c)
        traced_power = power[c]["emitted"] - power[c]["culled"]
        if lossless:
            assert int(ledger["power"][c, :, :2].sum()) == traced_power, (label, c)
        else:
            assert int(ledger["power"][c, :, :2].sum()) <= traced_power, (label, c)
        assert int(ledger["power"][c, 1:, itr.LANDED].sum()) == int(added_rflux[c].sum()), (label, c)


def check(bzr, dm, ref, got, label):
    """Every output against the reference, exactly; returns which rays the sphere cull drops."""
    flux, hist, rflux, rhist, stats, power, ledger = got
    shape = (ref.nchan, 48, 48)
    for a, dtype, want in ((flux, np.uint64, ref.flux), (hist, np.uint32, ref.hist), (rflux, np.uint64, ref.rflux),
                           (rhist, np.uint32, ref.rhist)):
        assert a.dtype == dtype and a.shape == shape, label
        assert np.array_equal(a, want), label
    culled = culled_by_sphere(bzr.bounding_sphere(dm), ref.rays)
    want_count, want_power = itr.ledger_for(ref, culled)
    q0 = power_ref.q32(ref.w0)
    assert len(stats) == len(power) == ref.nchan
    for c in range(ref.nchan):
        mine = culled & (ref.channel == c)
        assert stats[c] == dict(zip(KEYS, (ref.emitted[c], int(mine.sum()), int(want_count[c, :, itr.EXITED].sum()),
                                           int(ref.hist[c].sum())))), (label, c)
        assert power[c] == dict(zip(KEYS, (ref.emitted_q[c], int(q0[mine].sum()),
                                           int(want_power[c, :, itr.EXITED].sum()), int(ref.flux[c].sum())))), (label, c)
    for k, want in (("count", want_count), ("power", want_power)):
        assert ledger[k].dtype == np.uint64 and ledger[k].shape == (ref.nchan, itr.ROWS, itr.FIELDS), (label, k)
        assert np.array_equal(ledger[k], want), (label, k, ledger[k].sum(axis=0), want.sum(axis=0))
    identities(got, rflux, label)
    return culled


# ------------------------------------------------------------------ 1. bit-exact, near scene
@pytest.mark.parametrize("budget", (1, 4, 8))
def test_near_scene_bit_exact(bzr, ctx, pipe, world, budget):
    _, dms, ref = world
    r = ref("cfg2", itr.NEAR, budget)
    assert int(itr.reflected(r).sum()) >= 300
    got = run(bzr, ctx, dms["cfg2"], TABLE, itr.NEAR, budget, pipe)
    culled = check(bzr, dms["cfg2"][0], r, got, f"near, budget {budget}")
    assert not culled.any()  # the emitter lies inside the lens's sphere
    if budget == 4:
        assert got[6]["count"][:, 1:5].sum(axis=0).tolist() == [[10, 41, 0], [2, 174, 108], [0, 11, 0], [53, 103, 31]]


# ------------------------------------------------------------------ 2. far scene: culled and reflecting rays
def test_far_scene(bzr, ctx, pipe, world):
    """The emitter at (4, -3, 4.5): 5 356 of the 10 000 rays miss the lens's sphere and 130 reflect.  (At
    (4, -3, -1.5) the rectangle lies inside the sphere -- centre (9.92, 0.02, -1.89), radius 8.39 -- and no ray is
    culled; moved along x alone it gives 272 culled / 83 reflecting at x = 2 and 4 071 / 63 at x = 1.)"""
    _, dms, ref = world
    r = ref("cfg2", itr.FAR, 4)
    got = run(bzr, ctx, dms["cfg2"], TABLE, itr.FAR, 4, pipe)
    check(bzr, dms["cfg2"][0], r, got, "far, budget 4")
    stats, power, ledger = got[4], got[5], got[6]
    assert sum(s["culled"] for s in stats) > 2000
    assert int(itr.reflected(r).sum()) >= 80
    # the traced / culled split, whichever side of the sphere a borderline ray falls: the reference traces every ray
    for c in range(4):
        assert int(ledger["count"][c, 0, itr.LOST]) + stats[c]["culled"] == int(r.uncut_count[c, 0, itr.LOST]), c
        assert int(ledger["power"][c, 0, itr.LOST]) + power[c]["culled"] == int(r.uncut_power[c, 0, itr.LOST]), c


# ------------------------------------------------------------------ 3. three batches
@pytest.fixture(scope="module")
def cctx(bzr, ctx):
    """This module's own context: the session context never sees a lowered chunk cap."""
    c = bzr.Context(0)
    yield c
    c.close()


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4] and a[5] == b[5] and \
        all(np.array_equal(a[6][k], b[6][k]) for k in ("count", "power"))


def test_three_batches(bzr, cctx, pipe, world):
    """10 000 rays at a chunk cap of 4 096: batches two and three reuse batch one's bounce and pending rows, and most of
    their rays are culled -- a row left stale sends culled rays into the bounce stages or into the ledger's rows.
    With three channels the batches start in channels 0, 1 and 2."""
    lenses, _, ref = world
    dm = [bzr.DeviceMesh(cctx, lenses["cfg2"][0])]
    fused = pipe == bzr.PIPELINE_FUSED
    try:
        assert set_cap(bzr, cctx, 0) >= 1 << 14
        one = run(bzr, cctx, dm, TABLE, itr.FAR, 4, pipe)
        one3 = run(bzr, cctx, dm, TABLE3, itr.FAR, 4, pipe)
        assert set_cap(bzr, cctx, 4096) == 4096
        cctx.timing(True)
        cctx.timing_report()
        got = run(bzr, cctx, dm, TABLE, itr.FAR, 4, pipe)
        rep = cctx.timing_report()
        cctx.timing(False)
        got3 = run(bzr, cctx, dm, TABLE3, itr.FAR, 4, pipe)
    finally:
        cctx.timing(False)
        set_cap(bzr, cctx, 0)
    # fused: one k_trace per batch; staged: per batch the INSIDE stage and 1 + 4 OUTSIDE stages
    assert rep["k_trace" if fused else "k_traverse"][1] == (3 if fused else 3 * 6)
    assert same(got, one) and same(got3, one3)
    check(bzr, dm[0], ref("cfg2", itr.FAR, 4), got, "three batches, four channels")
    r3 = ref("cfg2x3", itr.FAR, 4)
    assert int(itr.reflected(r3).sum()) >= 20
    check(bzr, dm[0], r3, got3, "three batches, three channels")


# ------------------------------------------------------------------ 4. zero budget
@pytest.mark.parametrize("fast", (False, True))
def test_zero_budget_is_illuminate_spectral(bzr, ctx, pipe, world, fast):
    _, dms, _ = world
    mode = pipe | (bzr.MODE_FAST if fast else 0)
    want = bzr.illuminate_spectral(ctx, dms["cfg2"], TABLE, itr.emitter(bzr, itr.NEAR), N, itr.target(bzr), mode=mode)
    got = run(bzr, ctx, dms["cfg2"], TABLE, itr.NEAR, 0, mode)
    assert sum(s["landed"] for s in want[2]) > 2000
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[4] == want[2] and got[5] == want[3]
    assert not got[2].any() and not got[3].any()
    assert not got[6]["count"][:, 1:].any() and not got[6]["power"][:, 1:].any()
    identities(got, got[2], f"zero budget, fast={fast}")


# ------------------------------------------------------------------ 5. identities under FAST
def test_fast_identities(bzr, ctx, pipe, world):
    _, dms, _ = world
    got = run(bzr, ctx, dms["cfg2"], TABLE, itr.NEAR, 4, pipe | bzr.MODE_FAST)
    identities(got, got[2], "FAST, budget 4")
    assert int(got[6]["count"][:, 1:].sum()) >= 300 and int(got[3].sum()) >= 100


# ------------------------------------------------------------------ 6. accumulation and optional outputs
def raw(bzr, ctx, dms, table, origin, budget, out, flags=0, rad=(1, 1), n=N, nchan=None, nlens=None, null_table=False):
    """The C entry point itself; `out` maps OUTPUTS' names to arrays, a missing name is passed as NULL.  Returns the
    status."""
    em, tg = itr.emitter(bzr, origin), itr.target(bzr)
    handles = (ctypes.c_void_p * max(len(dms), 1))(*[m.handle for m in dms])
    tab = np.ascontiguousarray(table, F)
    r = bzr.Radiometry(*rad) if rad is not None else None
    p = [out[k].ctypes.data if out.get(k) is not None else None for k in OUTPUTS]
    return bzr.lib().bzr_illuminate_tir(ctx.handle, ctypes.cast(handles, ctypes.c_void_p),
                                        None if null_table else tab.ctypes.data,
                                        len(dms) if nlens is None else nlens, tab.shape[1] if nchan is None else nchan,
                                        ctypes.byref(em), n, ctypes.byref(tg), ctypes.byref(r) if r is not None else None,
                                        budget, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], flags)


def buffers(nchan=4, fill=0):
    return {"flux": np.full((nchan, 48, 48), fill, np.uint64), "hist": np.full((nchan, 48, 48), fill, np.uint32),
            "rflux": np.full((nchan, 48, 48), fill, np.uint64), "rhist": np.full((nchan, 48, 48), fill, np.uint32),
            "stats": np.full((nchan, 4), fill, np.uint64), "power": np.full((nchan, 4), fill, np.uint64),
            "lcount": np.full((nchan, itr.ROWS, itr.FIELDS), fill, np.uint64),
            "lpower": np.full((nchan, itr.ROWS, itr.FIELDS), fill, np.uint64)}


def test_accumulation(bzr, ctx, pipe, world):
    _, dms, ref = world
    r = ref("cfg2", itr.NEAR, 4)
    got = run(bzr, ctx, dms["cfg2"], TABLE, itr.NEAR, 4, pipe)
    again = run(bzr, ctx, dms["cfg2"], TABLE, itr.NEAR, 4, pipe, flux=got[0], hist=got[1], reflected_flux=got[2],
                reflected_hist=got[3])
    assert all(again[k] is got[k] for k in range(4))
    for a, want in zip(got[:4], (r.flux, r.hist, r.rflux, r.rhist)):
        assert np.array_equal(a, want * 2)
    assert again[4:6] == got[4:6] and np.array_equal(again[6]["count"], got[6]["count"])  # overwritten, not added


def test_optional_outputs_in_any_combination(bzr, ctx, pipe, world):
    _, dms, _ = world
    full = buffers()
    assert raw(bzr, ctx, dms["cfg2"], TABLE, itr.NEAR, 4, full, pipe) == 0
    assert full["rhist"].sum() >= 100
    optional = OUTPUTS[1:]  # flux_q32 is required
    for mask in itertools.product((False, True), repeat=len(optional)):
        out = buffers()
        for name, given in zip(optional, mask):
            if not given:
                del out[name]
        assert raw(bzr, ctx, dms["cfg2"], TABLE, itr.NEAR, 4, out, pipe) == 0, mask
        for name, a in out.items():
            assert np.array_equal(a, full[name]), (mask, name)


def test_uniform_lossless_is_the_count(bzr, ctx, pipe, world):
    _, dms, ref = world
    r = ref("cfg2", itr.NEAR, 4)
    flux, hist, rflux, rhist, stats, power, ledger = run(bzr, ctx, dms["cfg2"], TABLE, itr.NEAR, 4, pipe,
                                                         emission=bzr.EMISSION_UNIFORM, surface=bzr.SURFACE_LOSSLESS)
    assert np.array_equal(hist, r.hist) and np.array_equal(rhist, r.rhist)  # the rays refract and reflect as before
    assert np.array_equal(flux, hist.astype(np.uint64) << np.uint64(32))
    assert np.array_equal(rflux, rhist.astype(np.uint64) << np.uint64(32))
    assert np.array_equal(ledger["power"], ledger["count"] << np.uint64(32))
    assert int(rhist.sum()) >= 100
    for c in range(4):
        assert power[c] == {k: v << 32 for k, v in stats[c].items()}
    identities((flux, hist, rflux, rhist, stats, power, ledger), rflux, "uniform, lossless", lossless=True)
    # a Lambert emitter with lossless surfaces: the weights stay as emitted, so the traced power is all accounted for
    got = run(bzr, ctx, dms["cfg2"], TABLE, itr.FAR, 4, pipe, surface=bzr.SURFACE_LOSSLESS)
    identities(got, got[2], "Lambert, lossless, far", lossless=True)
    assert sum(s["culled"] for s in got[4]) > 2000


# ------------------------------------------------------------------ 7. device buffers
def test_device_buffers(bzr, ctx, pipe, world):
    torch = pytest.importorskip("torch")
    _, dms, _ = world
    want = run(bzr, ctx, dms["cfg2"], TABLE, itr.NEAR, 4, pipe)
    shape = (4, 48, 48)
    flux, rflux = (torch.zeros(shape, dtype=torch.int64, device="cuda") for _ in range(2))
    hist, rhist = (torch.zeros(shape, dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    ctx.use_torch_stream()
    try:
        got = run(bzr, ctx, dms["cfg2"], TABLE, itr.NEAR, 4, pipe, flux=flux, hist=hist, reflected_flux=rflux,
                  reflected_hist=rhist)
        torch.cuda.synchronize()
    finally:
        ctx.use_own_stream()
    assert got[0] is flux and got[3] is rhist
    for a, b, dtype in zip(got[:4], want[:4], (np.uint64, np.uint32, np.uint64, np.uint32)):
        assert np.array_equal(a.cpu().numpy().view(dtype), b)
    assert got[4:6] == want[4:6]
    assert all(np.array_equal(got[6][k], want[6][k]) for k in ("count", "power"))
    assert int(want[3].sum()) >= 100  # reflected rays land in the device maps


# ------------------------------------------------------------------ 8. bad arguments
def test_bad_arguments_leave_the_outputs_untouched(bzr, ctx, world):
    _, dms, _ = world
    dm = dms["cfg2"]

    def rejected(match, *args, drop=(), **kw):
        out = buffers(fill=5)
        given = {k: v for k, v in out.items() if k not in drop}
        assert raw(bzr, ctx, *args, given, **kw) == 1, match  # BZR_ERR_INVALID_ARGUMENT
        assert match in bzr.lib().bzr_last_error().decode(), (match, bzr.lib().bzr_last_error())
        for name, a in out.items():
            assert (a == 5).all(), (match, name)

    rejected("max_bounces", dm, TABLE, itr.NEAR, 9)
    rejected("radiometry", dm, TABLE, itr.NEAR, 4, rad=None)
    rejected("flux_q32", dm, TABLE, itr.NEAR, 4, drop=("flux",))
    rejected("ri_table", dm, TABLE, itr.NEAR, 4, null_table=True)
    rejected("nchan", dm, TABLE, itr.NEAR, 4, nchan=0)
    rejected("nchan", dm, np.full((1, 65), 1.3, F), itr.NEAR, 4)
    rejected("nlens", dm, TABLE, itr.NEAR, 4, nlens=0)
    rejected("nlens", dm * 9, np.full((9, 4), 1.3, F), itr.NEAR, 4)
    rejected("2^32", dm, TABLE, itr.NEAR, 4, n=1 << 32)
    rejected("emission", dm, TABLE, itr.NEAR, 4, rad=(2, 1))
    rejected("surface", dm, TABLE, itr.NEAR, 4, rad=(1, 2))
    flux = np.full((4, 48, 48), 5, np.uint64)
    with pytest.raises(bzr.BzrError, match="max_bounces"):  # through the wrapper
        run(bzr, ctx, dm, TABLE, itr.NEAR, 9, 0, flux=flux)
    assert (flux == 5).all()


# ------------------------------------------------------------------ 9. two lenses
def test_two_lenses(bzr, ctx, pipe, world):
    """Bounces are summed over the lenses, so a ray can carry more than one lens's budget: row min(bounces, 8)."""
    _, dms, ref = world
    r = ref("cfg4", itr.NEAR, 4)
    assert int(itr.reflected(r).sum()) >= 400 and int(r.bounces.max()) > 4
    after = [int(((r.channel == c) & itr.reflected(r) & (r.status == itr.RR_OUTSIDE)).sum()) for c in range(4)]
    assert min(after) >= 10, after
    got = run(bzr, ctx, dms["cfg4"], TABLE_CFG4, itr.NEAR, 4, pipe)
    check(bzr, dms["cfg4"][0], r, got, "cfg4, budget 4")
