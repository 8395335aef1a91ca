"""The illumination path's two ends in binary64: the emitter (bzr_emit) and the landing step of bzr_illuminate*.

A plain helper module like ref64.py / chain64.py (no fixtures, no plugin), written from include/bzr.h's text
(bzr_emitter, bzr_target), not from the device code or the oracle's restatement of it.  The counter-based stream is
exact (np.uint64 arithmetic wraps mod 2^64); everything real-valued is binary64 with numpy's cos / sin / arccos.

emit64    ray numbers first .. first + n - 1 of an emitter: origins, directions, the uniforms (exact), part, point
          number, patch number, and which rays sit too close to a belt's or a patch's edge to be numbered for sure
land64    where float32 result rays (read as binary64) meet a target: the cell, whether binary32 could decide
          otherwise (`unsure`), and the cells an unsure ray may be in
bounds    per-cell lower and upper bounds of a count or flux map from land64, optionally per key
q32       the 32.32 fixed point of a float32 weight
emitter, target, TARGETS, FIRSTS, BELTS, N_RAYS   the inputs the CPU and the GPU tests share
"""
from types import SimpleNamespace

import numpy as np

F = np.float32
U64 = np.uint64
RR_NONE, RR_OUTSIDE = 0, 2
GOLDEN = U64(0x9E3779B97F4A7C15)
CS_MIN = float(F(0.00001))     # |d . n| below this: the ray does not meet the plane
K_MARGIN = 32                  # land64's margin factor; pinned on the oracle by tests/test_illum64.py, never on the device
NEAR = 1e-5                    # patch_near: incidence / belt width or tf * count within this of an integer

# ------------------------------------------------------------------ shared inputs
N_RAYS = 30_000                # no multiple of 64, nor of the 77 rays of a part
FIRSTS = (0, 2 ** 32 - 1000, 2 ** 40 + 7)
BELTS = (1, 5, 33)
OBLIQUE_X, FAR_X = 6.0, -40.0
PLAIN = SimpleNamespace(Emitter=SimpleNamespace, Target=SimpleNamespace)   # emitter(PLAIN), target(PLAIN, name): no library


def emitter(mod, x=OBLIQUE_X, belts=5, seed=12345):
    """The oblique emitter (x = OBLIQUE_X) or the far one (FAR_X): a rectangle on no coordinate plane, 3 x 5 parts of
    7 points x 11 rays (77 rays per part: no multiple of 64)."""
    return mod.Emitter(origin=(x, -2.0, -1.0), edge_u=(0.5, 3.0, 0.4), edge_v=(-0.3, 0.2, 2.5), parts_u=3, parts_v=5,
                       points_per_part=7, rays_per_point=11, belts=belts, seed=seed)


def _tilted_axes():
    """The y and z axes rotated 20 degrees about z and then 10 degrees about y, rounded to float32."""
    a, b = np.radians(20.0), np.radians(10.0)
    rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    ry = np.array([[np.cos(b), 0.0, np.sin(b)], [0.0, 1.0, 0.0], [-np.sin(b), 0.0, np.cos(b)]])
    m = ry @ rz
    return tuple(float(v) for v in m[:, 1].astype(F)), tuple(float(v) for v in m[:, 2].astype(F))


_TILT_U, _TILT_V = _tilted_axes()
_PLAIN_U, _PLAIN_V = (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
# name -> (origin x, axis_u, axis_v, (size_u, size_v), (bins_u, bins_v)); "<name>_swapped" is its twin with u and v
# exchanged.  plain / coarse: cells 0.5 x 1.25 and 1 x 2.5, all exact, the coarse map is the fine one's 2 x 2 block sums.
_TARGETS = {
    "plain": (24.0, _PLAIN_U, _PLAIN_V, (20.0, 30.0), (40, 24)),
    "coarse": (24.0, _PLAIN_U, _PLAIN_V, (20.0, 30.0), (20, 12)),
    "tilted": (24.0, _TILT_U, _TILT_V, (22.0, 30.0), (40, 24)),
    "behind": (-5.0, _PLAIN_U, _PLAIN_V, (20.0, 30.0), (40, 24)),   # behind the emitter: nothing lands
    # for the block-sum identity on tilted axes only: the exact cells of plain / coarse
    "tilted20": (24.0, _TILT_U, _TILT_V, (20.0, 30.0), (40, 24)),
    "tilted20_coarse": (24.0, _TILT_U, _TILT_V, (20.0, 30.0), (20, 12)),
}
TARGETS = tuple(n + s for n in ("plain", "coarse", "tilted") for s in ("", "_swapped")) + ("behind",)


def target(mod, name):
    swapped = name.endswith("_swapped")
    x, au, av, size, bins = _TARGETS[name.removesuffix("_swapped")]
    if swapped:
        au, av, size, bins = av, au, size[::-1], bins[::-1]
    return mod.Target(origin=(x, -10.0, -14.0), axis_u=au, axis_v=av, size_u=size[0], size_v=size[1], bins_u=bins[0],
                      bins_v=bins[1])


# ------------------------------------------------------------------ the stream
def mix64(z):
    """The splitmix64 finaliser on a np.uint64 array."""
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def uniform2(seed, key, stream):
    """U(key, stream): two 24-bit uniforms in [0, 1) per key (np.uint64 array), exact in binary64."""
    key = np.asarray(key, U64)
    h = mix64(U64(seed) + GOLDEN * (U64(2) * key + U64(stream + 1)))
    return (h >> U64(40)).astype(np.float64) / 2.0 ** 24, ((h >> U64(16)) & U64(0xFFFFFF)).astype(np.float64) / 2.0 ** 24


def belt_counts(belts):
    """count[i] = ceil(4 belts sin((2 i + 1) pi / (4 belts))) and first[i] as int64 arrays.  The sine's argument is
    the binary32 value of (2 i + 1) / (4 belts) * pi, each step rounded, as the header states: where 4 belts sin(.) comes
    within rounding of an integer that decides the count (it does for one belt of 4096)."""
    i = np.arange(belts, dtype=F)
    arg = (F(2) * i + F(1)) / (F(4) * F(belts)) * F(np.pi)
    assert arg.dtype == F
    count = np.ceil(4.0 * belts * np.sin(arg.astype(np.float64))).astype(np.int64)
    return count, np.concatenate(([0], np.cumsum(count)[:-1]))


def _vec(v):
    return np.array([float(x) for x in v], np.float64)


def emit64(em, first, n):
    """Rays first .. first + n - 1 of `em` (a bzr_emitter-shaped structure)."""
    if not 1 <= em.belts <= 4096:
        raise ValueError("belts must be 1..4096")
    with np.errstate(over="ignore"):
        j = U64(first) + np.arange(n, dtype=U64)
        point = j // U64(em.rays_per_point)
        part = (j // U64(em.points_per_part * em.rays_per_point)) % U64(em.parts_u * em.parts_v)
        ci, tf = uniform2(em.seed, j, 0)
        u, v = uniform2(em.seed, point, 1)
    pu, pv = (part % U64(em.parts_u)).astype(np.int64), (part // U64(em.parts_u)).astype(np.int64)
    a, b = (pu + u) / em.parts_u, (pv + v) / em.parts_v
    o = _vec(em.origin)[:, None] + _vec(em.edge_u)[:, None] * a + _vec(em.edge_v)[:, None] * b
    si = np.sqrt(1.0 - ci * ci)
    turn = 2.0 * np.pi * tf
    d = np.stack([ci, si * np.cos(turn), si * np.sin(turn)])
    d /= np.sqrt((d * d).sum(axis=0))
    count, firsts = belt_counts(em.belts)
    x = np.arccos(ci) / (np.pi / 2.0 / em.belts)          # the incidence in belt widths
    belt = np.minimum(np.floor(x).astype(np.int64), em.belts - 1)
    y = tf * count[belt]
    patch = firsts[belt] + np.minimum(np.floor(y).astype(np.int64), count[belt] - 1)
    near = (np.abs(x - np.rint(x)) < NEAR) | (np.abs(y - np.rint(y)) < NEAR)
    return SimpleNamespace(o=o, d=d, ci=ci, tf=tf, pu=pu, pv=pv, point=point, patch=patch, patch_near=near, a=a, b=b)


def solve_ab(em, origins):
    """(a, b) of points on the emitter's plane, least squares in binary64 from the two edges."""
    m = np.stack([_vec(em.edge_u), _vec(em.edge_v)], axis=1)
    ab, *_ = np.linalg.lstsq(m, np.asarray(origins, np.float64) - _vec(em.origin)[:, None], rcond=None)
    return ab[0], ab[1]


DIR_TOL = 2e-6                 # per direction component: the polynomials truncate below 6e-8 and about 15 binary32
#                                roundings of <= 2^-24 act on magnitudes <= 1: under 1e-6, doubled
NORM_TOL = 4 * 2.0 ** -24      # | |d| - 1 |
NEAR_SHARE = 0.002             # patch_near may cover this share of the rays


def origin_tol(em):
    """Per component: 4 2^-23 (|origin| + |edge_u| + |edge_v|); three adds, two products and a quotient make at most
    3 of that unit."""
    return 4 * 2.0 ** -23 * (np.abs(_vec(em.origin)) + np.abs(_vec(em.edge_u)) + np.abs(_vec(em.edge_v)))


def check_emit(em, first, rays, patch):
    """Float32 rays [6, n] and patch numbers [n] claimed to be rays first .. first + n - 1 of `em`, against emit64 and
    the structure include/bzr.h promises.  Asserts; returns the measured maxima."""
    rays = np.asarray(rays)
    n = rays.shape[1]
    ref = emit64(em, first, n)
    r = rays.astype(np.float64)
    otol = origin_tol(em)
    derr, oerr = np.abs(r[3:] - ref.d).max(), np.abs(r[:3] - ref.o).max(axis=1)
    assert derr <= DIR_TOL, derr
    assert (oerr <= otol).all(), (oerr, otol)
    nerr = np.abs(np.sqrt((r[3:] * r[3:]).sum(axis=0)) - 1.0).max()
    assert nerr <= NORM_TOL, nerr
    differ = np.asarray(patch).astype(np.int64) != ref.patch
    assert not (differ & ~ref.patch_near).any(), np.flatnonzero(differ & ~ref.patch_near)[:8]
    assert ref.patch_near.mean() <= NEAR_SHARE, ref.patch_near.mean()
    # the rays of one point share one origin, bit for bit
    bits = rays[:3].view(np.uint32)
    same_point = ref.point[1:] == ref.point[:-1]
    assert same_point.sum() >= n - n // em.rays_per_point - 2
    assert (bits[:, 1:] == bits[:, :-1]).all(axis=0)[same_point].all()
    assert not (bits[:, 1:] == bits[:, :-1]).all(axis=0)[~same_point].any()
    # the origin lies in its part's sub-rectangle: (a, b) solved in binary64 from the edges
    a, b = solve_ab(em, r[:3])
    m = np.stack([_vec(em.edge_u), _vec(em.edge_v)], axis=1)
    abtol = np.sqrt((otol * otol).sum()) / np.linalg.svd(m, compute_uv=False).min()
    for got, want, p, parts in ((a, ref.a, ref.pu, em.parts_u), (b, ref.b, ref.pv, em.parts_v)):
        assert np.abs(got - want).max() <= abtol
        assert (want >= p / parts).all() and (want < (p + 1) / parts).all()
        assert (got >= p / parts - abtol).all() and (got <= (p + 1) / parts + abtol).all()
    # over a full cycle every part gets exactly points_per_part * rays_per_point rays: the part read off the rays
    per_part, parts = em.points_per_part * em.rays_per_point, em.parts_u * em.parts_v
    if n >= per_part * parts:
        got_part = np.floor(b * em.parts_v).astype(np.int64) * em.parts_u + np.floor(a * em.parts_u).astype(np.int64)
        start = (-first) % per_part                      # the first ray that begins a part
        cycle = got_part[start:start + per_part * parts]
        assert (np.bincount(cycle, minlength=parts) == per_part).all(), np.bincount(cycle, minlength=parts)
        assert (cycle.reshape(parts, per_part) == cycle.reshape(parts, per_part)[:, :1]).all()
        steps = np.diff(cycle.reshape(parts, per_part)[:, 0]) % parts
        assert (steps == 1).all(), steps                 # part by part, u fastest
    return {"direction": float(derr), "origin": float((oerr / otol).max()), "origin_abs": float(oerr.max()),
            "norm": float(nerr), "near": float(ref.patch_near.mean()), "patch_differs": int(differ.sum())}


# ------------------------------------------------------------------ landing
def _axis(coord, size, bins, margin):
    """One coordinate of the landing points: (index or -1 when off the target, near an edge, the edge's number)."""
    cell = size / bins
    with np.errstate(invalid="ignore"):
        k = np.clip(np.rint(coord / cell), 0, bins)       # the nearest grid line, the target's two edges included
        near = np.abs(coord - k * cell) < margin
        idx = np.where((coord >= 0.0) & (coord < size), np.minimum(np.floor(coord / cell), bins - 1), -1)
    return np.nan_to_num(idx, nan=-1).astype(np.int64), near & np.isfinite(coord), np.nan_to_num(k).astype(np.int64)


def land64(tg, rays, status, k_margin=K_MARGIN):
    """Float32 result rays [6, n] against `tg` (a bzr_target-shaped structure), per ray (rows of rays that did not end
    OUTSIDE are cell -1, sure, no candidates):
      cell [n]       the binary64 cell iv * bins_u + iu, or -1
      unsure [n]     binary32 might decide otherwise: within margin of a cell's or the target's edge, |t| < margin or
                     ||cs| - 1e-5| < 1e-7, margin = K 2^-23 (|s|_inf + |t| + |origin|_inf) / |cs|
      cand [n, 4]    the cells the ray may be in (-1: unused slot), the up to four around a corner for an unsure ray
      may_miss [n]   "none" is among the candidates
      exited [n]     status == OUTSIDE"""
    r = np.asarray(rays, F).astype(np.float64)
    s, d = r[:3], r[3:]
    exited = np.asarray(status) == RR_OUTSIDE
    org, au, av = _vec(tg.origin), _vec(tg.axis_u), _vec(tg.axis_v)
    nrm = np.cross(au, av)
    nrm /= np.sqrt(nrm @ nrm)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        cs = nrm @ d
        t = (nrm @ org - nrm @ s) / cs
        p = s + t * d - org[:, None]
        a, b = au @ p, av @ p
        margin = k_margin * 2.0 ** -23 * (np.abs(s).max(axis=0) + np.abs(t) + np.abs(org).max()) / np.abs(cs)
    margin = np.nan_to_num(margin, nan=np.inf)
    meets = (np.abs(cs) >= CS_MIN) & (t > 0.0)
    iu, near_u, ku = _axis(a, float(tg.size_u), tg.bins_u, margin)
    iv, near_v, kv = _axis(b, float(tg.size_v), tg.bins_v, margin)
    on = exited & meets & (iu >= 0) & (iv >= 0)
    cell = np.where(on, iv * tg.bins_u + iu, -1)
    with np.errstate(invalid="ignore"):
        plane_unsure = ~(np.abs(t) >= margin) | (np.abs(np.abs(cs) - CS_MIN) < 1e-7)
    # an edge matters only to a ray that meets the plane (or may) and is on the target in the other coordinate (or may be)
    edge_unsure = (near_u & ((iv >= 0) | near_v)) | (near_v & ((iu >= 0) | near_u))
    unsure = exited & (plane_unsure | (meets & edge_unsure))
    # candidates: per coordinate the index itself, or the two sides of the near edge (-1: off the target)
    us = np.stack([np.where(near_u, ku - 1, iu), np.where(near_u, np.where(ku < tg.bins_u, ku, -1), iu)])
    vs = np.stack([np.where(near_v, kv - 1, iv), np.where(near_v, np.where(kv < tg.bins_v, kv, -1), iv)])
    cand = np.full((len(cell), 4), -1, np.int64)
    for m, (x, y) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        ok = (us[x] >= 0) & (vs[y] >= 0)
        cand[:, m] = np.where(ok, vs[y] * tg.bins_u + us[x], -1)
    cand[~unsure] = -1
    cand[~unsure, 0] = cell[~unsure]
    cand[~exited] = -1
    # an unsure ray's own cell is always among its candidates; duplicates (a coordinate that is not near) are dropped
    for m in range(1, 4):
        dup = (cand[:, m:m + 1] == cand[:, :m]).any(axis=1)
        cand[dup, m] = -1
    may_miss = exited & np.where(unsure, plane_unsure | (us < 0).any(axis=0) | (vs < 0).any(axis=0) | ~meets, cell < 0)
    return SimpleNamespace(cell=cell, unsure=unsure, cand=cand, may_miss=may_miss, exited=exited)


def q32(w):
    """q(w) = trunc(w x 2^32) of float32 weights as uint64: the product is exact in binary64."""
    return np.trunc(np.asarray(w, F).astype(np.float64) * 2.0 ** 32).astype(U64)


def bounds(tg, rays, status, q=None, key=None, nkey=None, k_margin=K_MARGIN, landing=None):
    """Bounds of a target map from land64.  lo sums the sure rays, hi adds every unsure ray to each cell it may be in:
    lo, hi uint64 [bins_v, bins_u] or, with key [n] (small non-negative integers, a negative key leaves the ray out) and
    nkey, [nkey, bins_v, bins_u].  They count rays, or with q [n] (32.32 weights) sum q.  landed_lo / landed_hi [nkey]
    or scalars: the same for the map's total (an unsure ray counts once in landed_hi, and in landed_lo when it cannot
    miss).  unsure: how many of the rays taken are unsure."""
    ld = landing if landing is not None else land64(tg, rays, status, k_margin)
    n = len(ld.cell)
    scalar = key is None
    key = np.zeros(n, np.int64) if scalar else np.asarray(key).astype(np.int64)
    nk = 1 if scalar else int(nkey)
    wq = np.ones(n, U64) if q is None else np.asarray(q, U64)
    cells = tg.bins_u * tg.bins_v
    taken = ld.exited & (key >= 0)
    lo, hi = np.zeros(nk * cells, U64), np.zeros(nk * cells, U64)
    sure = taken & ~ld.unsure & (ld.cell >= 0)
    np.add.at(lo, key[sure] * cells + ld.cell[sure], wq[sure])
    hi += lo
    for m in range(4):
        c = ld.cand[:, m]
        mine = taken & ld.unsure & (c >= 0)
        np.add.at(hi, key[mine] * cells + c[mine], wq[mine])
    some = taken & ld.unsure & (ld.cand >= 0).any(axis=1)
    landed_lo, landed_hi = np.zeros(nk, U64), np.zeros(nk, U64)
    np.add.at(landed_lo, key[sure], wq[sure])
    certain = some & ~ld.may_miss
    np.add.at(landed_lo, key[certain], wq[certain])
    np.add.at(landed_hi, key[sure], wq[sure])
    np.add.at(landed_hi, key[some], wq[some])
    shape = (tg.bins_v, tg.bins_u) if scalar else (nk, tg.bins_v, tg.bins_u)
    return SimpleNamespace(lo=lo.reshape(shape), hi=hi.reshape(shape),
                           landed_lo=int(landed_lo[0]) if scalar else landed_lo,
                           landed_hi=int(landed_hi[0]) if scalar else landed_hi,
                           unsure=int((taken & ld.unsure).sum()), landing=ld)
