"""Far-field cells computed independently of the cell rule's operations, in numpy binary64: the polar angle by arccos,
the azimuth by arctan2, the radius rho = 2 sin(theta / 2) -- the textbook form of the Lambert azimuthal equal-area
projection -- and per-cell lower and upper bounds on what a binary32 evaluation of include/bzr.h's rule may count.
Nothing here comes from the code under test or from farfield_ref's restatement.

The margin.  For a direction d of length 1 +- 1e-6 the rule computes, with eps = 2^-24 the unit roundoff of binary32:
  mu, a, b   three products and two sums each, |d| |axis| ~ 1: an error of 3 eps at the most; the pole the device uses is
             the binary32 normalisation of axis_u x axis_v (two roundings per component of the cross product, one
             each for the norm's square root and the division): within 5 eps of the binary64 pole used here, so mu is
             within 8 eps;
  g = 1 + mu one rounding of a number below 2: within 10 eps of 1 + cos(theta);
  k = sqrt(2 / g)   the relative error of g halves under the root, plus one rounding each for the quotient and the
             root: |dk| / k <= 5 eps / g + 1.5 eps;
  X = a k    |dX| <= k 3 eps + |X| (5 eps / g + 1.5 eps) + eps |X|;
  u = X + R, u / cu   one rounding each of numbers below 2 R + |X|: 2 eps (|X| + 2 R) in units of X.
A direction that is not exactly unit moves X by |X| (1 + 1 / g) | |d| - 1 | at the most (a scales with |d|, g with its
cosine part).  arccos in binary64 loses half the digits at the pole: 2e-8 on theta there, which is added flat.  The sum,
doubled, is the ray's margin m; the same bound serves Y.  A ray counts towards a cell's lower bound when the four points
(X +- m, Y +- m) all lie in that cell, and towards the upper bound of every cell one of them lies in.
"""
import numpy as np

EPS = 2.0 ** -24


def project(fr, d):
    """(X, Y, margin) in binary64 for directions d [3, n] (any float type) and a farfield_ref.frame (its binary32 axes
    and extent are the inputs; the pole is made here)."""
    d = np.asarray(d, np.float64)
    au, av = np.asarray(fr.axis_u, np.float64), np.asarray(fr.axis_v, np.float64)
    pole = np.cross(au, av)
    pole /= np.linalg.norm(pole)
    length = np.linalg.norm(d, axis=0)
    theta = np.arccos(np.clip((pole @ d) / length, -1.0, 1.0))
    phi = np.arctan2(av @ d, au @ d)
    rho = 2.0 * np.sin(theta / 2.0)
    X, Y = rho * np.cos(phi), rho * np.sin(phi)
    g = 1.0 + np.cos(theta)
    k = np.sqrt(2.0 / g)
    R = float(fr.R)
    m = k * 3 * EPS + rho * (5 * EPS / g + 2.5 * EPS) + 2 * EPS * (rho + 2 * R) \
        + rho * (1 + 1 / g) * np.abs(length - 1.0) + 2e-8
    return X, Y, 2.0 * m


def cells(fr, X, Y):
    """Cell index of map points in binary64, -1 outside [-R, R)^2."""
    R = float(fr.R)
    u, v = X + R, Y + R
    ok = (u >= 0) & (u < 2 * R) & (v >= 0) & (v < 2 * R)
    iu = np.minimum(np.floor(np.where(ok, u, 0) / (2 * R / fr.bins_u)).astype(np.int64), fr.bins_u - 1)
    iv = np.minimum(np.floor(np.where(ok, v, 0) / (2 * R / fr.bins_v)).astype(np.int64), fr.bins_v - 1)
    return np.where(ok, iv * fr.bins_u + iu, -1)


def bounds(fr, d):
    """(lower, upper) int64 [bins_v, bins_u] on the count of each cell for directions d [3, n], every ray seen, and the
    number of rays whose cell the margin leaves open."""
    X, Y, m = project(fr, d)
    # a ray further than 0.05 outside the map's circumscribed circle is outside whatever its margin below 0.05 (the
    # margin grows as 1 / g towards the direction opposite the pole)
    out = np.hypot(X, Y) > np.sqrt(2.0) * float(fr.R) + 0.05
    assert np.isfinite(m).all() and (m[out] < 0.05).all()
    m = np.where(out, 0.0, m)
    assert m.max() < 0.1 * min(2 * float(fr.R) / fr.bins_u, 2 * float(fr.R) / fr.bins_v)
    corner = np.stack([cells(fr, X + sx * m, Y + sy * m) for sx in (-1, 1) for sy in (-1, 1)])
    sure = (corner == corner[0]).all(axis=0)
    lower = np.bincount(corner[0][sure & (corner[0] >= 0)], minlength=fr.cells)
    upper = lower.copy()
    for i in np.nonzero(~sure)[0]:
        for c in set(corner[:, i].tolist()) - {-1}:
            upper[c] += 1
    shape = (fr.bins_v, fr.bins_u)
    return lower.reshape(shape), upper.reshape(shape), int((~sure).sum())
