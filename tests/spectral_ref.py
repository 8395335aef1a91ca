"""Reference for the spectral tests: a chain over rays with mixed channels is, ray for ray, the union of the
single-index chains of each channel's rays.

Nothing here comes from the code under test.  For each channel present, power_ref.chain (the oracle composed segment
by segment, the Fresnel term in numpy float32) runs over that channel's rays with that channel's column of the index
table; the results are scattered back to the rays' places.  A ray whose channel is not below nchan is not traced: as
the contract says, it comes back with status NONE, one segment and its ray and weight as they were.
"""
import numpy as np

import power_ref

F = np.float32


def chain(orc, lenses, ri_table, rays, channel, weight=None):
    """(rays [6, n], weight [n], status [n], segments [n]) of the chain with ri_table[l][channel[i]] for ray i."""
    table = np.asarray(ri_table, F)
    rays = np.ascontiguousarray(rays, F)
    channel = np.asarray(channel)
    n = rays.shape[1]
    assert table.ndim == 2 and table.shape[0] == len(lenses) and channel.shape == (n,)
    out = rays.copy()
    w = np.ones(n, F) if weight is None else np.array(weight, F)
    status = np.zeros(n, np.uint32)
    seg = np.ones(n, np.uint32)
    for c in range(table.shape[1]):
        idx = np.nonzero(channel == c)[0]
        if idx.size == 0:
            continue
        o, wc, s, g = power_ref.chain(orc, lenses, [float(x) for x in table[:, c]], rays[:, idx], w[idx])
        out[:, idx], w[idx], status[idx], seg[idx] = o, wc, s, g
    return out, w, status, seg
