"""Test helpers (path cache handle lives in shadow-1_amd/sim.py)."""
import numpy as np

from sim import PathCache, SHD_PC_FORCE_ROWS  # noqa: F401


def oracle_table(g, att, rows):
    """The oracle's source rows `rows` (indices into `att`) to every attached
    target: lat, rel ((-1, -1) where computePathProperties fails), ok and hops
    as [len(rows), T] arrays, and the ties summed over those rows."""
    import oracle_ffi as O
    og = O.OGraph(g)
    n, T = len(rows), len(att)
    lat = np.empty((n, T)); rel = np.empty((n, T))
    ok = np.empty((n, T), np.int32); hops = np.empty((n, T), np.int32)
    ties = 0
    for k, r in enumerate(rows):
        lat[k], rel[k], ok[k], hops[k], t = og.row(att[r], att)
        ties += t
    lat[ok == 0] = -1.0
    rel[ok == 0] = -1.0
    return lat, rel, ok, hops, ties


def same_bits(a, b):
    """Bitwise equality of f64 arrays (NaN == NaN with the same payload)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
