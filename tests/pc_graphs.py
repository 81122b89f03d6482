"""Seeded graph builders and the case tables of the path-cache shape tests.

The GPU tests (test_pathcache_shapes_gpu.py, pc_switch_worker.py) and the CPU
test of their preconditions (test_pc_graphs_cpu.py) take their inputs from
here, so what the CPU test asserts is asserted of the very inputs the GPU
tests run.  numpy and the host library only: nothing here touches a device.
"""
import functools

import numpy as np

import shdgpu as S
import workloads as W


# ------------------------------------------------------------------ builders
def _vloss(rng, V, mode):
    """None: no vertex attribute; "all": a factor on every vertex (every target
    walks its parent chain); "mixed": absent (NaN) on even vertices."""
    if mode is None:
        return None
    assert mode in ("all", "mixed"), mode
    vl = rng.random(V) * 0.001
    if mode == "mixed":
        vl[::2] = np.nan
    return vl


def chain(V, seed=1, ring=False, self_loops=True, vertex_loss=None):
    """Path 0 - 1 - ... - V-1 (ring: closed by V-1 - 0), real-valued latencies
    1 + 9 U (no equal-cost paths), edges in a shuffled document order."""
    rng = np.random.default_rng(seed)
    src = np.arange(V - 1, dtype=np.int64)
    dst = src + 1
    if ring and V > 2:
        src = np.append(src, V - 1)
        dst = np.append(dst, 0)
    if self_loops:
        src = np.concatenate([src, np.arange(V)])
        dst = np.concatenate([dst, np.arange(V)])
    lat = 1.0 + 9.0 * rng.random(len(src))
    loss = rng.random(len(src)) * 0.01
    perm = rng.permutation(len(src))
    return S.GraphArrays(V, src[perm], dst[perm], lat[perm], loss[perm], _vloss(rng, V, vertex_loss))


def star(V, seed=1, self_loops_on="odd"):
    """Hub 0 joined to every other vertex (hub degree V - 1), latencies 1 + 9 U;
    self-loops on the "odd" vertices only, on "all" or on "none"."""
    rng = np.random.default_rng(seed)
    sl = {"odd": np.arange(1, V, 2), "all": np.arange(V), "none": np.zeros(0, np.int64)}[self_loops_on]
    src = np.concatenate([np.zeros(V - 1, np.int64), sl])
    dst = np.concatenate([np.arange(1, V), sl])
    lat = 1.0 + 9.0 * rng.random(len(src))
    loss = rng.random(len(src)) * 0.01
    perm = rng.permutation(len(src))
    return S.GraphArrays(V, src[perm], dst[perm], lat[perm], loss[perm])


def strip_self_loops(g, every):
    """g without the self-loop of every `every`-th vertex (0, every, ...)."""
    keep = ~((g.src == g.dst) & (g.src % every == 0))
    return S.GraphArrays(g.n_vertices, g.src[keep], g.dst[keep], g.latency[keep], g.loss[keep], g.vertex_loss,
                         directed=g.directed, prefer_direct=g.prefer_direct)


def with_prefer_direct(g):
    return S.GraphArrays(g.n_vertices, g.src, g.dst, g.latency, g.loss, g.vertex_loss, directed=g.directed,
                         prefer_direct=True)


def directed_geo(V, seed):
    """A geometric graph with every edge both ways, the way back up to twice as slow."""
    g0 = W.geometric_graph(V, seed=seed, loss_max=0.01)
    src, dst = g0.src.astype(np.int64), g0.dst.astype(np.int64)
    nsl = src != dst
    rng = np.random.default_rng(seed)
    return S.GraphArrays(V, np.concatenate([src, dst[nsl]]), np.concatenate([dst, src[nsl]]),
                         np.concatenate([g0.latency, g0.latency[nsl] * (1.0 + rng.random(int(nsl.sum())))]),
                         np.concatenate([g0.loss, g0.loss[nsl]]), directed=True)


def geometric(V, seed, vertex_loss=None):
    g = W.geometric_graph(V, seed=seed, vertex_loss=vertex_loss is not None)
    if vertex_loss == "mixed":
        vl = g.vertex_loss.copy()
        vl[::2] = np.nan
        g = S.GraphArrays(V, g.src, g.dst, g.latency, g.loss, vl)
    return g


def half_ms(g):
    """The same graph at half the latencies: ties kept (k / 2 is exact), the
    weights no longer whole numbers."""
    return S.GraphArrays(g.n_vertices, g.src, g.dst, g.latency * 0.5, g.loss, g.vertex_loss, directed=g.directed)


# ------------------------------------------------------------------ tiny graphs (whole tables, forced rows)
def _v1():
    return S.GraphArrays(1, [0], [0], [2.5], [0.004])


def _parallel2():
    # two parallel 3 ms edges of different loss: the other vertex has two exact
    # predecessor arcs at the same distance (one tie a row), the lowest edge id wins
    return S.GraphArrays(2, [0, 0, 0, 1], [1, 0, 1, 1], [3.0, 1.5, 3.0, 2.25], [0.03, 0.001, 0.007, 0.002])


def _directed2():
    return S.GraphArrays(2, [0, 1, 1, 0], [1, 1, 0, 0], [2.5, 1.25, 4.0, 1.75], [0.01, 0.002, 0.02, 0.003],
                         directed=True)


TINY = {
    "v1": _v1,
    "chain2": lambda: chain(2, seed=2),
    "chain3": lambda: chain(3, seed=3),
    "parallel2": _parallel2,
    "directed2": _directed2,
}
TINY_TIES = {"v1": 0, "chain2": 0, "chain3": 0, "parallel2": 2, "directed2": 0}   # over both rows


# ------------------------------------------------------------------ row cases
def _subset(V, n, seed):
    """a sorted subset of n vertices that contains 0 and V - 1"""
    rng = np.random.default_rng(seed)
    mid = rng.choice(np.arange(1, V - 1), n - 2, replace=False)
    return np.sort(np.concatenate([[0, V - 1], mid])).astype(np.int32)


def _all(V):
    return np.arange(V, dtype=np.int32)


def _ring_attached(V, n, seed):
    """n vertices with 0 and V // 2 first: one workgroup of the two-row kernel pairs them"""
    rng = np.random.default_rng(seed)
    rest = rng.choice(np.setdiff1d(np.arange(V), [0, V // 2]), n - 2, replace=False)
    return np.concatenate([[0, V // 2], np.sort(rest)]).astype(np.int32)


class RowCase:
    """graph(), attached, the rows (attached indices) a test compares, the
    first-pass kernel the build must pick; `all_rows`: rows covers the table."""

    def __init__(self, graph, attached, rows, kernel):
        self.graph, self._att, self._rows, self.kernel = graph, attached, rows, kernel

    @functools.cached_property
    def g(self):
        return self.graph()

    @functools.cached_property
    def att(self):
        return self._att(self.g.n_vertices)

    @functools.cached_property
    def rows(self):
        T = len(self.att)
        return list(range(T)) if self._rows is None else sorted(set(self._rows(T)))

    @property
    def all_rows(self):
        return self._rows is None


K1, K2, K3, K4 = S.SHD_PC_K_ROWS_LDS_256, S.SHD_PC_K_ROWS2_LDS, S.SHD_PC_K_ROWS_LDS_1024, S.SHD_PC_K_ROWS_GLOBAL


def _geo_all(V, seed):
    return RowCase(lambda: geometric(V, seed), _all, None, K1)


ROW_CASES = {
    # wave and block boundaries of rows_lds<256>
    "geo63": _geo_all(63, 21),
    "geo64": _geo_all(64, 22),
    "geo65": _geo_all(65, 23),
    "geo257": _geo_all(257, 24),
    "geo2048": RowCase(lambda: geometric(2048, 25), _all, lambda T: list(range(0, T, 32)) + [T - 1], K1),
    # dispatch boundaries; 2049 rows: odd (row 2048 unpaired) and past twice any CU count
    "geo2049": RowCase(lambda: geometric(2049, 26), _all, lambda T: list(range(0, T, 16)) + [T - 3, T - 2, T - 1], K2),
    "geo10080": RowCase(lambda: geometric(10080, 27), lambda V: _subset(V, 131, 1), None, K2),
    "geo10081": RowCase(lambda: geometric(10081, 28, "mixed"), lambda V: _subset(V, 131, 2), None, K3),
    "geo11701": RowCase(lambda: geometric(11701, 29), lambda V: _subset(V, 131, 3), None, K3),
    "geo11702": RowCase(lambda: geometric(11702, 30), lambda V: _subset(V, 131, 4), None, K4),
    # deep trees
    "chain700": RowCase(lambda: chain(700, seed=31, vertex_loss="all"), _all, None, K1),
    "ring2101": RowCase(lambda: chain(2101, seed=32, ring=True, vertex_loss="mixed"),
                        lambda V: _ring_attached(V, 65, 5), None, K2),
    "chain11702": RowCase(lambda: chain(11702, seed=33), lambda V: _subset(V, 33, 6), None, K4),
    # stars: one arc list thousands long, self-loops on the odd vertices only
    "star3000": RowCase(lambda: star(3000, seed=34), _all,
                        lambda T: [0, 1, 2, T - 1] + list(range(3, T, 47)), K2),
    "star300": RowCase(lambda: star(300, seed=35), _all, lambda T: [0, 1, 2, T - 1] + list(range(3, T, 7)), K1),
}


# ------------------------------------------------------------------ lazy-lookup cases
N_QUERIES = 3000

LOOKUP_CASES = {
    # name: (graph, failing queries expected: a row without its self-loop fails as a whole)
    "geo200_vloss_strip7": (lambda: strip_self_loops(geometric(200, 41, "all"), 7), True),
    "directed150": (lambda: directed_geo(150, 42), False),
    "directed150_strip5": (lambda: strip_self_loops(directed_geo(150, 42), 5), True),
    "geo200_strip4_prefer_direct": (lambda: with_prefer_direct(strip_self_loops(geometric(200, 43), 4)), True),
}


def lookup_queries(g, seed=7):
    """N_QUERIES seeded vertex pairs (every vertex attached), every 31st a self pair"""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, g.n_vertices, (N_QUERIES, 2)).astype(np.int32)
    q[::31, 1] = q[::31, 0]
    return q


# ------------------------------------------------------------------ graphs of the switch-selected kernels
SWITCH_GRAPHS = {
    # name: (graph, attached, rows compared)
    "grid30": lambda: (W.grid_graph(30, seed=2), None),
    "geo_half_ms_300": lambda: (half_ms(W.geometric_graph(300, seed=3, integer_latency=True)), None),
    "geo2049": lambda: (ROW_CASES["geo2049"].g, ROW_CASES["geo2049"].rows),
}
