"""The path cache's row kernels at their dispatch edges and on odd graphs,
bit for bit against the oracle (inputs and their preconditions: pc_graphs.py,
test_pc_graphs_cpu.py).

shd_pc_info.first_pass_kernel says which row kernel the build picked: every
case asserts it, so a case that lands on another kernel fails.
Reference: src/main/routing/topology.c (rows 1655-1875 + 1407-1523, self
1545-1653, lazy selection 1969-2051).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_ffi as O
import pc_graphs as G
import shdgpu as S
from pc_helpers import PathCache, SHD_PC_FORCE_ROWS, oracle_table, same_bits

pytestmark = pytest.mark.gpu


def _self_ref(g, att):
    og = O.OGraph(g)
    return np.array([og.self_path(v) for v in att]).reshape(len(att), 2)


def _gpu_rows(pc, rows):
    parts = [pc.rows(r, 1) for r in rows]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _assert_rows(lat, rel, olat, orel, rows):
    if same_bits(lat, olat) and same_bits(rel, orel):
        return
    bad = np.argwhere((lat.view(np.uint64) != olat.view(np.uint64)) | (rel.view(np.uint64) != orel.view(np.uint64)))
    k, j = bad[0]
    raise AssertionError(f"{len(bad)} entries differ, the first at row {rows[k]} column {j}: "
                         f"({lat[k, j]!r}, {rel[k, j]!r}) against the oracle's ({olat[k, j]!r}, {orel[k, j]!r})")


# ---- a. tiny graphs: whole tables, forced rows (one or two vertices with their self-loops are complete)
@pytest.mark.parametrize("name", sorted(G.TINY))
def test_tiny_graph_whole_table(name):
    g = G.TINY[name]()
    V = g.n_vertices
    att = np.arange(V, dtype=np.int32)
    pc = PathCache(g, att, flags=SHD_PC_FORCE_ROWS)
    info = pc.info()
    assert info.rows_computed == V and info.first_pass_kernel == S.SHD_PC_K_ROWS_LDS_256
    rows = list(range(V))
    olat, orel, ok, hops, ties = oracle_table(g, att, rows)
    lat, rel = pc.rows()
    _assert_rows(lat, rel, olat, orel, rows)
    assert ties == G.TINY_TIES[name] and info.n_ties == ties
    assert info.n_tie_rows == (V if ties else 0)   # parallel2: the tie kernel runs at V = 2
    assert info.max_hops == hops.max() and info.n_unroutable == int(np.sum(ok == 0)) == 0
    slat, srel = pc.self_values()
    ref = _self_ref(g, att)
    assert same_bits(slat, ref[:, 0]) and same_bits(srel, ref[:, 1])
    if name == "parallel2":
        # the lowest edge id of the two 3 ms edges (document order: edge 0, loss 0.03)
        assert lat[0, 1] == 3.0 and rel[0, 1] == 1.0 * (1.0 - np.float64(0.03)) == rel[1, 0]
    pc.close()


# ---- b-e. row cases
@functools.lru_cache(maxsize=None)
def _oracle_case(name):
    c = G.ROW_CASES[name]
    return oracle_table(c.g, c.att, c.rows)


def _run_row_case(name):
    c = G.ROW_CASES[name]
    g, att, rows = c.g, c.att, c.rows
    T = len(att)
    pc = PathCache(g, att)
    info = pc.info()
    assert info.first_pass_kernel == c.kernel, (info.first_pass_kernel, c.kernel)
    assert info.is_complete == 0 and info.rows_computed == T
    assert info.n_ties == 0 and info.n_tie_rows == 0   # tie-free: the first pass's own parents
    olat, orel, ok, hops, _ = _oracle_case(name)
    full = pc.rows() if c.all_rows or T <= 3000 else None
    lat, rel = (full[0][rows], full[1][rows]) if full else _gpu_rows(pc, rows)
    _assert_rows(lat, rel, olat, orel, rows)
    slat, srel = pc.self_values()
    ref = _self_ref(g, att)
    assert same_bits(slat, ref[:, 0]) and same_bits(srel, ref[:, 1])
    if c.all_rows:
        # max_hops: the most edges on a stored path between two different attached
        # vertices (the [src] self entry has none in the oracle either)
        assert info.max_hops == hops.max(), (info.max_hops, hops.max())
        assert info.n_unroutable == int(np.sum(ok == 0))
    else:
        assert info.max_hops >= hops.max()
    return pc, info, full


@pytest.mark.parametrize("name", ["geo63", "geo64", "geo65", "geo257", "geo2048"])
def test_wave_and_block_boundaries_of_the_256_thread_kernel(name):
    _run_row_case(name)[0].close()


@pytest.mark.parametrize("name", ["geo2049", "geo10080", "geo10081", "geo11701", "geo11702"])
def test_dispatch_boundaries(name):
    # kernels 2, 2, 3, 3, 4; at 2049 rows the two-row kernel's grid strides and its last
    # workgroup runs one row alone; elsewhere 131 rows (odd, T < V)
    _run_row_case(name)[0].close()


def test_chain_of_700_through_the_256_thread_kernel():
    pc, info, _ = _run_row_case("chain700")
    assert info.max_hops == 699
    assert info.sssp_iterations_max >= info.max_hops   # a frontier iteration advances one hop
    pc.close()


def test_ring_of_2101_rows_of_one_workgroup_far_apart():
    pc, info, _ = _run_row_case("ring2101")
    assert info.max_hops >= 1000 and info.sssp_iterations_max >= info.max_hops
    pc.close()


def test_chain_of_11702_through_the_global_memory_kernel():
    pc, info, _ = _run_row_case("chain11702")
    assert info.max_hops == 11701 and info.sssp_iterations_max >= info.max_hops
    pc.close()


@pytest.mark.parametrize("name", ["star3000", "star300"])
def test_star_with_self_loops_on_odd_vertices(name):
    pc, info, (lat, rel) = _run_row_case(name)
    c = G.ROW_CASES[name]
    g, att = c.g, c.att
    V = g.n_vertices
    d_lat, d_rel = np.diagonal(lat), np.diagonal(rel)
    even = np.arange(V) % 2 == 0
    assert np.all(d_lat[even] == -1.0) and np.all(d_rel[even] == -1.0)   # no self-loop: no [src] path
    assert np.all(d_lat[~even] > 0)
    # the oracle's failures over all rows: a star's only ones are those diagonals
    # (test_pc_graphs_cpu.py asserts that of the sampled rows; here of every row)
    og = O.OGraph(g)
    n_fail = 0
    for v in att:
        n_fail += int(np.sum(og.row(v, att, count_ties=False)[2] == 0))
    assert n_fail == int(even.sum()) and info.n_unroutable == n_fail
    assert info.max_hops == 2
    pc.close()


# ---- g. lazy lookup against the oracle's cache
@pytest.mark.parametrize("name", sorted(G.LOOKUP_CASES))
def test_lazy_lookup_matches_the_reference_cache(name):
    build, fails = G.LOOKUP_CASES[name]
    g = build()
    att = np.arange(g.n_vertices, dtype=np.int32)
    q = G.lookup_queries(g)
    ot = O.OTopo(O.OGraph(g), att)
    want = np.array([ot.get(int(s), int(d)) for s, d in q])
    want_min = O.lib().o_topo_min_latency(ot.ptr)
    assert (int(np.sum(want[:, 0] < 0)) > 0) == fails

    def stored_min(pc):
        m = C.c_double()
        S.check(S.lib().shd_pc_min_stored_latency(pc.ptr, C.byref(m)), "min")
        return m.value

    def first_diff(got):
        bad = np.nonzero(np.any(got.view(np.uint64) != want.view(np.uint64), axis=1))[0]
        return None if not len(bad) else (int(bad[0]), q[bad[0]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())

    a = PathCache(g, att)
    assert a.info().rows_computed == len(att)
    got = np.array([a.lookup(int(s), int(d)) for s, d in q])
    assert first_diff(got) is None, first_diff(got)
    assert stored_min(a) == want_min
    a.close()

    b = PathCache(g, att)
    parts = [b.lookup_batch(p[:, 0], p[:, 1]) for p in (q[:1300], q[1300:])]   # the second starts from the first's ranks
    got = np.stack([np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])], axis=1)
    assert first_diff(got) is None, first_diff(got)
    assert stored_min(b) == want_min
    b.close()
