"""What the path-cache shape tests rely on, asserted of their inputs by the
oracle alone (no device): a bad seed or builder is caught here.

Every input of test_pathcache_shapes_gpu.py and pc_switch_worker.py comes from
pc_graphs.py, as here.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_ffi as O
import pc_graphs as G
import shdgpu as S
from pc_helpers import oracle_table


def _check(g):
    p = S.GraphProps()
    assert S.lib().shd_graph_check(C.byref(g.struct), C.byref(p)) == 0   # valid, (strongly) connected
    return p


@pytest.mark.parametrize("name", sorted(G.TINY))
def test_tiny_graphs_are_valid_and_tie_as_stated(name):
    g = G.TINY[name]()
    _check(g)
    att = np.arange(g.n_vertices, dtype=np.int32)
    _, _, ok, _, ties = oracle_table(g, att, range(len(att)))
    assert ties == G.TINY_TIES[name]
    assert ok.all()   # every tiny graph has all its self-loops


@pytest.mark.parametrize("name", sorted(G.ROW_CASES))
def test_row_cases_are_valid_tie_free_and_shaped_as_stated(name):
    c = G.ROW_CASES[name]
    g, att, rows = c.g, c.att, c.rows
    p = _check(g)
    assert p.is_complete == 0   # the rows are built without SHD_PC_FORCE_ROWS
    assert len(set(att.tolist())) == len(att) and 0 <= att.min() and att.max() < g.n_vertices
    _, _, ok, hops, ties = oracle_table(g, att, rows)
    assert ties == 0   # one pass, no heap rerun: the first-pass kernel's own parents are compared
    T, V = len(att), g.n_vertices
    if name.startswith("geo") and name != "geo2049" and V > 2048:
        assert T == 131 and T % 2 == 1 and att[0] == 0 and att[-1] == V - 1 and np.all(np.diff(att) > 0)
    if name == "geo2049":
        assert T == 2049 and {0, T - 3, T - 2, T - 1} <= set(rows)   # row 2048: the unpaired one
    if name == "chain700":
        assert T == V == 700 and hops.max() == 699 and g.vertex_loss is not None and not np.isnan(g.vertex_loss).any()
    if name == "ring2101":
        # rows 0 and 1 share a workgroup of the two-row kernel
        assert T == 65 and att[0] == 0 and att[1] == 1050
        assert np.isnan(g.vertex_loss).any() and not np.isnan(g.vertex_loss).all()
    if name == "chain11702":
        assert T == 33 and g.vertex_loss is None and hops.max() == V - 1
    if name.startswith("star"):
        assert _check(g).max_out_degree >= V - 1
        assert {0, 1, 2, T - 1} <= set(rows)
        sl = set(g.src[g.src == g.dst].tolist())
        assert sl == set(range(1, V, 2))
        # exactly the diagonal of a vertex without a self-loop has no path
        bad = np.argwhere(ok == 0)
        assert all(rows[k] == j for k, j in bad) and {rows[k] for k, _ in bad} == {r for r in rows if r % 2 == 0}
    else:
        assert ok.all()


@pytest.mark.parametrize("name", sorted(G.LOOKUP_CASES))
def test_lookup_cases_fail_where_meant_and_seldom(name):
    build, fails = G.LOOKUP_CASES[name]
    g = build()
    _check(g)
    ot = O.OTopo(O.OGraph(g), np.arange(g.n_vertices, dtype=np.int32))
    q = G.lookup_queries(g)
    assert len(q) == G.N_QUERIES == 3000 and int(np.sum(q[:, 0] == q[:, 1])) >= 3000 // 31
    got = np.array([ot.get(int(s), int(d)) for s, d in q])
    failing = int(np.sum(got[:, 0] < 0))
    assert np.all((got[:, 0] < 0) == (got[:, 1] < 0))
    assert failing < 0.15 * len(q), failing
    assert (failing > 0) == fails, failing
    assert ot.rows_run() > 0   # not served from direct paths alone


@pytest.mark.parametrize("name", sorted(G.SWITCH_GRAPHS))
def test_switch_graphs_are_valid_and_tie_where_the_tie_kernels_need_them(name):
    g, rows = G.SWITCH_GRAPHS[name]()
    p = _check(g)
    assert p.is_complete == 0
    att = np.arange(g.n_vertices, dtype=np.int32)
    _, _, ok, _, ties = oracle_table(g, att, range(0, len(att), 29))
    assert ok.all()
    whole = bool(np.all(g.latency == np.floor(g.latency)))
    if name == "geo2049":
        assert ties == 0 and not whole   # the first-pass switches: the first pass's parents are the table's
    else:
        assert ties > 0                  # the tie switches: every sampled row goes through the tie kernel
        assert whole == (name == "grid30")   # grid30: 4-byte heap values; geo_half_ms_300: the 8-byte ones
