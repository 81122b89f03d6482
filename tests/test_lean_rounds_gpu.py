"""The untraced persistent rounds at small sizes against the serial oracle.

Tracing switches off the lean instantiations (k_round_ps<true>, k_round_sp<true>)
and the fused fast paths, so the traced small-model tests of test_engine_gpu.py
never run the code the flagship benchmark runs; the full-size fixtures do, at
one size.  Every case here runs with trace off, heartbeats off and no bootstrap
period, and compares every host's end state (Engine.digest()) and the event
counts with oracle_ffi.engine_run; each must have run persistent launches.  The
oracle reports no round count, so n_rounds is compared only between the forced
sparse kernel and the same model unforced.

Sizes (one wave of 64 lanes per block, one host per lane; the wave folds, the
share gather and the dirty mask are what the sizes aim at):
  1 host (one lane; its only destination is itself, and its one-vertex graph is
  complete, so no round waits for a first touch behind a state copy -- on a
  larger graph a lone host never logs one and never leaves the protected
  rounds), 63 and 64 (a block one lane short of full, an exactly full one), 65
  (a second block with one lane), 129, 300 (5 blocks, the last with 44 lanes),
  4160 hosts on 400 vertices (65 blocks: a second lane-group of shares in a
  gather chunk).
Chosen values, checked on the CPU with the oracle alone (each case runs there
in under 3 s):
  dense: 300 hosts, load=192 (at load=64 a host takes 0.8 arrivals a window and
    only 194 host-windows of 600 000 hold more than kDueCap = 6; at 192 it takes
    2.5, and 27 000 host-windows overflow the due list into the heap);
  codel: test_engine_gpu.py's configuration (payload=1000, bw_down=600,
    load=24, codelq_cap=256) on 150 hosts for 4 s -- the oracle drops 162
    packets by CoDel;
  three bins: whole-millisecond latencies (window 2 000 000 ns, bin width
    2^20 ns: 1.9 bins a window, so most windows span three bins and cross the
    bitmap's 32-bit words every 32 bins); 3 s is 1900 bins, the 256-bin ring
    wraps seven times;
  long: 300 hosts on the bundled complete graph (window 5 ms) for 8 s, about
    1400 rounds: a persistent batch of 1024 rounds (engine.hip kPsBatch) and a
    partial last one.
"""
import numpy as np
import pytest

import oracle_ffi as O
import shdgpu as S
import workloads as W
from sim import Engine, PathCache

pytestmark = pytest.mark.gpu

PS_BATCH = 1024   # engine.hip kPsBatch


def spread_hosts(n_hosts, n_vertices):
    """n_hosts hosts over n_vertices vertices, in registration order."""
    return (np.arange(n_hosts, dtype=np.int64) * n_vertices // n_hosts).astype(np.int32)


def make_case(name):
    """(graph, untraced model) of a case."""
    sec = S.SHD_SEC
    if name.startswith("hosts"):
        n = int(name[5:])
        if n == 4160:
            g, hv = W.geometric_graph(400, seed=2), spread_hosts(4160, 400)
        else:
            g, hv = W.geometric_graph(n, seed=2), W.hosts_on_vertices(n, 1)
        return g, W.phold_model(hv, end_time=3 * sec)
    if name == "dense":
        return W.geometric_graph(300, seed=2), W.phold_model(W.hosts_on_vertices(300, 1), end_time=3 * sec, load=192)
    if name == "codel":
        return W.geometric_graph(150, seed=8), W.phold_model(
            W.hosts_on_vertices(150, 1), end_time=4 * sec, load=24, payload=1000, bw_down=600, bw_up=100000,
            codelq_cap=256)
    if name == "sparse":
        return W.geometric_graph(400, seed=2), W.phold_model(W.hosts_on_vertices(400, 2), end_time=3 * sec)
    if name == "threebins":
        return (W.geometric_graph(200, seed=5, integer_latency=True),
                W.phold_model(W.hosts_on_vertices(200, 1), end_time=3 * sec))
    if name == "long":   # the bundled complete graph: no first touch is ever logged, so no batch halts
        g = W.bundled_graph()
        hv = np.sort(np.random.default_rng(0).integers(0, g.n_vertices, 300)).astype(np.int32)
        return g, W.phold_model(hv, end_time=8 * sec)
    raise KeyError(name)


_oracle = {}


def oracle_of(name, g, m):
    """The oracle's run of a case, computed once (digest, stats)."""
    if name not in _oracle:
        _, dg, st = O.engine_run(m, g)
        dg.setflags(write=False)
        _oracle[name] = (dg, st)
    return _oracle[name]


def run_gpu(g, m):
    assert not m.params["trace"] and m.params["bootstrap_end"] == 0
    assert not (int(m.params["queue_flags"]) & S.SHD_QF_HEARTBEATS)
    pc = PathCache(g, W.attached_vertices(m.host_vertex))
    eng = Engine(m, pc)
    st = eng.run()
    dg = eng.digest()
    eng.close()
    pc.close()
    return dg, st


def check(name, g, m, dg, st):
    odg, ost = oracle_of(name, g, m)
    print(f"{name}: hosts {m.n_hosts} rounds {st.n_rounds} batches {st.n_batches} persistent "
          f"{st.n_batches_persistent} sparse {st.n_batches_sparse} events {st.n_events}/{ost['n_events']} "
          f"packet events {st.n_pkt_events}/{ost['n_pkt_events']}")
    assert st.error == 0
    assert st.n_events == ost["n_events"]
    assert st.n_pkt_events == ost["n_pkt_events"]
    assert ost["n_pkt_events"] > 0 or m.n_hosts == 1   # (one host: every send is a loopback)
    assert np.array_equal(dg, odg)
    assert st.n_batches_persistent > 0
    return odg, ost


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 300, 4160])
def test_host_counts(n):
    name = f"hosts{n}"
    g, m = make_case(name)
    assert m.n_hosts == n
    dg, st = run_gpu(g, m)
    odg, _ = check(name, g, m, dg, st)
    if n > 1:
        assert int(odg["n_inet_drop"].sum()) > 0   # default edge loss: drops occur


def test_dense_windows_overflow_the_due_list():
    g, m = make_case("dense")
    dg, st = run_gpu(g, m)
    odg, _ = check("dense", g, m, dg, st)
    # arrivals per host and window over the application's 2 s: above 2 on average (the due list
    # holds 6; the count of overflowing host-windows is in the module docstring)
    windows = 2 * S.SHD_SEC / st.window_ns
    assert int(odg["n_recv"].sum()) / (m.n_hosts * windows) > 2.0


def test_codel_drops_untraced():
    g, m = make_case("codel")
    dg, st = run_gpu(g, m)
    odg, _ = check("codel", g, m, dg, st)
    assert int(odg["n_codel_drop"].sum()) > 0


@pytest.mark.parametrize("sph", [64, 256])
def test_forced_sparse_kernel(sph, monkeypatch):
    g, m = make_case("sparse")
    if "plain" not in _oracle:
        _oracle["plain"] = run_gpu(g, m)
    pdg, pst = _oracle["plain"]
    check("sparse", g, m, pdg, pst)
    assert pst.n_batches_sparse == 0
    monkeypatch.setenv("SHD_SP_HOSTS", str(sph))
    dg, st = run_gpu(g, m)
    check("sparse", g, m, dg, st)
    assert st.n_batches_sparse > 0
    assert st.n_rounds == pst.n_rounds


def test_window_spanning_three_bins():
    g, m = make_case("threebins")
    dg, st = run_gpu(g, m)
    check("threebins", g, m, dg, st)
    width = 1 << (int(st.window_ns).bit_length() - 1)           # the calendar's bin width
    print(f"threebins: window {st.window_ns} ns, bin width {width} ns")
    assert st.window_ns % 1_000_000 == 0 and st.window_ns > 1.9 * width
    assert (m.params["end_time"] - S.SHD_SEC) // width > 256    # the ring wraps


def test_long_batches():
    g, m = make_case("long")
    dg, st = run_gpu(g, m)
    check("long", g, m, dg, st)
    # rounds outside persistent launches: the protected ones and the 64-round batches.  Nothing
    # halts a batch on a complete graph, so the persistent launches are as few as their rounds
    # allow exactly when every one but the last ran its full length
    other = st.n_rounds_protected + 64 * (st.n_batches - st.n_batches_persistent)
    rounds = st.n_rounds - other
    print(f"long: {rounds} rounds in {st.n_batches_persistent} persistent launches, {other} outside them")
    assert rounds > PS_BATCH and rounds % PS_BATCH != 0
    assert st.n_batches_persistent == -(-rounds // PS_BATCH)
