"""The untraced persistent rounds at small sizes against the serial oracle.

Tracing switches off the lean instantiations (k_round_ps<true>, k_round_sp<true>)
and the fused fast paths, so the traced small-model tests of test_engine_gpu.py
never run the code the flagship benchmark runs; the full-size fixtures do, at
one size.  Every case here runs with trace off, heartbeats off and no bootstrap
period, and compares every host's end state (Engine.digest()) and the event
counts with oracle_ffi.engine_run; each must have run persistent launches.  The
oracle reports no round count, so n_rounds is compared only between the forced
sparse kernel and the same model unforced.

The cases, their sizes and what the oracle alone shows for each are in
lean_cases.py, which the multi-process and launch-per-round tests share.
"""
import numpy as np
import pytest

import shdgpu as S
import workloads as W
from lean_cases import check_lean, check_tor_inputs, make_case, oracle_of
from sim import Engine, PathCache

pytestmark = pytest.mark.gpu

PS_BATCH = 1024   # engine.hip kPsBatch


def run_gpu(g, m):
    check_lean(m)
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


_plain = {}   # the unforced run of the sparse case, shared by its two forced sizes


@pytest.mark.parametrize("sph", [64, 256])
def test_forced_sparse_kernel(sph, monkeypatch):
    g, m = make_case("sparse")
    if "plain" not in _plain:
        _plain["plain"] = run_gpu(g, m)
    pdg, pst = _plain["plain"]
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


def test_tor_classes_untraced():
    """Two host classes, each with its own destination row (the closed-destination
    fast path is off), untraced, on whichever round kernels the engine picks."""
    g, m = make_case("tor")
    assert m.n_classes == 2
    dg, st = run_gpu(g, m)
    odg, ost = oracle_of("tor", g, m)
    check_tor_inputs(m, odg)
    print(f"tor: hosts {m.n_hosts} rounds {st.n_rounds} batches {st.n_batches} persistent "
          f"{st.n_batches_persistent} sparse {st.n_batches_sparse} ticketless {st.n_batches_ticketless} "
          f"events {st.n_events}/{ost['n_events']} packet events {st.n_pkt_events}/{ost['n_pkt_events']}")
    ran = [k for k, v in (("persistent", st.n_batches_persistent), ("ticketless", st.n_batches_ticketless)) if v]
    print("tor: non-zero batch counters: " + (", ".join(ran) or "neither persistent nor ticketless"))
    assert st.error == 0
    assert st.n_events == ost["n_events"]
    assert st.n_pkt_events == ost["n_pkt_events"] > 0
    assert np.array_equal(dg, odg)
    assert st.n_batches > 0
