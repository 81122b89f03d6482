"""The untraced small models of the lean-round tests -- TEST INFRASTRUCTURE
(test_lean_rounds_gpu.py, test_xgroup_lean_gpu.py with xgroup_worker.py --case,
test_lean_launch_rounds_gpu.py with lean_rounds_worker.py: the test processes
and their child processes build the same model from the same name).

Every case runs with trace off, heartbeats off and no bootstrap period
(check_lean), so the engine takes the lean instantiations of its round kernels;
the oracle's run of a case is computed once a process and handed out read-only.

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
    partial last one;
  tor: the relay/client model of test_multiprocess_group_tor_model (40 relays,
    200 clients, load=4, 2.5 s on the bundled topology), untraced: two host
    classes with a destination row each, so the closed-destination fast path
    is off.  The oracle runs it in about 0.02 s: 67 619 events, 22 963 packet
    events; the relays send 15 459 packets and the clients 8 464 (both
    classes send), and 113 are dropped by path loss, so load and end time
    stay at the traced test's values.
"""
import numpy as np

import oracle_ffi as O
import shdgpu as S
import workloads as W

TOR_RELAYS, TOR_CLIENTS, TOR_LOAD, TOR_END_S = 40, 200, 4, 2.5


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
    if name == "tor":
        return W.tor_model(TOR_RELAYS, TOR_CLIENTS, end_time=int(TOR_END_S * sec), load=TOR_LOAD)
    raise KeyError(name)


def check_lean(m):
    """What switches the lean instantiations off (engine.hip lean_model) is off."""
    assert not m.params["trace"] and m.params["bootstrap_end"] == 0
    assert not (int(m.params["queue_flags"]) & S.SHD_QF_HEARTBEATS)


_oracle = {}


def oracle_of(name, g, m):
    """The oracle's run of a case, computed once (digest, stats)."""
    if name not in _oracle:
        _, dg, st = O.engine_run(m, g)
        dg.setflags(write=False)
        _oracle[name] = (dg, st)
    return _oracle[name]


def check_tor_inputs(m, odg):
    """What the tor case is for, on the oracle's output: both classes send, and
    packets are dropped on the way."""
    cls = np.asarray(m.host_class)
    out = odg["n_sent"].astype(np.int64) + odg["n_inet_drop"].astype(np.int64)
    assert cls.max() == 1 and int(out[cls == 0].sum()) > 0 and int(out[cls == 1].sum()) > 0
    assert int(odg["n_inet_drop"].sum()) > 0
