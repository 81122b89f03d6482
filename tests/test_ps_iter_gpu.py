"""The steady iteration of the persistent round's event loop (steady_iter in
eng_device.h, taken by the lean k_round_ps ahead of take_next + begin_event)
next to the general iteration, at small sizes against the serial oracle.

In the manner of test_ps_close_gpu.py, whose helpers this file imports: every
case runs untraced, without heartbeats and without a bootstrap period (the
lean instantiations), compares every host's end state (Engine.digest()) and
the event counts with oracle_ffi.engine_run, and must have run persistent
launches.  The cases were chosen and counted on the CPU with the oracle
alone.  routes() below steps the oracle through the engine's windows
(oracle_windows() of test_ps_close_gpu.py does the same for the sends) and
sorts every host-window by what its digest shows at the window's two ends:

  idle     no event;
  steady   events, and nothing but what the steady iteration takes: every
           packet of the window was received in it (no router queue before or
           after, no CoDel drop), every datagram read was answered by one
           deferred send (sent or dropped on the path), and both buckets hold
           an MTU at both ends;
  backlog  a router queue at either end, a CoDel drop, or a bucket below an
           MTU at either end: arrivals that queue, refills with work, sends
           that wait (begin_event's general cases and run_work);
  other    the rest: fewer deferred sends than datagrams received (a
           loopback, which run_work sends after a flush, or a draw without
           destination) or more (the application's start), or a datagram
           received without a packet event (the loopback's delivery).

The digest's counters do not show a tie (take_next_full) or a full pool.  Ties
are counted by refill_ties() below from the oracle's state stepped to just
before every millisecond boundary that has an arrival (the refill-pending
flag of the arrival's host); the pool from the sends per window.  Counts,
host-windows (steady / backlog / other / idle), from routes():

  near64, near65 (steady next to general in one wave): the three-vertex
  whole-millisecond graph (seed 121, W = 17 ms), load 1, 10 s.  near64: 518
  windows, 10 287 / 0 / 302 / 22 563; windows in which the block has steady
  and other host-windows side by side: 169.  near65: 519 windows, 10 962 / 0 /
  315 / 22 458, side by side in a block 186.  This graph has no tie: 63 (64)
  arrivals fall on a millisecond boundary, the first ones at 1017, 1019, 1022
  and 1026 ms, and at none of them is the host's refill pending (a refill is
  scheduled by a consumption and fires at the next boundary; the paths never
  differ by 1 ms).  The general lanes here are the `other` ones.

  tie64, tie65 (take_next_full beside steady lanes): the same graph with edge
  latencies of 18, 17 and 19 ms (self loops 20 ms), load 2, 10 s, W = 17 ms.
  A host hears from two vertices 1 ms apart: the arrival at 1017 ms (1018,
  1019) takes from the full bucket and schedules the refill for the next
  boundary, where the next arrival is.  tie64: 125 arrivals on a boundary, 23
  of them (at 1018, 1019 and 1020 ms, 20 hosts) at the host's pending refill's
  time; 527 windows, 18 099 / 0 / 545 / 15 084; every tie's window has steady
  host-windows in its block.  tie65: 127 and 23 (21 hosts); 525 windows,
  17 586 / 0 / 583 / 15 956.

  loopback: near64 again: 212 of its 302 `other` host-windows have fewer
  deferred sends than datagrams read, or a datagram received that no packet
  event brought (the loopback's delivery, a heap event) -- a self draw is one
  send in 64 -- in windows where the block's other lanes are steady.

  buckets and CoDel: 129 hosts on geometric_graph(129, seed=3), 1500-B
  payload.  down (512 KiB/s downlinks, codelq_cap 64, load 16, 3 s): 1731
  windows, 14 382 / 137 965 / 1 / 70 951; 414 CoDel drops, 66 478 host-windows
  that start with a router queue, 137 712 with the receive bucket below an MTU
  at an end; steady beside backlog in 3258 block-windows.  up (256 KiB/s
  uplinks, downlinks 10 240, load 8, 2 s): 856 windows, 2 180 / 93 182 / 0 /
  15 062, the send bucket below an MTU at an end in all 93 182 (sends that
  wait in the send queue); steady beside backlog in 1148 block-windows.

  pool: multi4 of test_ps_close_gpu.py (load 4, 64 hosts): 358 rounds above
  64 sends, 3 above 224 = kPool - 64 (the steady iteration reads the pool
  count once, gives out its slots by lane rank and stores the new count; a
  block past 224 leaves the steady route and flushes inside the loop):
  24 401 / 0 / 952 / 8 567.

  lossy: half_lossless, 3 s, 1625 windows: 2003 dropped sends, each giving its
  ID back at the flush (the ev_seq order across the arrival, the notification
  and the refill of one steady iteration): 41 764 / 0 / 410 / 167 451 (a send
  dropped on its path is a deferred send: steady).

  exits: near64 run to 5 000 000 195 ns, 1 ns after an arrival the traced
  oracle reports (the first after 5 s) -- its notification at +1 ns is not
  before the stop, so the steady iteration must leave it pending -- and to
  the stop times of test_ps_close_gpu.py inside windows, then to the end; the
  same in a child process with SHD_PS_BATCH=4.

  long window (results only, not the route): the near graph with its
  latencies times 300 (W = 5.1 s, above 2^32 ns), 64 hosts, load 1, 600 s:
  117 windows (the first batch of up to 64 launched rounds takes the first
  touches; persistent launches start behind it, so a run of a few windows
  would have none), 7 326 / 0 / 162 / 0.  The steady iteration compares 64-bit
  times and has no window limit of its own, so it does run here; the test
  checks that the results at such a window are the oracle's, and stands
  guard for 32-bit window offsets, should a later change bring them.

  idle: the 129-host idle case of test_ps_close_gpu.py: 96.6 % idle
  host-windows, lanes without a host in the third block: 5 464 / 0 / 162 /
  160 526.

  sparse: the lossy case forced onto k_round_sp (SHD_SP_HOSTS=64), which keeps
  the general iteration.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_ffi as O
import shdgpu as S
import workloads as W
from sim import Engine, PathCache
import test_ps_close_gpu as T

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "shadow-1_amd")
MTU = S.SHD_MTU


def tie_graph():
    """the three-vertex graph of the near cases with edge latencies of 18, 17 and 19 ms (self loops 20 ms):
    paths 1 ms apart, so a host hears from two vertices a millisecond apart"""
    g = W.geometric_graph(3, seed=121, integer_latency=True)
    assert list(g.src) == [0, 1, 0, 0, 1, 2] and list(g.dst) == [1, 2, 2, 0, 1, 2]
    return S.GraphArrays(g.n_vertices, g.src, g.dst, np.array([18.0, 17.0, 19.0, 20.0, 20.0, 20.0]), g.loss, g.vertex_loss)


def make_case(name, trace=False):
    sec = S.SHD_SEC
    if name.startswith("near") or name.startswith("tie"):
        near = name.startswith("near")
        g = W.geometric_graph(3, seed=121, integer_latency=True) if near else tie_graph()
        return g, W.phold_model(T.spread_hosts(int(name[4 if near else 3:]), 3), end_time=10 * sec, load=1 if near else 2,
                                seed=2, trace=trace)
    assert not trace
    if name == "down":
        return (W.geometric_graph(129, seed=3),
                W.phold_model(W.hosts_on_vertices(129, 1), end_time=3 * sec, load=16, payload=1500, bw_down=512,
                              bw_up=10240, codelq_cap=64))
    if name == "up":
        return (W.geometric_graph(129, seed=3),
                W.phold_model(W.hosts_on_vertices(129, 1), end_time=2 * sec, load=8, payload=1500, bw_down=10240,
                              bw_up=256))
    if name == "long":
        g = W.geometric_graph(3, seed=121, integer_latency=True)
        g = S.GraphArrays(g.n_vertices, g.src, g.dst, g.latency * 300.0, g.loss, g.vertex_loss)
        return g, W.phold_model(T.spread_hosts(64, 3), end_time=600 * sec, load=1, seed=2)
    return T.make_case(name)


_routes = {}
_bounds = {}   # per case, each window's (start, end)


def routes(name, g, m, window):
    """Per window and host, from the oracle stepped through the engine's
    windows: 0 idle, 1 steady, 2 backlog, 3 other (module docstring); and the
    CoDel drops, the host-windows that start with a router queue, with the
    receive bucket and with the send bucket below an MTU at an end, and those
    with fewer sends than datagrams read."""
    if name in _routes:
        return _routes[name]
    st = O.OState(m, g)
    end = int(m.params["end_time"])
    prev = st.digest().copy()
    cls, extra, bounds = [], np.zeros(5, dtype=np.int64), []
    i64 = lambda d, f: d[f].astype(np.int64)
    while True:
        ws = st.next_time()
        if ws >= end:
            break
        st.run_serial(min(ws + window, end))
        bounds.append((ws, min(ws + window, end)))
        d = st.digest().copy()
        ev = i64(d, "n_events") - i64(prev, "n_events")
        pkt = i64(d, "n_pkt_events") - i64(prev, "n_pkt_events")
        recv = i64(d, "n_recv") - i64(prev, "n_recv")
        sends = (i64(d, "n_sent") + i64(d, "n_inet_drop")) - (i64(prev, "n_sent") + i64(prev, "n_inet_drop"))
        cdrop = i64(d, "n_codel_drop") - i64(prev, "n_codel_drop")
        queue = (prev["codel_total"] != 0) | (d["codel_total"] != 0)
        rx_low = (prev["rx_remaining"] < MTU) | (d["rx_remaining"] < MTU)
        tx_low = (prev["tx_remaining"] < MTU) | (d["tx_remaining"] < MTU)
        backlog = (ev > 0) & (queue | (cdrop > 0) | rx_low | tx_low)
        other = (ev > 0) & ~backlog & ((sends != recv) | (pkt != recv))
        steady = (ev > 0) & ~backlog & ~other
        cls.append(np.where(steady, 1, np.where(backlog, 2, np.where(other, 3, 0))))
        extra += [int(cdrop.sum()), int(((ev > 0) & (prev["codel_total"] != 0)).sum()), int(((ev > 0) & rx_low).sum()),
                  int(((ev > 0) & tx_low).sum()), int((other & ((sends < recv) | (pkt < recv))).sum())]
        prev = d
    assert np.array_equal(prev, T.oracle_of(name, g, m)[0])   # the stepped oracle ends where engine_run does
    st.close()
    cls = np.array(cls)
    cls.setflags(write=False)
    _routes[name] = (cls, extra)
    _bounds[name] = bounds
    return _routes[name]


def counts(cls):
    return tuple(int((cls == k).sum()) for k in (1, 2, 3, 0))


def side_by_side(cls, a, b):
    """block-windows (64 hosts in registration order) that hold a host-window of class a and one of class b"""
    n = 0
    for lo in range(0, cls.shape[1], 64):
        blk = cls[:, lo:lo + 64]
        n += int(((blk == a).any(axis=1) & (blk == b).any(axis=1)).sum())
    return n


_gpu = {}


def gpu_of(name, g, m):
    if name not in _gpu:
        _gpu[name] = T.run_gpu(g, m)
    return _gpu[name]


def run_case(name):
    g, m = make_case(name)
    dg, st = gpu_of(name, g, m)
    T.check(name, g, m, dg, st)
    cls, extra = routes(name, g, m, int(st.window_ns))
    print(f"{name}: window {st.window_ns} ns, {len(cls)} windows, host-windows steady / backlog / other / idle "
          f"{counts(cls)}; steady beside other {side_by_side(cls, 1, 3)}, beside backlog {side_by_side(cls, 1, 2)}; "
          f"CoDel drops {extra[0]}, start with a queue {extra[1]}, rx below an MTU {extra[2]}, tx below an MTU {extra[3]}, "
          f"fewer sends than reads {extra[4]}")
    return g, m, st, cls, extra


@pytest.mark.parametrize("n", [64, 65])
def test_steady_next_to_general_in_one_wave(n):
    g, m, st, cls, _ = run_case(f"near{n}")
    assert st.window_ns == 17_000_000
    steady, _, other, _ = counts(cls)
    assert steady > 1000 and other > 100
    assert side_by_side(cls, 1, 3) > 100
    # (no tie here: the oracle shows none of this graph's arrivals at its host's refill time)
    on_boundary, ties = refill_ties(f"near{n}")
    print(f"near{n}: arrivals on a millisecond boundary {on_boundary}, at the host's refill time {len(ties)}")


@pytest.mark.parametrize("n", [64, 65])
def test_ties_with_the_refill_timer_beside_steady_lanes(n):
    name = f"tie{n}"
    g, m, st, cls, _ = run_case(name)
    assert st.window_ns == 17_000_000
    on_boundary, ties = refill_ties(name)
    beside = 0
    for t, h in ties:   # steady host-windows in the tie's own window and block
        i = next(k for k, (ws, we) in enumerate(_bounds[name]) if ws <= t < we)
        blk = cls[i, h // 64 * 64:h // 64 * 64 + 64]
        beside += int((np.delete(blk, h % 64) == 1).any())
    print(f"{name}: arrivals on a millisecond boundary {on_boundary}, at the host's refill time {len(ties)} "
          f"(hosts {len(set(h for _, h in ties))}), with steady host-windows in the window's block {beside}")
    assert len(ties) > 0 and beside == len(ties)
    assert counts(cls)[0] > 1000


def test_loopback_beside_steady_lanes():
    _, m, _, cls, extra = run_case("near64")
    assert m.n_hosts == 64
    assert extra[4] > 50            # host-windows with a datagram read and not answered by a deferred send
    assert side_by_side(cls, 1, 3) > 100


@pytest.mark.parametrize("name", ["down", "up"])
def test_buckets_and_codel(name):
    _, _, _, cls, extra = run_case(name)
    steady, backlog, _, _ = counts(cls)
    assert steady > 1000 and backlog > 1000 and side_by_side(cls, 1, 2) > 100
    if name == "down":
        assert extra[0] > 0 and extra[1] > 100 and extra[2] > 100   # CoDel drops, router queues, rx_rem < MTU
    else:
        assert extra[3] > 1000                                      # tx_rem < MTU: sends that wait in the send queue


def test_pool_count_and_early_flushes():
    g, m, st, cls, _ = run_case("multi4")
    sends, _, _ = T.oracle_windows("multi4", g, m, int(st.window_ns))
    print(f"multi4: rounds above 64 sends {int((sends > 64).sum())}, above {T.POOL_ROOM} {int((sends > T.POOL_ROOM).sum())}")
    assert int((sends > T.POOL_ROOM).sum()) >= 1 and int((sends > 64).sum()) > 100
    assert counts(cls)[0] > 10000


def test_lossy_ids_given_back():
    g, m, _, cls, _ = run_case("lossy")
    odg, _ = T.oracle_of("lossy", g, m)
    assert int(odg["n_inet_drop"].sum()) > 1000 and counts(cls)[0] > 10000


def test_idle_lanes():
    _, _, _, cls, _ = run_case("idle")
    steady, _, _, idle = counts(cls)
    assert cls.shape[1] == 129 and steady > 1000 and idle / cls.size > 0.9


def test_long_window_results_equal_the_oracle():
    """Results only: the steady iteration has no window limit and runs at this window too."""
    _, _, st, cls, _ = run_case("long")
    assert st.window_ns >= 1 << 32
    assert 64 < len(cls) < 200 and counts(cls)[0] > 1000


def test_forced_sparse_kernel(monkeypatch):
    g, m = make_case("lossy")
    pdg, pst = gpu_of("lossy", g, m)
    assert pst.n_batches_sparse == 0
    monkeypatch.setenv("SHD_SP_HOSTS", "64")
    dg, st = T.run_gpu(g, m)
    T.check("lossy", g, m, dg, st)
    assert st.n_batches_sparse > 0 and st.n_rounds == pst.n_rounds


_arrivals = {}


def arrivals(name):
    """(time, host) of every arrival of the traced oracle run of a case's model, once"""
    if name not in _arrivals:
        g, m = make_case(name)
        tr, dg, _ = O.engine_run(make_case(name, trace=True)[1], g)
        assert np.array_equal(dg, T.oracle_of(name, g, m)[0])   # tracing does not change the run
        a = tr[tr["kind"] == S.TR_ARRIVE][["time", "host"]].copy()
        a.setflags(write=False)
        _arrivals[name] = a
    return _arrivals[name]


def refill_ties(name):
    """Arrivals at the host's refill timer's own time (take_next_full), from the
    oracle: for every millisecond boundary T that has an arrival, the state
    stepped to just before T (every event before T run); a refill pending then
    fires at the first boundary behind the event that scheduled it, which is T,
    so an arrival at T at a host with the refill pending is a tie.  (the
    number of arrivals on a boundary, the ties as (time, host))"""
    g, m = make_case(name)
    a = arrivals(name)
    a = a[a["time"] % S.SHD_MS == 0]
    st = O.OState(m, g)
    ties = []
    for t in np.unique(a["time"]):
        st.run_serial(int(t))
        pending = (st.digest()["flags"] & 1) != 0
        ties += [(int(t), int(h)) for h in np.unique(a["host"][a["time"] == t]) if pending[h]]
    st.close()
    return len(a), ties


def arrival_stop(g, m):
    """1 ns after near64's first arrival after 5 s"""
    t = arrivals("near64")["time"]
    return int(t[t > 5 * S.SHD_SEC].min()) + 1


def stops(g, m):
    return sorted([arrival_stop(g, m)] + [int(x * S.SHD_SEC) for x in T.STEPS]) + [int(m.params["end_time"])]


def gpu_steps(g, m, times):
    pc = PathCache(g, W.attached_vertices(m.host_vertex))
    eng = Engine(m, pc)
    eng.boot()
    out, nev, npkt = [], 0, 0
    for t in times:
        st = eng.run_until(t)
        assert st.error == 0
        nev += st.n_events
        npkt += st.n_pkt_events
        out.append((eng.digest().copy(), nev, npkt, (st.n_rounds, st.n_batches, st.n_batches_persistent)))
    eng.close()
    pc.close()
    return out


def check_steps(tag, g, m, times, got):
    st = O.OState(m, g)
    for k, t in enumerate(times):
        st.run_serial(t)
        dg, nev, npkt, (rounds, batches, persistent) = got[k]
        onev, onpkt = st.counts()
        print(f"{tag}: step {k} to {t} ns: rounds {rounds} batches {batches} persistent {persistent} events {nev}/{onev} "
              f"packet events {npkt}/{onpkt}")
        assert (nev, npkt) == (onev, onpkt)
        assert np.array_equal(dg, st.digest())
        assert persistent > 0
    st.close()


def test_notification_across_the_stop():
    g, m = make_case("near64")
    times = stops(g, m)
    a = arrival_stop(g, m)
    assert a in times and a % 17_000_000 and all(t % 17_000_000 for t in times[:-1])   # inside windows
    check_steps("steps", g, m, times, gpu_steps(g, m, times))


CHILD = r"""
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import test_ps_iter_gpu as I
g, m = I.make_case("near64")
times = json.loads(sys.argv[4])
got = I.gpu_steps(g, m, times)
np.save(sys.argv[3], np.stack([x[0] for x in got]))
print(json.dumps([[int(x[1]), int(x[2]), [int(v) for v in x[3]]] for x in got]))
"""


def test_notification_across_the_stop_short_batches(tmp_path):
    """SHD_PS_BATCH is read once per process: the run is a child's."""
    g, m = make_case("near64")
    times = stops(g, m)
    out = tmp_path / "digests.npy"
    p = subprocess.run([sys.executable, "-c", CHILD, PKG, HERE, str(out), json.dumps(times)],
                       env=dict(os.environ, SHD_PS_BATCH="4"), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = json.loads(p.stdout.strip().splitlines()[-1])
    dgs = np.load(out)
    got = [(dgs[k], r[0], r[1], tuple(r[2])) for k, r in enumerate(rows)]
    check_steps("batch4", g, m, times, got)
    assert sum(x[3][2] for x in got) > 100
