"""The persistent round's tail -- the last flush's resolve and stores, the
close, the share gather -- at small sizes against the serial oracle.

In the style of test_lean_rounds_gpu.py: every case runs untraced, without
heartbeats and without a bootstrap period (the lean instantiations
k_round_ps<true> / k_round_sp<true>), compares every host's end state
(Engine.digest()) and the event counts with oracle_ffi.engine_run, and must
have run persistent launches.  The cases were chosen on the CPU with the
oracle alone (each runs there in under 1 s); what it shows:

  drop test (flush_wave: chance <= rel with chance = x / RAND_MAX, which is
  true for every draw on a path with rel >= 1.0 -- the two sides a shortcut for
  such paths would have to keep apart): a geometric graph whose edges
  lose up to 5 % has no path with rel == 1.0 at all (two hosts on a vertex
  talk over its self-loop, which loses too), so the lossy graph here is that
  graph with every second edge, in document order, lossless: 129 hosts on its
  129 vertices, seed 2, 3 s.  11.3 % of the host pairs' paths then have
  rel == 1.0 exactly, 11.0 % of the 38 254 sends take one, 1 973 sends are
  dropped, and 1 455 times two sends of one block's hosts less than 1 % of a
  window apart are one with rel == 1.0 and one with rel < 1.0 (a flush takes
  all of a block's sends since the last, so such a pair is in one batch unless
  a round's end falls into that 1 %): batches that hold both kinds.  The same
  model on the graph with loss_max = 0 has rel == 1.0 everywhere: nothing is
  dropped.

  destinations (closed_dest: the quotient by RAND_MAX and the exception
  list): engine.hip turns dest_closed on when host h sits on
  attached index h and the thresholds of the cumulative weights are
  floor((i + 1) RAND_MAX / H) but for at most 16 draws.  closed_exceptions()
  below mirrors that check.  With equal weights no host count from 65 to 300
  has an exception (the f64 sums are too exact at these sizes; 10 000 hosts
  have one), so the case with exceptions is 100 hosts whose host 50
  weighs 1 + 8e-9: four exceptions, and the list checks out at every
  threshold, so dest_closed stays on.  200 equally weighted hosts have none.
  150 hosts on 75 vertices have host_att[h] != h: dest_closed is off and the
  guide table picks.  (A draw is one of 2^31 values, so no run ever draws an
  exception: what the case runs is the list's select on every record.)

  store before prefetch (ps_loop_close stores the last flush's deliveries
  before it loads the next window's bins): three vertices, whole-millisecond
  latencies, seed 121: the window is the least edge latency, 17 ms, a calendar
  bin 2^24 ns, and the paths take 17, 19, 26, 34 and 38 ms (a vertex to itself:
  twice its nearest edge).  pf_lim is three bins from the bin of the window's
  end, so a delivery lands before it -- in a bin its receiver loads ahead --
  whenever it arrives less than two bins (33.5 ms) after the window's end: all
  of the 67.5 % of the 202 907 sends that take 17, 19 or 26 ms; the 34-ms ones
  (21 %) miss it only when sent in the last half millisecond of a window that
  ends less than half a millisecond before its bin does, the 38-ms ones (12 %)
  in about one case in thirty: nearly every delivery.  64 hosts: one block,
  every receiver in the sender's own; 65 hosts: host 64 alone in a second
  block, 3.1 % of the deliveries cross.  10 s: more than 520 rounds.

  gather past one chunk (ps_gather takes 64 * 4 = 256 shares a chunk): 16 385
  hosts on 400 vertices are 257 blocks, the last with one lane; load 1 for 2 s:
  951 148 events, 290 704 packet events.

  sparse kernel: the lossy model above forced onto k_round_sp (SHD_SP_HOSTS,
  as test_lean_rounds_gpu.py does), against its own unforced run.
"""
import bisect

import numpy as np
import pytest

import oracle_ffi as O
import shdgpu as S
import workloads as W
from sim import Engine, PathCache

pytestmark = pytest.mark.gpu

RAND_MAX = 2147483647
DEST_EXC = 16   # eng_device.h kDestExc


def spread_hosts(n_hosts, n_vertices):
    """n_hosts hosts over n_vertices vertices, in registration order."""
    return (np.arange(n_hosts, dtype=np.int64) * n_vertices // n_hosts).astype(np.int32)


def half_lossless(g):
    """g with every second edge (document order) lossless."""
    loss = g.loss.copy()
    loss[::2] = 0.0
    return S.GraphArrays(g.n_vertices, g.src, g.dst, g.latency, loss, g.vertex_loss)


def draw_threshold(c):
    """engine.hip draw_threshold: the largest draw x with x / RAND_MAX <= c."""
    def ok(x):
        return x / float(RAND_MAX) <= c
    if ok(RAND_MAX):
        return RAND_MAX
    x = min(max(int(c * float(RAND_MAX)), 0), RAND_MAX)
    while x >= 0 and not ok(x):
        x -= 1
    while ok(x + 1):
        x += 1
    return x


def closed_pick(x, n_hosts):
    """eng_device.h closed_dest's formula (engine.hip pick_closed)."""
    c = (x * n_hosts + RAND_MAX - 1) // RAND_MAX
    return c - 1 if c else 0


def closed_exceptions(cum):
    """engine.hip's creation-time check of the closed-form destinations of
    one class of cumulative weights (hosts on attached index h): the list of
    exceptions (draw, destination), or None where it turns dest_closed off."""
    n = len(cum)
    ty = [draw_threshold(float(c)) for c in cum]
    thr0 = ty[-1]
    exc = []
    for i in range(n):
        f = ((i + 1) * RAND_MAX) // n
        if f == ty[i]:
            continue
        for x in range(min(f, ty[i]) + 1, max(f, ty[i]) + 1):
            if x > thr0:
                break
            t = bisect.bisect_left(ty, x)
            if t != closed_pick(x, n):
                if len(exc) == DEST_EXC:
                    return None
                exc.append((x, t))
    ex = dict(exc)
    for i in range(n):
        for x in (0, ty[i] + 1, ((i + 1) * RAND_MAX) // n + 1):
            if x <= thr0 and ex.get(x, closed_pick(x, n)) != bisect.bisect_left(ty, x):
                return None
    return exc


def make_case(name):
    """(graph, untraced model) of a case."""
    sec = S.SHD_SEC
    if name in ("lossy", "lossless"):
        g = W.geometric_graph(129, seed=2, loss_max=0.05 if name == "lossy" else 0.0)
        if name == "lossy":
            g = half_lossless(g)
        return g, W.phold_model(W.hosts_on_vertices(129, 1), end_time=3 * sec)
    if name == "exc":
        w = np.ones(100)
        w[50] = 1.0 + 8e-9
        return W.geometric_graph(100, seed=2), W.phold_model(W.hosts_on_vertices(100, 1), end_time=3 * sec,
                                                            dest_cum=W.phold_cum(w))
    if name == "noexc":
        return W.geometric_graph(200, seed=2), W.phold_model(W.hosts_on_vertices(200, 1), end_time=3 * sec)
    if name == "guide":
        return W.geometric_graph(75, seed=2), W.phold_model(W.hosts_on_vertices(75, 2), end_time=3 * sec)
    if name.startswith("near"):
        n = int(name[4:])
        return (W.geometric_graph(3, seed=121, integer_latency=True),
                W.phold_model(spread_hosts(n, 3), end_time=10 * sec))
    if name == "chunk":
        return W.geometric_graph(400, seed=2), W.phold_model(spread_hosts(16385, 400), end_time=2 * sec, load=1)
    raise KeyError(name)


_oracle = {}
_gpu = {}


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
          f"packet events {st.n_pkt_events}/{ost['n_pkt_events']} drops {int(odg['n_inet_drop'].sum())}")
    assert st.error == 0
    assert st.n_events == ost["n_events"]
    assert st.n_pkt_events == ost["n_pkt_events"] > 0
    assert np.array_equal(dg, odg)
    assert st.n_batches_persistent > 0
    return odg, ost


def path_rel(g, hv):
    """rel of the path between every pair of attached vertices (a vertex to itself: its self path)."""
    og = O.OGraph(g)
    att = W.attached_vertices(hv)
    rel = np.array([og.row(int(a), att)[1] for a in att])
    for i, a in enumerate(att):
        rel[i, i] = og.self_path(int(a))[1]
    return rel


def test_drop_test_mixed_batches():
    g, m = make_case("lossy")
    rel = path_rel(g, m.host_vertex)
    share = float((rel == 1.0).mean())
    print(f"lossy: {share:.3f} of the paths have rel == 1.0, least rel {rel.min():.4f}")
    assert 0.05 < share < 0.5 and rel.max() == 1.0 and rel.min() < 1.0
    _gpu["lossy"] = run_gpu(g, m)
    odg, _ = check("lossy", g, m, *_gpu["lossy"])
    assert int(odg["n_inet_drop"].sum()) > 0


def test_drop_test_all_skipped():
    g, m = make_case("lossless")
    assert (path_rel(g, m.host_vertex) == 1.0).all()
    dg, st = run_gpu(g, m)
    odg, _ = check("lossless", g, m, dg, st)
    assert int(odg["n_inet_drop"].sum()) == 0


@pytest.mark.parametrize("name", ["exc", "noexc", "guide"])
def test_destinations(name):
    g, m = make_case(name)
    att = np.searchsorted(W.attached_vertices(m.host_vertex), m.host_vertex)   # the hosts' attached indices
    closed = bool((att == np.arange(m.n_hosts)).all())
    exc = closed_exceptions(np.asarray(m.dest_cum, dtype=np.float64).ravel()[:m.n_hosts]) if closed else None
    print(f"{name}: hosts {m.n_hosts}, host h on attached index h: {closed}, exceptions {exc}")
    if name == "exc":
        assert exc is not None and 0 < len(exc) <= DEST_EXC
    elif name == "noexc":
        assert exc == []
    else:
        assert not closed
    dg, st = run_gpu(g, m)
    check(name, g, m, dg, st)


@pytest.mark.parametrize("n", [64, 65])
def test_store_before_prefetch(n):
    name = f"near{n}"
    g, m = make_case(name)
    og = O.OGraph(g)
    lat = np.array([og.row(a, np.arange(3, dtype=np.int32))[0] for a in range(3)])
    for a in range(3):
        lat[a, a] = og.self_path(a)[0]
    lat = lat[np.ix_(m.host_vertex, m.host_vertex)] * 1e6   # per host pair, ns
    dg, st = run_gpu(g, m)
    check(name, g, m, dg, st)
    width = 1 << (int(st.window_ns).bit_length() - 1)   # the calendar's bin width
    near = float((lat <= 2 * width).mean())
    print(f"{name}: path latencies {sorted(set((lat / 1e6).ravel().tolist()))} ms, window {st.window_ns} ns, bin {width} ns, "
          f"{near:.3f} of the host pairs within two bins")
    # a delivery that arrives less than two bins after its round's end lands in a bin loaded
    # ahead: two thirds of the pairs always do, the rest are at most 0.3 windows longer
    assert st.window_ns == int(g.latency.min() * 1e6)
    assert near > 0.6 and lat.max() <= 2 * width + 0.3 * st.window_ns
    assert st.n_rounds >= 300


def test_gather_past_one_chunk():
    g, m = make_case("chunk")
    assert -(-m.n_hosts // 64) == 257
    dg, st = run_gpu(g, m)
    check("chunk", g, m, dg, st)


def test_forced_sparse_kernel_lossy(monkeypatch):
    g, m = make_case("lossy")
    if "lossy" not in _gpu:
        _gpu["lossy"] = run_gpu(g, m)
    pdg, pst = _gpu["lossy"]
    check("lossy", g, m, pdg, pst)
    assert pst.n_batches_sparse == 0
    monkeypatch.setenv("SHD_SP_HOSTS", "64")
    dg, st = run_gpu(g, m)
    check("lossy", g, m, dg, st)
    assert st.n_batches_sparse > 0
    assert st.n_rounds == pst.n_rounds
