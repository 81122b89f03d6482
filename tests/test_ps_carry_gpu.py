"""The persistent round's far deliveries, which complete behind the share
(ps_loop_close's CARRY, flush_finish_far, ps_publish's counted wait), at small
sizes against the serial oracle.

In the manner of test_ps_exit_gpu.py, whose helpers and those of
test_ps_iter_gpu.py and test_ps_close_gpu.py this file imports: every case
runs untraced (the lean kernels), compares every host's end state
(Engine.digest()) and the event counts with the oracle, and must have run
persistent launches.  What each case is for is counted on the CPU with the
oracle alone and asserted, so that a case cannot pass without holding what it
is here for.

The rule (eng_round.h): a delivery of the last flush of round i is far when
its calendar bin is not before b(min(N + W, stop)) + kPfBins, N the block's
next time after the round; a far delivery's stores stay in flight across the
share.  deliveries() below lists every delivery of the traced oracle run --
its send's time, sender and receiver from the SENT record, its arrival time
from the path latency between the two hosts' vertices -- and sorts it by the
window (the oracle stepped through [next time, min(next time + W, end)),
windows() of test_ps_exit_gpu.py) it was sent in; the rule is applied with N
the oracle's next time after that window, which is a lower bound of every
block's N, so the deliveries it marks near include the engine's near ones and
the ones it marks far may be far in the engine.  (The engine's rounds are a few
more than the oracle's windows, as a calendar bin's start stands for a time
not yet known; the counts below hold for the oracle's.)

  mixed64, mixed65: the three-vertex graph of the near cases with edge
  latencies of 17, 400 and 409 ms (self loops 20 ms): W = 17 ms, bins of 2^24
  ns; paths of 1 to 1.2 W beside paths of 23 W.  Near and far deliveries side
  by side in one block's window, and windows of one kind only.

  ring64, ring65: one host per vertex of a ring of 64 (65) vertices, edges of
  4 ms, self loops of 1 ms: W = 1 ms, bins of 2^19 ns, paths of 4 to 128 ms,
  3 s: a sparse model, nearly every window starts later than the previous one
  ended.  Deliveries kPfBins bins or more behind their window's end but
  inside, or within kPfBins bins behind, the next window: near by the rule's
  N -- a test on the bins behind the window's end alone would call them far.
  ring64: 517 windows, 487 starting late, 60 such deliveries (every near one),
  1852 far; ring65: 526, 495, 59, 1848.

  ping2: two hosts 50 ms apart on a graph whose self loops give W = 1 ms, one
  message each, 20 s: 401 windows, 718 deliveries of that kind, 40 far.  And
  a far delivery that is the model's only event behind the next window: the
  window after next starts at its time, which its receiver's bitmap of the
  round between may not show yet and the sender publishes in its place; the
  sender runs another event in the window between, so the time is not its
  min_emit there.  ping2 has 21, ring64 5, ring65 3.

  hub64, hub65: 63 (64) hosts on one vertex 100 ms from the hub's, every second
  draw the hub: deliveries from many lanes of one flush, and of both blocks,
  into one far bin of the hub, more than kBinCap = 4 of them.

  steps: mixed64 run to stops inside windows, and again with SHD_PS_BATCH=4 in
  a child process; ring65 on its fresh path cache, whose 4225 vertex pairs
  are first used all through the run (1140 after window 128, in 370 windows,
  each with far deliveries), so that batches halt on a first touch with far
  deliveries in hand.

  the routes that must not change: the lossy case forced onto k_round_sp, and
  near65's named host in the other block.
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
import test_ps_close_gpu as T
import test_ps_exit_gpu as X
import test_ps_iter_gpu as I

pytestmark = pytest.mark.gpu

K_PF_BINS = 3    # eng_round.h kPfBins
K_BIN_CAP = 4    # eng_device.h kBinCap
MS = S.SHD_MS


def graph3(lat):
    """the three-vertex graph of the near cases with its six latencies replaced (edges 0-1, 1-2, 0-2, three self loops)"""
    g = W.geometric_graph(3, seed=121, integer_latency=True)
    assert list(g.src) == [0, 1, 0, 0, 1, 2] and list(g.dst) == [1, 2, 2, 0, 1, 2]
    return S.GraphArrays(g.n_vertices, g.src, g.dst, np.array(lat, dtype=np.float64), g.loss * 0.0, g.vertex_loss)


def ring(n, edge_ms, self_ms):
    v = np.arange(n, dtype=np.int32)
    src = np.concatenate([v, v])
    dst = np.concatenate([(v + 1) % n, v]).astype(np.int32)
    lat = np.concatenate([np.full(n, float(edge_ms)), np.full(n, float(self_ms))])
    return S.GraphArrays(n, src, dst, lat, np.zeros(2 * n), np.zeros(n))


def hub_cum(n):
    """cumulative destination weights: host 0 one half, the others the rest evenly"""
    w = np.full(n, 0.5 / (n - 1))
    w[0] = 0.5
    cum = np.cumsum(w)
    cum[-1] = 1.0
    return cum


def make_case(name, trace=False):
    sec = S.SHD_SEC
    if name.startswith("mixed"):
        return (graph3([17.0, 400.0, 409.0, 20.0, 20.0, 20.0]),
                W.phold_model(T.spread_hosts(int(name[5:]), 3), end_time=10 * sec, load=1, seed=2, trace=trace))
    if name.startswith("ring"):
        n = int(name[4:])
        return ring(n, 4, 1), W.phold_model(W.hosts_on_vertices(n, 1), end_time=3 * sec, load=1, seed=2, trace=trace)
    if name == "ping2":
        return (graph3([50.0, 50.0, 50.0, 1.0, 1.0, 1.0]),
                W.phold_model(np.array([0, 1], dtype=np.int32), end_time=20 * sec, load=1, seed=2, trace=trace))
    if name.startswith("hub"):
        n = int(name[3:])
        hv = np.ones(n, dtype=np.int32)
        hv[0] = 0
        return (graph3([100.0, 100.0, 100.0, 17.0, 17.0, 17.0]),
                W.phold_model(hv, end_time=10 * sec, load=1, seed=2, trace=trace, dest_cum=hub_cum(n)))
    raise KeyError(name)


# the helpers of the files this one imports take their cases by name from their own make_case
_orig_make_case = I.make_case


def _make_case(name, trace=False):
    try:
        return make_case(name, trace)
    except KeyError:
        return _orig_make_case(name, trace)


@pytest.fixture(autouse=True)
def _cases(monkeypatch):
    monkeypatch.setattr(I, "make_case", _make_case)


_deliv = {}


def deliveries(name):
    """Every delivery of the traced oracle run: (send time, sender, receiver, arrival time), by send time."""
    if name in _deliv:
        return _deliv[name]
    g, m = _make_case(name)
    tr, dg, _ = O.engine_run(_make_case(name, trace=True)[1], g)
    assert np.array_equal(dg, T.oracle_of(name, g, m)[0])   # tracing does not change the run
    s = tr[(tr["kind"] == S.TR_SENT) & (tr["host"] != tr["peer"])]
    hv = np.asarray(m.host_vertex)
    att = W.attached_vertices(hv)
    og = O.OGraph(g)
    lat = {}
    for a in att:
        row = og.row(int(a), att)[0]
        for b, x in zip(att, row):
            lat[(int(a), int(b))] = float(x)
    ns = np.array([int(np.ceil(lat[(int(hv[h]), int(hv[p]))] * MS)) for h, p in zip(s["host"], s["peer"])], dtype=np.int64)
    t = s["time"].astype(np.int64)
    arr = t + ns
    keep = arr < int(m.params["end_time"])
    out = np.stack([t[keep], s["host"][keep].astype(np.int64), s["peer"][keep].astype(np.int64), arr[keep]], axis=1)
    out = out[np.argsort(out[:, 0], kind="stable")]
    # the arrivals the oracle reports are these
    a = tr[tr["kind"] == S.TR_ARRIVE]
    assert np.array_equal(np.sort(out[:, 3] * 4096 + out[:, 2]), np.sort(a["time"].astype(np.int64) * 4096 + a["host"]))
    out.setflags(write=False)
    _deliv[name] = out
    return out


def classify(name, window):
    """Per delivery: the window it was sent in, near by the rule with N the oracle's next time after that
    window, its bin, the bin of that window's end, and N."""
    bounds, _, _ = X.windows(name, window)
    d = deliveries(name)
    shift = int(window).bit_length() - 1
    stop = int(bounds[-1, 1])
    wi = np.searchsorted(bounds[:, 0], d[:, 0], side="right") - 1
    assert ((d[:, 0] >= bounds[wi, 0]) & (d[:, 0] < bounds[wi, 1])).all()
    nxt = np.append(bounds[1:, 0], stop)[wi]
    lim = np.minimum(nxt + window, stop)
    bb = d[:, 3] >> shift
    near = bb < (lim >> shift) + K_PF_BINS
    return wi, near, bb, bounds[wi, 1] >> shift, nxt


def run(name):
    g, m = make_case(name)
    dg, st = I.gpu_of(name, g, m)
    T.check(name, g, m, dg, st)
    return g, m, st


@pytest.mark.parametrize("name", ["mixed64", "mixed65"])
def test_near_and_far_side_by_side(name):
    _, m, st = run(name)
    w = int(st.window_ns)
    assert w == 17 * MS
    wi, near, _, _, _ = classify(name, w)
    d = deliveries(name)
    key = wi * 2 + d[:, 1] // 64          # (window, sender's block)
    both = np.intersect1d(key[near], key[~near])
    only_near = np.setdiff1d(key[near], key[~near])
    only_far = np.setdiff1d(key[~near], key[near])
    print(f"{name}: deliveries near {int(near.sum())} far {int((~near).sum())}; block-windows with both {len(both)}, "
          f"near only {len(only_near)}, far only {len(only_far)}")
    assert len(both) >= 100 and len(only_near) >= 30 and len(only_far) >= 10
    if name == "mixed65":   # the second block (host 64 alone) sends both kinds too, and receives far ones
        assert int((near & (d[:, 1] == 64)).sum()) >= 10 and int((~near & (d[:, 1] == 64)).sum()) >= 10
        assert int((~near & (d[:, 2] == 64) & (d[:, 1] < 64)).sum()) >= 10


@pytest.mark.parametrize("name", ["ring64", "ring65", "ping2"])
def test_windows_that_start_later(name):
    """Deliveries kPfBins bins or more behind their window's end that the next window, which starts later, takes in or
    has within kPfBins bins behind it: near by the rule, far by a test on the bins behind the window's end."""
    _, m, st = run(name)
    w = int(st.window_ns)
    assert w == MS
    later, _, _ = X.gap_counts(name, w)
    wi, near, bb, bwe, nxt = classify(name, w)
    ahead = near & (bb >= bwe + K_PF_BINS)
    inside = ahead & (deliveries(name)[:, 3] < nxt + w)
    print(f"{name}: windows starting after the previous end {later}; near deliveries at least {K_PF_BINS} bins "
          f"behind their window's end's {int(ahead.sum())}, inside the next window {int(inside.sum())}; far "
          f"{int((~near).sum())}")
    assert later >= 100 and int(ahead.sum()) >= 5 and int(inside.sum()) >= 5
    assert int((~near).sum()) >= 20


@pytest.mark.parametrize("name,least", [("ping2", 5), ("ring64", 5), ("ring65", 3)])
def test_far_delivery_is_the_next_event(name, least):
    """Windows whose start is the arrival of a far delivery sent two windows before (the sender ran another
    event in the window between): the receiver's bitmap of the round between may miss it."""
    _, m, st = run(name)
    w = int(st.window_ns)
    assert w == MS
    bounds, _, ev = X.windows(name, w)
    wi, near, _, _, _ = classify(name, w)
    d = deliveries(name)
    far = np.nonzero(~near & (wi + 2 < len(bounds)))[0]
    hit = [k for k in far if bounds[wi[k] + 2, 0] == d[k, 3]]
    busy = [k for k in hit if ev[wi[k] + 1, d[k, 1]] > 0]   # the sender has an event in the window between
    print(f"{name}: {len(bounds)} windows, far deliveries {len(far)}, the start of the window after next {len(hit)}, "
          f"with an event of the sender between {len(busy)}")
    assert len(busy) >= least


@pytest.mark.parametrize("name", ["hub64", "hub65"])
def test_far_bin_overflows(name):
    _, m, st = run(name)
    w = int(st.window_ns)
    assert w == 17 * MS
    wi, near, bb, _, _ = classify(name, w)
    d = deliveries(name)
    f = ~near
    key = np.stack([wi[f], d[f, 2], bb[f]], axis=1)
    u, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    over = np.nonzero(cnt > K_BIN_CAP)[0]
    two = 0
    for k in over:
        blocks = np.unique(d[f][inv.ravel() == k, 1] // 64)
        two += int(len(blocks) > 1)
    print(f"{name}: far (window, host, bin) with more than {K_BIN_CAP} deliveries {len(over)}, most {int(cnt.max())}, "
          f"from two blocks {two}")
    assert len(over) >= 20
    if name == "hub65":
        assert two >= 5


def far_stops(name, window):
    """Stop times 1 ns behind the send of the first far delivery after 3.5 s (behind the launched rounds of the
    run's start), 5.3333 s, 5.34 s and 7.0085 s, each inside its window; then the end: every step but the last
    leaves the round loop at the stop with a far delivery of that round in hand."""
    g, m = make_case(name)
    wi, near, _, _, _ = classify(name, window)
    bounds, _, _ = X.windows(name, window)
    d = deliveries(name)
    times = []
    for base in (3.5, 5.3333, 5.34, 7.0085):
        k = int(np.nonzero(~near & (d[:, 0] > int(base * S.SHD_SEC)))[0][0])
        t = int(d[k, 0]) + 1
        assert bounds[wi[k], 0] < t < bounds[wi[k], 1]
        times.append(t)
    assert times == sorted(set(times))
    return times + [int(m.params["end_time"])]


def test_stops_inside_windows():
    g, m = make_case("mixed64")
    times = far_stops("mixed64", 17 * MS)
    print(f"mixed64: stops {times}")
    I.check_steps("steps", g, m, times, I.gpu_steps(g, m, times))


CHILD = r"""
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import test_ps_iter_gpu as I
import test_ps_carry_gpu as C
g, m = C.make_case(sys.argv[5])
times = json.loads(sys.argv[4])
got = I.gpu_steps(g, m, times)
np.save(sys.argv[3], np.stack([x[0] for x in got]))
print(json.dumps([[int(x[1]), int(x[2]), [int(v) for v in x[3]]] for x in got]))
"""


def test_stops_inside_windows_short_batches(tmp_path):
    """SHD_PS_BATCH is read once per process: the run is a child's."""
    g, m = make_case("mixed64")
    times = far_stops("mixed64", 17 * MS)
    out = tmp_path / "digests.npy"
    p = subprocess.run([sys.executable, "-c", CHILD, I.PKG, I.HERE, str(out), json.dumps(times), "mixed64"],
                       env=dict(os.environ, SHD_PS_BATCH="4"), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = json.loads(p.stdout.strip().splitlines()[-1])
    dgs = np.load(out)
    got = [(dgs[k], r[0], r[1], tuple(r[2])) for k, r in enumerate(rows)]
    I.check_steps("batch4", g, m, times, got)
    assert sum(x[3][2] for x in got) > 100


def test_first_touches_late_in_the_run():
    """ring65 on a fresh path cache: a pair of vertices is first used whenever a host first draws a new
    destination, so batches halt on first touches long after persistent launches have begun, with the halting
    round's far deliveries in hand."""
    g, m, st = run("ring65")
    d = deliveries("ring65")
    wi, near, _, _, _ = classify("ring65", int(st.window_ns))
    pair = d[:, 1] * 65 + d[:, 2]
    _, first = np.unique(pair, return_index=True)
    late = first[wi[first] > 128]            # first touches behind the launched rounds of the run's start
    rounds = np.unique(wi[late])
    withfar = sum(int((~near & (wi == i)).any()) for i in rounds)
    print(f"ring65: pairs first used after window 128: {len(late)}, in {len(rounds)} windows, {withfar} of them with "
          f"far deliveries; batches {st.n_batches}, persistent {st.n_batches_persistent}")
    assert len(rounds) >= 50 and withfar >= 50


def test_sparse_kernel_keeps_its_flush(monkeypatch):
    g, m = I.make_case("lossy")
    pdg, pst = I.gpu_of("lossy", g, m)
    T.check("lossy", g, m, pdg, pst)
    assert pst.n_batches_sparse == 0
    monkeypatch.setenv("SHD_SP_HOSTS", "64")
    dg, st = T.run_gpu(g, m)
    T.check("lossy", g, m, dg, st)
    assert st.n_batches_sparse > 0 and st.n_rounds == pst.n_rounds


def test_named_host_in_the_other_block():
    """near65: every delivery between the blocks into bins staged ahead is near, is noted and names the
    receiver in the share, as before."""
    g, m, st, _, _ = I.run_case("near65")
    sends, _, _ = T.oracle_windows("near65", g, m, int(st.window_ns))
    wi, near, _, _, _ = classify("near65", int(st.window_ns))
    d = deliveries("near65")
    cross = (d[:, 1] // 64) != (d[:, 2] // 64)
    print(f"near65: deliveries between the blocks near {int((near & cross).sum())} far {int((~near & cross).sum())}")
    assert int((near & cross).sum()) >= 100
    assert st.window_ns == X.W17 and st.n_rounds >= len(sends) >= 500
