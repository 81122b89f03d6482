"""The persistent round's close under its last flush's path loads
(ps_loop_close: flush_last_issue, the close, flush_last_consume) at small
sizes against the serial oracle.

In the style of test_ps_tail_gpu.py, whose helpers this file imports: every
case runs untraced, without heartbeats and without a bootstrap period (the
lean instantiations k_round_ps<true> / k_round_sp<true>), compares every
host's end state (Engine.digest()) and the event counts with
oracle_ffi.engine_run, and must have run persistent launches.  The cases were
chosen on the CPU with the oracle alone: oracle_windows() below steps an
oracle state through the engine's own windows ([next time, next time + W),
W the least path latency) and counts each host's deferred sends (sent +
dropped, loopbacks are not deferred) and events per window; its end state is
engine_run's.  (The engine takes a calendar bin's start for a host's next
time when that is all it knows, so some of its rounds start earlier than the
oracle's next event and it runs a few more: 531 against 518 in the first case.
The counts that matter hold for any window of length W: at load 1 each host
has one message on its way, two sends of one message are a path latency >= W
apart, so no window has more than 64 sends of a block; and the sends of the
application's start are one instant's.)  A block is 64 hosts in registration order.  A round's last
flush takes the block's sends since its last flush inside the loop: it is
split around the close when they are 1 to 64; more than 64 keep the old order
(flush, then close); a block that has deferred more than 224 = kPool - 64
sends flushes inside the loop.  What each case was checked to contain:

  near (prefetch ahead of the resolve): the three-vertex whole-millisecond
  graph of test_ps_tail_gpu.py (seed 121: W = 17 ms, bins of 2^24 ns, paths
  of 17, 19, 26, 34 and 38 ms, two thirds of the host pairs within two bins),
  model seed 2, load 1, 10 s.  64 hosts: 518 rounds, 12 325 sends, 517 rounds
  with sends, none with more than 64 in the block -- every last flush is the
  split one, and with one block every receiver's bins are loaded ahead by the
  sender's own wave, before its stores.  65 hosts (host 64 alone in a second
  block, whose wave has 63 lanes without a host): 519 rounds, 678 block-rounds
  with sends, none above 64, 360 without a send.

  multi (the old order next to the new): the same graph, 64 hosts, model seed
  2, 10 s.  Load 1: no round above 64 sends; loads 2 and 3: 133 and 289 rounds
  above 64, none above 224; load 4, the case: 530 rounds, 358 above 64, 3
  above 224 (most 256), 171 with 1 to 64.

  idle (lanes and rounds with nothing to send): 129 hosts on the 129 vertices
  of geometric_graph(129, seed=3), load 1, 3 s: W = 1 116 581 ns, 1288
  rounds of three blocks (the third: host 128 and 63 lanes without one);
  1817 of the 3864 block-rounds have no send (1274 rounds have such a block),
  1626 no event at all, 96.6 % of the host-windows are idle and every host is
  idle in some window: those lanes take their next time from their timers and
  the bitmap in the hoisted close.

  lossy (drop test and ID fix-ups in the split resolve): the half-lossless
  graph of test_ps_tail_gpu.py from geometric_graph(129, seed=3,
  loss_max=0.05), 3 s: 12.3 % of the host pairs' paths have rel == 1.0
  exactly, the least is 0.7875; 38 464 sends, 2003 dropped (each drop moves
  the IDs of its host's later sends and timers of the batch), 3392
  block-rounds with 1 to 64 sends, 2 with more (the application's start).

  exits (every way out of the round loop): near64 run in five run_until steps
  whose stop times fall inside windows and inside a batch (a batch is up to
  1024 rounds; the whole run has 518), the state compared with the oracle's
  (OState.run_serial) after each; the same in a child process with
  SHD_PS_BATCH=4 (read once per process), where a batch ends every four
  rounds.  Every run here starts on a fresh path cache, so the first rounds
  halt on first touches (the three vertices' nine pairs).

  sparse: the lossy case forced onto k_round_sp (SHD_SP_HOSTS=64), which
  shares ps_loop_close and keeps the old order (flush, stores, close).
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
from test_ps_tail_gpu import half_lossless, path_rel, spread_hosts

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "shadow-1_amd")
POOL_ROOM = 288 - 64   # eng_device.h kPool - kBlock: a block with more sends deferred flushes inside the loop
STEPS = (2.5, 3.3333, 3.34, 7.0085)   # stop times of the `exits` case, s (then the end)


def make_case(name):
    """(graph, untraced model) of a case."""
    sec = S.SHD_SEC
    if name.startswith("near") or name.startswith("multi"):
        n, load = (int(name[4:]), 1) if name.startswith("near") else (64, int(name[5:]))
        return (W.geometric_graph(3, seed=121, integer_latency=True),
                W.phold_model(spread_hosts(n, 3), end_time=10 * sec, load=load, seed=2))
    if name == "idle":
        return W.geometric_graph(129, seed=3), W.phold_model(W.hosts_on_vertices(129, 1), end_time=3 * sec, load=1)
    if name == "lossy":
        return (half_lossless(W.geometric_graph(129, seed=3, loss_max=0.05)),
                W.phold_model(W.hosts_on_vertices(129, 1), end_time=3 * sec))
    raise KeyError(name)


_oracle = {}
_windows = {}


def oracle_of(name, g, m):
    """The oracle's run of a case, computed once (digest, stats)."""
    if name not in _oracle:
        _, dg, st = O.engine_run(m, g)
        dg.setflags(write=False)
        _oracle[name] = (dg, st)
    return _oracle[name]


def oracle_windows(name, g, m, window):
    """The oracle stepped through the engine's windows, once per case: per
    window and block of 64 hosts the deferred sends and the events, per window
    and host the events."""
    if name in _windows:
        return _windows[name]
    st = O.OState(m, g)
    end = int(m.params["end_time"])
    prev = st.digest().copy()
    sends, events = [], []
    while True:
        ws = st.next_time()
        if ws >= end:
            break
        st.run_serial(min(ws + window, end))
        d = st.digest().copy()
        sends.append((d["n_sent"] + d["n_inet_drop"]).astype(np.int64) - (prev["n_sent"] + prev["n_inet_drop"]).astype(np.int64))
        events.append(d["n_events"].astype(np.int64) - prev["n_events"].astype(np.int64))
        prev = d
    assert np.array_equal(prev, oracle_of(name, g, m)[0])   # the stepped oracle ends where engine_run does
    st.close()
    sends, events = np.array(sends), np.array(events)
    nb = -(-m.n_hosts // 64)
    per_block = lambda x: np.stack([x[:, 64 * b:64 * (b + 1)].sum(axis=1) for b in range(nb)], axis=1)
    for a in (sends, events):
        a.setflags(write=False)
    _windows[name] = (per_block(sends), per_block(events), events)
    return _windows[name]


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


@pytest.mark.parametrize("n", [64, 65])
def test_prefetch_ahead_of_the_resolve(n):
    name = f"near{n}"
    g, m = make_case(name)
    dg, st = run_gpu(g, m)
    check(name, g, m, dg, st)
    og = O.OGraph(g)
    lat = np.array([og.row(a, np.arange(3, dtype=np.int32))[0] for a in range(3)])
    for a in range(3):
        lat[a, a] = og.self_path(a)[0]
    lat = lat[np.ix_(m.host_vertex, m.host_vertex)] * 1e6   # per host pair, ns
    width = 1 << (int(st.window_ns).bit_length() - 1)   # the calendar's bin width
    sends, _, _ = oracle_windows(name, g, m, int(st.window_ns))
    print(f"{name}: window {st.window_ns} ns, bin {width} ns, {float((lat <= 2 * width).mean()):.3f} of the host pairs "
          f"within two bins; block-rounds with sends {int((sends > 0).sum())}, most sends {int(sends.max())}, "
          f"without {int((sends == 0).sum())}")
    assert st.window_ns == 17_000_000 and width == 1 << 24
    assert float((lat <= 2 * width).mean()) > 0.6 and lat.max() <= 2 * width + 0.3 * st.window_ns
    assert st.n_rounds >= len(sends) >= 500
    # every last flush is one batch: the split one
    assert sends.max() <= 64 and int((sends[:, 0] > 0).sum()) >= 500
    if n == 65:
        assert sends.shape[1] == 2 and int((sends[:, 1] > 0).sum()) > 100 and int((sends[:, 1] == 0).sum()) > 100


def test_more_than_one_batch_and_early_flushes():
    most = {}
    for load in (3, 4):
        name = f"multi{load}"
        g, m = make_case(name)
        if load == 4:
            dg, st = run_gpu(g, m)
            check(name, g, m, dg, st)
            assert st.window_ns == 17_000_000
        sends, _, _ = oracle_windows(name, g, m, 17_000_000)
        most[load] = sends
        print(f"{name}: rounds {len(sends)}, above 64 sends {int((sends > 64).sum())}, above {POOL_ROOM} "
              f"{int((sends > POOL_ROOM).sum())}, with 1 to 64 {int(((sends > 0) & (sends <= 64)).sum())}, most {int(sends.max())}")
    assert int((most[3] > POOL_ROOM).sum()) == 0   # the smallest load with an early flush is the next
    s = most[4]
    assert int((s > POOL_ROOM).sum()) >= 1 and int((s > 64).sum()) > 100 and int(((s > 0) & (s <= 64)).sum()) > 100


def test_idle_lanes_and_rounds_without_sends():
    g, m = make_case("idle")
    dg, st = run_gpu(g, m)
    check("idle", g, m, dg, st)
    sends, events, host_events = oracle_windows("idle", g, m, int(st.window_ns))
    print(f"idle: window {st.window_ns} ns, rounds {len(sends)}, block-rounds without a send {int((sends == 0).sum())} of "
          f"{sends.size} (rounds with one: {int((sends == 0).any(axis=1).sum())}), without an event {int((events == 0).sum())}, "
          f"idle host-windows {float((host_events == 0).mean()):.3f}, hosts idle in some window "
          f"{int((host_events == 0).any(axis=0).sum())}")
    assert st.n_rounds >= len(sends) and sends.shape[1] == 3
    assert int(((sends == 0) & (events > 0)).sum()) > 100   # blocks that ran events and sent nothing: no loads to hide under
    assert int((events == 0).sum()) > 100                  # blocks idle for a whole round
    assert int(((sends > 0) & (sends <= 64)).sum()) > 1000
    assert (host_events == 0).any(axis=0).all() and float((host_events == 0).mean()) > 0.9


_gpu = {}


def test_lossy_next_to_lossless():
    g, m = make_case("lossy")
    rel = path_rel(g, m.host_vertex)
    share = float((rel == 1.0).mean())
    print(f"lossy: {share:.3f} of the paths have rel == 1.0, least rel {rel.min():.4f}")
    assert 0.05 < share < 0.5 and rel.max() == 1.0 and rel.min() < 1.0
    _gpu["lossy"] = run_gpu(g, m)
    odg, _ = check("lossy", g, m, *_gpu["lossy"])
    sends, _, _ = oracle_windows("lossy", g, m, int(_gpu["lossy"][1].window_ns))
    assert int(odg["n_inet_drop"].sum()) > 1000
    assert int(((sends > 1) & (sends <= 64)).sum()) > 1000


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


def stop_times(m):
    return [int(t * S.SHD_SEC) for t in STEPS] + [int(m.params["end_time"])]


def oracle_steps(g, m):
    """The oracle's state after each stop time."""
    st = O.OState(m, g)
    out = []
    for t in stop_times(m):
        st.run_serial(t)
        out.append((st.digest().copy(), st.counts()))
    st.close()
    return out


def gpu_steps(g, m):
    """The engine run to each stop time in turn: (digest, events so far, packet events so far, stats)."""
    pc = PathCache(g, W.attached_vertices(m.host_vertex))
    eng = Engine(m, pc)
    eng.boot()
    out, nev, npkt = [], 0, 0
    for t in stop_times(m):
        st = eng.run_until(t)
        assert st.error == 0
        nev += st.n_events
        npkt += st.n_pkt_events
        out.append((eng.digest().copy(), nev, npkt, (st.n_rounds, st.n_batches, st.n_batches_persistent)))
    eng.close()
    pc.close()
    return out


def check_steps(tag, g, m, got):
    want = oracle_steps(g, m)
    for k, ((dg, nev, npkt, (rounds, batches, persistent)), (odg, (onev, onpkt))) in enumerate(zip(got, want)):
        print(f"{tag}: step {k} to {stop_times(m)[k]} ns: rounds {rounds} batches {batches} persistent {persistent} "
              f"events {nev}/{onev} packet events {npkt}/{onpkt}")
        assert (nev, npkt) == (onev, onpkt)
        assert np.array_equal(dg, odg)
        assert persistent > 0
    assert np.array_equal(got[-1][0], oracle_of("near64", g, m)[0])
    return [x[3] for x in got]


def test_exits_run_in_steps():
    g, m = make_case("near64")
    W17 = 17_000_000
    assert all(t % W17 for t in stop_times(m)[:-1])
    check_steps("steps", g, m, gpu_steps(g, m))


CHILD = r"""
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import test_ps_close_gpu as T
g, m = T.make_case("near64")
got = T.gpu_steps(g, m)
np.save(sys.argv[3], np.stack([x[0] for x in got]))
print(json.dumps([[int(x[1]), int(x[2]), [int(v) for v in x[3]]] for x in got]))
"""


def test_exits_short_batches(tmp_path):
    """SHD_PS_BATCH is read once per process: the run is a child's."""
    g, m = make_case("near64")
    env = dict(os.environ, SHD_PS_BATCH="4")
    out = tmp_path / "digests.npy"
    p = subprocess.run([sys.executable, "-c", CHILD, PKG, HERE, str(out)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = json.loads(p.stdout.strip().splitlines()[-1])
    dgs = np.load(out)
    got = [(dgs[k], r[0], r[1], tuple(r[2])) for k, r in enumerate(rows)]
    stats = check_steps("batch4", g, m, got)
    # a persistent batch every four rounds at the most (the others: up to 64 launched rounds)
    assert all(persistent * 4 + (batches - persistent) * 64 >= rounds for rounds, batches, persistent in stats)
    assert sum(persistent for _, _, persistent in stats) > 100
