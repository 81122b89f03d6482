"""The two ends of the persistent round's event loop in the lean k_round_ps:
the loop leaves in the iteration that ran its last event (ps_loop_close's
EXIT: the candidate time carried to steady_iter, the end test `t >= we` at the
iteration's bottom), and the fast round takes its due count and head from the
staging (pf_stage's PfDue, ps_prologue_pf), at small sizes against the serial
oracle.

In the manner of test_ps_iter_gpu.py, whose helpers and those of
test_ps_close_gpu.py this file imports: every case runs untraced (the lean
kernels), compares every host's end state (Engine.digest()) and the event
counts with the oracle, and must have run persistent launches.  What each case
is for was counted on the CPU with the oracle alone -- windows() below steps
oracle_ffi.OState through the windows [next time, min(next time + W, end)),
arrivals() of test_ps_iter_gpu.py is the traced oracle run -- and every test
recomputes its counts and asserts a bound on them, so that a case cannot pass
without holding what it is here for.  W = 17 ms in the near and tie cases.

  a window's end (the end test is `t >= we`: an arrival at `we` is the next
  round's, one at we - 1 runs and leaves its notification pending at `we`),
  arrivals at a window's end / 1 ns before one: near64 518 windows, 50 / 26;
  near65 519, 55 / 22; tie64 527, 91 / 28.

  a window that starts later than the previous one ended (the staging's
  count stops at L = previous end + W, clipped to the stop; the prologue goes
  on from there), windows starting after / exactly at the previous end, and
  arrivals in [previous end + W, start + W) inside their window: near64 345 /
  172, 160; near65 323 / 195, 185; tie64 261 / 265, 122.

  the loop leaves after 1, 2, 3, ... events: windows with 0 / 1 / 2 / 3 / 4 /
  5 packet events at the busiest host, near64: 2 / 60 / 277 / 138 / 34 / 7;
  tie64 goes up to 8.

  a lane whose last event leaves work (state 1 or 2, not 0): multi4 (a flush
  inside the loop), down and up (backlog, run_work), near64's loopbacks (a
  heap event as the remaining candidate), with the assertions
  test_ps_iter_gpu.py and test_ps_close_gpu.py make about them.

  a wave with no active lane (it does not enter the loop) and lanes without
  a host: the 129-host idle case, whose third block (one host) has no event
  in more than 100 windows.

  the stop inside a window (L clipped by the stop; the notification across
  it): near64 run in steps to the stop times of test_ps_iter_gpu.py's
  stops(), and the same in a child process with SHD_PS_BATCH=4.

  the routes that must not change: the lossy case forced onto k_round_sp
  (SHD_SP_HOSTS=64), and near65, where a delivery into the other block's
  staged bins names the host in the share: the non-fast prologue right after
  a fast one.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_ffi as O
import test_ps_close_gpu as T
import test_ps_iter_gpu as I

pytestmark = pytest.mark.gpu

W17 = 17_000_000
_windows = {}


def windows(name, window):
    """The oracle stepped through the windows, once per case: each window's
    (start, end) and per window and host the packet events and the events."""
    if name in _windows:
        return _windows[name]
    g, m = I.make_case(name)
    st = O.OState(m, g)
    end = int(m.params["end_time"])
    prev = st.digest().copy()
    bounds, pkt, ev = [], [], []
    while True:
        ws = st.next_time()
        if ws >= end:
            break
        we = min(ws + window, end)
        st.run_serial(we)
        d = st.digest().copy()
        bounds.append((ws, we))
        pkt.append(d["n_pkt_events"].astype(np.int64) - prev["n_pkt_events"].astype(np.int64))
        ev.append(d["n_events"].astype(np.int64) - prev["n_events"].astype(np.int64))
        prev = d
    assert np.array_equal(prev, T.oracle_of(name, g, m)[0])   # the stepped oracle ends where engine_run does
    st.close()
    out = (np.array(bounds, dtype=np.int64), np.array(pkt), np.array(ev))
    for a in out:
        a.setflags(write=False)
    _windows[name] = out
    return out


def end_counts(name, window):
    """(windows, arrivals at a window's end, arrivals 1 ns before one)"""
    bounds, _, _ = windows(name, window)
    t = I.arrivals(name)["time"].astype(np.int64)
    return len(bounds), int(np.isin(t, bounds[:, 1]).sum()), int(np.isin(t, bounds[:, 1] - 1).sum())


def gap_counts(name, window):
    """(windows that start after the previous end, exactly at it, arrivals in
    [previous end + W, start + W) inside their window): what the staging's
    count, which stops at L = min(previous end + W, stop), leaves to the
    prologue's continued scan"""
    bounds, _, _ = windows(name, window)
    stop = int(bounds[-1, 1])
    t = np.sort(I.arrivals(name)["time"].astype(np.int64))
    later = int((bounds[1:, 0] > bounds[:-1, 1]).sum())
    same = int((bounds[1:, 0] == bounds[:-1, 1]).sum())
    past = 0
    for (_, pwe), (ws, we) in zip(bounds[:-1], bounds[1:]):
        lim = min(int(pwe) + window, stop)
        past += int(np.searchsorted(t, we) - np.searchsorted(t, max(lim, int(ws)))) if lim < we else 0
    return later, same, past


@pytest.mark.parametrize("name", ["near64", "near65", "tie64"])
def test_window_ends_and_late_starts(name):
    _, _, st, _, _ = I.run_case(name)
    assert st.window_ns == W17
    n, at_end, before = end_counts(name, W17)
    later, same, past = gap_counts(name, W17)
    print(f"{name}: {n} windows, arrivals at a window's end {at_end}, 1 ns before one {before}; windows starting after "
          f"the previous end {later}, exactly at it {same}, arrivals past the staging's bound inside their window {past}")
    assert at_end >= 20 and before >= 10
    assert later >= 100 and past >= 50


@pytest.mark.parametrize("name", ["near64", "tie64"])
def test_loop_leaves_after_one_to_many_events(name):
    _, _, st, _, _ = I.run_case(name)
    _, pkt, _ = windows(name, int(st.window_ns))
    hist = np.bincount(pkt.max(axis=1))
    print(f"{name}: windows by the busiest host's packet events: {hist.tolist()}")
    assert int((hist >= 5).sum()) >= 4
    if name == "tie64":
        assert len(hist) - 1 >= 8


def test_last_event_leaves_a_flush_inside_the_loop():
    g, m, st, cls, _ = I.run_case("multi4")
    sends, _, _ = T.oracle_windows("multi4", g, m, int(st.window_ns))
    print(f"multi4: rounds above 64 sends {int((sends > 64).sum())}, above {T.POOL_ROOM} {int((sends > T.POOL_ROOM).sum())}")
    assert int((sends > T.POOL_ROOM).sum()) >= 1 and int((sends > 64).sum()) > 100
    assert I.counts(cls)[0] > 10000


@pytest.mark.parametrize("name", ["down", "up"])
def test_last_event_leaves_backlog(name):
    _, _, _, cls, extra = I.run_case(name)
    steady, backlog, _, _ = I.counts(cls)
    assert steady > 1000 and backlog > 1000 and I.side_by_side(cls, 1, 2) > 100
    if name == "down":
        assert extra[0] > 0 and extra[1] > 100 and extra[2] > 100   # CoDel drops, router queues, rx_rem < MTU
    else:
        assert extra[3] > 1000                                      # tx_rem < MTU: sends that wait in the send queue


def test_heap_event_as_the_remaining_candidate():
    _, m, _, cls, extra = I.run_case("near64")
    assert m.n_hosts == 64
    assert extra[4] > 50            # host-windows with a loopback: its delivery is a heap event
    assert I.side_by_side(cls, 1, 3) > 100


def test_wave_without_an_active_lane():
    g, m, st, cls, _ = I.run_case("idle")
    _, events, _ = T.oracle_windows("idle", g, m, int(st.window_ns))
    none = int((events[:, 2] == 0).sum())
    print(f"idle: {len(events)} windows, the third block (host 128 alone) without an event in {none}")
    assert cls.shape[1] == 129 and events.shape[1] == 3
    assert none > 100


def test_stop_inside_a_window():
    g, m = I.make_case("near64")
    times = I.stops(g, m)
    assert all(t % W17 for t in times[:-1])   # inside windows
    I.check_steps("steps", g, m, times, I.gpu_steps(g, m, times))


def test_stop_inside_a_window_short_batches(tmp_path):
    """SHD_PS_BATCH is read once per process: the run is a child's."""
    g, m = I.make_case("near64")
    times = I.stops(g, m)
    out = tmp_path / "digests.npy"
    p = subprocess.run([sys.executable, "-c", I.CHILD, I.PKG, I.HERE, str(out), json.dumps(times)],
                       env=dict(os.environ, SHD_PS_BATCH="4"), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = json.loads(p.stdout.strip().splitlines()[-1])
    dgs = np.load(out)
    got = [(dgs[k], r[0], r[1], tuple(r[2])) for k, r in enumerate(rows)]
    I.check_steps("batch4", g, m, times, got)
    assert sum(x[3][2] for x in got) > 100


def test_sparse_kernel_keeps_its_loop(monkeypatch):
    g, m = I.make_case("lossy")
    pdg, pst = I.gpu_of("lossy", g, m)
    T.check("lossy", g, m, pdg, pst)
    assert pst.n_batches_sparse == 0
    monkeypatch.setenv("SHD_SP_HOSTS", "64")
    dg, st = T.run_gpu(g, m)
    T.check("lossy", g, m, dg, st)
    assert st.n_batches_sparse > 0 and st.n_rounds == pst.n_rounds


def test_named_host_reads_its_window_again():
    """near65: host 64 alone in the second block; every delivery between the
    blocks into bins staged ahead names the receiver in the share, and its
    block's next round takes the non-fast prologue behind fast ones."""
    g, m, st, _, _ = I.run_case("near65")
    sends, _, _ = T.oracle_windows("near65", g, m, int(st.window_ns))
    assert st.window_ns == W17 and st.n_rounds >= len(sends) >= 500
    assert sends.shape[1] == 2 and sends.max() <= 64
    assert int((sends[:, 1] > 0).sum()) > 100 and int((sends[:, 1] == 0).sum()) > 100
