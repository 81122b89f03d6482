"""The five snapshot fields of shd_tcp_flow and shd_tcp_sample -- state, cwnd,
ssthresh, srtt, rttvar (csrc/tcp.hip: k_tcp_flow_write, series_take) -- against
the oracle's change log (oracle/o_tcp.c, o_tcp_out.log;
tests/tcp_snapshot_expect.py), which tests/test_tcp_snapshots_ref_cpu.py pins
to the reference's own tcp_getInfo values wherever a process can observe them.

A flow record holds its socket's values when the run ends: the log's last row
of that socket.  A sample labelled t holds them as they stood before the
host's first event at or past t: the log's last row of an event strictly
before t.  Every record and every sample is looked up by its addresses and
must be found: none is skipped.

Only the untraced run on the device's path cache is checked here; the traced,
tables and group variants are required byte-equal to it by
test_tcp_flows_gpu.py and test_tcp_series_gpu.py
(test_snapshot_fields_do_not_depend_on_the_mode,
test_group_records_concatenate_to_the_fixture,
test_group_samples_merge_to_the_fixture)."""
import functools
import json
import os

import numpy as np
import pytest

import oracle_ffi as O
import shdgpu as S
import tcp as TCPGPU
import tcp_cases as TC
import tcp_hub_cases as TH
import tcp_snapshot_expect as XE
import workloads as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FLOWS = json.load(open(os.path.join(HERE, "golden", "ref_tcp_flows.json")))
SERIES = json.load(open(os.path.join(HERE, "golden", "ref_tcp_series.json")))
SNAP = json.load(open(os.path.join(HERE, "golden", "ref_tcp_snapshots.json")))
SEC, MS = S.SHD_SEC, S.SHD_MS
# every case of the flow records' fixture and the snapshot fixture's own
FLOW_CASES = list(FLOWS) + [n for n in SNAP if n not in FLOWS]
SERIES_CASES = [(n, int(us)) for n, f in SERIES.items() for us in f["series"]] + [("hub3_slow", 100000), ("rto_reset", 100000)]
ST = {n: i for i, n in enumerate(S.TCP_STATE_NAMES)}


def build(name):
    return TH.build(name) if name in TH.CASES else TC.build(name)


def ips_of(name):
    return TC.ip_ints((FLOWS.get(name) or SNAP[name])["ips"])


@functools.lru_cache(maxsize=None)
def _log(name):
    """the oracle's change log of a case (computed once, never changed)"""
    c, m = build(name)
    o = O.tcp_run(m, c["graph"], ips_of(name), c["procs"], c["peers"], nbytes=c["nbytes"], qdisc=c.get("qdisc", 0),
                  udp=TC.udp_arg(c), lines=False, snapshots=True)
    return XE.Log(o["log"])


@functools.lru_cache(maxsize=None)
def _run(name, us=0):
    """one untraced run of a case on the device's path cache, with flow records (us = 0) or the series"""
    c, m = build(name)
    kw = dict(series_us=us) if us else dict(flows=True)
    return TCPGPU.run(m, c["graph"], ips_of(name), c["procs"], c["peers"], nbytes=c["nbytes"],
                      qdisc=c.get("qdisc", 0), udp=TC.udp_arg(c), mode="device", trace=False, **kw)


@pytest.mark.parametrize("name", FLOW_CASES)
def test_flow_records_hold_the_end_values(name):
    c, _ = build(name)
    f = _run(name)["flows"]
    assert len(f) == 2 * sum(1 for p in c["peers"] if p >= 0)
    XE.check_flows(f, _log(name), name)


@pytest.mark.parametrize("name,us", SERIES_CASES)
def test_samples_hold_the_values_before_their_boundary(name, us):
    r = _run(name, us)
    assert len(r["series"]) > 0
    XE.check_samples(r["series"], r["flows"], _log(name), (name, us))
    XE.check_flows(r["flows"], _log(name), (name, us))


def test_the_fixture_runs_move_every_field():
    """what the device is held to is not constant: over the cases' samples
    each of the five takes several values, and the states after a close (which
    only the oracle's log pins) are among the records' end states"""
    seen = {k: set() for k in XE.FIVE}
    for name, us in SERIES_CASES:
        for k in XE.FIVE:
            seen[k] |= set(_run(name, us)["series"][k].tolist())
    assert all(len(seen[k]) >= 5 for k in XE.FIVE), {k: len(v) for k, v in seen.items()}
    assert {ST["SYNSENT"], ST["SYNRECEIVED"], ST["ESTABLISHED"], ST["FINWAIT1"], ST["CLOSEWAIT"]} <= seen["state"]
    assert 0 in seen["srtt"] and min(seen["ssthresh"]) < XE.SSTHRESH_INIT in seen["ssthresh"]
    end = set()
    for name in FLOW_CASES:
        end |= set(_run(name)["flows"]["state"].tolist())
    assert {ST["CLOSED"], ST["TIMEWAIT"]} <= end


def test_a_sample_is_taken_before_the_crossing_event():
    """lossy_2pct at 1 ms: samples between almost every pair of events.  For
    many samples the interval's own events change the socket, so a sample that
    read its socket after the event that crosses the boundary, or a log read
    one event late, would not pass the comparison above"""
    us = 1000
    r, L = _run("lossy_2pct", us), _log("lossy_2pct")
    s, f = r["series"], r["flows"]
    assert r["series_info"]["drains"] > 1
    differ = at_once = 0
    for x in s:
        fl = f[int(x["flow"])]
        k = L.sock(fl["host"], fl["local_port"], fl["peer_ip"], fl["peer_port"])
        t = int(x["t"])
        differ += L.before(k, t) != L.up_to(k, t + us * 1000)
        at_once += L.before(k, t) != L.up_to(k, t)   # an event at the boundary itself opens the next interval
    assert differ >= 1 and at_once >= 1, (differ, at_once, len(s))
    print("lossy_2pct 1 ms: %d samples, %d change within the next interval, %d at the boundary's own instant"
          % (len(s), differ, at_once))


def test_hub_children_in_neighbouring_slots_differ():
    """hub12_fifo's hub holds its twelve children in neighbouring socket slots:
    their end values are not all the same, so a record written from the slot
    beside its own fails test_flow_records_hold_the_end_values"""
    f, L = _run("hub12_fifo")["flows"], _log("hub12_fifo")
    hub = f[(f["host"] == 0) & (f["role"] == 1)]
    assert len(hub) == 12
    want = [L.at_end(L.sock(r["host"], r["local_port"], r["peer_ip"], r["peer_port"])) for r in hub]
    assert len(set(want)) > 1, want
    assert any(a != b for a, b in zip(want, want[1:]))   # and next to each other in the records' order
    assert [XE.flow_five(r) for r in hub] == want


def _oracle_log(m, g, ips, procs, peers, nb):
    return XE.Log(O.tcp_run(m, g, ips, procs, peers, nbytes=nb, lines=False, snapshots=True)["log"])


def test_two_blocks_against_the_oracle_log():
    """bench.py --workload tcp's model at 96 hosts with loss at 100 ms (two
    blocks; test_tcp_series_gpu.py::test_two_blocks_appending_at_once's model)"""
    g, m, ips, procs, peers, nb = W.tcp_echo_model(96, 40, end_s=12, nbytes=60000, loss_max=0.02)
    r = TCPGPU.run(m, g, ips, procs, peers, nbytes=nb, trace=False, series_us=100000)
    L = _oracle_log(m, g, [int(x) for x in ips], procs, peers, nb)
    assert len(r["flows"]) == 96 and len(r["series"]) > 96
    XE.check_flows(r["flows"], L, "echo96")
    XE.check_samples(r["series"], r["flows"], L, "echo96")
    assert len(set(r["series"]["cwnd"].tolist())) > 10 and r["series"]["ssthresh"].min() < XE.SSTHRESH_INIT


def test_a_run_cut_short_holds_open_sockets():
    """tcp_cases' bulk_2mb pair ended at 2.5 s with the transfer running: both
    sockets ESTABLISHED with an open window when the run ends, the last samples
    one boundary earlier"""
    end = 2 * SEC + 500 * MS
    g = S.GraphArrays(1, [0], [0], [50.0], [0.0])
    m = W.phold_model(np.asarray([0, 0], dtype=np.int32), end_time=end, trace=True,
                      queue_flags=S.SHD_QF_TRACE_STATUS, load=0, payload=1)
    ips = TC.ip_ints(json.load(open(os.path.join(HERE, "golden", "ref_tcp.json")))["bulk_2mb"]["ips"])
    procs, peers, N = [(0, SEC), (1, 2 * SEC)], [-1, 0], 2000000
    r = TCPGPU.run(m, g, ips, procs, peers, nbytes=N, trace=False, series_us=250000)
    L = _oracle_log(m, g, ips, procs, peers, N)
    f, s = r["flows"], r["series"]
    assert len(f) == 2 and len(s) > 0 and s["t"].max() == 2 * SEC + 250 * MS
    XE.check_flows(f, L, "cut short")
    XE.check_samples(s, f, L, "cut short")
    assert (f["state"] == ST["ESTABLISHED"]).all() and (f["srtt"] > 0).all()
    cl = f[f["role"] == 0][0]
    assert cl["cwnd"] > 1 and cl["ssthresh"] == XE.SSTHRESH_INIT   # slow start, no loss: the window still opening
    last = s[s["t"] == s["t"].max()]
    assert any(XE.flow_five(x) != XE.flow_five(f[int(x["flow"])]) for x in last)   # the run went on after them


def test_a_first_touch_rerun_holds_the_last_runs_values():
    """test_tcp_series_gpu.py::test_series_starts_again_with_a_first_touch_rerun's
    model: the records and samples are the last run's alone"""
    g, m, ips, _, _, nb = W.tcp_echo_model(2, 30, end_s=6, nbytes=30000)
    procs = [(0, SEC), (1, SEC), (0, 2 * SEC + 10000), (1, 2 * SEC)]
    peers = [-1, -1, 1, 0]
    r = TCPGPU.run(m, g, ips, procs, peers, nbytes=nb, trace=False, series_us=250000)
    assert r["first_touch"] == "device" and r["first_touch_reruns"] >= 1
    L = _oracle_log(m, g, [int(x) for x in ips], procs, peers, nb)
    assert len(r["flows"]) == 4 and len(r["series"]) >= 4
    XE.check_flows(r["flows"], L, "rerun")
    XE.check_samples(r["series"], r["flows"], L, "rerun")
