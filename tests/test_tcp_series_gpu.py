"""The flow time series of the TCP path on the GPU (shd_tcp_model.options &
SHD_TCP_OPT_SERIES, shd_tcp_result_series; csrc/tcp.hip) against the
reference's own loop: on every case and interval of
tests/golden/ref_tcp_series.json the samples of an untraced and of a traced
run, with the path cache on the device and on tables, hold the fixture's rows
(tests/tcp_series_expect.py derives them from the reference's [STATUS] lines);
the five snapshot fields are required here not to depend on the run's mode;
their values are pinned by tests/test_tcp_snapshots_gpu.py (the oracle's change
log, which holds the reference's tcp_getInfo values from a socket's creation
until its process closes it; after the close, oracle-to-device only).  Models without a fixture are
compared with the rows derived from the oracle's lines (oracle/o_tcp.c, pinned
to the reference on the CPU)."""
import collections
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import oracle_ffi as O
import shdgpu as S
import tcp as TCPGPU
import tcp_cases as TC
import tcp_flow_expect as FE
import tcp_hub_cases as TH
import tcp_series_expect as SE
import workloads as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "ref_tcp_series.json")))
FLOWS = json.load(open(os.path.join(HERE, "golden", "ref_tcp_flows.json")))
SEC = S.SHD_SEC
RUNS = [(False, "device"), (False, "tables"), (True, "device"), (True, "tables")]   # (trace, mode)
CASES = [(n, int(us)) for n, f in FIX.items() for us in f["series"]]


def build(name):
    return TC.build(name) if name in TC.CASES else TH.build(name)


def rows(name, us):
    return FIX[name]["series"][str(us)]["rows"]


@functools.lru_cache(maxsize=None)
def _run(name, us, trace, mode):
    """one run of a fixture case with the series (computed once, never changed)"""
    c, m = build(name)
    return TCPGPU.run(m, c["graph"], TC.ip_ints(FIX[name]["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                      qdisc=c.get("qdisc", 0), udp=TC.udp_arg(c), mode=mode, trace=trace, series_us=us)


@pytest.mark.parametrize("trace,mode", RUNS)
@pytest.mark.parametrize("name,us", CASES)
def test_samples_equal_the_reference(name, us, trace, mode):
    r = _run(name, us, trace, mode)
    s = r["series"]
    assert s.dtype == S.TCP_SAMPLE_DTYPE
    SE.check(s, rows(name, us), (name, us, trace, mode))
    FE.check(r["flows"], FLOWS[name]["flows"], (name, us, trace, mode))   # series_us implies flows
    assert (s["host"] == r["flows"]["host"][s["flow"]]).all()
    assert not s["_pad"].any()
    assert r["series_info"]["drains"] >= 1 and 0 < r["series_info"]["peak"] <= r["series_info"]["capacity"]
    assert (len(r["lines"]) > 0) == trace
    if trace:   # and the run's own lines derive its own samples
        SE.check(s, SE.derive(r["lines"], us * 1000, FIX[name]["end_ns"]), (name, us, "own lines"))


@pytest.mark.parametrize("name,us", CASES)
def test_snapshot_fields_do_not_depend_on_the_mode(name, us):
    a = _run(name, us, *RUNS[0])["series"]
    assert (a["state"] <= 10).all() and (a["cwnd"] >= 1).all()   # (the values: tests/test_tcp_snapshots_gpu.py)
    for trace, mode in RUNS[1:]:
        b = _run(name, us, trace, mode)["series"]
        for k in SE.SNAPSHOT:
            assert a[k].tolist() == b[k].tolist(), (name, trace, mode, k)
        assert a.tobytes() == b.tobytes(), (name, trace, mode)


@pytest.mark.parametrize("name,us", [("lossy_2pct", 1000), ("hub12_fifo", 250000)])
def test_series_on_changes_nothing_else(name, us):
    c, m = build(name)
    on = _run(name, us, False, "device")
    off = TCPGPU.run(m, c["graph"], TC.ip_ints(FIX[name]["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                     qdisc=c.get("qdisc", 0), mode="device", trace=False, flows=True)
    assert "series" not in off
    for k in ("events", "rounds", "deliveries"):
        assert on[k] == off[k], k
    for k in ("next_event_id", "next_packet_id", "rng_probe"):
        assert on[k].tolist() == off[k].tolist(), k
    assert on["flows"].tobytes() == off["flows"].tobytes()


def _raw(name, **kw):
    """one shd_tcp_run of a fixture case on its first-guess tables: (rc, error, samples, info)"""
    c, m = build(name)
    lat, rel, hvi, _ = TCPGPU.path_table(m, c["graph"], c["procs"], c["peers"])
    tm, keep = TCPGPU.fill_model(m, TC.ip_ints(FIX[name]["ips"]), c["procs"], c["peers"], lat, rel, hvi, c["nbytes"],
                                 **kw)
    res = C.POINTER(S.TcpResult)()
    rc = S.lib().shd_tcp_run(C.byref(tm), 0, C.byref(res))
    del keep
    if rc:
        return rc, None, None, None
    try:
        recs, n = C.POINTER(S.TcpSample)(), C.c_uint64(99)
        assert S.lib().shd_tcp_result_series(res, C.byref(recs), C.byref(n), None) == 0
        s, info = S.tcp_result_series(res)
        assert (n.value, bool(recs)) == (len(s), len(s) > 0)
        return rc, int(res.contents.error), s, info
    finally:
        S.lib().shd_tcp_result_free(res)


def test_a_model_without_the_option_has_no_samples():
    """the accessor on a run that did not set SHD_TCP_OPT_SERIES: NULL and 0"""
    rc, err, s, info = _raw("lossy_2pct", flows=True)
    assert (rc, err, len(s)) == (0, 0, 0) and info == dict(drains=0, peak=0, capacity=0)
    rc, err, s, info = _raw("lossy_2pct", flows=True, series_us=250000)
    assert (rc, err) == (0, 0)
    SE.check(s, rows("lossy_2pct", 250000), "raw")


def test_two_blocks_appending_at_once():
    """bench.py --workload tcp's model at 96 hosts with loss at 100 ms,
    untraced: two blocks' lanes append to the one array concurrently"""
    g, m, ips, procs, peers, nb = W.tcp_echo_model(96, 40, end_s=12, nbytes=60000, loss_max=0.02)
    r = TCPGPU.run(m, g, ips, procs, peers, nbytes=nb, trace=False, series_us=100000)
    o = O.tcp_run(m, g, ips, procs, peers, nbytes=nb)
    want = SE.derive(o["lines"], 100 * S.SHD_MS, 12 * SEC)
    assert len(r["flows"]) == 96 and r["lines"] == [] and len(want) > 96
    SE.check(r["series"], want, "echo96")
    assert len(set(r["series"]["host"].tolist())) == 96
    assert r["series"]["retransmitted"].max() > 0


def test_several_records_of_one_host_at_one_boundary():
    """hub12_fifo's hub serves twelve clients: one boundary samples several of
    its records (the rows themselves are the parity test's)"""
    s = _run("hub12_fifo", 250000, False, "device")["series"]
    per = collections.Counter(zip(s["host"].tolist(), s["t"].tolist()))
    assert max(per.values()) >= 2
    assert len(set(zip(s["flow"].tolist(), s["t"].tolist()))) == len(s)   # one sample per record and boundary


def test_drains_and_a_full_array():
    """lossy_2pct at 1 ms: the array is emptied after every batch of rounds, so
    a capacity of the fullest drain carries the whole run; one record less and
    the append that finds it full sets SHD_TCP_ERR_SERIES -- rc 0, no fault"""
    rc, err, s, info = _raw("lossy_2pct", flows=True, series_us=1000)
    assert (rc, err) == (0, 0)
    SE.check(s, rows("lossy_2pct", 1000), "default capacity")
    assert info["capacity"] == 1 << 20 and info["drains"] > 1 and 0 < info["peak"] < len(s)
    peak = info["peak"]
    rc, err, s2, info2 = _raw("lossy_2pct", flows=True, series_us=1000, series_cap=peak)
    assert (rc, err) == (0, 0)
    assert s2.tobytes() == s.tobytes()
    assert info2 == dict(drains=info["drains"], peak=peak, capacity=peak)
    rc, err, s3, info3 = _raw("lossy_2pct", flows=True, series_us=1000, series_cap=peak - 1)
    assert rc == 0 and err & S.TCP_ERR_SERIES and not err & ~S.TCP_ERR_SERIES
    assert info3["capacity"] == peak - 1 and info3["peak"] <= peak - 1 and len(s3) < len(s)


def test_series_starts_again_with_a_first_touch_rerun():
    """test_tcp_flows_gpu.py's model whose first touches contradict the lanes'
    choice, so that shd_tcp_run runs it again from the start: the samples are
    the last run's alone"""
    g, m, ips, _, _, nb = W.tcp_echo_model(2, 30, end_s=6, nbytes=30000)
    assert m.host_vertex[0] != m.host_vertex[1]
    procs = [(0, SEC), (1, SEC), (0, 2 * SEC + 10000), (1, 2 * SEC)]
    peers = [-1, -1, 1, 0]
    r = TCPGPU.run(m, g, ips, procs, peers, nbytes=nb, trace=False, series_us=250000)
    assert r["first_touch"] == "device" and r["first_touch_reruns"] >= 1
    o = O.tcp_run(m, g, ips, procs, peers, nbytes=nb)
    want = SE.derive(o["lines"], 250 * S.SHD_MS, 6 * SEC)
    assert len(r["flows"]) == 4 and len(want) >= 4
    SE.check(r["series"], want, "rerun")


def _bulk_pair(end_ns, us):
    g = S.GraphArrays(1, [0], [0], [50.0], [0.0])
    m = W.phold_model(np.asarray([0, 0], dtype=np.int32), end_time=end_ns, trace=True,
                      queue_flags=S.SHD_QF_TRACE_STATUS, load=0, payload=1)
    ips = TC.ip_ints(json.load(open(os.path.join(HERE, "golden", "ref_tcp.json")))["bulk_2mb"]["ips"])
    procs, peers, N = [(0, SEC), (1, 2 * SEC)], [-1, 0], 2000000
    r = TCPGPU.run(m, g, ips, procs, peers, nbytes=N, trace=False, series_us=us)
    o = O.tcp_run(m, g, ips, procs, peers, nbytes=N)
    return r, o


def test_a_run_cut_short():
    """tcp_cases' bulk_2mb pair (50 ms each way, 2 MB) ended at 2.5 s with the
    transfer running: no sample at or past the end -- the last touches belong
    to the boundary 2.5 s, which the flow records stand for"""
    end = 2 * SEC + 500 * S.SHD_MS
    r, o = _bulk_pair(end, 250000)
    want = SE.derive(o["lines"], 250 * S.SHD_MS, end)
    SE.check(r["series"], want, "cut short")
    s, f = r["series"], r["flows"]
    assert len(s) > 0 and s["t"].max() == 2 * SEC + 250 * S.SHD_MS < end
    last = {int(x["flow"]): int(x["bytes_delivered"]) for x in s}
    assert any(int(f["bytes_delivered"][i]) > v for i, v in last.items())   # the run went on after the last sample
    p = S.flow_progress(s, f, 250 * S.SHD_MS, end)
    assert p.shape == (2, 10) and p[:, -1].tolist() == f["bytes_delivered"].tolist()


def test_an_interval_longer_than_the_run():
    end = 2 * SEC + 500 * S.SHD_MS
    r, _ = _bulk_pair(end, 3000000)
    assert len(r["series"]) == 0 and len(r["flows"]) == 2
    assert r["series_info"]["drains"] == 0 and r["series_info"]["peak"] == 0


def run_ranks(world, case, us, mode, tmp_path, timeout=240):
    """`world` ranks of tests/tcp_series_group_worker.py on one GPU (at most 3)"""
    assert world <= 3
    name = "shdtcp_" + uuid.uuid4().hex[:16]
    procs = [subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "tcp_series_group_worker.py"), "--rank", str(r),
                               "--world", str(world), "--name", name, "--out", str(tmp_path), "--case", case,
                               "--us", str(us), "--mode", mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(world)]
    outs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=timeout)
            outs.append(out.decode(errors="replace"))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} exited {p.returncode}:\n{outs[r][-3000:]}"
    return [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(world)]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("mode", ["tables", "device"])
@pytest.mark.parametrize("name", ["geo_pairs", "hub12_fifo"])
def test_group_samples_merge_to_the_fixture(name, mode, world, tmp_path):
    """shd_tcp_run_group over the host-memory communicator: each rank holds its
    own hosts' samples against its own flow array, and the ranks merged are
    the one-engine arrays"""
    us = 250000
    res = run_ranks(world, name, us, mode, tmp_path)
    for x in res:
        h0, nl = int(x["first_host"]), int(x["n_local_hosts"])
        s = x["series"]
        assert ((s["host"] >= h0) & (s["host"] < h0 + nl)).all()
        assert (s["flow"] < len(x["flows"])).all()
    flows, series = S.merge_tcp_series([(x["flows"], x["series"]) for x in res])
    SE.check(series, rows(name, us), (name, mode, world))
    assert sum(len(x["series"]) > 0 for x in res) >= 2   # the samples are spread over the ranks
    one = _run(name, us, False, mode)
    assert flows.tobytes() == one["flows"].tobytes()
    assert series.tobytes() == one["series"].tobytes()   # the snapshot fields too
