"""Flow records of the TCP path on the GPU (shd_tcp_model.options &
SHD_TCP_OPT_FLOWS, shd_tcp_result_flows; csrc/tcp.hip) against the reference's
own loop: on every case of tests/golden/ref_tcp_flows.json the records of an
untraced and of a traced run, with the path cache on the device and on tables,
hold the fixture's pinned fields (tests/tcp_flow_expect.py derives them from
the reference's [STATUS] lines); the five snapshot fields are required here not
to depend on the run's mode, and their values are pinned by
tests/test_tcp_snapshots_gpu.py (the oracle's change log, which holds the
reference's tcp_getInfo values from a socket's creation until its process
closes it; after the close, oracle-to-device only).
Models without a fixture are compared with the records derived from the
oracle's lines (oracle/o_tcp.c, pinned to the reference on the CPU)."""
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
import workloads as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "ref_tcp_flows.json")))
SEC = S.SHD_SEC
RUNS = [(False, "device"), (False, "tables"), (True, "device"), (True, "tables")]   # (trace, mode)


def build(name):
    return TC.build(name) if name in TC.CASES else TH.build(name)


@functools.lru_cache(maxsize=None)
def _run(name, trace, mode):
    """one run of a fixture case with flow records (computed once, never changed)"""
    c, m = build(name)
    return TCPGPU.run(m, c["graph"], TC.ip_ints(FIX[name]["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                      qdisc=c.get("qdisc", 0), udp=TC.udp_arg(c), mode=mode, trace=trace, flows=True)


def check_procs(flows, ips, procs, peers):
    """proc and role against the model: a connecting socket's process is a
    client on the record's host whose server sits at the peer address; a
    child's is a server on its host that some client at the peer address names"""
    for r in flows:
        k, h = int(r["proc"]), int(r["host"])
        assert 0 <= k < len(procs) and procs[k][0] == h, (k, h)
        assert int(r["local_ip"]) == ips[h]
        if r["role"] == 0:
            assert peers[k] >= 0 and ips[procs[peers[k]][0]] == int(r["peer_ip"]), (k, h)
        else:
            assert peers[k] == -1, (k, h)
            assert any(p == k and ips[procs[j][0]] == int(r["peer_ip"]) for j, p in enumerate(peers)), (k, h)


@pytest.mark.parametrize("trace,mode", RUNS)
@pytest.mark.parametrize("name", list(FIX))
def test_flow_records_equal_the_reference(name, trace, mode):
    c, _ = build(name)
    r = _run(name, trace, mode)
    assert r["flows"].dtype == S.TCP_FLOW_DTYPE
    FE.check(r["flows"], FIX[name]["flows"], (name, trace, mode))
    check_procs(r["flows"], TC.ip_ints(FIX[name]["ips"]), c["procs"], c["peers"])
    assert (len(r["lines"]) > 0) == trace
    if trace:   # and the run's own lines derive its own records
        FE.check(r["flows"], FE.rows(FE.derive(r["lines"])), (name, "own lines"))


@pytest.mark.parametrize("name", list(FIX))
def test_snapshot_fields_do_not_depend_on_the_mode(name):
    a = _run(name, *RUNS[0])["flows"]
    assert (a["state"] <= 10).all() and (a["cwnd"] >= 1).all()   # (the values: tests/test_tcp_snapshots_gpu.py)
    for trace, mode in RUNS[1:]:
        b = _run(name, trace, mode)["flows"]
        for k in FE.SNAPSHOT + ("proc",):
            assert a[k].tolist() == b[k].tolist(), (name, trace, mode, k)
        assert a.tobytes() == b.tobytes(), (name, trace, mode)


@pytest.mark.parametrize("name", ["lossy_2pct", "hub12_fifo"])
def test_flows_on_changes_nothing_else(name):
    c, m = build(name)
    on = _run(name, False, "device")
    off = TCPGPU.run(m, c["graph"], TC.ip_ints(FIX[name]["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                     qdisc=c.get("qdisc", 0), mode="device", trace=False)
    assert "flows" not in off
    for k in ("events", "rounds", "deliveries"):
        assert on[k] == off[k], k
    for k in ("next_event_id", "next_packet_id", "rng_probe"):
        assert on[k].tolist() == off[k].tolist(), k


def test_a_model_without_the_option_has_no_records():
    """the accessor on a run that did not set SHD_TCP_OPT_FLOWS: NULL and 0;
    with the option the same call hands out the records"""
    name = "lossy_2pct"
    c, m = build(name)
    ips = TC.ip_ints(FIX[name]["ips"])
    lat, rel, hvi, _ = TCPGPU.path_table(m, c["graph"], c["procs"], c["peers"])
    for flows in (False, True):
        tm, keep = TCPGPU.fill_model(m, ips, c["procs"], c["peers"], lat, rel, hvi, c["nbytes"], flows=flows)
        res = C.POINTER(S.TcpResult)()
        assert S.lib().shd_tcp_run(C.byref(tm), 0, C.byref(res)) == 0
        try:
            assert res.contents.error == 0
            recs, n = C.POINTER(S.TcpFlow)(), C.c_uint64(99)
            assert S.lib().shd_tcp_result_flows(res, C.byref(recs), C.byref(n)) == 0
            assert (n.value, bool(recs)) == ((2, True) if flows else (0, False))
            assert len(S.tcp_result_flows(res)) == n.value
        finally:
            S.lib().shd_tcp_result_free(res)


def test_records_start_again_with_a_first_touch_rerun():
    """test_tcp_gpu.py's model whose first touches contradict the lanes'
    choice, so that shd_tcp_run runs it again from the start: the records are
    the last run's alone"""
    g, m, ips, _, _, nb = W.tcp_echo_model(2, 30, end_s=6, nbytes=30000)
    assert m.host_vertex[0] != m.host_vertex[1]
    procs = [(0, SEC), (1, SEC), (0, 2 * SEC + 10000), (1, 2 * SEC)]
    peers = [-1, -1, 1, 0]
    r = TCPGPU.run(m, g, ips, procs, peers, nbytes=nb, trace=False, flows=True)
    assert r["first_touch"] == "device" and r["first_touch_reruns"] >= 1
    o = O.tcp_run(m, g, ips, procs, peers, nbytes=nb)
    want = FE.rows(FE.derive(o["lines"]))
    assert len(want) == 4
    FE.check(r["flows"], want, "rerun")
    check_procs(r["flows"], [int(x) for x in ips], procs, peers)


@pytest.mark.parametrize("end_ns,n", [(2 * SEC + 20 * S.SHD_MS, 1), (2 * SEC + 500 * S.SHD_MS, 2)])
def test_a_run_cut_short(end_ns, n):
    """tcp_cases' bulk_2mb pair (50 ms each way, 2 MB) ended 20 ms after the
    client starts -- its SYN is created and still under way -- and at 2.5 s,
    with the transfer running"""
    g = S.GraphArrays(1, [0], [0], [50.0], [0.0])
    m = W.phold_model(np.asarray([0, 0], dtype=np.int32), end_time=end_ns, trace=True,
                      queue_flags=S.SHD_QF_TRACE_STATUS, load=0, payload=1)
    ips = TC.ip_ints(json.load(open(os.path.join(HERE, "golden", "ref_tcp.json")))["bulk_2mb"]["ips"])
    procs, peers, N = [(0, SEC), (1, 2 * SEC)], [-1, 0], 2000000
    r = TCPGPU.run(m, g, ips, procs, peers, nbytes=N, trace=False, flows=True)
    o = O.tcp_run(m, g, ips, procs, peers, nbytes=N)
    want = FE.rows(FE.derive(o["lines"]))
    assert len(want) == n
    FE.check(r["flows"], want, end_ns)
    check_procs(r["flows"], ips, procs, peers)
    f = r["flows"]
    cl = f[f["role"] == 0][0]
    assert cl["host"] == 1 and cl["t_open"] == 2 * SEC and cl["t_fin"] == 0
    if n == 1:
        assert cl["t_established"] == 0 and cl["packets_created"] == 1 and cl["bytes_delivered"] == 0
        assert S.TCP_STATE_NAMES[cl["state"]] == "SYNSENT"
    else:
        assert cl["t_established"] >= 2 * SEC + 100 * S.SHD_MS   # the SYN and the SYN+ACK, 50 ms each
        ch = f[f["role"] == 1][0]   # the server reads everything before it echoes: only its side has delivered
        assert 0 < ch["bytes_delivered"] < N and cl["bytes_delivered"] == 0 and cl["bytes_created"] > 0
        assert S.TCP_STATE_NAMES[cl["state"]] == "ESTABLISHED"
        assert (f["t_fin"] == 0).all() and (f["t_established"] > 0).all()


def test_scaled_model_untraced_equals_oracle():
    """bench.py --workload tcp's model at 96 hosts with loss, untraced: 96
    records (48 connections), equal to the ones the oracle's lines derive"""
    g, m, ips, procs, peers, nb = W.tcp_echo_model(96, 40, end_s=12, nbytes=60000, loss_max=0.02)
    r = TCPGPU.run(m, g, ips, procs, peers, nbytes=nb, trace=False, flows=True)
    o = O.tcp_run(m, g, ips, procs, peers, nbytes=nb)
    want = FE.rows(FE.derive(o["lines"]))
    assert len(want) == 96 and r["lines"] == []
    FE.check(r["flows"], want, "echo96")
    check_procs(r["flows"], [int(x) for x in ips], procs, peers)
    assert r["flows"]["retransmitted"].sum() > 0 and r["flows"]["inet_dropped"].sum() > 0


def run_ranks(world, case, mode, tmp_path, timeout=240):
    """`world` ranks of tests/tcp_flows_group_worker.py on one GPU (at most 3)"""
    assert world <= 3
    name = "shdtcp_" + uuid.uuid4().hex[:16]
    procs = [subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "tcp_flows_group_worker.py"), "--rank", str(r),
                               "--world", str(world), "--name", name, "--out", str(tmp_path), "--case", case,
                               "--mode", mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
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
def test_group_records_concatenate_to_the_fixture(name, mode, world, tmp_path):
    """shd_tcp_run_group over the host-memory communicator: each rank holds the
    records of its own hosts' sockets only (a connection across ranks: one on
    each side), and the ranks' arrays in rank order are the one-engine array"""
    res = run_ranks(world, name, mode, tmp_path)
    at = 0
    for x in res:
        h0, nl = int(x["first_host"]), int(x["n_local_hosts"])
        assert h0 == at
        at += nl
        f = x["flows"]
        assert ((f["host"] >= h0) & (f["host"] < h0 + nl)).all()
    assert at == len(FIX[name]["ips"])
    cat = np.concatenate([x["flows"] for x in res])
    FE.check(cat, FIX[name]["flows"], (name, mode, world))
    assert sum(len(x["flows"]) > 0 for x in res) >= 2   # the records are spread over the ranks
    one = _run(name, False, mode)["flows"]
    assert cat.tobytes() == one.tobytes()   # the snapshot fields and proc too
