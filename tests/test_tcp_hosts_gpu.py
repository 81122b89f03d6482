"""The host records of the TCP path on the GPU (shd_tcp_model.options &
SHD_TCP_OPT_HOSTS, shd_tcp_result_hosts; csrc/tcp.hip) against the reference's
own loop: on every case of tests/golden/ref_tcp_hosts.json the records of an
untraced and of a traced run, with the path cache on the device and on tables,
equal the fixture's rows (tests/tcp_host_expect.py derives them from the
reference's [STATUS] lines), field by field -- every field is pinned.  Models
without a fixture are compared with the rows derived from the oracle's lines
(oracle/o_tcp.c, pinned to the reference on the CPU)."""
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
import tcp_host_expect as HE
import tcp_hub_cases as TH
import workloads as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "ref_tcp_hosts.json")))
SEC = S.SHD_SEC
RUNS = [(False, "device"), (False, "tables"), (True, "device"), (True, "tables")]   # (trace, mode)
# a slow_links run cut mid-transfer: tests/test_tcp_hosts_ref_cpu.py shows that
# the derivation leaves packets queued at this end time
CUT_END = 3 * SEC + 500 * S.SHD_MS


def build(name):
    return TC.build(name) if name in TC.CASES else TH.build(name)


def _case_run(name, **kw):
    c, m = build(name)
    return TCPGPU.run(m, c["graph"], TC.ip_ints(FIX[name]["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                      qdisc=c.get("qdisc", 0), udp=TC.udp_arg(c), **kw)


@functools.lru_cache(maxsize=None)
def _run(name, trace, mode):
    """one run of a fixture case with host records (computed once, never changed)"""
    return _case_run(name, mode=mode, trace=trace, hosts=True)


@pytest.mark.parametrize("trace,mode", RUNS)
@pytest.mark.parametrize("name", list(FIX))
def test_records_equal_the_reference(name, trace, mode):
    r = _run(name, trace, mode)
    h = r["hosts"]
    assert h.dtype == S.TCP_HOSTREC_DTYPE and len(h) == r["n_local_hosts"] == len(FIX[name]["rows"])
    HE.check(h, FIX[name]["rows"], (name, trace, mode))
    assert not h["_pad"].any()
    assert (len(r["lines"]) > 0) == trace
    if trace:   # and the run's own lines derive its own records
        HE.check(h, HE.rows(HE.derive(r["lines"], len(h))), (name, mode, "own lines"))


@pytest.mark.parametrize("name", ["hub40_slow", "lossy_2pct"])
def test_the_option_changes_nothing_else(name):
    on = _run(name, True, "device")
    off = _case_run(name, mode="device", trace=True)
    assert "hosts" not in off
    assert TC.digest(on["lines"]) == TC.digest(off["lines"]) and len(on["lines"]) == FIX[name]["n_status"]
    for k in ("events", "rounds", "deliveries"):
        assert on[k] == off[k], k
    for k in ("next_event_id", "next_packet_id", "rng_probe"):
        assert on[k].tolist() == off[k].tolist(), k


def test_every_option_at_once():
    """flows, paths, series and hosts in one untraced run: each is what it is alone"""
    al = _case_run("hub12_fifo", mode="device", trace=False, flows=True, paths=True, series_us=250000, hosts=True)
    HE.check(al["hosts"], FIX["hub12_fifo"]["rows"], "all options")
    rest = _case_run("hub12_fifo", mode="device", trace=False, flows=True, paths=True, series_us=250000)
    for k in ("flows", "paths", "series"):
        assert len(al[k]) > 0 and al[k].tobytes() == rest[k].tobytes(), k
    assert al["hosts"].tobytes() == _run("hub12_fifo", False, "device")["hosts"].tobytes()


def _raw(name, **kw):
    """one shd_tcp_run of a fixture case on its first-guess tables: (rc, error, records pointer set, n, records)"""
    c, m = build(name)
    lat, rel, hvi, _ = TCPGPU.path_table(m, c["graph"], c["procs"], c["peers"])
    tm, keep = TCPGPU.fill_model(m, TC.ip_ints(FIX[name]["ips"]), c["procs"], c["peers"], lat, rel, hvi, c["nbytes"],
                                 **kw)
    res = C.POINTER(S.TcpResult)()
    rc = S.lib().shd_tcp_run(C.byref(tm), 0, C.byref(res))
    del keep
    assert rc == 0
    try:
        recs, n = C.POINTER(S.TcpHostRec)(), C.c_uint64(99)
        assert S.lib().shd_tcp_result_hosts(res, C.byref(recs), C.byref(n)) == 0
        return int(res.contents.error), bool(recs), int(n.value), S.tcp_result_hosts(res)
    finally:
        S.lib().shd_tcp_result_free(res)


def test_a_model_without_the_option_has_no_records():
    """the accessor on a run that did not set SHD_TCP_OPT_HOSTS: NULL and 0"""
    err, have, n, h = _raw("lossy_2pct", flows=True)
    assert (err, have, n, len(h)) == (0, False, 0, 0)
    err, have, n, h = _raw("lossy_2pct", hosts=True)
    assert (err, have, n) == (0, True, 2)
    HE.check(h, FIX["lossy_2pct"]["rows"], "raw")


def test_more_hosts_than_one_block():
    """tcp_hub_cases.hub100: 100 hosts, two blocks of lanes, lossy links; a record per host"""
    g, m, ips, procs, peers, nb = TH.hub100()
    r = TCPGPU.run(m, g, ips, procs, peers, nbytes=nb, trace=False, hosts=True)
    want = HE.rows(HE.derive(TH.hub100_oracle()["lines"], 100))
    HE.check(r["hosts"], want, "hub100")
    h = r["hosts"]
    assert len(h) == 100 and h["host"].tolist() == list(range(100)) and (h["router_enqueued"] > 0).all()
    assert h["depth_max"][[0, 25, 50, 75]].min() > h["depth_max"][1]   # the hubs' queues are the deep ones


def test_a_run_cut_short():
    """slow_links ended at 3.5 s with the transfer running: packets are still
    queued at a router, and depth_end says how many"""
    c, m = build("slow_links")
    m.struct.end_time = CUT_END
    ips = TC.ip_ints(FIX["slow_links"]["ips"])
    r = TCPGPU.run(m, c["graph"], ips, c["procs"], c["peers"], nbytes=c["nbytes"], trace=False, hosts=True)
    o = O.tcp_run(m, c["graph"], ips, c["procs"], c["peers"], nbytes=c["nbytes"])
    want = HE.rows(HE.derive(o["lines"], 2))
    HE.check(r["hosts"], want, "cut short")
    h = r["hosts"]
    assert h["depth_end"].max() > 0
    assert (h["depth_end"] == h["router_enqueued"] - h["router_dequeued"] - h["router_dropped"]).all()
    assert h["t_last"].max() < CUT_END


def test_records_start_again_with_a_first_touch_rerun():
    """test_tcp_series_gpu.py's model whose first touches contradict the lanes'
    choice, so that shd_tcp_run runs it again from the start: the records are
    the last run's alone"""
    g, m, ips, _, _, nb = W.tcp_echo_model(2, 30, end_s=6, nbytes=30000)
    assert m.host_vertex[0] != m.host_vertex[1]
    procs = [(0, SEC), (1, SEC), (0, 2 * SEC + 10000), (1, 2 * SEC)]
    peers = [-1, -1, 1, 0]
    r = TCPGPU.run(m, g, ips, procs, peers, nbytes=nb, trace=False, hosts=True)
    assert r["first_touch"] == "device" and r["first_touch_reruns"] >= 1
    o = O.tcp_run(m, g, ips, procs, peers, nbytes=nb)
    want = HE.rows(HE.derive(o["lines"], 2))
    assert sum(x[HE.SCALARS.index("router_enqueued")] for x in want) > 0
    HE.check(r["hosts"], want, "rerun")


def run_ranks(world, case, mode, tmp_path, timeout=240):
    """`world` ranks of tests/tcp_hosts_group_worker.py on one GPU (at most 3)"""
    assert world <= 3
    name = "shdtcp_" + uuid.uuid4().hex[:16]
    procs = [subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "tcp_hosts_group_worker.py"), "--rank", str(r),
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


@pytest.mark.parametrize("world,mode", [(2, "tables"), (3, "device")])
@pytest.mark.parametrize("name", ["geo_pairs", "hub40_slow"])
def test_group_records_merge_to_the_fixture(name, world, mode, tmp_path):
    """shd_tcp_run_group over the host-memory communicator: each rank holds its
    own hosts' records, and the ranks concatenated are the one-engine array"""
    res = run_ranks(world, name, mode, tmp_path)
    for x in res:
        h0, nl = int(x["first_host"]), int(x["n_local_hosts"])
        assert x["hosts"]["host"].tolist() == list(range(h0, h0 + nl))
    hosts = S.merge_tcp_hosts([x["hosts"] for x in res])
    HE.check(hosts, FIX[name]["rows"], (name, mode, world))
    assert hosts.tobytes() == _run(name, False, mode)["hosts"].tobytes()
