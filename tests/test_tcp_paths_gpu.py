"""Path records of the TCP path on the GPU (shd_tcp_model.options &
SHD_TCP_OPT_PATHS, shd_tcp_result_paths; csrc/tcp.hip) against the reference's
own loop: on every case of tests/golden/ref_tcp_paths.json the records of an
untraced and of a traced run, with the path cache on the device and on tables,
equal the fixture field by field (tests/tcp_path_expect.py derives them from
the reference's INET_SENT / INET_DROPPED [STATUS] lines), and the four arrays
are equal byte for byte.  Models without a fixture are compared with the
records derived from the oracle's lines (oracle/o_tcp.c, pinned to the
reference on the CPU)."""
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
import sim
import tcp as TCPGPU
import tcp_cases as TC
import tcp_hub_cases as TH
import tcp_path_expect as PE
import workloads as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "ref_tcp_paths.json")))
SEC = S.SHD_SEC
RUNS = [(False, "device"), (False, "tables"), (True, "device"), (True, "tables")]   # (trace, mode)


def build(name):
    return TC.build(name) if name in TC.CASES else TH.build(name)


@functools.lru_cache(maxsize=None)
def _run(name, trace, mode, flows=False, paths=True):
    """one run of a fixture case (computed once, never changed)"""
    c, m = build(name)
    return TCPGPU.run(m, c["graph"], TC.ip_ints(FIX[name]["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                      qdisc=c.get("qdisc", 0), udp=TC.udp_arg(c), mode=mode, trace=trace, flows=flows, paths=paths)


@pytest.mark.parametrize("trace,mode", RUNS)
@pytest.mark.parametrize("name", list(FIX))
def test_path_records_equal_the_reference(name, trace, mode):
    c, _ = build(name)
    r = _run(name, trace, mode)
    assert r["paths"].dtype == S.TCP_PATH_DTYPE
    PE.check(r["paths"], FIX[name]["rows"], (name, trace, mode))
    assert (len(r["lines"]) > 0) == trace
    if trace:   # and the run's own lines derive its own records
        PE.check(r["paths"], PE.rows(PE.derive(r["lines"], TC.ip_ints(FIX[name]["ips"]), c["hv"])), (name, "own lines"))
        assert PE.counted(r["lines"]) == (FIX[name]["n_inet_sent"], FIX[name]["n_inet_dropped"])


@pytest.mark.parametrize("name", list(FIX))
def test_the_four_runs_give_the_same_bytes(name):
    """graph vertex ids in both path modes: the device-mode array and the tables-mode array are equal"""
    a = _run(name, *RUNS[0])["paths"]
    assert len(a) == len(FIX[name]["rows"])
    for trace, mode in RUNS[1:]:
        assert a.tobytes() == _run(name, trace, mode)["paths"].tobytes(), (name, trace, mode)


@pytest.mark.parametrize("name", ["lossy_2pct", "hub12_fifo", "mixed_hosts"])
def test_paths_on_changes_nothing_else(name):
    on = _run(name, False, "device", True, True)
    off = _run(name, False, "device", True, False)
    assert "paths" not in off and len(on["paths"]) == len(FIX[name]["rows"])
    for k in ("events", "rounds", "deliveries"):
        assert on[k] == off[k], k
    for k in ("next_event_id", "next_packet_id", "rng_probe"):
        assert on[k].tolist() == off[k].tolist(), k
    assert on["flows"].tobytes() == off["flows"].tobytes()
    # and the records do not depend on the flow records being kept
    assert on["paths"].tobytes() == _run(name, False, "device")["paths"].tobytes()


def test_a_model_without_the_option_has_no_records():
    """the accessor on a run that did not set SHD_TCP_OPT_PATHS: NULL and 0;
    with the option the same call hands out the records"""
    name = "lossy_2pct"
    c, m = build(name)
    ips = TC.ip_ints(FIX[name]["ips"])
    lat, rel, hvi, _ = TCPGPU.path_table(m, c["graph"], c["procs"], c["peers"])
    for paths in (False, True):
        tm, keep = TCPGPU.fill_model(m, ips, c["procs"], c["peers"], lat, rel, hvi, c["nbytes"], paths=paths)
        res = C.POINTER(S.TcpResult)()
        assert S.lib().shd_tcp_run(C.byref(tm), 0, C.byref(res)) == 0
        try:
            assert res.contents.error == 0
            recs, n = C.POINTER(S.TcpPath)(), C.c_uint64(99)
            assert S.lib().shd_tcp_result_paths(res, C.byref(recs), C.byref(n)) == 0
            assert (n.value, bool(recs)) == ((1, True) if paths else (0, False))
            assert len(S.tcp_result_paths(res)) == n.value
        finally:
            S.lib().shd_tcp_result_free(res)


def test_flow_records_drops_sum_to_the_path_records():
    """geo_pairs (echo processes only): each connection endpoint's inet_dropped,
    summed per (vertex of its host, vertex of its peer), is the pair's packets_dropped"""
    name = "geo_pairs"
    c, _ = build(name)
    r = _run(name, False, "device", True, True)
    ips = TC.ip_ints(FIX[name]["ips"])
    host_of = {ip: h for h, ip in enumerate(ips)}
    want = {}
    for f in r["flows"]:
        key = (c["hv"][int(f["host"])], c["hv"][host_of[int(f["peer_ip"])]])
        want[key] = want.get(key, 0) + int(f["inet_dropped"])
    got = {(int(p["v_src"]), int(p["v_dst"])): int(p["packets_dropped"]) for p in r["paths"]}
    assert got == want and sum(got.values()) == FIX[name]["n_inet_dropped"] > 0
    assert len(want) == 2 * sum(1 for p in c["peers"] if p >= 0)   # every connection has a pair of its own here


def _cache_counts(pc, vertices):
    out = {}
    for i, a in enumerate(vertices):
        for b in vertices[i:]:
            n = C.c_uint64(1 << 60)
            S.check(S.lib().shd_pc_packet_count(pc.ptr, int(a), int(b), C.byref(n)), "shd_pc_packet_count")
            out[(int(a), int(b))] = int(n.value)
    return out


def _run_on_cache(m, g, ips, procs, peers, nbytes, hv, paths, qdisc=0, udp=None):
    """shd_tcp_run in path_cache mode on a cache of this call's own: (the run, the cache's packet counts)"""
    hv = np.asarray(hv, dtype=np.int32)
    att = np.unique(hv)
    pc = sim.PathCache(g, att)
    try:
        before = _cache_counts(pc, att)
        assert not any(before.values())
        out = TCPGPU._run_once(m, ips, procs, peers, None, None, hv, nbytes, False, TCPGPU.RECV_BUF, TCPGPU.SEND_BUF,
                               TCPGPU.TCP_WINDOW, 0, False, qdisc, pc=pc, udp=udp, paths=paths)
        assert out is not None   # (the device's first-touch choices stood)
        return out, _cache_counts(pc, att)
    finally:
        pc.close()


@pytest.mark.parametrize("name", ["lossy_2pct", "geo_pairs", "hub12_fifo", "mixed_hosts"])
def test_sends_fold_into_the_path_cache(name):
    """path_cache mode: afterwards shd_pc_packet_count is sent[a->b] + sent[b->a]
    (sent[a->a] once), the reference's Path.packetCount; without the option the counter stays 0"""
    c, m = build(name)
    args = (m, c["graph"], TC.ip_ints(FIX[name]["ips"]), c["procs"], c["peers"], c["nbytes"], c["hv"])
    kw = dict(qdisc=c.get("qdisc", 0), udp=TC.udp_arg(c))
    out, counts = _run_on_cache(*args, True, **kw)
    PE.check(out["paths"], FIX[name]["rows"], name)
    want = PE.symmetric_sent(FIX[name]["rows"])
    assert {k: v for k, v in counts.items() if v} == want
    assert sum(counts.values()) == FIX[name]["n_inet_sent"]
    out, counts = _run_on_cache(*args, False, **kw)
    assert "paths" not in out and not any(counts.values())


def test_records_start_again_with_a_first_touch_rerun():
    """test_tcp_flows_gpu.py's model whose first touches contradict the lanes'
    choice, so that shd_tcp_run runs it again from the start: the records and
    the counts folded into the cache are the last run's alone"""
    g, m, ips, _, _, nb = W.tcp_echo_model(2, 30, end_s=6, nbytes=30000)
    hv = [int(m.host_vertex[0]), int(m.host_vertex[1])]
    assert hv[0] != hv[1]
    procs = [(0, SEC), (1, SEC), (0, 2 * SEC + 10000), (1, 2 * SEC)]
    peers = [-1, -1, 1, 0]
    out, counts = _run_on_cache(m, g, ips, procs, peers, nb, hv, True)
    assert out["first_touch_reruns"] >= 1
    o = O.tcp_run(m, g, ips, procs, peers, nbytes=nb)
    want = PE.rows(PE.derive(o["lines"], [int(x) for x in ips], hv))
    assert sorted((r[0], r[1]) for r in want) == sorted([(hv[0], hv[1]), (hv[1], hv[0])])
    PE.check(out["paths"], want, "rerun")
    assert {k: v for k, v in counts.items() if v} == PE.symmetric_sent(want)
    assert sum(counts.values()) == PE.counted(o["lines"])[0]
    # and through tcp.run, which makes its own cache
    r = TCPGPU.run(m, g, ips, procs, peers, nbytes=nb, trace=False, paths=True)
    assert r["first_touch"] == "device" and r["first_touch_reruns"] >= 1
    PE.check(r["paths"], want, "rerun, tcp.run")


_OVERFLOW_CHILD = """
import ctypes as C, json, os, sys
sys.path[:0] = [%r, %r]
import shdgpu as S, tcp as TCPGPU, tcp_cases as TC, tcp_hub_cases as TH
fix = json.load(open(os.path.join(%r, "golden", "ref_tcp_paths.json")))["hub12_fifo"]
c, m = TH.build("hub12_fifo")
lat, rel, hvi, _ = TCPGPU.path_table(m, c["graph"], c["procs"], c["peers"])
tm, keep = TCPGPU.fill_model(m, TC.ip_ints(fix["ips"]), c["procs"], c["peers"], lat, rel, hvi, c["nbytes"], paths=True)
res = C.POINTER(S.TcpResult)()
rc = S.lib().shd_tcp_run(C.byref(tm), 0, C.byref(res))
print("rc", rc, "error", res.contents.error if rc == 0 else -1, "records", len(S.tcp_result_paths(res)) if rc == 0 else -1)
"""


@pytest.mark.parametrize("slots", ["2", None])
def test_a_full_pair_table_is_an_error(slots):
    """hub12_fifo uses 22 pairs: a table forced to 2 entries (SHD_TCP_PATH_SLOTS
    in a child process's environment) ends the run with SHD_TCP_ERR_PATHS in
    its error bits -- an error, never a lost count or a fault; unset, the same
    run has no error"""
    env = {k: v for k, v in os.environ.items() if k != "SHD_TCP_PATH_SLOTS"}
    if slots is not None:
        env["SHD_TCP_PATH_SLOTS"] = slots
    src = _OVERFLOW_CHILD % (os.path.join(os.path.dirname(HERE), "shadow-1_amd"), HERE, HERE)
    p = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    w = p.stdout.split()
    rc, err, n = int(w[1]), int(w[3]), int(w[5])
    assert rc == 0
    if slots is not None:
        assert err & S.TCP_ERR_PATHS and n <= 2, p.stdout
    else:
        assert err == 0 and n == len(FIX["hub12_fifo"]["rows"]) == 22, p.stdout


def run_ranks(world, case, mode, tmp_path, timeout=240):
    """`world` ranks of tests/tcp_paths_group_worker.py on one GPU (at most 3)"""
    assert world <= 3
    name = "shdtcp_" + uuid.uuid4().hex[:16]
    procs = [subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "tcp_paths_group_worker.py"), "--rank", str(r),
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


@pytest.mark.parametrize("mode", ["tables", "device"])
@pytest.mark.parametrize("name", ["hub12_fifo", "mixed_hosts"])
def test_group_records_merge_to_the_fixture(name, mode, tmp_path):
    """shd_tcp_run_group over the host-memory communicator, 2 ranks: each rank
    holds its own hosts' sends (nothing is exchanged), and the ranks' arrays
    merged are the one-engine array"""
    c, _ = build(name)
    res = run_ranks(2, name, mode, tmp_path)
    at = 0
    for x in res:
        h0, nl = int(x["first_host"]), int(x["n_local_hosts"])
        assert h0 == at
        at += nl
        local = {c["hv"][h] for h in range(h0, h0 + nl)}
        assert len(x["paths"]) > 0 and set(x["paths"]["v_src"].tolist()) <= local, (name, h0, nl)
    assert at == len(FIX[name]["ips"])
    merged = S.merge_tcp_paths([x["paths"] for x in res])
    PE.check(merged, FIX[name]["rows"], (name, mode))
    assert merged.tobytes() == _run(name, False, mode)["paths"].tobytes()
