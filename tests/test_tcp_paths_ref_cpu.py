"""The path records' fixture (tests/golden/ref_tcp_paths.json) is the reference's
own loop's, derived by tests/tcp_path_expect.py; the oracle's restatement
(oracle/o_tcp.c) derives the same records where it reproduces the lines; and
the C ABI's new pieces (shd_tcp_path, SHD_TCP_OPT_PATHS, shd_tcp_result_paths)
sit where include/shdtcp.h puts them.  No device.

Where the reference's loop is built (oracle/Makefile `ref`), three cases run
through it again and must reproduce the committed fixture.  hub40_slow is
compared with the reference alone: the oracle loses ROUTER_DROPPED lines there
(tests/test_tcp_hub_ref_cpu.py)."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_ffi as O
import ref_loop_ffi as R
import shdgpu as S
import tcp as TCPGPU
import tcp_cases as TC
import tcp_hub_cases as TH
import tcp_path_expect as PE

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
FIX = json.load(open(os.path.join(HERE, "golden", "ref_tcp_paths.json")))

CASES = ["lossy_2pct", "geo_pairs", "shared_hosts_rr", "loopback_mixed", "mixed_hosts", "mixed_slow_rr", "hub12_fifo",
         "hub40_slow"]
ORACLE = [n for n in CASES if n != "hub40_slow"]
LIVE = ["lossy_2pct", "mixed_hosts", "hub12_fifo"]


def build(name):
    return TC.build(name) if name in TC.CASES else TH.build(name)


def col(name, field):
    i = PE.FIELDS.index(field)
    return [r[i] for r in FIX[name]["rows"]]


def test_every_case_has_a_fixture():
    assert sorted(FIX) == sorted(CASES)
    for name, f in FIX.items():
        c, _ = build(name)
        assert f["fields"] == list(PE.FIELDS), name
        assert len(f["ips"]) == len(c["hv"]), name
        assert f["rows"] and all(len(r) == len(PE.FIELDS) for r in f["rows"]), name
        keys = [(r[0], r[1]) for r in f["rows"]]
        assert keys == sorted(set(keys)), name   # one record per ordered pair, sorted by it
        assert {v for k in keys for v in k} <= set(c["hv"]), name
        for r in f["rows"]:
            d = dict(zip(PE.FIELDS, r))
            assert d["packets_sent"] + d["packets_dropped"] > 0 and 0 < d["t_first"] <= d["t_last"], (name, d)
            assert d["control_sent"] <= d["packets_sent"], (name, d)
            assert (d["bytes_dropped"] > 0) == (d["packets_dropped"] > 0), (name, d)   # payload 0 is never dropped


def test_every_counted_line_is_some_records():
    """the rows' sums are the numbers of INET_SENT and INET_DROPPED lines of the reference's run"""
    for name, f in FIX.items():
        assert sum(col(name, "packets_sent")) == f["n_inet_sent"] > 0, name
        assert sum(col(name, "packets_dropped")) == f["n_inet_dropped"], name
        assert f["n_inet_sent"] + f["n_inet_dropped"] < f["n_status"], name


def test_fixture_is_not_vacuous():
    """what the cases are there for, as the reference's loop gives it"""
    assert sum(sum(col(n, "packets_dropped")) for n in FIX) > 0
    assert all(sum(col(n, "packets_dropped")) > 0 for n in FIX)
    # two hosts on one vertex: both lanes feed the one key (0, 0)
    assert [(r[0], r[1]) for r in FIX["lossy_2pct"]["rows"]] == [(0, 0)]
    # loopback_mixed: host 0 (vertex 0) serves its own client; that connection
    # never reaches worker_sendPacket, so no (v, v) row exists (the hosts sit on two vertices)
    c, _ = build("loopback_mixed")
    assert c["procs"][c["peers"][3]][0] == c["procs"][3][0] == 0 and len(set(c["hv"])) == len(c["hv"])
    assert all(r[0] != r[1] for r in FIX["loopback_mixed"]["rows"])
    assert sorted((r[0], r[1]) for r in FIX["loopback_mixed"]["rows"]) == [(0, 3), (3, 0)]
    # the mixed cases: datagram sockets whose destination changes give pairs no echo connection has
    for name in ("mixed_hosts", "mixed_slow_rr"):
        c, _ = build(name)
        echo = set()
        for k, p in enumerate(c["peers"]):
            if p >= 0:
                a, b = c["hv"][c["procs"][k][0]], c["hv"][c["procs"][p][0]]
                echo |= {(a, b), (b, a)}
        assert {(r[0], r[1]) for r in FIX[name]["rows"]} - echo, name
    # the hub cases: several hosts per vertex all send to vertex 0 (a key fed by
    # at least 3 hosts), and the hub's sockets feed the reverse keys
    for name in ("hub12_fifo", "hub40_slow"):
        c, _ = build(name)
        keys = {(r[0], r[1]) for r in FIX[name]["rows"]}
        per_vertex = {v: c["hv"].count(v) for v in set(c["hv"])}
        fed = [v for v, n in per_vertex.items() if n >= 3 and (v, 0) in keys and (0, v) in keys]
        assert (name == "hub40_slow") == bool(fed), (name, per_vertex)
    c, _ = build("hub40_slow")
    assert len(c["hv"]) == 41 and len(FIX["hub40_slow"]["rows"]) == 22


@functools.lru_cache(maxsize=None)
def _oracle_lines(name):
    c, m = build(name)
    o = O.tcp_run(m, c["graph"], TC.ip_ints(FIX[name]["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                  qdisc=c.get("qdisc", 0), udp=TC.udp_arg(c))
    return o["lines"]


@pytest.mark.parametrize("name", ORACLE)
def test_oracle_lines_derive_the_fixture(name):
    c, _ = build(name)
    lines = _oracle_lines(name)
    ips = TC.ip_ints(FIX[name]["ips"])
    assert PE.rows(PE.derive(lines, ips, c["hv"])) == FIX[name]["rows"]
    # the sums and the extremes do not depend on the lines' order across hosts
    assert PE.rows(PE.derive(TC.by_host(lines), ips, c["hv"])) == FIX[name]["rows"]
    assert PE.counted(lines) == (FIX[name]["n_inet_sent"], FIX[name]["n_inet_dropped"])


@pytest.mark.skipif(not R.available(), reason="oracle/_ref/libshdref_loop.so not built (needs the reference tree)")
@pytest.mark.parametrize("name", LIVE)
def test_reference_loop_reproduces_the_fixture(name):
    c, m = build(name)
    r = R.run(m, c["graph"], procs=c["procs"], tcp=TC.tcp_arg(c))
    st = TC.status_lines(r["lines"])
    assert r["ip"] == FIX[name]["ips"] and len(st) == FIX[name]["n_status"]
    assert PE.rows(PE.derive(st, TC.ip_ints(r["ip"]), c["hv"])) == FIX[name]["rows"]


def test_derive_reads_both_forms_of_a_line():
    ips, hv = [0x0B000001, 0x0B000002, 0x0B000003], [5, 9, 5]
    lines = [
        (100, 0, "[INET_SENT] packetID=0:1 11.0.0.1:40000 -> 11.0.0.2:80 seq=0 ack=0 sack=NA window=65535 bytes=0 "
                 "header=SYN tsval=1 tsechoreply=0"),
        (200, 0, "[INET_DROPPED] packetID=0:2 11.0.0.1:40000 -> 11.0.0.2:80 seq=1 ack=1 sack=1-2 3-4 window=65535 "
                 "bytes=1434 header=ACK tsval=1 tsechoreply=0"),
        (150, 2, "[INET_SENT] packetID=2:1 11.0.0.3:8998 -> 11.0.0.1:8998 bytes=700"),
        (160, 0, "[SND_INTERFACE_SENT] packetID=0:3 11.0.0.1:1 -> 11.0.0.3:2 bytes=700"),
        (170, 0, "[INET_SENT] packetID=0:3 11.0.0.1:1 -> 11.0.0.3:2 bytes=700"),
    ]
    assert PE.rows(PE.derive(lines, ips, hv)) == [[5, 5, 2, 1400, 0, 0, 0, 150, 170], [5, 9, 1, 0, 1, 1, 1434, 100, 200]]
    assert PE.counted(lines) == (3, 1)
    assert PE.symmetric_sent(PE.rows(PE.derive(lines, ips, hv))) == {(5, 5): 2, (5, 9): 1}


def test_path_struct_layout_matches_the_header(tmp_path):
    """the ctypes mirror and the dtype of shd_tcp_path against gcc's layout;
    the option and error bits; the two pinned structs unchanged"""
    names = [n for n, _ in S.TcpPath._fields_]
    assert names == list(S.TCP_PATH_DTYPE.names) == list(PE.FIELDS)
    src = tmp_path / "p.c"
    body = "".join('printf("%%zu\\n", offsetof(shd_tcp_path, %s));' % n for n in names)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s/include/shdtcp.h"\n'
                   'int main(void){printf("%%zu\\n", sizeof(shd_tcp_path));%s'
                   'printf("%%zu %%zu %%d %%d %%d %%d\\n", sizeof(shd_tcp_model), sizeof(shd_tcp_result),'
                   ' (int)SHD_TCP_OPT_PATHS, (int)SHD_TCP_OPT_FLOWS, (int)SHD_TCP_ERR_PATHS,'
                   ' (int)SHD_TCP_SOCK_BYTES);return 0;}\n' % (REPO, body))
    exe = tmp_path / "p"
    subprocess.run(["gcc", "-Wall", "-Werror", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(S.TcpPath) == S.TCP_PATH_DTYPE.itemsize == 64
    assert got[1:1 + len(names)] == [getattr(S.TcpPath, n).offset for n in names]
    assert got[1:1 + len(names)] == [S.TCP_PATH_DTYPE.fields[n][1] for n in names]
    assert [S.TCP_PATH_DTYPE.fields[n][0].itemsize for n in names] == [getattr(S.TcpPath, n).size for n in names]
    assert got[1 + len(names):] == [240, 224, 2, 1, 2048, 141888]
    assert (C.sizeof(S.TcpModel), C.sizeof(S.TcpResult)) == (240, 224)
    assert (S.TCP_OPT_PATHS, S.TCP_OPT_FLOWS, S.TCP_ERR_PATHS) == (2, 1, 2048)


def test_fill_model_sets_the_option():
    c, m = TC.build("lossy_2pct")
    args = (m, TC.ip_ints(FIX["lossy_2pct"]["ips"]), c["procs"], c["peers"], np.full((1, 1), 50.0),
            np.full((1, 1), 0.98), np.zeros(2, dtype=np.int32), c["nbytes"])
    assert int(TCPGPU.fill_model(*args)[0].options) == 0
    assert int(TCPGPU.fill_model(*args, paths=False)[0].options) == 0
    assert int(TCPGPU.fill_model(*args, flows=True)[0].options) == 1
    assert int(TCPGPU.fill_model(*args, paths=True)[0].options) == S.TCP_OPT_PATHS == 2
    assert int(TCPGPU.fill_model(*args, flows=True, paths=True)[0].options) == 3


def test_result_paths_refuses_null_arguments():
    recs, n = C.POINTER(S.TcpPath)(), C.c_uint64()
    res = S.TcpResult()   # never read: every call is refused before
    f = S.lib().shd_tcp_result_paths
    assert f(None, C.byref(recs), C.byref(n)) == -22
    assert f(C.byref(res), None, C.byref(n)) == -22
    assert f(C.byref(res), C.byref(recs), None) == -22
    assert "shd_tcp_result_paths" in S.exported_symbols()


def _arr(rows):
    a = np.zeros(len(rows), dtype=S.TCP_PATH_DTYPE)
    for i, r in enumerate(rows):
        for k, v in zip(PE.FIELDS, r):
            a[k][i] = v
    return a


def test_merge_tcp_paths_sums_a_shared_key():
    a = _arr([[0, 3, 10, 1000, 4, 1, 100, 50, 900], [2, 0, 1, 0, 1, 0, 0, 70, 70]])
    b = _arr([[0, 1, 5, 500, 0, 0, 0, 10, 20], [0, 3, 7, 2**40, 1, 2, 300, 40, 800]])
    m = S.merge_tcp_paths([a, b])
    assert m.dtype == S.TCP_PATH_DTYPE
    assert PE.from_array(m) == [[0, 1, 5, 500, 0, 0, 0, 10, 20], [0, 3, 17, 1000 + 2**40, 5, 3, 400, 40, 900],
                                [2, 0, 1, 0, 1, 0, 0, 70, 70]]
    assert PE.from_array(S.merge_tcp_paths([b, a])) == PE.from_array(m)
    assert PE.from_array(S.merge_tcp_paths([a])) == sorted(PE.from_array(a))
    assert len(S.merge_tcp_paths([])) == 0 and len(S.merge_tcp_paths([a[:0], b[:0]])) == 0


def test_write_paths_csv(tmp_path):
    a = _arr([[0, 3, 10, 2**40, 4, 1, 100, 50, 900], [2, 0, 1, 0, 1, 0, 0, 70, 70]])
    p = tmp_path / "paths.csv"
    assert S.write_paths_csv(p, a) == 2
    rows = p.read_text().splitlines()
    assert rows[0].split(",") == list(PE.FIELDS) and len(rows) == 3
    assert [int(x) for x in rows[1].split(",")] == [0, 3, 10, 2**40, 4, 1, 100, 50, 900]
    assert [int(x) for x in rows[2].split(",")] == [2, 0, 1, 0, 1, 0, 0, 70, 70]
    assert S.write_paths_csv(tmp_path / "none.csv", np.zeros(0, dtype=S.TCP_PATH_DTYPE)) == 0
