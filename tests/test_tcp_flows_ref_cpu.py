"""The flow records' fixture (tests/golden/ref_tcp_flows.json) is the reference's
own loop's, derived by tests/tcp_flow_expect.py; the oracle's restatement
(oracle/o_tcp.c) derives the same records where it reproduces the lines; and
the C ABI's new pieces (shd_tcp_flow, shd_tcp_model.options,
shd_tcp_result_flows) sit where include/shdtcp.h puts them.  No device.

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
import tcp_flow_expect as FE
import tcp_hub_cases as TH

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
FIX = json.load(open(os.path.join(HERE, "golden", "ref_tcp_flows.json")))

ECHO = ["ref_epoll_lossy", "lossy_2pct", "slow_links", "heavy_loss", "geo_pairs", "shared_hosts_rr", "server_first",
        "loopback_pair", "loopback_mixed", "mixed_hosts", "mixed_slow_rr"]
HUB = ["hub12_fifo", "hub40_slow", "fan_out20"]
ORACLE = [n for n in ECHO + HUB if n != "hub40_slow"]
LIVE = ["lossy_2pct", "loopback_pair", "hub12_fifo"]


def build(name):
    return TC.build(name) if name in TC.CASES else TH.build(name)


def col(name, field):
    i = FE.PINNED.index(field)
    return [r[i] for r in FIX[name]["flows"]]


def test_every_case_has_a_fixture():
    assert sorted(FIX) == sorted(ECHO + HUB)
    for name, f in FIX.items():
        c, _ = build(name)
        assert f["fields"] == list(FE.PINNED), name
        assert len(f["ips"]) == len(c["hv"]), name
        assert all(len(r) == len(FE.PINNED) for r in f["flows"]), name
        # a record per endpoint of every echo connection: each client process and its server's child
        assert len(f["flows"]) == 2 * sum(1 for k, p in enumerate(c["peers"]) if p >= 0), name
        assert col(name, "host") == sorted(col(name, "host")), name
        assert all(t > 0 for t in col(name, "t_open")), name


def test_fixture_is_not_vacuous():
    """what the cases are there for, as the reference's loop gives it"""
    n = FIX["geo_pairs"]
    assert len(n["flows"]) == 20
    open_end = [r for r in n["flows"] if r[FE.PINNED.index("t_fin")] == 0]
    assert len(open_end) == 2
    # one of the two is incomplete (a client that has not read everything back); the other has all its bytes
    assert sorted(r[FE.PINNED.index("bytes_delivered")] < 100000 for r in open_end) == [False, True]
    h = FIX["hub40_slow"]
    assert len(h["flows"]) == 80
    rd, sd = col("hub40_slow", "router_dropped"), col("hub40_slow", "socket_dropped")
    assert sum(rd) == 199 and sum(1 for x in rd if x) == 34
    assert sum(sd) == 6 and sum(1 for x in sd if x) == 1
    assert sum(col("slow_links", "router_dropped")) == 42
    assert sorted(col("lossy_2pct", "retransmitted")) == [9, 17]
    a, b = FIX["loopback_pair"]["flows"]
    i = FE.PINNED.index
    assert a[i("local_ip")] == a[i("peer_ip")] == b[i("local_ip")] == b[i("peer_ip")]
    assert (a[i("local_port")], a[i("peer_port")]) == (b[i("peer_port")], b[i("local_port")])
    assert sum(sum(col(n, "inet_dropped")) for n in FIX) > 100
    # every ROUTER_DROPPED line of a TCP packet is some record's
    for name, f in FIX.items():
        assert f["n_router_unattributed"] == 0, name
        assert sum(col(name, "router_dropped")) == f["n_router_dropped_tcp"], name


def test_fixture_records_are_consistent():
    """what holds for any run: both roles per connection, the handshake's
    order, a completed client's last delivery is its FIN (test_tcp.c closes
    right after its last read)"""
    i = FE.PINNED.index
    done = {}
    for name, f in FIX.items():
        c, _ = build(name)
        by = {(r[i("local_ip")], r[i("local_port")], r[i("peer_ip")], r[i("peer_port")]): r for r in f["flows"]}
        assert len(by) == len(f["flows"]), name
        for k, r in by.items():
            peer = by[(k[2], k[3], k[0], k[1])]
            assert {r[i("role")], peer[i("role")]} == {0, 1}, (name, k)
            assert r[i("t_established")] == 0 or r[i("t_open")] <= r[i("t_established")], (name, k)
            assert r[i("bytes_delivered")] <= peer[i("bytes_created")], (name, k)
            if r[i("role")] == 0 and r[i("bytes_delivered")] == c["nbytes"]:   # a client that completed
                assert r[i("t_last_delivered")] > 0 and r[i("t_fin")] > 0, (name, k)
                n, eq = done.get(name, (0, 0))
                done[name] = (n + 1, eq + (r[i("t_last_delivered")] == r[i("t_fin")]))
    # the completion time is t_last_delivered; t_fin equals it wherever the close
    # found the socket's output empty and the peer's FIN had not overtaken
    # retransmitted data (the answer to that FIN carries FIN itself: earlier) --
    # everywhere but one connection of geo_pairs (150.6 ms later) and five of
    # hub40_slow (5 to 66 ms earlier)
    other = {"geo_pairs": (9, 8), "hub40_slow": (40, 35)}
    for name, (n, eq) in done.items():
        assert (n, eq) == other.get(name, (n, n)), (name, n, eq)
    assert sum(n for n, _ in done.values()) == 97


@functools.lru_cache(maxsize=None)
def _oracle_lines(name):
    c, m = build(name)
    o = O.tcp_run(m, c["graph"], TC.ip_ints(FIX[name]["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                  qdisc=c.get("qdisc", 0), udp=TC.udp_arg(c))
    return o["lines"]


@pytest.mark.parametrize("name", ORACLE)
def test_oracle_lines_derive_the_fixture(name):
    lines = _oracle_lines(name)
    assert FE.rows(FE.derive(lines)) == FIX[name]["flows"]
    # a record reads its own host's lines only: grouped by host the same records come out
    assert FE.rows(FE.derive(TC.by_host(lines))) == FIX[name]["flows"]


@pytest.mark.skipif(not R.available(), reason="oracle/_ref/libshdref_loop.so not built (needs the reference tree)")
@pytest.mark.parametrize("name", LIVE)
def test_reference_loop_reproduces_the_fixture(name):
    c, m = build(name)
    r = R.run(m, c["graph"], procs=c["procs"], tcp=TC.tcp_arg(c))
    st = TC.status_lines(r["lines"])
    assert r["ip"] == FIX[name]["ips"] and len(st) == FIX[name]["n_status"]
    assert FE.rows(FE.derive(st)) == FIX[name]["flows"]
    assert FE.unattributed_router_drops(st) == 0


def test_flow_struct_layout_matches_the_header(tmp_path):
    """the ctypes mirror and the dtype of shd_tcp_flow against gcc's layout"""
    names = [n for n, _ in S.TcpFlow._fields_]
    assert names == list(S.TCP_FLOW_DTYPE.names)
    src = tmp_path / "f.c"
    body = "".join('printf("%%zu\\n", offsetof(shd_tcp_flow, %s));' % n for n in names)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s/include/shdtcp.h"\n'
                   'int main(void){printf("%%zu\\n", sizeof(shd_tcp_flow));%s'
                   'printf("%%zu %%zu %%zu %%d\\n", sizeof(shd_tcp_model), offsetof(shd_tcp_model, options),'
                   ' sizeof(shd_tcp_result), (int)SHD_TCP_OPT_FLOWS);return 0;}\n' % (REPO, body))
    exe = tmp_path / "f"
    subprocess.run(["gcc", "-Wall", "-Werror", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(S.TcpFlow) == S.TCP_FLOW_DTYPE.itemsize and got[0] % 8 == 0
    assert got[1:1 + len(names)] == [getattr(S.TcpFlow, n).offset for n in names]
    assert got[1:1 + len(names)] == [S.TCP_FLOW_DTYPE.fields[n][1] for n in names]
    assert [S.TCP_FLOW_DTYPE.fields[n][0].itemsize for n in names] == [getattr(S.TcpFlow, n).size for n in names]
    assert got[1 + len(names):] == [C.sizeof(S.TcpModel), S.TcpModel.options.offset, C.sizeof(S.TcpResult),
                                    S.TCP_OPT_FLOWS]


def test_options_sits_in_the_old_pad_word():
    """between qdisc and path_cache, four bytes: no offset moved, no size grew"""
    T = S.TcpModel
    assert T.options.offset == T.qdisc.offset + 4 == 136 and T.options.size == 4
    assert T.path_cache.offset == 144   # (four bytes of alignment follow the word, as they followed the pad)
    assert T.qdisc.offset == T.packets_per_host.offset + 4
    assert C.sizeof(T) == T.host_heartbeat.offset + 8 == 240
    assert C.sizeof(S.TcpResult) == S.TcpResult.sock_bytes.offset + 8 == 224


def test_fill_model_sets_the_option():
    c, m = TC.build("lossy_2pct")
    args = (m, TC.ip_ints(FIX["lossy_2pct"]["ips"]), c["procs"], c["peers"], np.full((1, 1), 50.0),
            np.full((1, 1), 0.98), np.zeros(2, dtype=np.int32), c["nbytes"])
    assert int(TCPGPU.fill_model(*args)[0].options) == 0
    assert int(TCPGPU.fill_model(*args, flows=True)[0].options) == S.TCP_OPT_FLOWS == 1


def test_result_flows_refuses_null_arguments():
    recs, n = C.POINTER(S.TcpFlow)(), C.c_uint64()
    res = S.TcpResult()   # never read: every call is refused before
    f = S.lib().shd_tcp_result_flows
    assert f(None, C.byref(recs), C.byref(n)) == -22
    assert f(C.byref(res), None, C.byref(n)) == -22
    assert f(C.byref(res), C.byref(recs), None) == -22


def test_write_flows_csv(tmp_path):
    """one line per record, dotted addresses, the state by name"""
    a = np.zeros(2, dtype=S.TCP_FLOW_DTYPE)
    a["host"] = [0, 3]
    a["proc"] = [1, 0]
    a["role"] = [0, 1]
    a["local_ip"] = [0x0B000001, 0x0B000004]
    a["peer_ip"] = [0x0B000004, 0x0B000001]
    a["local_port"] = [45963, 80]
    a["peer_port"] = [80, 45963]
    a["state"] = [8, 0]
    a["t_open"] = [2 * 10**9, 2 * 10**9 + 50]
    a["bytes_delivered"] = [2**40, 7]
    a["srtt"] = [-1, 100]
    p = tmp_path / "flows.csv"
    assert S.write_flows_csv(p, a) == 2
    rows = p.read_text().splitlines()
    assert rows[0].split(",") == list(S.FLOW_CSV_FIELDS) and len(rows) == 3
    r0 = dict(zip(S.FLOW_CSV_FIELDS, rows[1].split(",")))
    r1 = dict(zip(S.FLOW_CSV_FIELDS, rows[2].split(",")))
    assert (r0["local"], r0["peer"], r0["state"], r0["role"]) == ("11.0.0.1:45963", "11.0.0.4:80", "TIMEWAIT", "0")
    assert (r1["local"], r1["peer"], r1["state"], r1["host"]) == ("11.0.0.4:80", "11.0.0.1:45963", "CLOSED", "3")
    assert r0["bytes_delivered"] == str(2**40) and r0["srtt"] == "-1" and r1["t_open"] == "2000000050"
    assert S.write_flows_csv(tmp_path / "none.csv", np.zeros(0, dtype=S.TCP_FLOW_DTYPE)) == 0
