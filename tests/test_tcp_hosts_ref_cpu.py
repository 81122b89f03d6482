"""The host records' fixture (tests/golden/ref_tcp_hosts.json) is the
reference's own loop's, derived by tests/tcp_host_expect.py; the oracle's
restatement (oracle/o_tcp.c) derives the same rows wherever it reproduces the
reference's lines; and the C ABI's new pieces (shd_tcp_hostrec,
SHD_TCP_OPT_HOSTS, shd_tcp_result_hosts) sit where include/shdtcp.h puts them
without growing a pinned struct.  No device.

Where the reference's loop is built (oracle/Makefile `ref`), two cases run
through it again and must reproduce the committed fixture."""
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
import tcp_host_expect as HE
import tcp_hub_cases as TH

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
FIX = json.load(open(os.path.join(HERE, "golden", "ref_tcp_hosts.json")))
# what the issue sets: the cases, and per case (enqueued, dequeued, dropped,
# deepest queue, hosts that reached it, longest sojourn of a dequeued packet)
CASES = ["hub40_slow", "slow_links", "mixed_slow_rr", "hub12_fifo", "geo_pairs", "loopback_pair", "lossy_2pct"]
TABLE = {"hub40_slow": (2598, 2399, 199, 173, 1, 133744046), "slow_links": (987, 945, 42, 29, 2, 100000000),
         "mixed_slow_rr": (1049, 1031, 18, 24, None, 78612045), "hub12_fifo": (888, 888, 0, 12, None, 1036122),
         "geo_pairs": (2231, 2231, 0, 8, None, 520850)}
# hub40_slow: the oracle's lines differ from the reference's there
# (tcp_hub_cases.ORACLE_COUNTERS): the reference fixture alone pins the case
ORACLE = [n for n in CASES if n not in TH.ORACLE_COUNTERS]
LIVE = ["hub40_slow", "mixed_slow_rr"]
I = {k: j for j, k in enumerate(HE.SCALARS)}
# a slow_links run cut mid-transfer (tests/test_tcp_hosts_gpu.py runs the same end time)
CUT_END = 3 * S.SHD_SEC + 500 * S.SHD_MS


def build(name):
    return TC.build(name) if name in TC.CASES else TH.build(name)


def test_every_case_has_a_fixture():
    assert sorted(FIX) == sorted(CASES)
    assert os.path.getsize(os.path.join(HERE, "golden", "ref_tcp_hosts.json")) < 100000
    for name, f in FIX.items():
        c, _ = build(name)
        assert f["fields"] == list(HE.FIELDS), name
        assert len(f["ips"]) == len(f["rows"]) == len(c["hv"]), name
        assert [r[0] for r in f["rows"]] == list(range(len(c["hv"]))), name   # dense, in host order
        assert all(len(r) == len(HE.FIELDS) and len(r[-1]) == 16 for r in f["rows"]), name


def test_fixture_is_not_vacuous():
    """the issue's table: the five cases' totals, and what the other fields need to be worth comparing"""
    for name, want in TABLE.items():
        got = HE.totals(FIX[name]["rows"])
        assert tuple(g for g, w in zip(got, want) if w is not None) == tuple(w for w in want if w is not None), name
    hub = FIX["hub40_slow"]["rows"]
    assert len(hub) == 41 and [i for i in range(16) if sum(r[-1][i] for r in hub)] == list(range(12))
    assert sum(r[I["if_dropped"]] for r in FIX["mixed_slow_rr"]["rows"]) == 5
    lo = FIX["loopback_pair"]["rows"]
    assert len(lo) == 1 and lo[0][I["if_sent"]] == lo[0][I["if_received"]] == 464 and lo[0][I["router_enqueued"]] == 0
    assert HE.totals(FIX["lossy_2pct"]["rows"]) == (1011, 1011, 0, 7, 1, 0)
    assert sum(r[I["tcp_throttled"]] for r in FIX["slow_links"]["rows"]) > 0
    assert sum(r[I["tcp_unordered"]] for r in FIX["lossy_2pct"]["rows"]) > 0


@pytest.mark.parametrize("name", CASES)
def test_fixture_rows_obey_their_identities(name):
    for r in FIX[name]["rows"]:
        g = lambda k: r[I[k]]   # noqa: E731
        assert g("depth_end") == g("router_enqueued") - g("router_dequeued") - g("router_dropped"), (name, r)
        assert sum(r[-1]) == g("router_dequeued"), (name, r)
        assert g("sojourn_max") <= g("sojourn_sum"), (name, r)
        assert g("if_received") >= g("router_dequeued"), (name, r)
        assert g("t_first") <= g("t_last"), (name, r)
        assert g("depth_max") <= g("router_enqueued") and (g("depth_max") > 0) == (g("router_enqueued") > 0), (name, r)
        if g("router_enqueued"):   # (a loopback host's packets never see the router)
            assert g("t_first") <= g("t_depth_max") <= g("t_last"), (name, r)
        if g("router_dequeued"):
            assert g("t_first") <= g("t_sojourn_max") <= g("t_last"), (name, r)
        else:
            assert g("t_sojourn_max") == g("sojourn_sum") == 0, (name, r)
        if not g("t_first"):   # a host that saw no packet: zero apart from `host`
            assert r[1:-1] == [0] * (len(HE.SCALARS) - 1) and not any(r[-1]), (name, r)


@functools.lru_cache(maxsize=None)
def _oracle_lines(name, end_ns=0):
    c, m = build(name)
    if end_ns:
        m.struct.end_time = end_ns
    o = O.tcp_run(m, c["graph"], TC.ip_ints(FIX[name]["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                  qdisc=c.get("qdisc", 0), udp=TC.udp_arg(c))
    return o["lines"]


@pytest.mark.parametrize("name", ORACLE)
def test_oracle_lines_derive_the_fixture(name):
    lines = _oracle_lines(name)
    H = len(FIX[name]["rows"])
    assert HE.rows(HE.derive(lines, H)) == FIX[name]["rows"]
    # a record reads its own host's lines only: grouped by host the same rows come out
    assert HE.rows(HE.derive(TC.by_host(lines), H)) == FIX[name]["rows"]


def test_a_cut_run_leaves_packets_queued():
    """slow_links ended at 3.5 s, mid-transfer: what tests/test_tcp_hosts_gpu.py
    compares a cut run with has depth_end > 0 on a host"""
    rows = HE.rows(HE.derive(_oracle_lines("slow_links", CUT_END), 2))
    assert max(r[I["depth_end"]] for r in rows) > 0
    for r in rows:
        assert r[I["depth_end"]] == r[I["router_enqueued"]] - r[I["router_dequeued"]] - r[I["router_dropped"]]


@pytest.mark.skipif(not R.available(), reason="oracle/_ref/libshdref_loop.so not built (needs the reference tree)")
@pytest.mark.parametrize("name", LIVE)
def test_reference_loop_reproduces_the_fixture(name):
    c, m = build(name)
    r = R.run(m, c["graph"], procs=c["procs"], tcp=TC.tcp_arg(c))
    st = TC.status_lines(r["lines"])
    assert r["ip"] == FIX[name]["ips"] and len(st) == FIX[name]["n_status"]
    assert HE.rows(HE.derive(st, len(c["hv"]))) == FIX[name]["rows"]


def _ln(st, pid, n, udp=False):
    if udp:   # the datagram form: no TCP header fields
        return f"[{st}] packetID={pid} 11.0.0.2:2000 -> 11.0.0.1:1000 bytes={n}"
    return f"[{st}] packetID={pid} 11.0.0.2:2000 -> 11.0.0.1:1000 seq=1 ack=1 sack=NA window=1 bytes={n} " \
           f"header=ACK status=x"


def test_derivation_on_a_hand_made_trace():
    """the rule on ten lines: an enqueue into an empty queue dequeued at the
    same instant (sojourn 0, depth 1), a run of two drops before a dequeue in
    one event, a sojourn of exactly 65 536 ns (bucket 1), a datagram line"""
    T = 400 + 65536
    lines = [(100, 0, _ln("ROUTER_ENQUEUED", "2:1", 10)),
             (100, 0, _ln("ROUTER_DEQUEUED", "2:1", 10)),
             (100, 0, _ln("RCV_INTERFACE_RECEIVED", "2:1", 10)),
             (150, 1, _ln("SND_INTERFACE_SENT", "2:9", 55)),
             (200, 0, _ln("ROUTER_ENQUEUED", "2:2", 20)),
             (300, 0, _ln("ROUTER_ENQUEUED", "2:3", 700, udp=True)),
             (400, 0, _ln("ROUTER_ENQUEUED", "2:4", 30)),
             (T, 0, _ln("ROUTER_DROPPED", "2:2", 20)),
             (T, 0, _ln("ROUTER_DROPPED", "2:3", 700, udp=True)),
             (T, 0, _ln("ROUTER_DEQUEUED", "2:4", 30)),
             (T + 5, 0, _ln("SND_CREATED", "1:1", 99))]   # not a counted status
    a, b, idle = HE.derive(lines, 3)
    hist = [1, 1] + [0] * 14
    assert a == dict(host=0, depth_max=3, depth_end=0, router_enqueued=4, router_enqueued_bytes=760,
                     router_dequeued=2, router_dequeued_bytes=40, router_dropped=2, router_dropped_bytes=720,
                     t_depth_max=400, sojourn_sum=65536, sojourn_max=65536, t_sojourn_max=T, if_received=1,
                     if_received_bytes=10, if_dropped=0, if_sent=0, if_sent_bytes=0, tcp_throttled=0,
                     tcp_unordered=0, t_first=100, t_last=T, sojourn_hist=hist)
    assert (b["if_sent"], b["if_sent_bytes"], b["t_first"], b["t_last"], b["router_enqueued"]) == (1, 55, 150, 150, 0)
    assert HE.rows([idle]) == [[2] + [0] * (len(HE.SCALARS) - 1) + [[0] * 16]]
    # only the first dequeue's sojourn 0 so far: its time is t_sojourn_max
    first = HE.derive(lines[:3], 1)[0]
    assert (first["depth_max"], first["sojourn_max"], first["t_sojourn_max"], first["sojourn_hist"][0]) == (1, 0, 100, 1)
    assert HE.derive(lines[:7], 2)[0]["depth_end"] == 3
    assert [HE.bucket(x) for x in (0, 65535, 65536, 131071, 131072, 2**30 - 1, 2**30, 2**40)] == \
        [0, 0, 1, 1, 2, 14, 15, 15]
    with pytest.raises(AssertionError):   # a dequeue that does not name the queue's head
        HE.derive(lines[:7] + [(T, 0, _ln("ROUTER_DEQUEUED", "2:3", 700, udp=True))], 2)
    with pytest.raises(AssertionError):   # a drop from an empty queue
        HE.derive([(T, 0, _ln("ROUTER_DROPPED", "2:2", 20))], 1)


def test_hostrec_struct_layout_matches_the_header(tmp_path):
    """the ctypes mirror and the dtype against gcc's layout: shd_tcp_hostrec is
    232 bytes, the model and the result kept their sizes"""
    names = [n for n, _ in S.TcpHostRec._fields_]
    assert names == list(S.TCP_HOSTREC_DTYPE.names)
    src = tmp_path / "h.c"
    body = "".join('printf("%%zu\\n", offsetof(shd_tcp_hostrec, %s));' % n for n in names)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s/include/shdtcp.h"\n'
                   'int main(void){printf("%%zu\\n", sizeof(shd_tcp_hostrec));%s'
                   'printf("%%zu %%zu %%zu %%d\\n", sizeof(shd_tcp_model), sizeof(shd_tcp_result),'
                   ' sizeof(((shd_tcp_hostrec*)0)->sojourn_hist), (int)SHD_TCP_OPT_HOSTS);return 0;}\n' % (REPO, body))
    exe = tmp_path / "h"
    subprocess.run(["gcc", "-Wall", "-Werror", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(S.TcpHostRec) == S.TCP_HOSTREC_DTYPE.itemsize == 232
    assert got[1:1 + len(names)] == [getattr(S.TcpHostRec, n).offset for n in names]
    assert got[1:1 + len(names)] == [S.TCP_HOSTREC_DTYPE.fields[n][1] for n in names]
    assert [S.TCP_HOSTREC_DTYPE.fields[n][0].itemsize for n in names] == [getattr(S.TcpHostRec, n).size for n in names]
    assert got[1 + len(names):] == [240, 224, 64, S.TCP_OPT_HOSTS]
    assert C.sizeof(S.TcpModel) == 240 and C.sizeof(S.TcpResult) == 224 and S.TCP_OPT_HOSTS == 8
    assert set(HE.FIELDS) == set(names) - {"_pad"}


def _model(**kw):
    c, m = TC.build("lossy_2pct")
    return TCPGPU.fill_model(m, TC.ip_ints(FIX["lossy_2pct"]["ips"]), c["procs"], c["peers"], np.full((1, 1), 50.0),
                             np.full((1, 1), 0.98), np.zeros(2, dtype=np.int32), c["nbytes"], **kw)


def test_fill_model_sets_the_option():
    assert int(_model()[0].options) == 0
    assert int(_model(hosts=True)[0].options) == S.TCP_OPT_HOSTS == 8
    tm, _ = _model(flows=True, paths=True, series_us=1000, hosts=True)
    assert int(tm.options) == 15   # the bit stands alone, beside the others


def test_result_hosts_refuses_null_arguments():
    recs, n = C.POINTER(S.TcpHostRec)(), C.c_uint64()
    res = S.TcpResult()   # never read: every call is refused before
    f = S.lib().shd_tcp_result_hosts
    assert f(None, C.byref(recs), C.byref(n)) == -22
    assert f(C.byref(res), None, C.byref(n)) == -22
    assert f(C.byref(res), C.byref(recs), None) == -22


def _as_array(name):
    """the fixture's rows as the library's array"""
    rows = FIX[name]["rows"]
    a = np.zeros(len(rows), dtype=S.TCP_HOSTREC_DTYPE)
    for j, k in enumerate(HE.SCALARS):
        a[k] = [r[j] for r in rows]
    a["sojourn_hist"] = [r[-1] for r in rows]
    return a


def test_the_array_round_trips_the_rows():
    for name in CASES:
        HE.check(_as_array(name), FIX[name]["rows"], name)


def test_merge_tcp_hosts_concatenates_in_rank_order():
    a = _as_array("hub40_slow")
    m = S.merge_tcp_hosts([a[:14], a[14:28], a[28:]])
    assert m.dtype == S.TCP_HOSTREC_DTYPE and m.tobytes() == a.tobytes()
    with pytest.raises(ValueError):
        S.merge_tcp_hosts([a[14:], a[:14]])   # not in rank order
    with pytest.raises(ValueError):
        S.merge_tcp_hosts([a[:14], a[28:]])   # a rank missing
    e = S.merge_tcp_hosts([])
    assert len(e) == 0 and e.dtype == S.TCP_HOSTREC_DTYPE


def test_write_hosts_csv(tmp_path):
    a = _as_array("slow_links")
    p = tmp_path / "hosts.csv"
    assert S.write_hosts_csv(p, a) == 2
    lines = p.read_text().splitlines()
    head = lines[0].split(",")
    assert head == list(S.HOSTS_CSV_FIELDS) and len(lines) == 3
    assert not any("pad" in k for k in head) and head[-16:] == ["sojourn_hist_%d" % i for i in range(16)]
    assert set(head[:-16]) == set(HE.SCALARS)
    for line, want in zip(lines[1:], FIX["slow_links"]["rows"]):
        r = dict(zip(head, line.split(",")))
        assert [int(r[k]) for k in HE.SCALARS] == want[:-1]
        assert [int(r["sojourn_hist_%d" % i]) for i in range(16)] == want[-1]
    assert S.write_hosts_csv(tmp_path / "none.csv", np.zeros(0, dtype=S.TCP_HOSTREC_DTYPE)) == 0
