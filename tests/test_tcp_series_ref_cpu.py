"""The flow time series' fixture (tests/golden/ref_tcp_series.json) is the
reference's own loop's, derived by tests/tcp_series_expect.py; the oracle's
restatement (oracle/o_tcp.c) derives the same rows; and the C ABI's new pieces
(shd_tcp_sample, SHD_TCP_OPT_SERIES, shd_tcp_model.series_interval_us /
series_cap, shd_tcp_result_series) sit where include/shdtcp.h puts them, in
the model's two former padding words.  No device.

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
import tcp_flow_expect as FE
import tcp_hub_cases as TH
import tcp_series_expect as SE

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
FIX = json.load(open(os.path.join(HERE, "golden", "ref_tcp_series.json")))
FLOWS = json.load(open(os.path.join(HERE, "golden", "ref_tcp_flows.json")))
# what the issue sets: the cases and their intervals in microseconds
CASES = {"lossy_2pct": [250000, 1000], "heavy_loss": [250000], "geo_pairs": [250000], "loopback_pair": [1000],
         "mixed_hosts": [250000], "shared_hosts_rr": [100000], "hub12_fifo": [250000]}
RUNS = [(n, us) for n, v in CASES.items() for us in v]
LIVE = [("lossy_2pct", 1000), ("hub12_fifo", 250000)]


def build(name):
    return TC.build(name) if name in TC.CASES else TH.build(name)


def rows(name, us):
    return FIX[name]["series"][str(us)]["rows"]


def test_every_case_has_a_fixture():
    assert {n: sorted(int(us) for us in f["series"]) for n, f in FIX.items()} == {n: sorted(v) for n, v in CASES.items()}
    assert os.path.getsize(os.path.join(HERE, "golden", "ref_tcp_series.json")) < 100000
    for name, f in FIX.items():
        _, m = build(name)
        assert f["fields"] == list(SE.FIELDS), name
        assert f["end_ns"] == int(m.struct.end_time), name
        assert f["ips"] == FLOWS[name]["ips"] and f["n_flows"] == len(FLOWS[name]["flows"]), name
        for us, s in f["series"].items():
            assert all(len(r) == len(SE.FIELDS) for r in s["rows"]), (name, us)
            assert s["rows"] == sorted(s["rows"]), (name, us)


def test_fixture_is_not_vacuous():
    """the sample counts a derivation with the rule right gives, and the lines
    that sit exactly on a 1 ms boundary (they belong to the interval after)"""
    n = {(name, us): len(rows(name, us)) for name, us in RUNS}
    assert n[("lossy_2pct", 250000)] == 53 and n[("lossy_2pct", 1000)] == 269
    assert n[("heavy_loss", 250000)] == 68 and n[("geo_pairs", 250000)] == 258
    assert n[("loopback_pair", 1000)] == 66 and n[("mixed_hosts", 250000)] == 19
    assert n[("shared_hosts_rr", 100000)] > 0 and n[("hub12_fifo", 250000)] > 0
    f = FIX["lossy_2pct"]
    assert (f["series"]["1000"]["n_boundary_lines"], f["n_status"]) == (10969, 14735)


@pytest.mark.parametrize("name,us", RUNS)
def test_fixture_rows_follow_the_rule(name, us):
    """per record: boundaries strictly increasing, multiples of the interval,
    before the end; counters monotone and never past the flow record's; every
    record of the run has at least one sample unless it opened in the last
    interval"""
    I, end = us * 1000, FIX[name]["end_ns"]
    fl = FLOWS[name]["flows"]
    ci = [FE.PINNED.index(k) for k in SE.COUNTS]
    last = {}
    for r in rows(name, us):
        flow, t, cnt = r[0], r[1], r[2:]
        assert 0 <= flow < len(fl) and t % I == 0 and 0 < t < end, (name, r)
        if flow in last:
            assert t > last[flow][0] and all(a >= b for a, b in zip(cnt, last[flow][1])), (name, r)
            assert cnt != last[flow][1], (name, r)   # a sample exists because a counter moved
        assert all(a <= fl[flow][j] for a, j in zip(cnt, ci)), (name, r)
        assert t > fl[flow][FE.PINNED.index("t_open")], (name, r)
        last[flow] = (t, cnt)
    for i, f in enumerate(fl):
        if (f[FE.PINNED.index("t_open")] // I + 1) * I < end:
            assert i in last, (name, i)


@functools.lru_cache(maxsize=None)
def _oracle_lines(name):
    c, m = build(name)
    o = O.tcp_run(m, c["graph"], TC.ip_ints(FIX[name]["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                  qdisc=c.get("qdisc", 0), udp=TC.udp_arg(c))
    return o["lines"]


@pytest.mark.parametrize("name,us", RUNS)
def test_oracle_lines_derive_the_fixture(name, us):
    lines = _oracle_lines(name)
    end = FIX[name]["end_ns"]
    assert SE.derive(lines, us * 1000, end) == rows(name, us)
    # a record reads its own host's lines only: grouped by host the same rows come out
    assert SE.derive(TC.by_host(lines), us * 1000, end) == rows(name, us)


@pytest.mark.skipif(not R.available(), reason="oracle/_ref/libshdref_loop.so not built (needs the reference tree)")
@pytest.mark.parametrize("name,us", LIVE)
def test_reference_loop_reproduces_the_fixture(name, us):
    c, m = build(name)
    r = R.run(m, c["graph"], procs=c["procs"], tcp=TC.tcp_arg(c))
    st = TC.status_lines(r["lines"])
    assert r["ip"] == FIX[name]["ips"] and len(st) == FIX[name]["n_status"]
    assert SE.derive(st, us * 1000, FIX[name]["end_ns"]) == rows(name, us)
    assert SE.boundary_lines(st, us * 1000) == FIX[name]["series"][str(us)]["n_boundary_lines"]


def test_derivation_on_a_hand_made_trace():
    """the rule on six lines: a touch at a boundary belongs after it, an
    interval without a touch has no sample, RCV_SOCKET_PROCESSED does not
    touch, the last touch is sampled only when its boundary is before the end"""
    def ln(st, a, b, n, flags="ACK"):
        return f"[{st}] packetID=1:1 11.0.0.{a}:{1000 + a} -> 11.0.0.{b}:{1000 + b} seq=1 ack=1 sack=NA window=1 " \
               f"bytes={n} header={flags} status=x"
    lines = [(50, 0, ln("SND_CREATED", 1, 2, 0, "SYN")),
             (100, 0, ln("SND_CREATED", 1, 2, 10)),       # exactly on the boundary 100: sampled at 200
             (150, 0, ln("RCV_SOCKET_PROCESSED", 2, 1, 5)),
             (420, 0, ln("RCV_SOCKET_DELIVERED", 2, 1, 5)),
             (430, 0, ln("ROUTER_DROPPED", 2, 1, 7)),
             (910, 0, ln("SND_TCP_RETRANSMITTED", 1, 2, 10))]
    got =SE.derive(lines, 100, 1000)
    assert got == [[0, 100, 0, 1, 0, 0, 0, 0, 0], [0, 200, 0, 2, 10, 0, 0, 0, 0], [0, 500, 5, 2, 10, 0, 0, 0, 1]]
    assert SE.derive(lines, 100, 1001)[-1] == [0, 1000, 5, 2, 10, 1, 0, 0, 1]
    assert SE.derive(lines, 2000, 1000) == []


def test_sample_struct_layout_matches_the_header(tmp_path):
    """the ctypes mirrors and the dtype against gcc's layout: shd_tcp_sample is
    96 bytes, the model and the result kept their sizes, and the two new model
    fields sit in the former padding words"""
    names = [n for n, _ in S.TcpSample._fields_]
    assert names == list(S.TCP_SAMPLE_DTYPE.names)
    src = tmp_path / "s.c"
    body = "".join('printf("%%zu\\n", offsetof(shd_tcp_sample, %s));' % n for n in names)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s/include/shdtcp.h"\n'
                   'int main(void){printf("%%zu\\n", sizeof(shd_tcp_sample));%s'
                   'printf("%%zu %%zu %%zu %%zu %%zu %%d %%d\\n", sizeof(shd_tcp_model), sizeof(shd_tcp_result),'
                   ' offsetof(shd_tcp_model, series_cap), offsetof(shd_tcp_model, series_interval_us),'
                   ' sizeof(shd_tcp_series_info), (int)SHD_TCP_OPT_SERIES, (int)SHD_TCP_ERR_SERIES);return 0;}\n'
                   % (REPO, body))
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-Wall", "-Werror", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(S.TcpSample) == S.TCP_SAMPLE_DTYPE.itemsize == 96
    assert got[1:1 + len(names)] == [getattr(S.TcpSample, n).offset for n in names]
    assert got[1:1 + len(names)] == [S.TCP_SAMPLE_DTYPE.fields[n][1] for n in names]
    assert [S.TCP_SAMPLE_DTYPE.fields[n][0].itemsize for n in names] == [getattr(S.TcpSample, n).size for n in names]
    T = S.TcpModel
    assert got[1 + len(names):] == [240, 224, T.series_cap.offset, T.series_interval_us.offset,
                                    C.sizeof(S.TcpSeriesInfo), S.TCP_OPT_SERIES, S.TCP_ERR_SERIES]
    assert C.sizeof(T) == 240 and C.sizeof(S.TcpResult) == 224
    assert T.series_cap.offset == T.n_classes.offset + 4 and T.pcap_host.offset == T.series_cap.offset + 4
    assert T.series_interval_us.offset == T.pcap_ring.offset + 4
    assert T.bootstrap_end.offset == T.series_interval_us.offset + 4
    assert (S.TCP_OPT_SERIES, S.TCP_ERR_SERIES) == (4, 4096)


def _model(**kw):
    c, m = TC.build("lossy_2pct")
    return TCPGPU.fill_model(m, TC.ip_ints(FIX["lossy_2pct"]["ips"]), c["procs"], c["peers"], np.full((1, 1), 50.0),
                             np.full((1, 1), 0.98), np.zeros(2, dtype=np.int32), c["nbytes"], **kw)


def test_fill_model_sets_the_option():
    assert int(_model()[0].options) == 0
    tm, _ = _model(flows=True, series_us=250000, series_cap=77)
    assert int(tm.options) == S.TCP_OPT_FLOWS | S.TCP_OPT_SERIES == 5
    assert (int(tm.series_interval_us), int(tm.series_cap)) == (250000, 77)


def test_the_bit_alone_is_refused():
    """SHD_TCP_OPT_SERIES without SHD_TCP_OPT_FLOWS, or without an interval: an
    invalid model (-22), decided before anything touches a device"""
    for kw, interval in ((dict(flows=False, series_us=1000), 1000), (dict(flows=True, series_us=1000), 0)):
        tm, keep = _model(**kw)
        tm.series_interval_us = interval
        assert int(tm.options) & S.TCP_OPT_SERIES
        res = C.POINTER(S.TcpResult)()
        assert S.lib().shd_tcp_run(C.byref(tm), 0, C.byref(res)) == -22
        assert not res
        del keep


def test_result_series_refuses_null_arguments():
    recs, n, info = C.POINTER(S.TcpSample)(), C.c_uint64(), S.TcpSeriesInfo()
    res = S.TcpResult()   # never read: every call is refused before
    f = S.lib().shd_tcp_result_series
    assert f(None, C.byref(recs), C.byref(n), C.byref(info)) == -22
    assert f(C.byref(res), None, C.byref(n), C.byref(info)) == -22
    assert f(C.byref(res), C.byref(recs), None, None) == -22


def _as_arrays(name, us):
    """the fixture's flow records and samples as the library's arrays"""
    fl = np.zeros(len(FLOWS[name]["flows"]), dtype=S.TCP_FLOW_DTYPE)
    for j, k in enumerate(FE.PINNED):
        fl[k] = [r[j] for r in FLOWS[name]["flows"]]
    se = np.zeros(len(rows(name, us)), dtype=S.TCP_SAMPLE_DTYPE)
    for j, k in enumerate(SE.FIELDS):
        se[k] = [r[j] for r in rows(name, us)]
    return fl, se


@pytest.mark.parametrize("name,us", RUNS)
def test_flow_progress_ends_at_the_flow_record(name, us):
    fl, se = _as_arrays(name, us)
    I, end = us * 1000, FIX[name]["end_ns"]
    p = S.flow_progress(se, fl, I, end)
    K = (end - 1) // I
    assert p.shape == (len(fl), K + 1) and p.dtype == np.uint64
    assert p[:, -1].tolist() == fl["bytes_delivered"].tolist()
    assert (np.diff(p.astype(np.int64), axis=1) >= 0).all()   # forward-filled cumulative curves
    for r in rows(name, us):   # every sample sits in its boundary's column
        assert p[r[0], r[1] // I - 1] == r[2]
    # the last boundary's column already holds the end state wherever the record's last touch was sampled
    sampled_last = {r[0]: r[2] for r in rows(name, us)}
    for i in range(len(fl)):
        if K:
            assert p[i, K - 1] == sampled_last.get(i, 0)


def test_merge_tcp_series_offsets_the_flow_index():
    fl, se = _as_arrays("geo_pairs", 250000)
    cut = 7   # records [0, 7) on rank 0, the rest on rank 1
    a = (fl[:cut], se[se["flow"] < cut])
    s1 = se[se["flow"] >= cut].copy()
    s1["flow"] -= cut
    mf, ms = S.merge_tcp_series([a, (fl[cut:], s1)])
    assert mf.tobytes() == fl.tobytes() and ms.tobytes() == se.tobytes()
    mf, ms = S.merge_tcp_series([])
    assert len(mf) == 0 and len(ms) == 0 and ms.dtype == S.TCP_SAMPLE_DTYPE


def test_write_series_csv(tmp_path):
    a = np.zeros(2, dtype=S.TCP_SAMPLE_DTYPE)
    a["t"] = [250 * 10**6, 500 * 10**6]
    a["flow"] = [0, 3]
    a["host"] = [1, 2]
    a["bytes_delivered"] = [2**40, 7]
    a["srtt"] = [-1, 100]
    a["state"] = [4, 8]
    p = tmp_path / "series.csv"
    assert S.write_series_csv(p, a) == 2
    lines = p.read_text().splitlines()
    assert lines[0].split(",") == list(S.SERIES_CSV_FIELDS) and "_pad" not in lines[0] and len(lines) == 3
    r0 = dict(zip(S.SERIES_CSV_FIELDS, lines[1].split(",")))
    r1 = dict(zip(S.SERIES_CSV_FIELDS, lines[2].split(",")))
    assert (r0["t"], r0["flow"], r0["bytes_delivered"], r0["srtt"], r0["state"]) == \
        ("250000000", "0", str(2**40), "-1", "ESTABLISHED")
    assert (r1["host"], r1["state"]) == ("2", "TIMEWAIT")
    assert S.write_series_csv(tmp_path / "none.csv", np.zeros(0, dtype=S.TCP_SAMPLE_DTYPE)) == 0
