"""The TCP path's host-record series (shd_tcp_model.options &
SHD_TCP_OPT_HOST_SERIES, shd_host_sample, shd_tcp_result_host_series) without a
device: the fixture tests/golden/ref_tcp_hseries.json is the reference's own
loop's (tests/golden/make_ref_tcp_hseries.py), what tests/eng_series_expect.py
derives from its [STATUS] lines at thirteen (case, interval) pairs; the
oracle's restatement (oracle/o_tcp.c) derives the same rows wherever it
reproduces the reference's lines; the one-pass derivation is the brute-force
definition; and the C ABI's new pieces sit where include/shdtcp.h puts them and
refuse what the header says they refuse, before any device call.

hub40_slow: the oracle's lines differ from the reference's there
(tcp_hub_cases.ORACLE_COUNTERS -- its dequeues do not follow the queue's order,
so the derivation does not apply to them): the reference fixture alone pins the
case's two pairs, here where the reference's loop is built and on the device in
tests/test_tcp_hseries_gpu.py."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import eng_series_expect as SE
import oracle_ffi as O
import ref_loop_ffi as R
import shdgpu as S
import tcp as TCPGPU
import tcp_cases as TC
import tcp_host_expect as HE
import tcp_hub_cases as TH

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_ref_tcp_hseries as GEN  # noqa: E402

FIX = json.load(open(os.path.join(HERE, "golden", "ref_tcp_hseries.json")))
HOSTS = json.load(open(os.path.join(HERE, "golden", "ref_tcp_hosts.json")))
MS = 1000
PAIRS = list(GEN.PAIRS)
IDS = [GEN.key(*p) for p in PAIRS]
ORACLE = [p for p in PAIRS if p[0] not in TH.ORACLE_COUNTERS]


def test_every_pair_has_a_fixture():
    """the issue's table: samples, the fewest and the most of a host, counted lines on a boundary"""
    assert sorted(k for k in FIX if k != "fields") == sorted(IDS) and len(IDS) == 13
    assert FIX["fields"] == list(SE.FIELDS)
    assert os.path.getsize(os.path.join(HERE, "golden", "ref_tcp_hseries.json")) < 100000
    for (name, us), (n, lo, hi, onb) in GEN.PAIRS.items():
        f = FIX[GEN.key(name, us)]
        assert f["n"] == n == sum(f["per_host"]) and f["interval_us"] == us, (name, us)
        assert len(f["per_host"]) == len(HOSTS[name]["rows"]), (name, us)
        assert (min(f["per_host"]), max(f["per_host"])) == (lo, hi), (name, us)
        assert onb is None or f["on_boundary"] == onb, (name, us)
        assert ("hosts" in f) == (us == 100 * MS)
    hub = FIX["hub40_slow@100000"]
    assert hub["deepest"] == 0 and hub["per_host"][0] == 33 and list(hub["hosts"]) == ["0"]
    # the one boundary of slow_links at 60 s is end_time: no sample
    assert FIX["slow_links@60000000"]["n"] == 0
    lo = FIX["loopback_pair@10000"]   # one host, its packets never see the router
    assert lo["per_host"] == [7]
    # the 1 ms pairs decide "an event at exactly T_k belongs to the interval after it"
    assert min(FIX[k]["on_boundary"] for k in IDS if k.endswith("@1000")) >= 1932


@functools.lru_cache(maxsize=None)
def oracle_lines(name):
    """the case's lines from the oracle (computed once, never changed): (lines, hosts, end_time)"""
    c, m = GEN.build(name)
    o = O.tcp_run(m, c["graph"], TC.ip_ints(HOSTS[name]["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                  qdisc=c.get("qdisc", 0), udp=TC.udp_arg(c))
    return o["lines"], len(c["hv"]), int(m.struct.end_time)


@pytest.mark.parametrize("name,us", ORACLE, ids=[GEN.key(*p) for p in ORACLE])
def test_oracle_lines_derive_the_fixture(name, us):
    st, H, end = oracle_lines(name)
    f = FIX[GEN.key(name, us)]
    rows = SE.derive(st, H, 1000 * us, end)
    assert len(rows) == f["n"] and SE.per_host(rows, H) == f["per_host"] and SE.digest(rows) == f["sha256"]
    assert SE.on_boundary(st, 1000 * us) == f["on_boundary"]
    for h, want in f.get("hosts", {}).items():
        assert [r for r in rows if r[1] == int(h)] == want, (name, us, h)
    # the last sample of a host whose final interval ends before end_time is its final record
    final = HOSTS[name]["rows"]
    for h in range(H):
        mine = [r for r in rows if r[1] == h]
        t_last = final[h][HE.SCALARS.index("t_last")]
        if mine and (t_last // (1000 * us) + 1) * 1000 * us < end:
            assert mine[-1][1:] == final[h], (name, us, h)


@pytest.mark.parametrize("name,us", [("slow_links", 10 * MS), ("mixed_slow_rr", 100 * MS)])
def test_one_pass_rows_are_the_prefix_records(name, us):
    """the brute-force definition: sample (h, T) = tcp_host_expect.derive(lines
    with t < T)[h], depth_end the queue's length then"""
    st, H, end = oracle_lines(name)
    Ins = 1000 * us
    rows = SE.derive(st, H, Ins, end)
    assert len(rows) == FIX[GEN.key(name, us)]["n"] > 0
    prefix = {}
    for r in rows:
        T, h = r[0], r[1]
        if T not in prefix:
            prefix[T] = HE.rows(HE.derive([x for x in st if x[0] < T], H))
        assert r[1:] == prefix[T][h], (T, h)
        assert T % Ins == 0 and 0 < T < end
    assert [(r[1], r[0]) for r in rows] == sorted({(r[1], r[0]) for r in rows})   # sorted by (host, t), no duplicate
    touched = {(h, (t // Ins + 1) * Ins) for t, h, b in st if b[1:b.index("]")] in HE.COUNTED}
    assert {(r[1], r[0]) for r in rows} == {x for x in touched if x[1] < end}


@pytest.mark.skipif(not R.available(), reason="oracle/_ref/libshdref_loop.so not built (needs the reference tree)")
def test_generator_reproduces_the_committed_fixture():
    got = GEN.entries()
    assert sorted(got) == sorted(IDS)
    for k in IDS:
        assert got[k] == FIX[k], k


def _snippet(tmp_path, body):
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s/include/shdtcp.h"\n'
                   'int main(void){%s return 0;}\n' % (REPO, body))
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-Wall", "-Werror", str(src), "-o", str(exe)], check=True)
    return [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]


def test_the_interface_matches_the_header(tmp_path):
    """the enum values and the two fields' offsets against gcc; the model, the
    result and the sample keep their sizes"""
    got = _snippet(tmp_path, 'printf("%d %d %zu %zu %zu %zu %zu %zu\\n", (int)SHD_TCP_OPT_HOST_SERIES,'
                             ' (int)SHD_TCP_ERR_HSERIES, offsetof(shd_tcp_model, host_series_interval_us),'
                             ' offsetof(shd_tcp_model, host_series_cap), sizeof(shd_tcp_model), sizeof(shd_tcp_result),'
                             ' sizeof(shd_host_sample), offsetof(shd_host_sample, rec));')
    T = S.TcpModel
    assert got == [S.TCP_OPT_HOST_SERIES, S.TCP_ERR_HSERIES, T.host_series_interval_us.offset, T.host_series_cap.offset,
                   C.sizeof(T), C.sizeof(S.TcpResult), C.sizeof(S.HostSample), S.HostSample.rec.offset]
    assert (S.TCP_OPT_HOST_SERIES, S.TCP_ERR_HSERIES) == (16, 8192)
    assert S.HOST_SAMPLE_DTYPE.itemsize == C.sizeof(S.HostSample) == 240
    assert T.host_series_interval_us.size == T.host_series_cap.size == 4
    assert "shd_tcp_result_host_series" in S._SIGS


def _model(end_time=0, **kw):
    c, m = TC.build("lossy_2pct")
    if end_time:
        m.struct.end_time = end_time
    return TCPGPU.fill_model(m, TC.ip_ints(HOSTS["lossy_2pct"]["ips"]), c["procs"], c["peers"], np.full((1, 1), 50.0),
                             np.full((1, 1), 0.98), np.zeros(2, dtype=np.int32), c["nbytes"], **kw)


def test_fill_model_sets_the_option():
    assert int(_model(hosts=True)[0].options) == S.TCP_OPT_HOSTS
    tm, _ = _model(hosts=True, host_series_us=250000, host_series_cap=77)
    assert int(tm.options) == S.TCP_OPT_HOSTS | S.TCP_OPT_HOST_SERIES == 24
    assert (int(tm.host_series_interval_us), int(tm.host_series_cap)) == (250000, 77)
    tm, _ = _model(flows=True, paths=True, series_us=1000, hosts=True, host_series_us=1000)
    assert int(tm.options) == 31   # the bit stands beside the others


def _refused(tm):
    res = C.POINTER(S.TcpResult)()
    rc = S.lib().shd_tcp_run(C.byref(tm), 0, C.byref(res))
    assert not res
    return rc


def test_invalid_models_are_refused_before_any_device_call():
    """-22 for the bit without SHD_TCP_OPT_HOSTS, a zero interval, end_time / I
    >= 2^32 and a capacity above 2^24 (this machine needs no device for it)"""
    tm, keep = _model(host_series_us=1000)   # the bit alone
    assert int(tm.options) == S.TCP_OPT_HOST_SERIES and _refused(tm) == -22
    tm, keep = _model(hosts=True, host_series_us=1000)
    tm.host_series_interval_us = 0
    assert int(tm.options) & S.TCP_OPT_HOST_SERIES and _refused(tm) == -22
    tm, keep = _model(end_time=1000 << 32, hosts=True, host_series_us=1)   # I = 1000 ns: end_time / I = 2^32
    assert _refused(tm) == -22
    tm, keep = _model(hosts=True, host_series_us=1000, host_series_cap=(1 << 24) + 1)
    assert _refused(tm) == -22
    del keep


def test_result_host_series_refuses_null_arguments():
    recs, n, info = C.POINTER(S.HostSample)(), C.c_uint64(), S.TcpSeriesInfo()
    res = S.TcpResult()   # never read: every call is refused before
    f = S.lib().shd_tcp_result_host_series
    assert f(None, C.byref(recs), C.byref(n), C.byref(info)) == -22
    assert f(C.byref(res), None, C.byref(n), C.byref(info)) == -22
    assert f(C.byref(res), C.byref(recs), None, None) == -22
