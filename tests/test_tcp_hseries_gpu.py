"""The host records' series of the TCP path on the GPU (shd_tcp_model.options &
SHD_TCP_OPT_HOST_SERIES, shd_tcp_result_host_series; csrc/tcp.hip host_sample)
against the reference's own loop: at every (case, interval) pair of
tests/golden/ref_tcp_hseries.json the samples of an untraced run, with the path
cache on the device and on tables, have the fixture's count, per-host counts,
digest and stored rows (tests/eng_series_expect.py derives them from the
reference's [STATUS] lines).  Models without a fixture are compared with the
rows derived from the oracle's lines (oracle/o_tcp.c, pinned to the reference
on the CPU)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import eng_series_expect as SE
import oracle_ffi as O
import shdgpu as S
import tcp as TCPGPU
import tcp_cases as TC
import tcp_host_expect as HE
import tcp_hub_cases as TH
import workloads as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "ref_tcp_hseries.json")))
HOSTS = json.load(open(os.path.join(HERE, "golden", "ref_tcp_hosts.json")))
SEC, MS_NS = S.SHD_SEC, S.SHD_MS
PAIRS = [tuple(k.split("@")) for k in FIX if k != "fields"]
PAIRS = [(n, int(us)) for n, us in PAIRS]
IDS = ["%s@%d" % p for p in PAIRS]
# one pair per case also runs traced: the run's own lines derive its own samples
TRACED = [("hub40_slow", 100000), ("slow_links", 10000), ("mixed_slow_rr", 1000), ("hub12_fifo", 100000),
          ("geo_pairs", 1000000), ("loopback_pair", 10000), ("lossy_2pct", 1000)]
CUT_END = 3 * SEC + 500 * MS_NS   # tests/test_tcp_hosts_gpu.py's cut run of slow_links


def build(name):
    return TC.build(name) if name in TC.CASES else TH.build(name)


def _case_run(name, **kw):
    c, m = build(name)
    return TCPGPU.run(m, c["graph"], TC.ip_ints(HOSTS[name]["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                      qdisc=c.get("qdisc", 0), udp=TC.udp_arg(c), **kw)


@functools.lru_cache(maxsize=None)
def _run(name, us, trace, mode):
    """one run of a fixture case with host records and their series (computed once, never changed)"""
    return _case_run(name, mode=mode, trace=trace, hosts=True, host_series_us=us)


def _end(name):
    return int(build(name)[1].struct.end_time)


def _well_formed(s, interval_ns, end_ns, hosts):
    """sorted by (host, t) with no duplicate, labelled with boundaries before the end, padding zero"""
    assert s.dtype == S.HOST_SAMPLE_DTYPE
    keys = list(zip(s["rec"]["host"].tolist(), s["t"].tolist()))
    assert keys == sorted(set(keys))
    assert not s["rec"]["_pad"].any()
    if len(s):
        assert (s["t"] % np.uint64(interval_ns) == 0).all() and s["t"].min() > 0 and s["t"].max() < end_ns
        assert set(s["rec"]["host"].tolist()) <= set(hosts)
        r = s["rec"]
        assert (r["depth_end"] == r["router_enqueued"] - r["router_dequeued"] - r["router_dropped"]).all()


def _against_fixture(s, name, us, what):
    f = FIX["%s@%d" % (name, us)]
    H = len(HOSTS[name]["rows"])
    _well_formed(s, 1000 * us, _end(name), range(H))
    rows = SE.from_array(s)
    assert len(rows) == f["n"], (what, len(rows), f["n"])
    assert SE.per_host(rows, H) == f["per_host"], what
    for h, want in f.get("hosts", {}).items():
        SE.check(s[s["rec"]["host"] == int(h)], want, (what, "host", h))
    assert SE.digest(rows) == f["sha256"], what


@pytest.mark.parametrize("mode", ["device", "tables"])
@pytest.mark.parametrize("name,us", PAIRS, ids=IDS)
def test_samples_equal_the_reference(name, us, mode):
    r = _run(name, us, False, mode)
    assert r["lines"] == []
    _against_fixture(r["host_series"], name, us, (name, us, mode))
    h = r["hosts"]
    HE.check(h, HOSTS[name]["rows"], (name, us, mode, "records"))
    assert not h["_pad"].any()
    info = r["host_series_info"]
    assert info["capacity"] == 1 << 18 and info["peak"] <= len(r["host_series"])
    assert (info["drains"] > 0) == (info["peak"] > 0)


@pytest.mark.parametrize("name,us", TRACED, ids=["%s@%d" % p for p in TRACED])
def test_a_traced_run_derives_its_own_samples(name, us):
    r = _run(name, us, True, "device")
    assert len(r["lines"]) == HOSTS[name]["n_status"]
    _against_fixture(r["host_series"], name, us, (name, us, "traced"))
    want = SE.derive(r["lines"], len(r["hosts"]), 1000 * us, _end(name))
    SE.check(r["host_series"], want, (name, us, "own lines"))
    assert r["host_series"].tobytes() == _run(name, us, False, "device")["host_series"].tobytes()


@pytest.mark.parametrize("name,us", [("hub40_slow", 100000), ("lossy_2pct", 1000)])
def test_the_option_changes_nothing_else(name, us):
    on = _run(name, us, True, "device")
    off = _case_run(name, mode="device", trace=True, hosts=True)
    assert "host_series" not in off
    assert TC.digest(on["lines"]) == TC.digest(off["lines"]) and len(on["lines"]) == HOSTS[name]["n_status"]
    for k in ("events", "rounds", "deliveries"):
        assert on[k] == off[k], k
    for k in ("next_event_id", "next_packet_id", "rng_probe"):
        assert on[k].tolist() == off[k].tolist(), k
    assert on["hosts"].tobytes() == off["hosts"].tobytes()
    bare = _case_run(name, mode="device", trace=False, hosts=True)
    assert _run(name, us, False, "device")["hosts"].tobytes() == bare["hosts"].tobytes()
    for k in ("events", "rounds", "deliveries"):
        assert bare[k] == on[k], k


@pytest.mark.parametrize("name,us", [("hub40_slow", 100000), ("lossy_2pct", 1000), ("hub12_fifo", 100000)])
def test_every_option_at_once(name, us):
    """flows, paths, flow series (at 250 ms), hosts and host series (at its own
    interval) in one untraced run: each is what it is alone.  The two series
    share series_limit / series_cross; hub40_slow has CoDel drops, lossy_2pct
    losses and retransmissions."""
    al = _case_run(name, mode="device", trace=False, flows=True, paths=True, series_us=250000, hosts=True,
                   host_series_us=us)
    _against_fixture(al["host_series"], name, us, (name, "all options"))
    flows = _case_run(name, mode="device", trace=False, flows=True)
    paths = _case_run(name, mode="device", trace=False, paths=True)
    series = _case_run(name, mode="device", trace=False, series_us=250000)   # (implies flows: the series names them)
    assert len(al["flows"]) > 0 and al["flows"].tobytes() == flows["flows"].tobytes() == series["flows"].tobytes()
    assert len(al["paths"]) > 0 and al["paths"].tobytes() == paths["paths"].tobytes()
    assert len(al["series"]) > 0 and al["series"].tobytes() == series["series"].tobytes()
    assert al["series_info"] == series["series_info"]
    hosts = _case_run(name, mode="device", trace=False, hosts=True)
    assert al["hosts"].tobytes() == hosts["hosts"].tobytes()
    alone = _run(name, us, False, "device")
    assert al["hosts"].tobytes() == alone["hosts"].tobytes()
    assert al["host_series"].tobytes() == alone["host_series"].tobytes()
    assert al["host_series_info"] == alone["host_series_info"]
    for k in ("events", "rounds", "deliveries"):
        assert al[k] == alone[k] == flows[k], k


@functools.lru_cache(maxsize=None)
def _hub100(us):
    g, m, ips, procs, peers, nb = TH.hub100()
    return TCPGPU.run(m, g, ips, procs, peers, nbytes=nb, trace=False, hosts=True, host_series_us=us), \
        int(m.struct.end_time)


@pytest.mark.parametrize("us,n,lo,hi,onb", [(100000, 781, 1, 26, None), (1000, 2505, None, None, 1439)])
def test_two_blocks_appending_at_once(us, n, lo, hi, onb):
    """tcp_hub_cases.hub100: 100 hosts, two blocks of lanes appending to the one array"""
    r, end = _hub100(us)
    st = TH.hub100_oracle()["lines"]
    want = SE.derive(st, 100, 1000 * us, end)
    per = SE.per_host(want, 100)
    assert len(want) == n and (lo is None or (min(per), max(per)) == (lo, hi))
    assert onb is None or SE.on_boundary(st, 1000 * us) == onb
    s = r["host_series"]
    _well_formed(s, 1000 * us, end, range(100))
    SE.check(s, want, ("hub100", us))
    HE.check(r["hosts"], HE.rows(HE.derive(st, 100)), ("hub100", us, "records"))


def _raw(name, **kw):
    """one shd_tcp_run of a fixture case on its first-guess tables: (error, pointer set, n, samples, info)"""
    c, m = build(name)
    lat, rel, hvi, _ = TCPGPU.path_table(m, c["graph"], c["procs"], c["peers"])
    tm, keep = TCPGPU.fill_model(m, TC.ip_ints(HOSTS[name]["ips"]), c["procs"], c["peers"], lat, rel, hvi, c["nbytes"],
                                 **kw)
    res = C.POINTER(S.TcpResult)()
    rc = S.lib().shd_tcp_run(C.byref(tm), 0, C.byref(res))
    del keep
    assert rc == 0
    try:
        recs, n, info = C.POINTER(S.HostSample)(), C.c_uint64(99), S.TcpSeriesInfo(7, 7, 7)
        assert S.lib().shd_tcp_result_host_series(res, C.byref(recs), C.byref(n), C.byref(info)) == 0
        assert S.lib().shd_tcp_result_host_series(res, C.byref(recs), C.byref(n), None) == 0   # info is optional
        s, d = S.tcp_result_host_series(res)
        assert d == dict(drains=int(info.drains), peak=int(info.peak), capacity=int(info.capacity))
        return int(res.contents.error), bool(recs), int(n.value), s, d
    finally:
        S.lib().shd_tcp_result_free(res)


def test_drains_and_a_full_array():
    """slow_links at 1 ms: the array is emptied after every batch of rounds, so
    a capacity of the fullest drain carries the whole run; one record less and
    the append that finds it full sets SHD_TCP_ERR_HSERIES -- rc 0, no fault,
    and what is returned is whole rows of the full run"""
    err, have, n, s, info = _raw("slow_links", hosts=True, host_series_us=1000)
    assert (err, have, n) == (0, True, len(s))
    _against_fixture(s, "slow_links", 1000, "default capacity")
    assert info["capacity"] == 1 << 18 and info["drains"] > 1 and 1 < info["peak"] < len(s)
    peak = info["peak"]
    err, _, _, s2, info2 = _raw("slow_links", hosts=True, host_series_us=1000, host_series_cap=peak)
    assert err == 0 and s2.tobytes() == s.tobytes()
    assert info2 == dict(drains=info["drains"], peak=peak, capacity=peak)
    err, _, _, s3, info3 = _raw("slow_links", hosts=True, host_series_us=1000, host_series_cap=peak - 1)
    assert err & S.TCP_ERR_HSERIES and not err & ~S.TCP_ERR_HSERIES
    assert info3["capacity"] == peak - 1 and info3["peak"] <= peak - 1
    _well_formed(s3, 1000 * 1000, _end("slow_links"), range(2))
    full = {x.tobytes() for x in s}
    mine = [x.tobytes() for x in s3]
    assert 0 < len(mine) < len(s) and len(set(mine)) == len(mine) and set(mine) < full   # none duplicated, none torn


def test_a_run_cut_short():
    """slow_links ended at 3.5 s with the transfer running (tests/test_tcp_hosts_gpu.py's
    model): the last sample still has packets queued"""
    c, m = build("slow_links")
    m.struct.end_time = CUT_END
    ips = TC.ip_ints(HOSTS["slow_links"]["ips"])
    r = TCPGPU.run(m, c["graph"], ips, c["procs"], c["peers"], nbytes=c["nbytes"], trace=False, hosts=True,
                   host_series_us=100000)
    o = O.tcp_run(m, c["graph"], ips, c["procs"], c["peers"], nbytes=c["nbytes"])
    want = SE.derive(o["lines"], 2, 100 * MS_NS, CUT_END)
    s = r["host_series"]
    _well_formed(s, 100 * MS_NS, CUT_END, range(2))
    SE.check(s, want, "cut short")
    assert len(s) > 0 and s["t"].max() == CUT_END - 100 * MS_NS
    last = s[np.argmax(s["t"])]
    assert last["rec"]["depth_end"] > 0
    HE.check(r["hosts"], HE.rows(HE.derive(o["lines"], 2)), "cut short, records")


def test_series_starts_again_with_a_first_touch_rerun():
    """tests/test_tcp_hosts_gpu.py's model whose first touches contradict the
    lanes' choice, so that shd_tcp_run runs it again from the start: the
    samples are the last run's alone"""
    g, m, ips, _, _, nb = W.tcp_echo_model(2, 30, end_s=6, nbytes=30000)
    assert m.host_vertex[0] != m.host_vertex[1]
    procs = [(0, SEC), (1, SEC), (0, 2 * SEC + 10000), (1, 2 * SEC)]
    peers = [-1, -1, 1, 0]
    r = TCPGPU.run(m, g, ips, procs, peers, nbytes=nb, trace=False, hosts=True, host_series_us=100000)
    assert r["first_touch"] == "device" and r["first_touch_reruns"] >= 1
    o = O.tcp_run(m, g, ips, procs, peers, nbytes=nb)
    want = SE.derive(o["lines"], 2, 100 * MS_NS, 6 * SEC)
    assert len(want) > 2
    _well_formed(r["host_series"], 100 * MS_NS, 6 * SEC, range(2))
    SE.check(r["host_series"], want, "rerun")
    HE.check(r["hosts"], HE.rows(HE.derive(o["lines"], 2)), "rerun, records")


def run_ranks(world, case, us, mode, tmp_path, timeout=240):
    """`world` ranks of tests/tcp_hseries_group_worker.py on one GPU (at most 3)"""
    assert world <= 3
    name = "shdtcp_" + uuid.uuid4().hex[:16]
    procs = [subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "tcp_hseries_group_worker.py"), "--rank", str(r),
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


@pytest.mark.parametrize("world,mode", [(2, "tables"), (3, "device")])
@pytest.mark.parametrize("name", ["geo_pairs", "hub40_slow"])
def test_group_samples_merge_to_the_one_engine_array(name, world, mode, tmp_path):
    """shd_tcp_run_group over the host-memory communicator: each rank holds its
    own hosts' samples, nothing is exchanged, and merge_host_series of the
    ranks is the one-engine array"""
    res = run_ranks(world, name, 100000, mode, tmp_path)
    seen = 0
    for x in res:
        h0, nl = int(x["first_host"]), int(x["n_local_hosts"])
        s = x["host_series"]
        _well_formed(s, 100 * MS_NS, _end(name), range(h0, h0 + nl))
        seen += len(s) > 0
    assert seen >= 2
    merged = S.merge_host_series([x["host_series"] for x in res])
    _against_fixture(merged, name, 100000, (name, mode, world))
    assert merged.tobytes() == _run(name, 100000, False, mode)["host_series"].tobytes()
    hosts = S.merge_tcp_hosts([x["hosts"] for x in res])
    assert hosts.tobytes() == _run(name, 100000, False, mode)["hosts"].tobytes()


def test_a_model_without_the_option_has_no_samples():
    """the accessor on a run that did not set SHD_TCP_OPT_HOST_SERIES: NULL, 0 and a zeroed info"""
    err, have, n, s, info = _raw("lossy_2pct", hosts=True)
    assert (err, have, n, len(s)) == (0, False, 0, 0) and info == dict(drains=0, peak=0, capacity=0)
    err, have, n, s, info = _raw("lossy_2pct", hosts=True, host_series_us=100000)
    assert (err, have, n) == (0, True, 160)
    _against_fixture(s, "lossy_2pct", 100000, "raw")


def test_progress_and_csv(tmp_path):
    """host_progress fills a fixture host's sparse samples forward to a row per
    boundary, ending at the host's final record; write_host_series_csv writes
    every sample"""
    name, us = "hub40_slow", 100000
    r = _run(name, us, False, "device")
    s, end, Ins = r["host_series"], _end(name), 1000 * us
    for h in (0, 7):
        dense = S.host_progress(s, h, Ins, end)
        assert len(dense) == (end - 1) // Ins and dense["t"][-1] == ((end - 1) // Ins) * Ins
        assert dense["rec"][-1].tobytes() == r["hosts"][h].tobytes()   # the last row is the final record apart from t
        mine = s[s["rec"]["host"] == h]
        assert len(mine) == FIX["%s@%d" % (name, us)]["per_host"][h] < len(dense)
        assert (np.diff(dense["rec"]["router_enqueued"].astype(np.int64)) >= 0).all()
    n = S.write_host_series_csv(tmp_path / "hs.csv", s)
    text = (tmp_path / "hs.csv").read_text().splitlines()
    assert n == len(s) == len(text) - 1 and text[0].split(",") == list(S.HOST_SERIES_CSV_FIELDS)
