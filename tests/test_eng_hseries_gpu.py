"""The host records' per-interval series of the packet engine
(SHD_QF_HOST_SERIES, shd_eng_host_series) on the device, against the
reference's own loop.

tests/golden/ref_eng_hseries.json holds what tests/eng_series_expect.py derives
from the reference loop's [STATUS] lines at ten (case, interval) pairs.  The
engine runs the same models UNTRACED with the two flags alone and must return
those samples; the flag must change nothing else of a run; every round-kernel
family, the chunked run calls, a group of engines, and the rollback and replay
of rounds must give the same samples.

Shapes: the cases are the fixture's (40-100 hosts, 3 s, each a few seconds);
`backlog` (eng_hosts_cases.py: 400 hosts, several blocks appending at once) is
the two-block and rollback model.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import eng_hosts_cases as EC
import eng_hseries_cases as SC
import eng_series_expect as SE
import oracle_ffi as O
import ref_loop_cases as RC
import shdgpu as S
import tcp_host_expect as HE
import workloads as W
from test_eng_hosts_gpu import rows_from_trace

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "ref_eng_hseries.json")) as f:
    FIX = json.load(f)
with open(os.path.join(HERE, "golden", "ref_eng_hosts.json")) as f:
    HOSTS = json.load(f)
MS = 1000
PAIRS = [("codel", 100 * MS), ("udp_echo_codel", 100 * MS), ("udp_mix_codel", 100 * MS), ("bootstrap", 100 * MS),
         ("phold_v100", 100 * MS), ("codel", 1 * MS), ("udp_mix_codel", 1 * MS), ("bootstrap", 10 * MS),
         ("phold_v100", 1000 * MS), ("udp_echo_codel", 5000 * MS)]
IDS = ["%s@%d" % p for p in PAIRS]
FAMILIES = [("codel", 10 * MS), ("phold_v100", 100 * MS)]
ENV_SWITCHES = ("SHD_NO_PS", "SHD_NO_TL", "SHD_SP_HOSTS", "SHD_PS_BATCH", "SHDGPU_LIB", "SHD_FORCE_AMBIG",
                "SHD_PROTECT_ALL", "SHD_NO_PROTECT", "SHD_SNAP_NO_DEVICE", "SHD_HOST_SERIES_CAP")
TH = os.path.join(os.path.dirname(HERE), "shadow-1_amd", "libshdgpu_th.so")

_untraced = {}


def untraced(name, us):
    """the pair untraced, with the two flags alone, on the default kernel
    selection and capacity: dict(samples, records, digest, tot, info), once"""
    if (name, us) not in _untraced:
        g, m, pushes = SC.case(name, us)
        r = SC.run(g, m, pushes)
        assert len(r["trace"]) == 0
        r.pop("engine").close()
        for k in ("samples", "records", "digest"):
            r[k].setflags(write=False)
        _untraced[name, us] = r
    return _untraced[name, us]


def check_order(a):
    key = list(zip(a["rec"]["host"].tolist(), a["t"].tolist()))
    assert key == sorted(set(key))   # sorted by (host, t), no duplicate


def run_child(name, us, steps, tmp_path, timeout=180, **env_set):
    env = {k: v for k, v in os.environ.items() if k not in ENV_SWITCHES}
    env.update(env_set)
    out = os.path.join(tmp_path, f"{name}.npz")
    p = subprocess.run([sys.executable, "-u", os.path.join(HERE, "eng_hseries_worker.py"), name, str(us), str(steps),
                        out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    text = p.stdout.decode(errors="replace")
    assert p.returncode == 0, text[-3000:]
    print(text.strip().splitlines()[-1])
    z = np.load(out)
    return z["samples"], z["records"], z["digest"], json.loads(text.strip().splitlines()[-1])


# ---- 1. the reference pin, untraced ----
@pytest.mark.parametrize("name,us", PAIRS, ids=IDS)
def test_untraced_samples_are_the_references(name, us):
    r, f = untraced(name, us), FIX["%s@%d" % (name, us)]
    a = r["samples"]
    rows = SE.from_array(a)
    H = len(f["per_host"])
    print(name, us, len(a), r["info"])
    assert r["tot"]["n_pkt_events"] > 0
    check_order(a)
    assert len(a) == f["n"]
    assert SE.per_host(rows, H) == f["per_host"]
    assert SE.digest(rows) == f["sha256"]
    for h, want in f.get("hosts", {}).items():
        SE.check(a[a["rec"]["host"] == int(h)], want, (name, us, h))
    assert r["info"]["samples"] <= len(a) and r["info"]["peak"] <= r["info"]["capacity"] == 1 << 18
    # the series leaves the records alone
    HE.check(r["records"], HOSTS[name]["rows"], name)


# ---- 2. the option changes nothing else ----
@pytest.mark.parametrize("name", EC.CASES)
def test_the_option_changes_nothing_else(name):
    """the case's own flags (trace, status trace, heartbeats) with and without
    the series: the same digest, trace, heartbeats, event counts and records;
    the samples are (1)'s and what the engine's own status lines derive"""
    us = 100 * MS
    flags = int(RC.CASES[name]()["model"].params["queue_flags"])
    g, m1, pushes = SC.case(name, us, True, flags | SC.HS)
    r1 = SC.run(g, m1, pushes)
    eng1 = r1.pop("engine")
    lines = sorted(eng1.status_lines(HOSTS[name]["ips"]), key=lambda x: (x[0], x[1]))
    hb1 = eng1.heartbeats()
    eng1.close()
    _, m0, _ = SC.case(name, us, True, flags | EC.HR)   # the interval alone is ignored
    r0 = SC.run(g, m0, pushes)
    eng0 = r0.pop("engine")
    hb0 = eng0.heartbeats()
    n = C.c_uint64(7)
    buf = np.zeros(4, dtype=S.HOST_SAMPLE_DTYPE)
    assert S.lib().shd_eng_host_series(eng0.ptr, buf.ctypes.data, 4, C.byref(n)) == -22   # refused without the flag
    eng0.close()
    assert np.array_equal(r1["digest"], r0["digest"]) and np.array_equal(r1["trace"], r0["trace"])
    assert np.array_equal(hb1, hb0)
    assert (r1["tot"]["n_events"], r1["tot"]["n_pkt_events"]) == (r0["tot"]["n_events"], r0["tot"]["n_pkt_events"])
    assert r1["records"].tobytes() == r0["records"].tobytes()
    want = untraced(name, us)
    assert np.array_equal(r1["digest"], want["digest"])
    assert r1["samples"].tobytes() == want["samples"].tobytes()
    assert len(lines) == HOSTS[name]["n_status"]
    SE.check(r1["samples"], SE.derive(lines, int(m1.n_hosts), 1000 * us, int(m1.params["end_time"])), name)


# ---- 3. every round-kernel family ----
@pytest.mark.parametrize("name,us", FAMILIES)
def test_launch_per_round_kernels(name, us, tmp_path):
    """SHD_NO_PS=1 (k_round_tl<false> and the ticketed k_round_dev), and with
    SHD_NO_TL=1 the ticketed kernels alone; read once a process: a child each"""
    want = untraced(name, us)
    a, _, dg, st = run_child(name, us, 1, tmp_path, SHD_NO_PS="1")
    assert st["n_batches_persistent"] == 0 and st["n_batches_ticketless"] > 0
    assert a.tobytes() == want["samples"].tobytes() and np.array_equal(dg, want["digest"])
    a, _, dg, st = run_child(name, us, 1, tmp_path, SHD_NO_PS="1", SHD_NO_TL="1")
    assert st["n_batches_persistent"] == 0 and st["n_batches_ticketless"] == 0 and st["n_batches"] > 0
    assert a.tobytes() == want["samples"].tobytes() and np.array_equal(dg, want["digest"])


@pytest.mark.parametrize("name,us", FAMILIES)
def test_persistent_sparse_host_driven_and_stepped(name, us, monkeypatch):
    want = untraced(name, us)
    assert want["tot"]["n_batches_persistent"] > 0 and want["tot"]["n_batches_sparse"] == 0   # k_round_ps<false>
    assert len(want["samples"]) > 0
    g, m, pushes = SC.case(name, us)
    # the default's samples are what the oracle's lines derive (no fixture at codel's 10 ms)
    c = RC.CASES[name]()
    tr, _, _ = O.engine_run(c["model"], c["graph"], pushes=c.get("pushes"))
    st = sorted(S.status_lines(tr, HOSTS[name]["ips"], payload=int(m.struct.payload), app_peer=m.status_peer),
                key=lambda x: (x[0], x[1]))
    SE.check(want["samples"], SE.derive(st, int(m.n_hosts), 1000 * us, int(m.params["end_time"])), name)
    # the host drives every round (shd_eng_run_round: k_round)
    r = SC.run(g, m, pushes, rounds=True)
    r.pop("engine").close()
    assert r["tot"]["n_pkt_events"] == want["tot"]["n_pkt_events"] and r["error"] == 0
    assert r["samples"].tobytes() == want["samples"].tobytes() and np.array_equal(r["digest"], want["digest"])
    # run_until in three unequal steps: each step's read is the full run's rows with T <= that stop
    r = SC.run(g, m, pushes, steps=3)
    again = r["engine"].host_series()   # the call reads, it does not reset
    r.pop("engine").close()
    assert r["samples"].tobytes() == want["samples"].tobytes() == again.tobytes()
    assert np.array_equal(r["digest"], want["digest"])
    assert len(r["reads"]) == 3
    for stop, part in r["reads"]:
        full = want["samples"][want["samples"]["t"] <= stop]
        assert part.tobytes() == full.tobytes(), (name, stop, len(part), len(full))
    # (the first step stops before the application starts at 1 s)
    assert 0 == len(r["reads"][0][1]) < len(r["reads"][1][1]) < len(want["samples"])
    # the sparse persistent kernel (k_round_sp<false>), blocks of 64 hosts
    monkeypatch.setenv("SHD_SP_HOSTS", "64")
    r = SC.run(g, m, pushes)
    r.pop("engine").close()
    assert r["tot"]["n_batches_sparse"] > 0
    assert r["samples"].tobytes() == want["samples"].tobytes() and np.array_equal(r["digest"], want["digest"])


# ---- 4. chunking ----
def test_one_interval_a_chunk(monkeypatch):
    """SHD_HOST_SERIES_CAP=60 on 60 hosts: q = 1, a chunk per interval -- the
    default capacity's samples, digest and event count, and no error bit"""
    want = untraced("codel", 10 * MS)
    assert want["info"]["chunks"] == 0
    g, m, pushes = SC.case("codel", 10 * MS)
    monkeypatch.setenv("SHD_HOST_SERIES_CAP", "60")
    r = SC.run(g, m, pushes)
    r.pop("engine").close()
    print(r["info"])
    assert r["info"]["capacity"] == 60 and r["info"]["peak"] <= 60
    assert r["info"]["chunks"] == 299   # the boundaries before 3 s
    assert r["samples"].tobytes() == want["samples"].tobytes() and np.array_equal(r["digest"], want["digest"])
    assert (r["tot"]["n_events"], r["tot"]["n_pkt_events"]) == (want["tot"]["n_events"], want["tot"]["n_pkt_events"])
    monkeypatch.setenv("SHD_HOST_SERIES_CAP", "59")   # below the local hosts
    from sim import Engine, PathCache
    with pytest.raises(S.ShdError, match="-22"):
        Engine(m, PathCache(g, W.attached_vertices(m.host_vertex)))


def test_host_driven_rounds_with_a_short_capacity(monkeypatch):
    """the host drives the rounds, so its windows decide what a round appends:
    with the array one sample short of the fullest round the run ends with
    SHD_ERR_HOST_SERIES, and what it returns is still rows of the full run --
    none duplicated, none torn"""
    name, us = "codel", 1 * MS
    want = untraced(name, us)   # (1) pins it to the fixture
    g, m, pushes = SC.case(name, us)
    r = SC.run(g, m, pushes, rounds=True)
    r.pop("engine").close()
    assert r["samples"].tobytes() == want["samples"].tobytes() and r["error"] == 0
    peak = r["info"]["peak"]
    print("host-driven rounds:", r["info"])
    assert peak - 1 >= int(m.n_hosts), (peak, "no round fills more than a sample a host")
    monkeypatch.setenv("SHD_HOST_SERIES_CAP", str(peak - 1))
    r = SC.run(g, m, pushes, rounds=True, stop_on_error=True)
    r.pop("engine").close()
    assert r["error"] & S.ERR_HOST_SERIES, hex(r["error"])
    got = r["samples"]
    check_order(got)
    rows = {(x[1], x[0]): x for x in SE.from_array(want["samples"])}
    assert 0 < len(got) < len(want["samples"])
    for x in SE.from_array(got):
        assert rows.get((x[1], x[0])) == x, x[:3]


# ---- 5. two blocks, and rounds that run twice ----
_backlog = {}


def backlog_rows(us):
    """the backlog model's expected samples from the oracle's trace: rows_from_trace
    on the trace before each boundary, for the hosts touched in the interval"""
    if us not in _backlog:
        g, m = EC.backlog(True, 0)
        tr, dg, _ = O.engine_run(m, g)
        dg.setflags(write=False)
        H, end, Ins = int(m.n_hosts), int(m.params["end_time"]), 1000 * us
        counted = np.isin(tr["kind"], (S.TR_ARRIVE, S.TR_CODEL_DROP, S.TR_RECV, S.TR_IF_DROP, S.TR_SENT,
                                       S.TR_INET_DROP, S.TR_LOCAL))
        per = [[] for _ in range(H)]
        for T in range(Ins, end, Ins):
            if T >= end:
                break
            hit = counted & (tr["time"] >= T - Ins) & (tr["time"] < T)
            hosts = np.unique(tr["host"][hit]).tolist()
            if not hosts:
                continue
            rows = rows_from_trace(tr[tr["time"] < T], H, 1500)
            for h in hosts:
                per[h].append([T] + rows[h])
        _backlog[us] = ([r for p in per for r in p], dg)
    return _backlog[us]


def test_two_blocks_append_at_once():
    rows, odg = backlog_rows(100 * MS)
    g, m, _ = SC.case("backlog", 100 * MS)
    r = SC.run(g, m)
    r.pop("engine").close()
    assert np.array_equal(r["digest"], odg)
    assert len(rows) > 400 * 10
    SE.check(r["samples"], rows, "backlog")


@pytest.mark.parametrize("setting", ["rollback", "replay", "snap_host"])
def test_rerun_rounds_sample_once(setting, tmp_path):
    """test_eng_hosts_gpu.test_rerun_rounds_count_once's three settings: rounds
    rolled back and rerun, rounds replayed from the last restore point over
    three run_until steps, and the state copy in host memory"""
    env, steps = dict(SHDGPU_LIB=TH), 1
    if setting == "rollback":
        env.update(SHD_PROTECT_ALL="1", SHD_FORCE_AMBIG="1")
    elif setting == "replay":
        env.update(SHD_FORCE_AMBIG="1", SHD_NO_PROTECT="1")
        steps = 3
    else:
        env.update(SHD_SNAP_NO_DEVICE="1")
    a, _, dg, st = run_child("backlog", 100 * MS, steps, tmp_path, **env)
    assert st["lib"] == "libshdgpu_th.so"
    rows, odg = backlog_rows(100 * MS)
    if setting == "rollback":
        assert st["n_rounds_rerun"] > 0 and st["n_rounds_protected"] >= st["n_rounds"]
    elif setting == "replay":
        assert st["n_rounds_replayed"] > 0
    else:
        assert st["n_rounds_protected"] > 0
    assert np.array_equal(dg, odg)
    SE.check(a, rows, setting)


# ---- 6. a group of engines ----
@pytest.mark.parametrize("parts", [2, 3])
def test_group_samples_merge(parts):
    from driver import partition
    from sim import Engine, PathCache, XGroup
    want = untraced("codel", 100 * MS)
    g, m, _ = SC.case("codel", 100 * MS)
    pc = PathCache(g, W.attached_vertices(m.host_vertex))
    pb = partition(m.n_hosts, parts)
    engines = [Engine(m, pc, pb[i], pb[i + 1]) for i in range(parts)]
    grp = XGroup.local(engines)
    grp.run()
    per = [e.host_series() for e in engines]
    for i, a in enumerate(per):
        assert len(a) and pb[i] <= a["rec"]["host"].min() and a["rec"]["host"].max() < pb[i + 1]
    merged = S.merge_host_series(per)
    dg = np.concatenate([e.digest() for e in engines])
    grp.close()
    assert np.array_equal(dg, want["digest"])
    assert merged.tobytes() == want["samples"].tobytes()


# ---- 7. API edges ----
def test_api_edges():
    from sim import Engine, PathCache
    g = W.geometric_graph(20, seed=3)
    hv = W.hosts_on_vertices(20, 1)
    pc = PathCache(g, W.attached_vertices(hv))
    f = S.lib().shd_eng_host_series
    n = C.c_uint64(77)
    buf = np.zeros(64, dtype=S.HOST_SAMPLE_DTYPE)
    # the flag without the records flag, and with a zero interval: SHD_EINVAL
    with pytest.raises(S.ShdError, match="-22"):
        Engine(W.phold_model(hv, end_time=2 * S.SHD_SEC, queue_flags=S.SHD_QF_HOST_SERIES, hostrec_interval_us=1000), pc)
    with pytest.raises(S.ShdError, match="-22"):
        Engine(W.phold_model(hv, end_time=2 * S.SHD_SEC, queue_flags=SC.HS), pc)
    with pytest.raises(S.ShdError, match="-22"):   # end_time / I >= 2^32
        Engine(W.phold_model(hv, end_time=(1 << 32) * 1000, hosts=True, host_series_us=1), pc)
    # the records alone (the interval is ignored): the read call is refused
    eng = Engine(W.phold_model(hv, end_time=2 * S.SHD_SEC, hosts=True, hostrec_interval_us=1000), pc)
    eng.run()
    assert f(eng.ptr, buf.ctypes.data, 64, C.byref(n)) == -22
    assert S.lib().shd_eng_host_series_info(eng.ptr, (C.c_uint64 * 5)()) == -22
    eng.close()
    eng = Engine(W.phold_model(hv, end_time=2 * S.SHD_SEC, hosts=True, host_series_us=500 * MS), pc)
    assert len(eng.host_series()) == 0   # a read before any run
    assert f(eng.ptr, buf.ctypes.data, 64, C.byref(n)) == 0 and n.value == 0
    eng.run()
    assert f(eng.ptr, buf.ctypes.data, 64, None) == -22 and f(None, buf.ctypes.data, 64, C.byref(n)) == -22
    assert f(eng.ptr, None, 64, C.byref(n)) == -22
    a = eng.host_series()
    # the application starts at 1 s: every host is touched in [1 s, 1.5 s) and in [1.5 s, 2 s); the
    # second interval's boundary is end_time, which yields no sample
    assert len(a) == 20 and set(a["t"].tolist()) == {1500 * S.SHD_MS} and a["rec"]["host"].tolist() == list(range(20))
    assert f(eng.ptr, buf.ctypes.data, 19, C.byref(n)) == -34 and n.value == 20   # a short cap: SHD_ERANGE, the count
    assert f(eng.ptr, None, 0, C.byref(n)) == -34 and n.value == 20
    eng.close()
    # a partial engine labels its rows with the model's host indices (host-driven rounds; its
    # sends to the other hosts are dropped here: only the labels are looked at)
    m = W.phold_model(hv, end_time=2 * S.SHD_SEC, hosts=True, host_series_us=100 * MS)
    eng = Engine(m, pc, 5, 12)
    eng.boot()
    w, nxt = eng.window, eng.next_time()
    while nxt < 2 * S.SHD_SEC:
        nxt = eng.run_round(nxt, min(nxt + w, 2 * S.SHD_SEC)).next_time
    a = eng.host_series()
    eng.close()
    assert len(a) and sorted(set(a["rec"]["host"].tolist())) == list(range(5, 12))
