"""Host records of the packet engine (SHD_QF_HOST_RECORDS, shd_eng_host_records)
on the device, against the reference's own loop.

tests/golden/ref_eng_hosts.json holds what tests/tcp_host_expect.py derives from
the [STATUS] lines the reference's serial loop logged for five models of
tests/ref_loop_cases.py.  The engine runs the same models UNTRACED with the
flag alone and must return those rows field by field; the flag must change
nothing else of a run; every round-kernel family, a group of engines, and the
rollback and replay of rounds must give the same records.

Shapes: the cases are the fixture's (40-100 hosts, 3 s, each a few seconds);
`backlog` (eng_hosts_cases.py: 400 hosts on 200 vertices, 1500-B datagrams into
512 KiB/s buckets) is the rollback model the issue sets.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import eng_hosts_cases as EC
import oracle_ffi as O
import shdgpu as S
import tcp_host_expect as HE
import workloads as W

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "ref_eng_hosts.json")) as f:
    FIX = json.load(f)
ENV_SWITCHES = ("SHD_NO_PS", "SHD_NO_TL", "SHD_SP_HOSTS", "SHD_PS_BATCH", "SHDGPU_LIB", "SHD_FORCE_AMBIG",
                "SHD_PROTECT_ALL", "SHD_NO_PROTECT", "SHD_SNAP_NO_DEVICE")


def rows_from_trace(trace, n_hosts, payload):
    """Host-record rows (tcp_host_expect.FIELDS order) from an engine trace in
    execution order (the oracle's), every host reading its own records:
      SHD_TR_ARRIVE                       an enqueue at its time
      SHD_TR_CODEL_DROP                   a drop of the queue's head
      SHD_TR_RECV / SHD_TR_IF_DROP from another host
                                          a dequeue of the head at its time
      SHD_TR_RECV (any peer)              an interface receive; SHD_TR_IF_DROP an interface drop
      SHD_TR_SENT, SHD_TR_INET_DROP, SHD_TR_LOCAL
                                          one interface send each, at the sender
    Bytes are payload x count.  Pinned against the reference's fixture in
    tests/test_eng_hosts_ref_cpu.py."""
    recs = []
    for h in range(n_hosts):
        r = dict.fromkeys(HE.SCALARS, 0)
        r.update(host=h, sojourn_hist=[0] * 16)
        recs.append(r)
    queue = [[] for _ in range(n_hosts)]
    counted = (S.TR_ARRIVE, S.TR_CODEL_DROP, S.TR_RECV, S.TR_IF_DROP, S.TR_SENT, S.TR_INET_DROP, S.TR_LOCAL)
    for t, h, peer, kind in zip(trace["time"].tolist(), trace["host"].tolist(), trace["peer"].tolist(),
                                trace["kind"].tolist()):
        if kind not in counted:
            continue
        r, q = recs[h], queue[h]
        if not r["t_first"]:
            r["t_first"] = t
        r["t_last"] = t
        if kind == S.TR_ARRIVE:
            q.append(t)
            r["router_enqueued"] += 1
            if len(q) > r["depth_max"]:
                r["depth_max"], r["t_depth_max"] = len(q), t
        elif kind == S.TR_CODEL_DROP:
            q.pop(0)
            r["router_dropped"] += 1
        elif kind in (S.TR_RECV, S.TR_IF_DROP):
            if peer != h:
                so = t - q.pop(0)
                r["sojourn_sum"] += so
                if r["router_dequeued"] == 0 or so > r["sojourn_max"]:
                    r["sojourn_max"], r["t_sojourn_max"] = so, t
                r["router_dequeued"] += 1
                r["sojourn_hist"][HE.bucket(so)] += 1
            r["if_received" if kind == S.TR_RECV else "if_dropped"] += 1
        else:
            r["if_sent"] += 1
    for r, q in zip(recs, queue):
        r["depth_end"] = len(q)
        for k in ("router_enqueued", "router_dequeued", "router_dropped", "if_received", "if_sent"):
            r[k + "_bytes"] = payload * r[k]
    return HE.rows(recs)


_untraced = {}


def untraced(name):
    """the case untraced, with the flag alone, on the default kernel selection:
    (records, digest, statistics), computed once"""
    if name not in _untraced:
        g, m, pushes = EC.ref_case(name, False, EC.HR)
        recs, dg, tr, eng, tot = EC.engine_records(g, m, pushes)
        assert len(tr) == 0
        eng.close()
        recs.setflags(write=False)
        dg.setflags(write=False)
        _untraced[name] = (recs, dg, tot)
    return _untraced[name]


def run_child(name, steps, tmp_path, timeout=180, **env_set):
    env = {k: v for k, v in os.environ.items() if k not in ENV_SWITCHES}
    env.update(env_set)
    out = os.path.join(tmp_path, f"{name}.npz")
    p = subprocess.run([sys.executable, "-u", os.path.join(HERE, "eng_hosts_worker.py"), name, str(steps), out],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    text = p.stdout.decode(errors="replace")
    assert p.returncode == 0, text[-3000:]
    print(text.strip().splitlines()[-1])
    z = np.load(out)
    return z["records"], z["digest"], json.loads(text.strip().splitlines()[-1])


# ---- 1. the reference pin, untraced ----
@pytest.mark.parametrize("name", EC.CASES)
def test_untraced_records_are_the_references(name):
    recs, _, tot = untraced(name)
    assert tot["n_pkt_events"] > 0
    HE.check(recs, FIX[name]["rows"], name)


# ---- 2. the flag stands alone ----
@pytest.mark.parametrize("name", EC.CASES)
def test_the_flag_changes_nothing_else(name):
    """the case's own flags (trace, status trace, heartbeats) with and without
    the bit: the same digest, trace and event counts; the records are (1)'s and
    what the engine's own status lines derive"""
    import ref_loop_cases as RC
    case = RC.CASES[name]()
    flags = int(case["model"].params["queue_flags"])
    g, m1, pushes = EC.ref_case(name, True, flags | EC.HR)
    recs, dg1, tr1, eng1, tot1 = EC.engine_records(g, m1, pushes)
    lines = sorted(eng1.status_lines(FIX[name]["ips"]), key=lambda x: (x[0], x[1]))
    hb1 = eng1.heartbeats()
    eng1.close()
    _, m0, _ = EC.ref_case(name, True, flags)
    _, dg0, tr0, eng0, tot0 = EC.engine_records(g, m0, pushes)
    hb0 = eng0.heartbeats()
    with pytest.raises(S.ShdError, match="-22"):   # without the bit the call is refused
        eng0.host_records()
    eng0.close()
    assert np.array_equal(dg1, dg0) and np.array_equal(tr1, tr0) and np.array_equal(hb1, hb0)
    assert (tot1["n_events"], tot1["n_pkt_events"]) == (tot0["n_events"], tot0["n_pkt_events"])
    assert len(lines) == FIX[name]["n_status"]
    assert np.array_equal(dg1, untraced(name)[1])
    assert recs.tobytes() == untraced(name)[0].tobytes()
    HE.check(recs, HE.rows(HE.derive(lines, int(m1.n_hosts))), name)


# ---- 3. every kernel family ----
@pytest.mark.parametrize("name", ["codel", "phold_v100"])
def test_launch_per_round_kernels(name, tmp_path):
    """SHD_NO_PS=1 (k_round_tl<false> and the ticketed k_round_dev), and with
    SHD_NO_TL=1 the ticketed kernels alone; read once a process: a child each"""
    want, wdg, _ = untraced(name)
    recs, dg, st = run_child(name, 1, tmp_path, SHD_NO_PS="1")
    assert st["n_batches_persistent"] == 0 and st["n_batches_ticketless"] > 0
    assert recs.tobytes() == want.tobytes() and np.array_equal(dg, wdg)
    recs, dg, st = run_child(name, 1, tmp_path, SHD_NO_PS="1", SHD_NO_TL="1")
    assert st["n_batches_persistent"] == 0 and st["n_batches_ticketless"] == 0 and st["n_batches"] > 0
    assert recs.tobytes() == want.tobytes() and np.array_equal(dg, wdg)


@pytest.mark.parametrize("name", ["codel", "phold_v100"])
def test_persistent_sparse_and_host_driven_rounds(name, monkeypatch):
    want, wdg, tot = untraced(name)
    assert tot["n_batches_persistent"] > 0 and tot["n_batches_sparse"] == 0   # the default: k_round_ps<false>
    g, m, pushes = EC.ref_case(name, False, EC.HR)
    # the host drives every round (shd_eng_run_round: k_round)
    recs, dg, _, eng, rt = EC.engine_records(g, m, pushes, rounds=True)
    eng.close()
    assert rt["n_pkt_events"] == tot["n_pkt_events"]
    assert recs.tobytes() == want.tobytes() and np.array_equal(dg, wdg)
    # run_until in three unequal steps
    recs, dg, _, eng, st = EC.engine_records(g, m, pushes, steps=3)
    again = eng.host_records()   # the call reads, it does not reset
    eng.close()
    assert st["n_pkt_events"] == tot["n_pkt_events"]
    assert recs.tobytes() == want.tobytes() == again.tobytes() and np.array_equal(dg, wdg)
    # the sparse persistent kernel (k_round_sp<false>), blocks of 64 hosts
    monkeypatch.setenv("SHD_SP_HOSTS", "64")
    recs, dg, _, eng, st = EC.engine_records(g, m, pushes)
    eng.close()
    assert st["n_batches_sparse"] > 0
    assert recs.tobytes() == want.tobytes() and np.array_equal(dg, wdg)


def test_records_grow_between_steps():
    """read after each run_until step: every count only grows, and the last
    read is the whole run's"""
    from sim import Engine, PathCache
    g, m, _ = EC.ref_case("codel", False, EC.HR)
    eng = Engine(m, PathCache(g, W.attached_vertices(m.host_vertex)))
    end = int(m.params["end_time"])
    prev = None
    for t in (end // 3, end // 2 + 7, end):
        eng.run_until(t)
        a = eng.host_records()
        assert int(a["t_last"].max()) < t
        if prev is not None:
            for k in ("router_enqueued", "router_dequeued", "router_dropped", "if_received", "if_sent", "sojourn_sum",
                      "depth_max", "sojourn_max"):
                assert np.all(a[k] >= prev[k]), k
        prev = a
    eng.close()
    assert prev.tobytes() == untraced("codel")[0].tobytes()


# ---- 4. a group of engines ----
@pytest.mark.parametrize("parts", [2, 3])
def test_group_records_concatenate(parts):
    from driver import partition
    from sim import Engine, PathCache, XGroup
    g, m, _ = EC.ref_case("codel", False, EC.HR)
    pc = PathCache(g, W.attached_vertices(m.host_vertex))
    pb = partition(m.n_hosts, parts)
    engines = [Engine(m, pc, pb[i], pb[i + 1]) for i in range(parts)]
    grp = XGroup.local(engines)
    grp.run()
    per = [e.host_records() for e in engines]
    assert [len(a) for a in per] == [pb[i + 1] - pb[i] for i in range(parts)]
    recs = S.merge_tcp_hosts(per)
    dg = np.concatenate([e.digest() for e in engines])
    grp.close()
    assert np.array_equal(dg, untraced("codel")[1])
    assert recs.tobytes() == untraced("codel")[0].tobytes()
    HE.check(recs, FIX["codel"]["rows"], f"group of {parts}")


# ---- 5. rollback and replay ----
_backlog = {}


def backlog_rows():
    """the backlog model's expected rows, from the oracle's trace, once"""
    if not _backlog:
        g, m = EC.backlog(True, 0)
        tr, dg, _ = O.engine_run(m, g)
        dg.setflags(write=False)
        _backlog.update(rows=rows_from_trace(tr, int(m.n_hosts), 1500), digest=dg)
    return _backlog["rows"], _backlog["digest"]


TH = os.path.join(os.path.dirname(HERE), "shadow-1_amd", "libshdgpu_th.so")


@pytest.mark.parametrize("setting", ["rollback", "replay", "snap_host"])
def test_rerun_rounds_count_once(setting, tmp_path):
    """rounds rolled back to their state copy and rerun (SHD_PROTECT_ALL +
    SHD_FORCE_AMBIG), rounds replayed from the last restore point
    (SHD_FORCE_AMBIG + SHD_NO_PROTECT, three run_until steps), and the state
    copy in host memory (SHD_SNAP_NO_DEVICE): the records are in the copied
    state, so they equal what the oracle's trace derives"""
    env, steps = dict(SHDGPU_LIB=TH), 1
    if setting == "rollback":
        env.update(SHD_PROTECT_ALL="1", SHD_FORCE_AMBIG="1")
    elif setting == "replay":
        env.update(SHD_FORCE_AMBIG="1", SHD_NO_PROTECT="1")
        steps = 3
    else:
        env.update(SHD_SNAP_NO_DEVICE="1")
    recs, dg, st = run_child("backlog", steps, tmp_path, **env)
    assert st["lib"] == "libshdgpu_th.so"
    rows, odg = backlog_rows()
    if setting == "rollback":
        assert st["n_rounds_rerun"] > 0 and st["n_rounds_protected"] >= st["n_rounds"]
    elif setting == "replay":
        assert st["n_rounds_replayed"] > 0
    else:
        assert st["n_rounds_protected"] > 0
    assert np.array_equal(dg, odg)
    HE.check(recs, rows, setting)
    assert HE.totals(rows)[3] > 4   # queues did build


# ---- 6. API edges ----
def test_api_edges():
    import ctypes as C
    from sim import Engine, PathCache
    g = W.geometric_graph(20, seed=3)
    hv = W.hosts_on_vertices(20, 1)
    pc = PathCache(g, W.attached_vertices(hv))
    f = S.lib().shd_eng_host_records
    n = C.c_uint64(77)
    buf = np.zeros(20, dtype=S.TCP_HOSTREC_DTYPE)
    # without the flag: SHD_EINVAL, nothing allocated
    eng = Engine(W.phold_model(hv, end_time=2 * S.SHD_SEC), pc)
    eng.run()
    assert f(eng.ptr, buf.ctypes.data, 20, C.byref(n)) == -22
    eng.close()
    # a model that stops before the application starts: no host saw a packet
    eng = Engine(W.phold_model(hv, end_time=S.SHD_SEC // 2, queue_flags=EC.HR), pc)
    eng.run()
    assert f(eng.ptr, buf.ctypes.data, 20, None) == -22 and f(None, buf.ctypes.data, 20, C.byref(n)) == -22
    assert f(eng.ptr, None, 20, C.byref(n)) == -22
    # a cap that is too small: the neighbouring calls' SHD_ERANGE, with the count
    assert f(eng.ptr, buf.ctypes.data, 19, C.byref(n)) == -34 and n.value == 20
    assert f(eng.ptr, None, 0, C.byref(n)) == -34 and n.value == 20
    a = eng.host_records()
    eng.close()
    want = np.zeros(20, dtype=S.TCP_HOSTREC_DTYPE)
    want["host"] = np.arange(20)
    assert a.tobytes() == want.tobytes()   # zero apart from `host`
    # a partial engine's records carry the model's host index
    eng = Engine(W.phold_model(hv, end_time=S.SHD_SEC // 2, queue_flags=EC.HR), pc, 5, 12)
    assert eng.host_records()["host"].tolist() == list(range(5, 12))
    eng.close()
