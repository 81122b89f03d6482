"""The packet engine's host-record fixture (tests/golden/ref_eng_hosts.json) is
the reference's own loop's, derived by tests/tcp_host_expect.py from the
datagram [STATUS] lines of five cases of tests/ref_loop_cases.py; its rows obey
the record's identities; the trace-to-records rule that
tests/test_eng_hosts_gpu.py applies to the oracle's trace of a model the
reference never ran reproduces the fixture's `codel` case; and the C ABI's new
pieces (SHD_QF_HOST_RECORDS, shd_eng_host_records) refuse what they must
before any device call.  No device.

Where the reference's loop is built (oracle/Makefile `ref`), every case runs
through it again and must reproduce the committed fixture."""
import ctypes as C
import json
import os

import pytest

import eng_hosts_cases as EC
import oracle_ffi as O
import ref_loop_cases as RC
import ref_loop_ffi as R
import shdgpu as S
import tcp_host_expect as HE
from test_eng_hosts_gpu import rows_from_trace

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "ref_eng_hosts.json")))
with open(os.path.join(HERE, "golden", "ref_loop.json")) as f:
    LOOP = json.load(f)
I = {k: j for j, k in enumerate(HE.SCALARS)}
# what the issue sets: per case (hosts, enqueued, dequeued, dropped, deepest
# queue, longest sojourn of a dequeued packet in ns, if_sent), summed over hosts
TABLE = {"codel": (60, 31376, 30186, 1182, 48, 115259205, 32648),
         "udp_echo_codel": (40, 8054, 8012, 41, 26, 75908789, 8268),
         "udp_mix_codel": (60, 3931, 3751, 180, 43, 178341299, 4122),
         "bootstrap": (40, 6783, 6783, 0, 5, 12516036, 7216),
         "phold_v100": (100, 26750, 26750, 0, 1, 0, 27839)}


def col(name, k):
    return [r[I[k]] for r in FIX[name]["rows"]]


def test_every_case_has_a_fixture():
    assert sorted(FIX) == sorted(EC.CASES) == sorted(TABLE)
    assert os.path.getsize(os.path.join(HERE, "golden", "ref_eng_hosts.json")) < 100000
    for name, f in FIX.items():
        H = int(RC.CASES[name]()["model"].n_hosts)
        assert f["fields"] == list(HE.FIELDS), name
        assert len(f["ips"]) == len(f["rows"]) == H, name
        assert col(name, "host") == list(range(H)), name   # dense, in host order
        assert all(len(r) == len(HE.FIELDS) and len(r[-1]) == 16 for r in f["rows"]), name
        assert f["n_status"] == LOOP[name]["n_status"], name   # the run ref_loop.json recorded


@pytest.mark.parametrize("name", EC.CASES)
def test_fixture_totals_are_the_issues(name):
    enq, deq, drop, dmax, _, smax = HE.totals(FIX[name]["rows"])
    assert (len(FIX[name]["rows"]), enq, deq, drop, dmax, smax, sum(col(name, "if_sent"))) == TABLE[name]
    assert sum(col(name, "if_dropped")) == sum(col(name, "tcp_throttled")) == sum(col(name, "tcp_unordered")) == 0


def test_fixture_is_not_vacuous():
    """what each case is in the fixture for"""
    assert sum(1 for d in col("codel", "depth_end") if d > 0) == 5   # queues still hold packets at the end
    ph = FIX["phold_v100"]["rows"]   # the all-fast-path case: depth 1, sojourn 0, loopback sends
    assert all(r[I["depth_max"]] == 1 and r[I["sojourn_sum"]] == 0 and sum(r[-1][1:]) == 0 for r in ph)
    assert sum(col("phold_v100", "if_sent")) > sum(col("phold_v100", "router_enqueued"))
    assert sum(col("phold_v100", "if_received")) > sum(col("phold_v100", "router_dequeued"))   # loopback deliveries
    mix = FIX["udp_mix_codel"]["rows"]
    assert max(i for r in mix for i in range(16) if r[-1][i]) == 12


@pytest.mark.parametrize("name", EC.CASES)
def test_fixture_rows_obey_their_identities(name):
    payload = int(RC.CASES[name]()["model"].params["payload"])
    for r in FIX[name]["rows"]:
        g = lambda k: r[I[k]]   # noqa: E731
        assert sum(r[-1]) == g("router_dequeued"), (name, r)
        assert g("depth_end") == g("router_enqueued") - g("router_dequeued") - g("router_dropped"), (name, r)
        for k in ("router_enqueued", "router_dequeued", "router_dropped", "if_received", "if_sent"):
            assert g(k + "_bytes") == payload * g(k), (name, k, r)   # bytes are payload x count
        assert g("sojourn_max") <= g("sojourn_sum"), (name, r)
        assert g("t_first") <= g("t_last"), (name, r)
        assert g("depth_max") <= g("router_enqueued") and (g("depth_max") > 0) == (g("router_enqueued") > 0), (name, r)
        if g("router_enqueued"):
            assert g("t_first") <= g("t_depth_max") <= g("t_last"), (name, r)
        if g("router_dequeued"):
            assert g("t_first") <= g("t_sojourn_max") <= g("t_last"), (name, r)
        else:
            assert g("t_sojourn_max") == g("sojourn_sum") == 0, (name, r)
        if not g("t_first"):   # a host that saw no packet: zero apart from `host`
            assert r[1:-1] == [0] * (len(HE.SCALARS) - 1) and not any(r[-1]), (name, r)


def test_the_array_round_trips_the_rows():
    for name in EC.CASES:
        HE.check(EC.array_of(FIX[name]["rows"]), FIX[name]["rows"], name)


def test_with_flags_keeps_the_model():
    """the rebuilt model differs from the case's in trace and queue_flags alone"""
    for name in EC.CASES:
        m0 = RC.CASES[name]()["model"]
        _, m, _ = EC.ref_case(name, False, EC.HR)
        for k, _t in S.Model._fields_:
            a, b = getattr(m0.struct, k), getattr(m.struct, k)
            if k == "trace":
                assert (a, b) == (1, 0)
            elif k == "queue_flags":
                assert (a, b) == (RC.TS | (a & S.SHD_QF_NO_APP_START), EC.HR)
            elif not isinstance(a, int):
                assert bool(a) == bool(b), (name, k)   # a pointer: the arrays are compared below
            else:
                assert a == b, (name, k)
        for k in ("host_vertex", "host_rng", "bw_down", "bw_up", "dest_cum", "host_class", "host_heartbeat",
                  "app_peer", "host_app"):
            a, b = getattr(m0, k), getattr(m, k)
            assert (a is None) == (b is None) and (a is None or a.tobytes() == b.tobytes()), (name, k)
        if m0.app_specs is not None:
            assert bytes(m0.app_specs) == bytes(m.app_specs)


def test_trace_rule_reproduces_the_codel_fixture():
    """rows_from_trace (tests/test_eng_hosts_gpu.py: an arrival is an enqueue, a
    CoDel drop drops the head, a receive from another host dequeues it, a send
    leaves the interface), applied to the oracle's trace of the `codel` case,
    gives the reference's rows: the rule is pinned before the rollback and
    replay tests trust it on a model the reference never ran"""
    case = RC.CASES["codel"]()
    tr, _, _ = O.engine_run(case["model"], case["graph"])
    rows = rows_from_trace(tr, int(case["model"].n_hosts), int(case["model"].params["payload"]))
    assert rows == FIX["codel"]["rows"]


def test_backlog_model_builds_queues():
    """the rollback and replay model is worth its name: on the oracle's trace
    queues build, CoDel drops and some hosts end with packets queued"""
    g, m = EC.backlog(True, 0)
    tr, _, _ = O.engine_run(m, g)
    rows = rows_from_trace(tr, int(m.n_hosts), 1500)
    enq, deq, drop, dmax, _, smax = HE.totals(rows)
    print("backlog:", enq, deq, drop, dmax, smax)
    assert m.n_hosts == 400 and enq > 10000 and dmax > 4 and smax > 10 * S.SHD_MS


@pytest.mark.skipif(not R.available(), reason="oracle/_ref/libshdref_loop.so not built (needs the reference tree)")
@pytest.mark.parametrize("name", EC.CASES)
def test_reference_loop_reproduces_the_fixture(name):
    case = RC.CASES[name]()
    r = R.run(case["model"], case["graph"], procs=RC.procs_of(case), echo=case["model"].app_peer)
    st, _ = RC.split_lines(r["lines"])
    assert r["ip"] == FIX[name]["ips"] and len(st) == FIX[name]["n_status"]
    assert HE.rows(HE.derive(st, int(case["model"].n_hosts))) == FIX[name]["rows"]


def test_abi_pieces():
    """the flag's value, the prototype, and the refusals that need no engine"""
    assert S.SHD_QF_HOST_RECORDS == 32
    with open(os.path.join(os.path.dirname(HERE), "include", "shdgpu.h")) as fh:
        text = fh.read()
    assert "SHD_QF_HOST_RECORDS = 32" in text
    assert "int shd_eng_host_records(shd_eng* e, struct shd_tcp_hostrec* out, uint64_t cap, uint64_t* n);" in text
    f = S.lib().shd_eng_host_records
    n = C.c_uint64()
    buf = (S.TcpHostRec * 1)()
    assert f(None, buf, 1, C.byref(n)) == -22    # SHD_EINVAL: no engine
    assert f(None, buf, 1, None) == -22
    assert C.sizeof(S.TcpHostRec) == S.TCP_HOSTREC_DTYPE.itemsize == 232
