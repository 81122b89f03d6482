"""The packet engine's host-record series fixture
(tests/golden/ref_eng_hseries.json) is the reference's own loop's: what
tests/eng_series_expect.py derives in one pass from the [STATUS] lines of cases
of tests/ref_loop_cases.py, at ten (case, interval) pairs.  Here, with no
device:

* the one-pass derivation is the definition -- on `udp_mix_codel` at 100 ms
  every row equals tcp_host_expect.derive over the lines before its boundary;
* each host's last sample is its final record (ref_eng_hosts.json) or less,
  and equal in every field that no later line touches;
* the oracle's traced run, whose lines are the reference's (ref_loop.json's
  digest), derives the fixture at every pair;
* where the reference's loop is built, two pairs run through it again.

The lines come from the oracle (oracle/o_engine.c), checked against
ref_loop.json's line digest before they are used.
"""
import json
import os

import numpy as np
import pytest

import eng_series_expect as SE
import ref_loop_cases as RC
import ref_loop_ffi as R
import shdgpu as S
import tcp_host_expect as HE
from test_ref_loop_cpu import oracle_lines

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "ref_eng_hseries.json")))
HOSTS = json.load(open(os.path.join(HERE, "golden", "ref_eng_hosts.json")))
LOOP = json.load(open(os.path.join(HERE, "golden", "ref_loop.json")))
MS = 1000
# the issue's table: (case, interval us) -> samples
PAIRS = {("codel", 100 * MS): 1140, ("udp_echo_codel", 100 * MS): 737, ("udp_mix_codel", 100 * MS): 535,
         ("bootstrap", 100 * MS): 724, ("phold_v100", 100 * MS): 1900, ("codel", 1 * MS): 42965,
         ("udp_mix_codel", 1 * MS): 4737, ("bootstrap", 10 * MS): 3939, ("phold_v100", 1000 * MS): 100,
         ("udp_echo_codel", 5000 * MS): 0}
IDS = ["%s@%d" % p for p in PAIRS]
I = {k: j for j, k in enumerate(SE.FIELDS)}
_lines = {}


def lines_of(name):
    """the case's [STATUS] lines from the oracle, checked to be the reference's, once"""
    if name not in _lines:
        case = RC.CASES[name]()
        st, _, _ = oracle_lines(case, LOOP[name])
        assert len(st) == LOOP[name]["n_status"] and RC.digest_lines(st) == LOOP[name]["status_sha256"], name
        m = case["model"]
        _lines[name] = (st, int(m.n_hosts), int(m.params["end_time"]))
    return _lines[name]


def test_every_pair_has_a_fixture():
    assert sorted(k for k in FIX if k != "fields") == sorted(IDS)
    assert FIX["fields"] == list(SE.FIELDS)
    assert os.path.getsize(os.path.join(HERE, "golden", "ref_eng_hseries.json")) < 612 * 1024
    for (name, us), n in PAIRS.items():
        f = FIX["%s@%d" % (name, us)]
        H = int(RC.CASES[name]()["model"].n_hosts)
        assert f["n"] == n == sum(f["per_host"]) and len(f["per_host"]) == H and f["interval_us"] == us
        assert ("hosts" in f) == (us == 100 * MS)
    assert set(FIX["codel@100000"]["per_host"]) == {19}
    assert set(FIX["phold_v100@1000000"]["per_host"]) == {1}
    # the two pairs that decide "an event at exactly T_k belongs to the interval after it"
    assert FIX["codel@1000"]["on_boundary"] == 44432 and FIX["udp_mix_codel@1000"]["on_boundary"] == 2868


def test_one_pass_rows_are_the_prefix_records():
    """sample (h, T) = tcp_host_expect.derive(lines with t < T)[h], field for field"""
    st, H, end = lines_of("udp_mix_codel")
    rows = SE.derive(st, H, 100 * MS * 1000, end)
    assert len(rows) == 535
    prefix = {}
    for r in rows:
        T, h = r[0], r[1]
        if T not in prefix:
            prefix[T] = HE.rows(HE.derive([x for x in st if x[0] < T], H))
        assert r[1:] == prefix[T][h], (T, h)
        assert T % (100 * MS * 1000) == 0 and 0 < T < end
    assert [(r[1], r[0]) for r in rows] == sorted((r[1], r[0]) for r in rows)   # sorted by (host, t), no duplicate
    assert len({(r[1], r[0]) for r in rows}) == len(rows)
    # sparse: a host has a sample at T only if one of its lines lies in [T - I, T)
    touched = {(h, (t // (100 * MS * 1000) + 1) * 100 * MS * 1000) for t, h, b in st
               if b[1:b.index("]")] in HE.COUNTED}
    assert {(r[1], r[0]) for r in rows} == {x for x in touched if x[1] < end}


@pytest.mark.parametrize("name", ["codel", "udp_echo_codel", "udp_mix_codel", "bootstrap", "phold_v100"])
def test_last_sample_against_the_final_record(name):
    st, H, end = lines_of(name)
    Ins = 100 * MS * 1000
    rows = SE.derive(st, H, Ins, end)
    final = HOSTS[name]["rows"]
    # the fields a status's lines touch (t_last: any of them)
    touches = {"ROUTER_ENQUEUED": ("router_enqueued", "router_enqueued_bytes", "depth_max", "t_depth_max"),
               "ROUTER_DEQUEUED": ("router_dequeued", "router_dequeued_bytes", "sojourn_sum", "sojourn_max",
                                   "t_sojourn_max"),
               "ROUTER_DROPPED": ("router_dropped", "router_dropped_bytes"),
               "RCV_INTERFACE_RECEIVED": ("if_received", "if_received_bytes"),
               "RCV_INTERFACE_DROPPED": ("if_dropped",), "SND_INTERFACE_SENT": ("if_sent", "if_sent_bytes"),
               "SND_TCP_ENQUEUE_THROTTLED": ("tcp_throttled",), "RCV_TCP_ENQUEUE_UNORDERED": ("tcp_unordered",)}
    last_line = {}   # (host, status) -> its last line's time
    for t, h, b in st:
        last_line[(h, b[1:b.index("]")])] = t
    grow = [k for k in HE.SCALARS if k not in ("host", "depth_end", "t_first")]
    seen = 0
    for h in range(H):
        mine = [r for r in rows if r[1] == h]
        if not mine:
            continue
        r, f = mine[-1], final[h]
        for k in grow:
            assert r[I[k]] <= f[I[k] - 1], (name, h, k)
        assert all(a <= b for a, b in zip(r[-1], f[-1])), (name, h)
        assert r[I["t_first"]] == f[I["t_first"] - 1]
        for status, fields in touches.items():
            if last_line.get((h, status), 0) < r[0]:   # no line of this status at or after the last boundary
                for k in fields:
                    assert r[I[k]] == f[I[k] - 1], (name, h, k)
                    seen += 1
                if status == "ROUTER_DEQUEUED":
                    assert r[-1] == f[-1], (name, h)
    assert seen > 0, name


@pytest.mark.parametrize("name,us", list(PAIRS), ids=IDS)
def test_oracle_lines_derive_the_fixture(name, us):
    st, H, end = lines_of(name)
    f = FIX["%s@%d" % (name, us)]
    rows = SE.derive(st, H, 1000 * us, end)
    assert len(rows) == f["n"] and SE.per_host(rows, H) == f["per_host"] and SE.digest(rows) == f["sha256"]
    assert SE.on_boundary(st, 1000 * us) == f["on_boundary"]
    for h, want in f.get("hosts", {}).items():
        assert [r for r in rows if r[1] == int(h)] == want, (name, us, h)


def test_array_rows_round_trip_and_fill_forward(tmp_path):
    """HOST_SAMPLE_DTYPE <-> rows; merge_host_series sorts by (host, t);
    host_progress fills forward; write_host_series_csv writes every row"""
    st, H, end = lines_of("udp_mix_codel")
    Ins = 100 * MS * 1000
    rows = SE.derive(st, H, Ins, end)
    a = np.zeros(len(rows), dtype=S.HOST_SAMPLE_DTYPE)
    a["t"] = [r[0] for r in rows]
    for j, k in enumerate(HE.SCALARS):
        a["rec"][k] = [r[1 + j] for r in rows]
    a["rec"]["sojourn_hist"] = [r[-1] for r in rows]
    SE.check(a, rows)
    assert S.HOST_SAMPLE_DTYPE.itemsize == 240
    cut = len(a) // 3
    merged = S.merge_host_series([a[cut:], a[:cut]])
    assert merged.tobytes() == a.tobytes()
    K = (end - 1) // Ins
    for h in (0, int(FIX["udp_mix_codel@100000"]["deepest"])):
        dense = S.host_progress(a, h, Ins, end)
        assert len(dense) == K and dense["t"].tolist() == [(k + 1) * Ins for k in range(K)]
        mine = {r[0]: r for r in rows if r[1] == h}
        cur = [0] * len(HE.SCALARS) + [[0] * 16]
        cur[0] = h
        for d in SE.from_array(dense):
            cur = mine.get(d[0], [None] + cur)[1:]
            assert d[1:] == cur, (h, d[0])
    n = S.write_host_series_csv(tmp_path / "s.csv", a)
    text = (tmp_path / "s.csv").read_text().splitlines()
    assert n == len(a) == len(text) - 1 and text[0].split(",")[:3] == ["t", "host", "depth_max"]
    assert text[1].split(",")[0] == str(rows[0][0]) and len(text[1].split(",")) == len(S.HOST_SERIES_CSV_FIELDS)


@pytest.mark.skipif(not R.available(), reason="oracle/_ref/libshdref_loop.so not built (needs the reference tree)")
@pytest.mark.parametrize("name,us", [("codel", 1 * MS), ("bootstrap", 10 * MS)])
def test_reference_loop_reproduces_the_fixture(name, us):
    case = RC.CASES[name]()
    r = R.run(case["model"], case["graph"], procs=RC.procs_of(case), echo=case["model"].app_peer)
    st, _ = RC.split_lines(r["lines"])
    m = case["model"]
    rows = SE.derive(st, int(m.n_hosts), 1000 * us, int(m.params["end_time"]))
    f = FIX["%s@%d" % (name, us)]
    assert len(rows) == f["n"] and SE.per_host(rows, int(m.n_hosts)) == f["per_host"] and SE.digest(rows) == f["sha256"]
