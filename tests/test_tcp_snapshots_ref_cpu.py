"""The five snapshot values of a TCP socket -- state, cwnd, ssthresh, srtt,
rttvar, the last five fields of shd_tcp_flow and shd_tcp_sample -- pinned to
the reference's own tcp.c.  No device.

tests/golden/ref_tcp_snapshots.json holds what the reference's tcp_getInfo gave
for the TCP descriptors of every echo process each time the process ran, after
its connect call and before each of its closes
(oracle/ref_harness/ref_loop.c; tests/golden/make_ref_tcp_snapshots.py).  The
oracle (oracle/o_tcp.c, o_tcp_out.obs) must give the same rows, every field of
every row; where the reference's loop is built it must reproduce them too; and
the oracle's change log (o_tcp_out.log), which tests/test_tcp_snapshots_gpu.py
holds the device to, must agree with the oracle's own observations.

The limit of the pin: the reference is observed from a socket's creation until
its process closes it.  The transitions after the close (FINWAIT1/2, CLOSING,
LASTACK, TIMEWAIT, CLOSED) happen where no process runs; they are in the
oracle's log only and so pinned oracle-to-device.

The srtt reset of tcp.c's ACK processing (backoff > 2: srtt = rttvar = 0) is
observed by the reference in one case, rto_reset (tcp_cases.SNAPSHOT_CASES):
srtt 60 -> 0 with ssthresh halved by the timeouts before it.  heavy_loss
reaches the reset only after its processes' last runs (in the oracle's log).
loopback_pair and loopback_mixed also show srtt going 1 -> 0, but that is the
estimator's integer arithmetic (7 * 1 / 8 + rtt / 8 == 0), not the reset, and
is not counted as one."""
import functools
import json
import os

import pytest

import oracle_ffi as O
import ref_loop_ffi as R
import shdgpu as S
import tcp_cases as TC
import tcp_hub_cases as TH
import tcp_snapshot_expect as XE

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "ref_tcp_snapshots.json")))
FLOWS = json.load(open(os.path.join(HERE, "golden", "ref_tcp_flows.json")))

# ref_tcp_flows.json's 14 cases less the five the size limit leaves out
# (make_ref_tcp_snapshots.py's docstring), and the fixture's own two small cases
CASES = ["ref_epoll_lossy", "lossy_2pct", "slow_links", "heavy_loss", "shared_hosts_rr", "server_first",
         "loopback_pair", "loopback_mixed", "mixed_hosts", "hub3_slow", "rto_reset"]
LIVE = ["lossy_2pct", "loopback_pair", "hub3_slow", "rto_reset"]
ST = {n: i for i, n in enumerate(S.TCP_STATE_NAMES)}
I = {k: i for i, k in enumerate(XE.OBS_FIELDS)}


def build(name):
    return TH.build(name) if name in TH.CASES else TC.build(name)


@functools.lru_cache(maxsize=None)
def rows(name):
    return XE.unpack(FIX[name])


@functools.lru_cache(maxsize=None)
def oracle(name):
    c, m = build(name)
    return O.tcp_run(m, c["graph"], TC.ip_ints(FIX[name]["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                     qdisc=c.get("qdisc", 0), udp=TC.udp_arg(c), snapshots=True)


def by_socket(obs):
    """observation rows by (host, process, local address, peer address)"""
    out = {}
    for r in obs:
        out.setdefault(tuple(r[1:7]), []).append(r)
    return out


def test_every_case_has_a_fixture():
    assert sorted(FIX) == sorted(CASES)
    assert os.path.getsize(os.path.join(HERE, "golden", "ref_tcp_snapshots.json")) <= max(
        os.path.getsize(os.path.join(HERE, "golden", f)) for f in os.listdir(os.path.join(HERE, "golden"))
        if f.startswith("ref_tcp_") and f.endswith(".json") and f != "ref_tcp_snapshots.json")
    for name, f in FIX.items():
        c, _ = build(name)
        assert XE.OBS_FIELDS == R.OBS_FIELDS == O.TCP_OBS_FIELDS[:12]
        assert all(len(k) == 6 for k in f["sockets"]) and all(len(v) == len(XE.FIVE) for v in f["values"]), name
        assert len(f["ips"]) == len(c["hv"]), name
        if name in FLOWS:   # the same run as the flow records' fixture: the observation changed no line
            assert (f["ips"], f["n_status"]) == (FLOWS[name]["ips"], FLOWS[name]["n_status"]), name
        obs = rows(name)
        assert len(obs) == len(f["rows"]) > 0 and all(len(r) == 12 for r in obs), name
        assert all(0 <= r[I["state"]] <= 10 for r in obs), name
        # every echo process is observed, on its own host, and a server's listener beside its child
        echo = [k for k in range(len(c["procs"])) if c.get("apps", [-1] * len(c["procs"]))[k] < 0]
        assert sorted({r[I["proc"]] for r in obs}) == echo, name
        assert all(c["procs"][r[I["proc"]]][0] == r[I["host"]] for r in obs), name
        for k in echo:
            states = {r[I["state"]] for r in obs if r[I["proc"]] == k}
            assert (ST["LISTEN"] in states) == (c["peers"][k] < 0), (name, k)


@pytest.mark.parametrize("name", CASES)
def test_oracle_observations_equal_the_reference(name):
    """row for row, all twelve fields, integers: no tolerance"""
    o = oracle(name)
    got = [r[:12] for r in o["obs"]]
    want = rows(name)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (name, i, dict(zip(XE.OBS_FIELDS, a)), dict(zip(XE.OBS_FIELDS, b)))
    assert len(got) == len(want), name


@pytest.mark.skipif(not R.observes(), reason="oracle/_ref/libshdref_loop.so not built with the observation "
                                             "(needs the reference tree)")
@pytest.mark.parametrize("name", LIVE)
def test_reference_loop_reproduces_the_fixture(name):
    c, m = build(name)
    r = R.run(m, c["graph"], procs=c["procs"], tcp=TC.tcp_arg(c), observe=True)
    assert r["ip"] == FIX[name]["ips"] and len(TC.status_lines(r["lines"])) == FIX[name]["n_status"]
    assert r["obs"] == rows(name)
    assert XE.pack(r["obs"]) == {k: FIX[name][k] for k in ("sockets", "values", "rows")}


@pytest.mark.parametrize("name", CASES)
def test_log_is_consistent_with_the_observations(name):
    """An observation is taken inside an event, the log's row after it.  Where
    the socket has no log row at the observation's own time -- no event of that
    instant changed it -- the log's latest row carries the observation's five
    values exactly.  Where it has one, the observation stands on one side of
    that instant's changes: it equals the log just before the instant or the
    log after it (a process is observed as it starts to run and again before
    it closes; its own calls change the socket in between)."""
    o = oracle(name)
    L = XE.Log(o["log"])
    assert O.TCP_LOG_FIELDS[7:] == XE.FIVE and O.TCP_OBS_FIELDS[7:12] == XE.FIVE
    strict = 0
    for r in o["obs"]:
        s, t, five = r[12], r[0], tuple(r[7:12])
        before, after = L.up_to(s, t - 1), L.up_to(s, t)
        assert after is not None, (name, r)
        if before == after:
            strict += 1
            assert five == after, (name, r, after)
        else:
            assert five in (before, after), (name, r, before, after)
    assert strict >= len(o["obs"]) // 2, (name, strict, len(o["obs"]))
    # the log's own shape: a socket's first row is its creation, and every later row differs from the one before
    for s, rr in L.by_sock.items():
        assert all(a[7:12] != b[7:12] for a, b in zip(rr, rr[1:])), (name, s)
        assert rr[0][7] in (ST["CLOSED"], ST["LISTEN"], ST["SYNSENT"], ST["SYNRECEIVED"]), (name, s, rr[0])
        assert rr[0][8:12] == [1, XE.SSTHRESH_INIT, 0, 0], (name, s, rr[0])


def meets(obs):
    """which of the conditions below one case's observation rows meet"""
    m = set()
    if any(r[I["ssthresh"]] < XE.SSTHRESH_INIT for r in obs):
        m.add("ssthresh")
    m |= {S.TCP_STATE_NAMES[r[I["state"]]] for r in obs}
    for v in by_socket(obs).values():
        cw = [r[I["cwnd"]] for r in v]
        if any(b > a for a, b in zip(cw, cw[1:])) and any(b < a for a, b in zip(cw, cw[1:])):
            m.add("cwnd_up_down")
        if len({(r[I["srtt"]], r[I["rttvar"]]) for r in v if r[I["srtt"]] > 0}) >= 3:
            m.add("rtt_moves")
        if any(is_rto_reset(a[7:12], b[7:12]) for a, b in zip(v, v[1:])):
            m.add("srtt_reset")
    return m


def is_rto_reset(a, b):
    """the five values of one socket before (a) and after (b): the reset of
    tcp.c's ACK processing after more than two back-offs.  srtt and rttvar are
    both 0 again, and reno's timeouts before it have brought ssthresh down and
    cwnd back to slow start.  The estimator's own update cannot do this from
    srtt >= 8: 7 * srtt / 8 stays positive (it takes srtt to 0 only from 1,
    as on the loopback pairs, and leaves cwnd and ssthresh alone)."""
    return (a[3] >= 8 and b[3] == 0 and b[4] == 0 and b[2] < XE.SSTHRESH_INIT and b[1] <= 10 + b[2])


# what each case's rows show, as the reference's loop gave them
MEETS = {
    "ref_epoll_lossy": {"ssthresh", "rtt_moves"},
    "lossy_2pct": {"ssthresh", "rtt_moves"},
    "slow_links": {"ssthresh", "rtt_moves", "cwnd_up_down"},
    "heavy_loss": {"ssthresh"},
    "shared_hosts_rr": {"ssthresh", "rtt_moves"},
    "server_first": {"ssthresh", "rtt_moves"},
    "loopback_pair": set(),
    "loopback_mixed": {"ssthresh", "rtt_moves"},
    "mixed_hosts": {"ssthresh", "rtt_moves"},
    "hub3_slow": {"ssthresh", "rtt_moves", "CLOSEWAIT"},
    "rto_reset": {"ssthresh", "srtt_reset"},
}


def test_fixture_is_not_vacuous():
    """on the reference's rows alone: the five fields move in the fixture, so
    the pin cannot hold on values that never change.  An echo process finds its
    sockets in four states only: LISTEN, SYNSENT (after its connect call),
    ESTABLISHED and -- when the peer's FIN arrives before the last data,
    hub3_slow -- CLOSEWAIT."""
    allm = set()
    for name in CASES:
        m = meets(rows(name))
        assert m - set(ST) == MEETS[name] - set(ST), (name, sorted(m))
        assert m & set(ST) == {"LISTEN", "SYNSENT", "ESTABLISHED"} | (MEETS[name] & set(ST)), (name, sorted(m))
        allm |= m
    assert {"ssthresh", "cwnd_up_down", "rtt_moves", "srtt_reset", "SYNSENT", "ESTABLISHED", "CLOSEWAIT"} <= allm


def test_the_logs_reach_what_follows_the_close():
    """only the oracle sees these (no process runs there): across the fixture
    cases' change logs some socket reaches FINWAIT1, TIMEWAIT or CLOSED, and
    LASTACK; and heavy_loss's log holds the srtt reset its observations miss.
    In rto_reset the observed reset is one event of the log, after three
    timeouts of that socket (cwnd back to 10 each time)"""
    seen = set()
    for name in CASES:
        seen |= {S.TCP_STATE_NAMES[r[7]] for r in oracle(name)["log"]}
    assert {"FINWAIT1", "FINWAIT2", "TIMEWAIT", "CLOSED", "LASTACK", "CLOSEWAIT", "CLOSING", "SYNRECEIVED"} <= seen
    for name in ("heavy_loss", "rto_reset"):
        L = XE.Log(oracle(name)["log"])
        hits = [(rr, i) for rr in L.by_sock.values() for i, (a, b) in enumerate(zip(rr, rr[1:]))
                if is_rto_reset(a[7:12], b[7:12])]
        assert len(hits) == 1, (name, len(hits))
        rr, i = hits[0]
        # ssthresh moves only in reno's timeout and its third duplicate ACK; the timeout alone leaves cwnd at 10
        assert sum(1 for a, b in zip(rr[:i + 1], rr[1:i + 1]) if b[8] == 10 and b[9] == a[8] // 2 + 1) >= 3, name
    for name in ("loopback_pair", "loopback_mixed"):   # no loss on a loopback path: no reset in the log either
        L = XE.Log(oracle(name)["log"])
        assert not any(is_rto_reset(a[7:12], b[7:12]) for rr in L.by_sock.values() for a, b in zip(rr, rr[1:])), name


def test_snapshots_off_records_nothing():
    """the flag off (bench.py's baseline, every other test): no rows, the same run"""
    c, m = build("lossy_2pct")
    o = O.tcp_run(m, c["graph"], TC.ip_ints(FIX["lossy_2pct"]["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"])
    assert "obs" not in o and "log" not in o
    assert o["lines"] == oracle("lossy_2pct")["lines"] and o["events"] == oracle("lossy_2pct")["events"]


def test_pack_round_trip():
    obs = [[5, 0, 1, 0, 80, 0, 0, 1, 1, XE.SSTHRESH_INIT, 0, 0], [5, 1, 0, 7, 9, 8, 80, 2, 1, XE.SSTHRESH_INIT, 0, 0],
           [9, 0, 1, 0, 80, 0, 0, 1, 1, XE.SSTHRESH_INIT, 0, 0]]
    p = XE.pack(obs)
    assert p["rows"] == [[5, 0, 0], [0, 1, 1], [4, 0, 0]] and len(p["sockets"]) == 2 and len(p["values"]) == 2
    assert XE.unpack(p) == obs
