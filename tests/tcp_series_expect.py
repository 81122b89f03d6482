"""What a run's flow time series (include/shdtcp.h shd_tcp_sample,
SHD_TCP_OPT_SERIES) must hold, derived from [STATUS] lines -- TEST
INFRASTRUCTURE (tests/test_tcp_series_ref_cpu.py, tests/test_tcp_series_gpu.py,
tests/golden/make_ref_tcp_series.py).

The rule (shdtcp.h): the boundaries are T_k = k * I for k >= 1 and T_k <
end_time.  A flow record is touched when one of the six counted statuses is
attributed to it (tcp_flow_expect's attribution: SND_CREATED,
SND_TCP_RETRANSMITTED, INET_DROPPED to the sending tuple; RCV_SOCKET_DELIVERED,
RCV_SOCKET_DROPPED, ROUTER_DROPPED to the mirrored one; RCV_SOCKET_PROCESSED
sets t_established and does not count).  A touched record yields one sample
labelled with the first boundary after the touch -- a touch at exactly T_k
belongs to T_(k+1) -- holding its cumulative counters after every event of its
host before that boundary.  An interval without a touch yields no sample; a
last touch whose boundary is not before end_time yields none either (the flow
record is the end state).

A record's counters change with its own touches only, all raised on its own
host, so each record is followed along its host's lines in their order: the
sample of a touched record is taken when its next touch comes at or past the
boundary, or at the end of the lines.

The five snapshot fields of a sample (SNAPSHOT) are not in the lines: they are
held to the oracle's change log just before the sample's boundary
(tests/tcp_snapshot_expect.py, tests/test_tcp_snapshots_gpu.py), which is
pinned to the reference's tcp_getInfo values from a socket's creation until
its process closes it, and oracle-to-device only after the close.

Rows are [flow, t, bytes_delivered, packets_created, bytes_created,
retransmitted, inet_dropped, socket_dropped, router_dropped], flow the
record's index in tcp_flow_expect.derive's order, sorted by (flow, t).
"""
import numpy as np

import tcp_flow_expect as FE

COUNTS = FE.COUNTS
FIELDS = ("flow", "t") + COUNTS
SNAPSHOT = FE.SNAPSHOT


def derive(lines, interval_ns, end_ns):
    """rows from (t, host, body) lines (any order that keeps each host's own)"""
    interval_ns, end_ns = int(interval_ns), int(end_ns)
    assert interval_ns > 0
    flows = {}
    order = []
    out = []   # (key, boundary, counters)

    def touch(key, f, t):
        if f["due"] and t >= f["due"]:
            out.append((key, f["due"], [f[k] for k in COUNTS]))
        f["due"] = (t // interval_ns + 1) * interval_ns

    for t, h, body in lines:
        st = body[1:body.index("]")]
        if st not in FE._SENDER and st not in FE._RECEIVER:
            continue
        m = FE._LINE.match(body)
        if not m:
            continue   # a datagram's line: datagram sockets have no record
        g = m.groups()
        src, sport, dst, dport = FE._ip(g[1:5]), int(g[5]), FE._ip(g[6:10]), int(g[10])
        nbytes = int(g[14])
        if st in FE._SENDER:
            key = (src, sport, dst, dport)
            f = flows.get(key)
            if st == "SND_CREATED":
                if f is None:
                    f = dict.fromkeys(COUNTS, 0)
                    f.update(host=h, due=0)
                    flows[key] = f
                    order.append(key)
                assert f["host"] == h, (key, h)
                touch(key, f, t)
                f["packets_created"] += 1
                f["bytes_created"] += nbytes
            elif f is not None:
                assert f["host"] == h, (key, h)
                touch(key, f, t)
                f["retransmitted" if st == "SND_TCP_RETRANSMITTED" else "inet_dropped"] += 1
        else:
            key = (dst, dport, src, sport)
            f = flows.get(key)
            if f is None or f["host"] != h or st == "RCV_SOCKET_PROCESSED":
                continue
            touch(key, f, t)
            if st == "RCV_SOCKET_DELIVERED":
                f["bytes_delivered"] += nbytes
            elif st == "RCV_SOCKET_DROPPED":
                f["socket_dropped"] += 1
            else:
                f["router_dropped"] += 1
    for key in order:
        f = flows[key]
        if f["due"] and f["due"] < end_ns:
            out.append((key, f["due"], [f[k] for k in COUNTS]))
    pos = {k: i for i, k in enumerate(order)}
    idx = {k: i for i, k in enumerate(sorted(order, key=lambda k: (flows[k]["host"], pos[k])))}
    return sorted([idx[k], b] + c for k, b, c in out)


def from_array(a):
    """a structured array of shd_tcp_sample records as rows in FIELDS order"""
    a = np.asarray(a)
    return [list(x) for x in zip(*(a[k].tolist() for k in FIELDS))] if len(a) else []


def check(series, want_rows, what=""):
    """the run's samples against the derived rows, row by row"""
    got = from_array(series)
    for i, (x, y) in enumerate(zip(got, want_rows)):
        assert x == list(y), (what, i, dict(zip(FIELDS, x)), dict(zip(FIELDS, y)))
    assert len(got) == len(want_rows), (what, len(got), len(want_rows))


def boundary_lines(lines, interval_ns):
    """how many lines fall exactly on a boundary (the "at T_k belongs after" rule at work)"""
    return sum(1 for t, _, _ in lines if t % int(interval_ns) == 0)
