"""What a run's host-record series (include/shdtcp.h shd_host_sample; the
packet engine's SHD_QF_HOST_SERIES) must hold, derived from [STATUS] lines in
one pass -- TEST INFRASTRUCTURE (tests/test_eng_hseries_ref_cpu.py,
tests/test_eng_hseries_gpu.py, tests/golden/make_ref_eng_hseries.py).

The rule (include/shdgpu.h, shd_eng_host_series): with boundaries T_k = k I,
k >= 1, T_k < end, a host's record is touched by every line of a status the
record counts (tcp_host_expect.COUNTED); a touch at time t yields a sample
labelled with the first boundary after t, T = (t // I + 1) I -- a line at
exactly T_k belongs to the interval after it -- and the sample is the host's
whole record after every one of its lines with t < T, depth_end the queue's
length then.  No line in an interval: no sample; a boundary that is not before
`end`: no sample.

So the sample (h, T) is tcp_host_expect.derive(lines with t < T, H)[h], which is
how tests/test_eng_hseries_ref_cpu.py checks this module; here the records are
carried along the lines once and a host's sample is taken when its first line
at or past its pending boundary comes (or when the lines end).

A row is [t] + tcp_host_expect.FIELDS; rows are sorted by (host, t).
"""
import hashlib

import numpy as np

import tcp_host_expect as HE

FIELDS = ("t",) + HE.FIELDS


def _row(T, r, depth):
    return [T] + [depth if k == "depth_end" else int(r[k]) for k in HE.SCALARS] + [list(r["sojourn_hist"])]


def derive(lines, n_hosts, interval_ns, end_ns):
    """rows [t] + tcp_host_expect.FIELDS sorted by (host, t), from (t, host,
    body) lines in an order that keeps every host's own"""
    I, end_ns = int(interval_ns), int(end_ns)
    recs = []
    for h in range(n_hosts):
        r = dict.fromkeys(HE.SCALARS, 0)
        r.update(host=h, sojourn_hist=[0] * 16)
        recs.append(r)
    queue = [[] for _ in range(n_hosts)]
    pending = [0] * n_hosts    # the boundary a host's next sample is labelled with; 0: none
    out = [[] for _ in range(n_hosts)]
    for t, h, body in lines:
        st = body[1:body.index("]")]
        if st not in HE.COUNTED:
            continue
        m = HE._LINE.match(body)
        assert m, body
        pid, nbytes = m.group(2), int(m.group(3))
        r, q = recs[h], queue[h]
        if pending[h] and t >= pending[h]:   # the record before this line is the record at the boundary
            if pending[h] < end_ns:
                out[h].append(_row(pending[h], r, len(q)))
            pending[h] = 0
        if not pending[h]:
            pending[h] = (t // I + 1) * I
        if not r["t_first"]:
            r["t_first"] = t
        r["t_last"] = t
        if st == "ROUTER_ENQUEUED":
            q.append((pid, t))
            r["router_enqueued"] += 1
            r["router_enqueued_bytes"] += nbytes
            if len(q) > r["depth_max"]:
                r["depth_max"], r["t_depth_max"] = len(q), t
        elif st == "ROUTER_DEQUEUED":
            assert q and q[0][0] == pid, ("a dequeue that is not the queue's head", t, h, body)
            so = t - q.pop(0)[1]
            r["router_dequeued"] += 1
            r["router_dequeued_bytes"] += nbytes
            r["sojourn_sum"] += so
            if r["router_dequeued"] == 1 or so > r["sojourn_max"]:
                r["sojourn_max"], r["t_sojourn_max"] = so, t
            r["sojourn_hist"][HE.bucket(so)] += 1
        elif st == "ROUTER_DROPPED":
            assert q and q[0][0] == pid, ("a drop that is not the queue's head", t, h, body)
            q.pop(0)
            r["router_dropped"] += 1
            r["router_dropped_bytes"] += nbytes
        elif st == "RCV_INTERFACE_RECEIVED":
            r["if_received"] += 1
            r["if_received_bytes"] += nbytes
        elif st == "RCV_INTERFACE_DROPPED":
            r["if_dropped"] += 1
        elif st == "SND_INTERFACE_SENT":
            r["if_sent"] += 1
            r["if_sent_bytes"] += nbytes
        elif st == "SND_TCP_ENQUEUE_THROTTLED":
            r["tcp_throttled"] += 1
        else:
            r["tcp_unordered"] += 1
    for h in range(n_hosts):
        if pending[h] and pending[h] < end_ns:
            out[h].append(_row(pending[h], recs[h], len(queue[h])))
    return [row for per in out for row in per]


def on_boundary(lines, interval_ns):
    """the counted lines whose time is exactly a boundary"""
    I = int(interval_ns)
    return sum(1 for t, _, body in lines if t % I == 0 and t and body[1:body.index("]")] in HE.COUNTED)


def per_host(rows, n_hosts):
    """samples of each host"""
    n = [0] * n_hosts
    for r in rows:
        n[r[1]] += 1
    return n


def digest(rows) -> str:
    """SHA-256 of the canonical rows: one line per row, the values in FIELDS
    order (the histogram's 16 buckets last), decimal, comma-separated"""
    h = hashlib.sha256()
    for r in rows:
        h.update((",".join(str(int(v)) for v in r[:-1]) + "," + ",".join(str(int(v)) for v in r[-1]) + "\n").encode())
    return h.hexdigest()


def from_array(a):
    """an S.HOST_SAMPLE_DTYPE array as rows"""
    a = np.asarray(a)
    if not len(a):
        return []
    rec = a["rec"]
    return [list(x) for x in zip(*([a["t"].tolist()] + [rec[k].tolist() for k in HE.SCALARS] +
                                   [rec["sojourn_hist"].tolist()]))]


def check(samples, want_rows, what=""):
    """the run's samples against the expected rows, field by field"""
    got = from_array(samples)
    for i, (x, y) in enumerate(zip(got, want_rows)):
        assert x == list(y), (what, i, dict(zip(FIELDS, x)), dict(zip(FIELDS, y)))
    assert len(got) == len(want_rows), (what, len(got), len(want_rows))
