"""What a run's host records (include/shdtcp.h shd_tcp_hostrec) must hold,
derived from [STATUS] lines -- TEST INFRASTRUCTURE
(tests/test_tcp_hosts_ref_cpu.py, tests/test_tcp_hosts_gpu.py,
tests/golden/make_ref_tcp_hosts.py).

Every field of a record is a count of lines of one status that the host itself
executed (the line's host), or follows from their times.  Each status prints a
[STATUS] line with the packet's ID and payload (packet.c:552-615, 647-659), the
TCP form

    [ROUTER_ENQUEUED] packetID=h:n a.b.c.d:p -> a.b.c.d:p seq=... window=... bytes=N header=...

and the datagram form, which has no TCP header fields

    [ROUTER_ENQUEUED] packetID=h:n a.b.c.d:p -> a.b.c.d:p bytes=N

  ROUTER_ENQUEUED (router.c:113)            router_enqueued, _bytes; the packet joins the
                                            host's queue with its time; depth_max is the
                                            queue's length right after, t_depth_max the
                                            first enqueue that reached it
  ROUTER_DEQUEUED (router.c:129)            router_dequeued, _bytes; the packet is the
                                            queue's head (asserted); its sojourn, the
                                            line's time minus its enqueue's, goes into
                                            sojourn_sum, sojourn_max (t_sojourn_max: the
                                            first dequeue that reached it) and bucket
                                            min(15, bit_length(sojourn >> 16)) of
                                            sojourn_hist
  ROUTER_DROPPED (router_queue_codel.c:139) router_dropped, _bytes; the packet is the
                                            queue's head (asserted): CoDel drops at the
                                            head, and the queue has no size limit
  RCV_INTERFACE_RECEIVED (network_interface.c:382)  if_received, _bytes
  RCV_INTERFACE_DROPPED (:411)              if_dropped
  SND_INTERFACE_SENT (:545)                 if_sent, _bytes
  SND_TCP_ENQUEUE_THROTTLED (tcp.c:743)     tcp_throttled
  RCV_TCP_ENQUEUE_UNORDERED (tcp.c:758)     tcp_unordered
  any of them                               t_first (the first), t_last (the last)

depth_end is what the queue still holds after the last line.  A record reads its
own host's lines in that host's order only, so the serial loop's lines and
lines grouped by host derive the same records.  One record per host, in host
order; a host without such a line has a record that is zero apart from `host`.
"""
import re

import numpy as np

_LINE = re.compile(r"\[(\w+)\] packetID=(\d+:\d+) \S+ -> \S+ (?:seq=.*? )?bytes=(\d+)(?: |$)")

SCALARS = ("host", "depth_max", "depth_end", "router_enqueued", "router_enqueued_bytes", "router_dequeued",
           "router_dequeued_bytes", "router_dropped", "router_dropped_bytes", "t_depth_max", "sojourn_sum",
           "sojourn_max", "t_sojourn_max", "if_received", "if_received_bytes", "if_dropped", "if_sent",
           "if_sent_bytes", "tcp_throttled", "tcp_unordered", "t_first", "t_last")
FIELDS = SCALARS + ("sojourn_hist",)   # a row: the scalars, then the 16 buckets as a list
COUNTED = {"ROUTER_ENQUEUED", "ROUTER_DEQUEUED", "ROUTER_DROPPED", "RCV_INTERFACE_RECEIVED",
           "RCV_INTERFACE_DROPPED", "SND_INTERFACE_SENT", "SND_TCP_ENQUEUE_THROTTLED", "RCV_TCP_ENQUEUE_UNORDERED"}


def bucket(sojourn_ns):
    """min(15, bit_length(sojourn_ns >> 16)): an integer rule, exact"""
    return min(15, (int(sojourn_ns) >> 16).bit_length())


def derive(lines, n_hosts):
    """[record dicts with the FIELDS keys], one per host 0 .. n_hosts-1, from
    (t, host, body) lines"""
    recs = []
    for h in range(n_hosts):
        r = dict.fromkeys(SCALARS, 0)
        r.update(host=h, sojourn_hist=[0] * 16)
        recs.append(r)
    queue = [[] for _ in range(n_hosts)]   # each host's router queue: (packetID, enqueue time), head first
    for t, h, body in lines:
        st = body[1:body.index("]")]
        if st not in COUNTED:
            continue
        m = _LINE.match(body)
        assert m, body   # every line of a counted status counts: an unread one is an error
        pid, nbytes = m.group(2), int(m.group(3))
        r, q = recs[h], queue[h]
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
            assert q and q[0][0] == pid, ("a dequeue that is not the queue's head", t, h, body, q[:1])
            so = t - q.pop(0)[1]
            r["router_dequeued"] += 1
            r["router_dequeued_bytes"] += nbytes
            r["sojourn_sum"] += so
            if r["router_dequeued"] == 1 or so > r["sojourn_max"]:
                r["sojourn_max"], r["t_sojourn_max"] = so, t
            r["sojourn_hist"][bucket(so)] += 1
        elif st == "ROUTER_DROPPED":
            assert q and q[0][0] == pid, ("a drop that is not the queue's head", t, h, body, q[:1])
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
    for r, q in zip(recs, queue):
        r["depth_end"] = len(q)
    return recs


def rows(recs):
    """record dicts as lists in FIELDS order (what the fixture stores)"""
    return [[int(r[k]) for k in SCALARS] + [[int(v) for v in r["sojourn_hist"]]] for r in recs]


def from_array(a):
    """a structured array of shd_tcp_hostrec records as lists in FIELDS order"""
    a = np.asarray(a)
    if not len(a):
        return []
    return [list(x) for x in zip(*([a[k].tolist() for k in SCALARS] + [a["sojourn_hist"].tolist()]))]


def check(hosts, want_rows, what=""):
    """the run's records against the expected rows, field by field"""
    got = from_array(hosts)
    for i, (x, y) in enumerate(zip(got, want_rows)):
        assert x == list(y), (what, i, dict(zip(FIELDS, x)), dict(zip(FIELDS, y)))
    assert len(got) == len(want_rows), (what, len(got), len(want_rows))


def totals(want_rows):
    """what the issue's table lists of a case's rows: (enqueued, dequeued,
    dropped, deepest queue, hosts that reached it, longest sojourn)"""
    i = {k: j for j, k in enumerate(SCALARS)}
    dm = max(r[i["depth_max"]] for r in want_rows)
    return (sum(r[i["router_enqueued"]] for r in want_rows), sum(r[i["router_dequeued"]] for r in want_rows),
            sum(r[i["router_dropped"]] for r in want_rows), dm,
            sum(1 for r in want_rows if r[i["depth_max"]] == dm), max(r[i["sojourn_max"]] for r in want_rows))
