"""What a run's path records (include/shdtcp.h shd_tcp_path) must hold, derived
from [STATUS] lines -- TEST INFRASTRUCTURE (tests/test_tcp_paths_ref_cpu.py,
tests/test_tcp_paths_gpu.py, tests/golden/make_ref_tcp_paths.py).

worker_sendPacket raises exactly one status for every packet it handles:
INET_SENT when the packet goes on (worker.c:290-306, also when its delivery
would fall past the end), INET_DROPPED when the path lost it (worker.c:319).
Each status prints a [STATUS] line with the packet's addresses and payload
(packet.c:552-615, 647-659): the TCP form

    [INET_SENT] packetID=h:n a.b.c.d:p -> a.b.c.d:p seq=... window=... bytes=N header=...

and the datagram form, which has no TCP header fields

    [INET_SENT] packetID=h:n a.b.c.d:p -> a.b.c.d:p bytes=N

So the records follow from the lines of a traced run: every such line of
either form counts once, under the key (vertex of the host that owns the
source address, vertex of the host that owns the destination address).  A
host's packets to its own address never reach worker_sendPacket (the loopback
task, network_interface.c:548-555) and print neither status.

Records come sorted by (v_src, v_dst), as shd_tcp_result_paths hands them out.
"""
import re

import numpy as np

_LINE = re.compile(r"\[(INET_SENT|INET_DROPPED)\] packetID=\d+:\d+ (\d+)\.(\d+)\.(\d+)\.(\d+):\d+ -> "
                   r"(\d+)\.(\d+)\.(\d+)\.(\d+):\d+ (?:seq=.*? )?bytes=(\d+)(?: |$)")

KEY = ("v_src", "v_dst")
COUNTS = ("packets_sent", "bytes_sent", "control_sent", "packets_dropped", "bytes_dropped")
TIMES = ("t_first", "t_last")
FIELDS = KEY + COUNTS + TIMES


def _ip(q):
    return (int(q[0]) << 24) | (int(q[1]) << 16) | (int(q[2]) << 8) | int(q[3])


def counted(lines):
    """(number of INET_SENT lines, number of INET_DROPPED lines) among (t, host, body) lines"""
    s = sum(1 for _, _, body in lines if body.startswith("[INET_SENT]"))
    d = sum(1 for _, _, body in lines if body.startswith("[INET_DROPPED]"))
    return s, d


def derive(lines, ips, hv):
    """[record dicts with the FIELDS keys] from (t, host, body) lines; ips:
    each host's address (host-order integer), hv: each host's vertex"""
    host_of = {}
    for h, ip in enumerate(ips):
        host_of.setdefault(int(ip), h)   # an address's first host (host order)
    recs = {}
    for t, h, body in lines:
        if not (body.startswith("[INET_SENT]") or body.startswith("[INET_DROPPED]")):
            continue
        m = _LINE.match(body)
        assert m, body   # every line of the two statuses counts: an unread one is an error
        g = m.groups()
        src, dst, nbytes = host_of[_ip(g[1:5])], host_of[_ip(g[5:9])], int(g[9])
        assert src == h, (body, h)   # raised by the sending host
        key = (int(hv[src]), int(hv[dst]))
        r = recs.get(key)
        if r is None:
            r = recs[key] = dict.fromkeys(COUNTS, 0)
            r.update(v_src=key[0], v_dst=key[1], t_first=t, t_last=t)
        r["t_first"] = min(r["t_first"], t)
        r["t_last"] = max(r["t_last"], t)
        if g[0] == "INET_SENT":
            r["packets_sent"] += 1
            r["bytes_sent"] += nbytes
            r["control_sent"] += nbytes == 0
        else:
            r["packets_dropped"] += 1
            r["bytes_dropped"] += nbytes
    return [recs[k] for k in sorted(recs)]


def rows(recs):
    """record dicts as lists in FIELDS order (what the fixture stores)"""
    return [[int(r[k]) for k in FIELDS] for r in recs]


def from_array(a):
    """a structured array of shd_tcp_path records as lists in FIELDS order"""
    a = np.asarray(a)
    return [list(x) for x in zip(*(a[k].tolist() for k in FIELDS))] if len(a) else []


def check(paths, want_rows, what=""):
    """the run's records against the expected rows, field by field"""
    got = from_array(paths)
    for i, (x, y) in enumerate(zip(got, want_rows)):
        assert x == list(y), (what, i, dict(zip(FIELDS, x)), dict(zip(FIELDS, y)))
    assert len(got) == len(want_rows), (what, len(got), len(want_rows))


def symmetric_sent(want_rows):
    """{(a, b) with a <= b: packets sent over the unordered pair} -- what the
    path cache's counter holds after the run (the reference's Path.packetCount:
    sent[a->b] + sent[b->a], or sent[a->a] once)"""
    out = {}
    i = FIELDS.index("packets_sent")
    for r in want_rows:
        k = (min(r[0], r[1]), max(r[0], r[1]))
        out[k] = out.get(k, 0) + r[i]
    return out
