"""What a run's flow records (include/shdtcp.h shd_tcp_flow) must hold, derived
from [STATUS] lines -- TEST INFRASTRUCTURE (tests/test_tcp_flows_ref_cpu.py,
tests/test_tcp_flows_gpu.py, tests/golden/make_ref_tcp_flows.py).

Every pinned field of a record is defined by a packet status the reference
raises (packet_addDeliveryStatus), and each status prints a [STATUS] line with
the packet's addresses, flags and payload (packet.c:552-615, 647-659).  So the
records follow from the lines of a traced run, keyed by the endpoint's
4-tuple (local ip, local port, peer ip, peer port):

  statuses the SENDING socket raises go to (src, sport, dst, dport):
    SND_CREATED            a record exists from its first one on (t_open);
                           packets_created, bytes_created; the first that
                           carries FIN is t_fin (tcp.c:791-835)
    SND_TCP_RETRANSMITTED  retransmitted (tcp.c:1060)
    INET_DROPPED           inet_dropped (worker.c:281-290)
  statuses raised where the packet ARRIVES go to the mirrored tuple
  (dst, dport, src, sport), the endpoint the packet is addressed to:
    RCV_SOCKET_PROCESSED   the first one of a packet carrying ACK is
                           t_established: a SYNSENT socket's first packet from
                           its peer with ACK is the SYN+ACK (tcp.c:1859-1865),
                           and a SYNRECEIVED child is established by any ACK
                           (tcp.c:1885-1887); the child's record exists from
                           its SYN+ACK on, so the SYN that made it (no ACK, and
                           before the record) never counts
    RCV_SOCKET_DELIVERED   t_last_delivered, bytes_delivered (tcp.c:2226, 2266)
    RCV_SOCKET_DROPPED     socket_dropped
    ROUTER_DROPPED         router_dropped (router_queue_codel.c's drop, at the
                           receiving host's upstream router)
  A status whose tuple has no record (a SYN dropped at a listener's router
  before any child exists) is counted nowhere.

All of one record's statuses are raised on its own host, so each record
depends on that host's lines in that host's order only: the derivation gives
the same records from the serial loop's lines and from lines grouped by host.

Records come in the order of the run's: by host, then by the socket's
creation on its host -- a connecting socket and a listener's child create
their first packet in the event that creates the socket, so that is the order
of the first SND_CREATED lines of the host.

The five snapshot fields (state, cwnd, ssthresh, srtt, rttvar) and proc are not
in the lines; role is (0: the first packet is a SYN without ACK).  The five are
pinned elsewhere: to the oracle's change log (tests/tcp_snapshot_expect.py,
tests/test_tcp_snapshots_gpu.py), which holds the reference's tcp_getInfo values
from a socket's creation until its process closes it
(tests/test_tcp_snapshots_ref_cpu.py); after the close, oracle-to-device only.
"""
import re

import numpy as np

_LINE = re.compile(r"\[(\w+)\] packetID=\d+:\d+ (\d+)\.(\d+)\.(\d+)\.(\d+):(\d+) -> (\d+)\.(\d+)\.(\d+)\.(\d+):(\d+) "
                   r"seq=(\d+) ack=(\d+) sack=[-0-9NA ]+? window=(\d+) bytes=(\d+) header=(\S*) ")

ADDR = ("host", "local_ip", "local_port", "peer_ip", "peer_port", "role")
TIMES = ("t_open", "t_established", "t_last_delivered", "t_fin")
COUNTS = ("bytes_delivered", "packets_created", "bytes_created", "retransmitted", "inet_dropped", "socket_dropped",
          "router_dropped")
PINNED = ADDR + TIMES + COUNTS
SNAPSHOT = ("state", "cwnd", "ssthresh", "srtt", "rttvar")

_SENDER = {"SND_CREATED", "SND_TCP_RETRANSMITTED", "INET_DROPPED"}
_RECEIVER = {"RCV_SOCKET_PROCESSED", "RCV_SOCKET_DELIVERED", "RCV_SOCKET_DROPPED", "ROUTER_DROPPED"}


def _ip(q):
    return (int(q[0]) << 24) | (int(q[1]) << 16) | (int(q[2]) << 8) | int(q[3])


def derive(lines):
    """[record dicts with the PINNED keys] from (t, host, body) lines, in the
    records' order (by host, then by first SND_CREATED on the host)"""
    flows = {}
    order = []
    for t, h, body in lines:
        st = body[1:body.index("]")]
        if st not in _SENDER and st not in _RECEIVER:
            continue
        m = _LINE.match(body)
        if not m:
            continue   # a datagram's line (no seq=): datagram sockets have no record
        g = m.groups()
        src, sport, dst, dport = _ip(g[1:5]), int(g[5]), _ip(g[6:10]), int(g[10])
        nbytes, flags = int(g[14]), g[15]
        if st in _SENDER:
            key = (src, sport, dst, dport)
            f = flows.get(key)
            if st == "SND_CREATED":
                if f is None:
                    f = dict.fromkeys(TIMES + COUNTS, 0)
                    f.update(host=h, local_ip=src, local_port=sport, peer_ip=dst, peer_port=dport,
                             role=0 if ("SYN" in flags and "ACK" not in flags) else 1, t_open=t)
                    flows[key] = f
                    order.append(key)
                assert f["host"] == h, (key, h)
                f["packets_created"] += 1
                f["bytes_created"] += nbytes
                if "FIN" in flags and not f["t_fin"]:
                    f["t_fin"] = t
            elif f is not None:
                assert f["host"] == h, (key, h)
                f["retransmitted" if st == "SND_TCP_RETRANSMITTED" else "inet_dropped"] += 1
        else:
            f = flows.get((dst, dport, src, sport))
            if f is None or f["host"] != h:
                continue
            if st == "RCV_SOCKET_PROCESSED":
                if not f["t_established"] and "ACK" in flags:
                    f["t_established"] = t
            elif st == "RCV_SOCKET_DELIVERED":
                f["t_last_delivered"] = t
                f["bytes_delivered"] += nbytes
            elif st == "RCV_SOCKET_DROPPED":
                f["socket_dropped"] += 1
            else:
                f["router_dropped"] += 1
    pos = {k: i for i, k in enumerate(order)}
    return [flows[k] for k in sorted(order, key=lambda k: (flows[k]["host"], pos[k]))]


def rows(recs):
    """record dicts as tuples in PINNED order (what the fixture stores)"""
    return [[int(r[k]) for k in PINNED] for r in recs]


def from_array(a):
    """a structured array of shd_tcp_flow records as tuples in PINNED order"""
    a = np.asarray(a)
    return [list(x) for x in zip(*(a[k].tolist() for k in PINNED))] if len(a) else []


def check(flows, want_rows, what=""):
    """the run's records against the derived rows, field by field"""
    got = from_array(flows)
    for i, (x, y) in enumerate(zip(got, want_rows)):
        assert x == list(y), (what, i, dict(zip(PINNED, x)), dict(zip(PINNED, y)))
    assert len(got) == len(want_rows), (what, len(got), len(want_rows))


def unattributed_router_drops(lines):
    """ROUTER_DROPPED lines of TCP packets whose tuple has no record when the
    line is raised (the derivation counts them nowhere)"""
    seen, n = set(), 0
    for t, h, body in lines:
        m = _LINE.match(body)
        if not m:
            continue
        g = m.groups()
        src, sport, dst, dport = _ip(g[1:5]), int(g[5]), _ip(g[6:10]), int(g[10])
        if g[0] == "SND_CREATED":
            seen.add((src, sport, dst, dport))
        elif g[0] == "ROUTER_DROPPED" and (dst, dport, src, sport) not in seen:
            n += 1
    return n
