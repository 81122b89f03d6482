"""What a host's pcap capture must hold, derived from [STATUS] lines -- TEST
INFRASTRUCTURE (tests/test_tcp_pcap_gpu.py).

The reference captures a packet at two code points of its interface
(network_interface.c:416-418 after a receive, :572-574 after a send).  Each
sits a few statements after a packet_addDeliveryStatus call by the same host at
the same simulated time: PDS_RCV_INTERFACE_RECEIVED (:382) and
PDS_SND_INTERFACE_SENT (:545), whose [STATUS] line prints every header field
the capture record holds (packet.c:552-615).  So a host's capture is its
lines with these two statuses, in order, per direction.  The lines themselves
are pinned to the reference's loop (tests/golden/ref_tcp.json, oracle/o_tcp.c).

The interleaving of the two directions inside one nanosecond is NOT derivable
from the lines: the received packet is captured after its socket processed it
(socket_pushInPacket, :408), and the socket may send inside that call
(tcp.c's _tcp_sendControlPacket / _tcp_flush -> socket_addToOutputBuffer ->
networkinterface_wantsSend -> _networkinterface_sendPackets, :604), whose
capture then precedes the received packet's although its line follows.  The
comparison therefore holds each direction's order within a timestamp, and
the sequence of timestamps, but not the interleaving.
"""
import re

import numpy as np

import shdgpu as S

_LINE = re.compile(r"\[(\w+)\] packetID=\d+:\d+ (\d+)\.(\d+)\.(\d+)\.(\d+):(\d+) -> (\d+)\.(\d+)\.(\d+)\.(\d+):(\d+) "
                   r"seq=(\d+) ack=(\d+) sack=[-0-9NA ]+? window=(\d+) bytes=(\d+) header=(\S*) ")   # sack: "34-62 64"
_DIR = {"SND_INTERFACE_SENT": S.PCAP_OUT, "RCV_INTERFACE_RECEIVED": S.PCAP_IN}
FIELDS = ("time", "dir", "src_ip", "dst_ip", "src_port", "dst_port", "seq", "ack", "win", "len", "flags")


def _flags(header):
    h = header.replace("DUPACK", "")   # packet.c:603-606 prints DUPACK beside ACK: not a header bit of its own
    return ((S.PCAP_RST if "RST" in h else 0) | (S.PCAP_SYN if "SYN" in h else 0) |
            (S.PCAP_FIN if "FIN" in h else 0) | (S.PCAP_ACK if "ACK" in h else 0))


def expect(lines, hosts):
    """{host: [record tuples in FIELDS order]} from (t, host, body) lines, each
    host's in its own order"""
    out = {h: [] for h in hosts}
    for t, h, body in lines:
        if h not in out or not body.startswith(("[SND_INTERFACE_SENT]", "[RCV_INTERFACE_RECEIVED]")):
            continue
        m = _LINE.match(body)
        assert m, body   # a datagram's line has no seq=: capture hosts run TCP only
        g = m.groups()
        ip = lambda q: (int(q[0]) << 24) | (int(q[1]) << 16) | (int(q[2]) << 8) | int(q[3])  # noqa: E731
        out[h].append((t, _DIR[g[0]], ip(g[1:5]), ip(g[6:10]), int(g[5]), int(g[10]), int(g[11]), int(g[12]),
                       int(g[13]), int(g[14]), _flags(g[15])))
    return out


def tuples(records):
    """a host's capture records (S.PCAP_DTYPE) as tuples in FIELDS order"""
    r = np.asarray(records, dtype=S.PCAP_DTYPE)
    return list(zip(*(r[f].tolist() for f in FIELDS)))


def check_host(records, want, host=None):
    """The comparison: the sequence of distinct timestamps is equal, and within
    one timestamp the out records are equal and in order, and the in records
    are equal and in order (hence the multisets are equal)."""
    got = tuples(records)
    times = lambda x: [t for i, t in enumerate(r[0] for r in x) if i == 0 or x[i - 1][0] != t]  # noqa: E731
    assert times(got) == times(want), (host, "timestamps", len(got), len(want))
    assert [r[0] for r in got] == sorted(r[0] for r in got), (host, "time goes backwards")
    for d in (S.PCAP_OUT, S.PCAP_IN):
        a, b = [r for r in got if r[1] == d], [r for r in want if r[1] == d]
        for i, (x, y) in enumerate(zip(a, b)):
            assert x == y, (host, "dir", d, i, dict(zip(FIELDS, x)), dict(zip(FIELDS, y)))
        assert len(a) == len(b), (host, "dir", d, len(a), len(b))


def check(pcap_records, lines):
    """every captured host of a run against the lines' expectation"""
    want = expect(lines, list(pcap_records))
    for h, r in pcap_records.items():
        check_host(r, want[h], h)
