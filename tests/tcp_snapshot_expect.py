"""The five snapshot fields of shd_tcp_flow / shd_tcp_sample (state, cwnd,
ssthresh, srtt, rttvar) as the oracle's change log gives them -- TEST
INFRASTRUCTURE.

The pin has two links.  The reference exports the five through tcp_getInfo
(tcp.c; getsockopt(TCP_INFO)'s source), but it can be observed only where a
process runs: oracle/ref_harness/ref_loop.c records them each time an echo
process runs, after its connect call and before each of its closes
(tests/golden/ref_tcp_snapshots.json), and the oracle (oracle/o_tcp.c,
o_tcp_out.obs) must give the same rows (tests/test_tcp_snapshots_ref_cpu.py).
The device samples at interval boundaries and at the end of the run, where no
process runs: there the oracle's change log (o_tcp_out.log: a row after every
event that changed one of a socket's five) is the expectation
(tests/test_tcp_snapshots_gpu.py).  So the reference pins a socket from its
creation until its process closes it; what follows the close (the FIN
exchange, TIMEWAIT, CLOSED) is pinned oracle-to-device only.

pack / unpack: the fixture's encoding of observation rows (every row kept: a
table of the sockets' addresses, a table of the distinct value tuples, and per
row the time since the row before and an index into each).
Log: a change log by socket, read at a sample's label or at the end.
"""
import bisect

FIVE = ("state", "cwnd", "ssthresh", "srtt", "rttvar")
# ref_loop_ffi.OBS_FIELDS / oracle_ffi.TCP_OBS_FIELDS[:12]
OBS_FIELDS = ("t", "host", "proc", "local_ip", "local_port", "peer_ip", "peer_port") + FIVE
SSTHRESH_INIT = 0x7fffffff   # tcp_cong_reno_init


def pack(obs):
    """observation rows (OBS_FIELDS) -> dict(sockets, values, rows)"""
    socks, vals, rows = {}, {}, []
    last = 0
    for r in obs:
        assert len(r) == len(OBS_FIELDS) and r[0] >= last
        s = socks.setdefault(tuple(r[1:7]), len(socks))
        v = vals.setdefault(tuple(r[7:12]), len(vals))
        rows.append([r[0] - last, s, v])
        last = r[0]
    return dict(sockets=[list(k) for k in socks], values=[list(k) for k in vals], rows=rows)


def unpack(f):
    """pack's inverse"""
    out, t = [], 0
    for dt, s, v in f["rows"]:
        t += dt
        out.append([t] + list(f["sockets"][s]) + list(f["values"][v]))
    return out


class Log:
    """o_tcp_out.log (oracle_ffi.TCP_LOG_FIELDS: t, host, sock, local ip, local
    port, peer ip, peer port, the five) by socket.  A socket is named by (host,
    local port, peer ip, peer port) as its last row has them: the host stands
    for the local address, which for a listener's child is the listener's
    INADDR_ANY in the reference and the host's address in a flow record."""

    def __init__(self, log):
        self.by_sock = {}
        for r in log:
            self.by_sock.setdefault(r[2], []).append(r)
        self.key = {}
        for s, rows in self.by_sock.items():
            assert all(a[0] <= b[0] for a, b in zip(rows, rows[1:])), s
            _, host, _, _, lport, pip, pport = rows[-1][:7]
            if pport == 0:   # a listener, or a socket that never connected: no flow record
                continue
            k = (host, lport, pip, pport)
            assert k not in self.key, k
            self.key[k] = s
        self.times = {s: [r[0] for r in rows] for s, rows in self.by_sock.items()}

    def n_connections(self):
        """sockets with a peer: the ones that have a flow record"""
        return len(self.key)

    def sock(self, host, local_port, peer_ip, peer_port):
        return self.key[(int(host), int(local_port), int(peer_ip), int(peer_port))]

    def at_end(self, s):
        """the five when the run ends: the socket's last row"""
        return tuple(self.by_sock[s][-1][7:12])

    def before(self, s, t):
        """the five as a sample labelled t holds them: the last row of an event
        strictly before t (an event at a boundary opens the next interval)"""
        i = bisect.bisect_left(self.times[s], int(t))
        assert i > 0, (s, t)   # a sampled record was touched before its boundary
        return tuple(self.by_sock[s][i - 1][7:12])

    def up_to(self, s, t):
        """the five after every event at or before t (None: no row yet)"""
        i = bisect.bisect_right(self.times[s], int(t))
        return tuple(self.by_sock[s][i - 1][7:12]) if i else None


def flow_five(r):
    return tuple(int(r[k]) & 0xffffffff for k in FIVE)


def check_flows(flows, log, what=""):
    """every flow record's five fields against the log's last row of its socket"""
    L = log if isinstance(log, Log) else Log(log)
    assert len(flows) == L.n_connections(), (what, len(flows), L.n_connections())
    seen = set()
    for r in flows:
        s = L.sock(r["host"], r["local_port"], r["peer_ip"], r["peer_port"])
        assert s not in seen, (what, s)
        seen.add(s)
        assert flow_five(r) == L.at_end(s), (what, int(r["host"]), int(r["local_port"]), flow_five(r), L.at_end(s))
    return L


def check_samples(series, flows, log, what=""):
    """every sample's five fields against the log just before its label"""
    L = log if isinstance(log, Log) else Log(log)
    for x in series:
        f = flows[int(x["flow"])]
        assert int(f["host"]) == int(x["host"])
        s = L.sock(f["host"], f["local_port"], f["peer_ip"], f["peer_port"])
        want = L.before(s, x["t"])
        assert flow_five(x) == want, (what, int(x["host"]), int(f["local_port"]), int(x["t"]), flow_five(x), want)
    return L
