"""TCP models with hub hosts: one host that many others talk to -- TEST
INFRASTRUCTURE.

test_tcp.c's server makes a listener and one child per connecting peer and
serves one peer, so a host that serves n clients runs n server processes and
ends the run holding 2 n sockets; a host with n clients holds n.  The
reference's own loop (oracle/_ref/libshdref_loop.so, app 1) runs the cases
for tests/golden/ref_tcp_hub.json (tests/golden/make_ref_tcp_hub.py); the
oracle (oracle/o_tcp.c) and the GPU's TCP path must reproduce that
(tests/test_tcp_hub_ref_cpu.py, tests/test_tcp_hub_gpu.py).

All but hub12_mixed sit on W.geometric_graph(12, seed=5, loss_max=0.01) with
the hub on vertex 0 and the other hosts on vertices 1 + i % 11, end at 40 s.

  hub12_fifo   host 0: 12 servers at 1 s + i ns; hosts 1..12: one client each
               at 2 s + i us; 40 000 B.  24 sockets and 12 processes on one
               host: past 8 of either, past 16 entries in the interface's queue
  hub40_rr     the same with 40 servers, 20 000 B, the round-robin qdisc: 80
               sockets -- the ring and the socket directory past one wave's
               width, round robin over 40 children
  hub40_slow   40 servers, 20 000 B, fifo, 1024 KiB/s both ways: the hub's
               CoDel queue fills (ROUTER_DROPPED, retransmissions).  The oracle
               loses 69 of the reference's ROUTER_DROPPED lines here (and their
               PDS_DESTROYED lines) while its counters agree: ORACLE_LINES
               leaves the case out
  fan_out20    host 0: 20 clients at 2 s + 777 i ns; hosts 1..20: one server
               each at 1 s; 30 000 B: many client sockets and ports drawn from
               one RNG, the port search over 20 sockets
  hub12_mixed  hub12_fifo at 30 000 B, end 30 s, loss 0.02, plus a datagram
               process on the hub (a socket per datagram to a weighted host,
               3 at start, one per datagram read) and a listener on host 1 that
               answers each datagram: 24 TCP sockets and the per-datagram ones
               in one directory, slots released and reused.  The hub's
               weights send every datagram to host 1.
"""
import functools

import numpy as np

import shdgpu as S
import tcp_cases as TC
import workloads as W

SEC = S.SHD_SEC


def _hub(n, nbytes, end=40, loss=0.01, **extra):
    g = W.geometric_graph(12, seed=5, loss_max=loss)
    procs = [(0, SEC + i) for i in range(n)] + [(1 + i, 2 * SEC + i * 1000) for i in range(n)]
    c = dict(graph=g, hv=[0] + [1 + i % 11 for i in range(n)], procs=procs, peers=[-1] * n + list(range(n)),
             nbytes=nbytes, end=end, bw={})
    c.update(extra)
    return c


def _fan_out(n, nbytes):
    g = W.geometric_graph(12, seed=5, loss_max=0.01)
    procs = [(1 + i, SEC) for i in range(n)] + [(0, 2 * SEC + 777 * i) for i in range(n)]
    return dict(graph=g, hv=[0] + [1 + i % 11 for i in range(n)], procs=procs, peers=[-1] * n + list(range(n)),
                nbytes=nbytes, end=40, bw={})


def _hub_mixed():
    c = _hub(12, 30000, end=30, loss=0.02)
    H = len(c["hv"])
    c["procs"] = c["procs"] + [(0, SEC + 500), (1, SEC)]
    c["peers"] = c["peers"] + [-1, -1]
    c["apps"] = [-1] * 24 + [0, 1]
    c["specs"] = [(TC.EACH, TC.WEIGHTED, 3, 1), (TC.LISTENER, TC.REPLY, 0, 1)]
    c["app_peer"] = [-1] * H
    c["payload"] = 700
    w = np.zeros(H)
    w[1] = 1.0   # every weighted draw picks host 1, the one datagram listener
    c["dest_cum"] = W.phold_cum(w)
    return c


CASES = {
    "hub12_fifo": lambda: _hub(12, 40000),
    "hub40_rr": lambda: _hub(40, 20000, qdisc=1),
    "hub40_slow": lambda: _hub(40, 20000, bw=dict(bw_down=1024, bw_up=1024)),
    "fan_out20": lambda: _fan_out(20, 30000),
    "hub12_mixed": _hub_mixed,
}

# the cases whose lines the oracle reproduces, and the one of which it
# reproduces the counters only (the module comment)
ORACLE_LINES = ["hub12_fifo", "hub40_rr", "fan_out20", "hub12_mixed"]
ORACLE_COUNTERS = ["hub40_slow"]
# the cases the CPU test reruns through the reference's loop
LIVE = ["hub12_fifo", "fan_out20"]


def build(name):
    """(case dict as tcp_cases.CASES makes them, model)"""
    c = CASES[name]()
    m = W.phold_model(np.asarray(c["hv"], dtype=np.int32), end_time=c["end"] * SEC, trace=True,
                      queue_flags=S.SHD_QF_TRACE_STATUS, load=0, payload=c.get("payload", 1),
                      dest_cum=c.get("dest_cum"), **c["bw"])
    return c, m


def slots_by_rule(procs, peers, apps=None):
    """each host's socket slots by include/shdtcp.h's rule, as {host: slots}:
    a listener and a child per client naming it for each server, one per
    client, 16 for a datagram process"""
    out = {}
    for k, (h, _) in enumerate(procs):
        if apps is not None and apps[k] >= 0:
            n = 16
        elif peers[k] >= 0:
            n = 1
        else:
            n = 1 + sum(1 for p in peers if p == k)
        out[h] = out.get(h, 0) + n
    return out


def procs_per_host(procs):
    out = {}
    for h, _ in procs:
        out[h] = out.get(h, 0) + 1
    return out


def hub100():
    """workloads.tcp_hub_model at 100 hosts: four hubs of 24 clients each (48
    sockets, 24 processes), two blocks of lanes, the hubs at hosts 0, 25, 50
    (one block) and 75 (the other); lossy links"""
    g, m, ips, procs, peers, nb = W.tcp_hub_model(4, 24, 40, nbytes=20000, loss_max=0.02)
    return g, m, ips, procs, peers, nb


@functools.lru_cache(maxsize=None)
def hub100_oracle():
    """the oracle's run of hub100 (computed once, never changed)"""
    import oracle_ffi as O
    g, m, ips, procs, peers, nb = hub100()
    return O.tcp_run(m, g, ips, procs, peers, nbytes=nb)
