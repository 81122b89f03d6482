"""Fixtures of the TCP models with hub hosts, from the reference's own loop --
TEST INFRASTRUCTURE.  Runs each case of tests/tcp_hub_cases.py through
oracle/_ref/libshdref_loop.so (the reference's worker.c, network_interface.c,
tracker.c, tcp.c ... compiled unmodified; oracle/Makefile `ref`) and stores
what a run must reproduce, with ref_tcp_options.json's keys: the host IPs, the
number and SHA-256 of the [STATUS] lines (in the serial order, and grouped by
host in each host's order) and of the tracker's [node] lines (by time and
host), every host's next event ID, next packet ID and RNG draw at the end; the
number of INET_DROPPED and ROUTER_DROPPED lines and the time of the first of
each (-1: none); plus the number of datagram [STATUS] lines and of
retransmission lines.

    python tests/golden/make_ref_tcp_hub.py [case ...]   # -> tests/golden/ref_tcp_hub.json
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "shadow-1_amd")]

import ref_loop_ffi as R  # noqa: E402
import tcp_cases as TC  # noqa: E402
import tcp_hub_cases as TH  # noqa: E402
import tcp_option_cases as TO  # noqa: E402


def record(name):
    """one case through the reference's loop: its fixture entry"""
    c, m = TH.build(name)
    r = R.run(m, c["graph"], procs=c["procs"], tcp=TC.tcp_arg(c))
    st = TC.status_lines(r["lines"])
    hb = TC.node_lines(r["lines"])
    n_inet, t_inet = TO.first_time(st, "INET_DROPPED")
    n_router, t_router = TO.first_time(st, "ROUTER_DROPPED")
    n_dgram = sum(1 for _, _, body in st if " bytes=" in body and " seq=" not in body)
    if "apps" in c:   # a mixed case must carry both transports
        assert n_dgram > 0, (name, "no datagram [STATUS] lines")
        assert n_dgram < len(st), name
    return dict(ips=r["ip"], n_status=len(st), status_sha256=TC.digest(st),
                n_heartbeat=len(hb), heartbeat_sha256=TC.digest(hb),
                status_by_host_sha256=TC.digest(TC.by_host(st)),
                next_event_id=[int(x) for x in r["next_event_id"]],
                next_packet_id=[int(x) for x in r["next_packet_id"]],
                rng_probe=[int(x) for x in r["rng_probe"]],
                n_inet_dropped=n_inet, first_inet_dropped=t_inet,
                n_router_dropped=n_router, first_router_dropped=t_router,
                n_datagram=n_dgram, n_retransmitted=TO.first_time(st, "[SND_TCP_RETRANSMITTED]")[0])


def main():
    path = os.path.join(HERE, "ref_tcp_hub.json")
    out = json.load(open(path)) if os.path.exists(path) else {}
    for name in sys.argv[1:] or list(TH.CASES):
        out[name] = record(name)
        print(name, out[name]["n_status"], out[name]["status_sha256"][:12], out[name]["n_heartbeat"],
              out[name]["n_inet_dropped"], out[name]["n_router_dropped"], out[name]["n_datagram"],
              out[name]["n_retransmitted"], flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
