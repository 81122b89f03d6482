"""Fixture of the TCP path's flow records (shd_tcp_flow), from the reference's
own loop -- TEST INFRASTRUCTURE.  Runs each case through
oracle/_ref/libshdref_loop.so (the reference's worker.c, network_interface.c,
tcp.c ... compiled unmodified; oracle/Makefile `ref`) and stores what
tests/tcp_flow_expect.py derives from its [STATUS] lines: per case the host
IPs, the records' pinned fields (tcp_flow_expect.PINNED, one row per record in
the records' order) and a few sums the CPU test's conditions read.  Nothing
stored comes from the oracle's restatement.

    python tests/golden/make_ref_tcp_flows.py [case ...]   # -> tests/golden/ref_tcp_flows.json
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "shadow-1_amd")]

import ref_loop_ffi as R  # noqa: E402
import tcp_cases as TC  # noqa: E402
import tcp_flow_expect as FE  # noqa: E402
import tcp_hub_cases as TH  # noqa: E402

ECHO = ["ref_epoll_lossy", "lossy_2pct", "slow_links", "heavy_loss", "geo_pairs", "shared_hosts_rr", "server_first",
        "loopback_pair", "loopback_mixed", "mixed_hosts", "mixed_slow_rr"]
HUB = ["hub12_fifo", "hub40_slow", "fan_out20"]
CASES = ECHO + HUB


def build(name):
    """(case dict, model) of a fixture case, from whichever module defines it"""
    return TC.build(name) if name in TC.CASES else TH.build(name)


def record(name):
    """one case through the reference's loop: its fixture entry"""
    c, m = build(name)
    r = R.run(m, c["graph"], procs=c["procs"], tcp=TC.tcp_arg(c))
    st = TC.status_lines(r["lines"])
    recs = FE.derive(st)
    n_router = sum(1 for _, _, body in st if body.startswith("[ROUTER_DROPPED]") and " seq=" in body)
    return dict(ips=r["ip"], n_status=len(st), fields=list(FE.PINNED), flows=FE.rows(recs),
                n_router_dropped_tcp=n_router, n_router_unattributed=FE.unattributed_router_drops(st))


def main():
    path = os.path.join(HERE, "ref_tcp_flows.json")
    out = json.load(open(path)) if os.path.exists(path) else {}
    for name in sys.argv[1:] or CASES:
        out[name] = record(name)
        f = out[name]
        i = {k: j for j, k in enumerate(FE.PINNED)}
        print(name, len(f["flows"]), "router", sum(x[i["router_dropped"]] for x in f["flows"]), f["n_router_dropped_tcp"],
              "socket", sum(x[i["socket_dropped"]] for x in f["flows"]),
              "retx", [x[i["retransmitted"]] for x in f["flows"]][:4], flush=True)
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")


if __name__ == "__main__":
    main()
