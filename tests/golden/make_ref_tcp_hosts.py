"""Fixture of the TCP path's host records (shd_tcp_hostrec), from the
reference's own loop -- TEST INFRASTRUCTURE.  Runs each case through
oracle/_ref/libshdref_loop.so (the reference's worker.c, router.c,
router_queue_codel.c, network_interface.c, tcp.c ... compiled unmodified;
oracle/Makefile `ref`) and stores what tests/tcp_host_expect.py derives from its
[STATUS] lines: per case the host IPs, the number of [STATUS] lines, the field
names and one row per host (tcp_host_expect.FIELDS: the scalars, then the
histogram's 16 buckets).  Nothing stored comes from the oracle's restatement.

    python tests/golden/make_ref_tcp_hosts.py [case ...]   # -> tests/golden/ref_tcp_hosts.json
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "shadow-1_amd")]

import ref_loop_ffi as R  # noqa: E402
import tcp_cases as TC  # noqa: E402
import tcp_host_expect as HE  # noqa: E402
import tcp_hub_cases as TH  # noqa: E402

CASES = ["hub40_slow", "slow_links", "mixed_slow_rr", "hub12_fifo", "geo_pairs", "loopback_pair", "lossy_2pct"]


def build(name):
    """(case dict, model) of a fixture case, from whichever module defines it"""
    return TC.build(name) if name in TC.CASES else TH.build(name)


def record(name):
    """one case through the reference's loop: its fixture entry"""
    c, m = build(name)
    r = R.run(m, c["graph"], procs=c["procs"], tcp=TC.tcp_arg(c))
    st = TC.status_lines(r["lines"])
    return dict(ips=r["ip"], n_status=len(st), fields=list(HE.FIELDS), rows=HE.rows(HE.derive(st, len(c["hv"]))))


def main():
    path = os.path.join(HERE, "ref_tcp_hosts.json")
    out = json.load(open(path)) if os.path.exists(path) else {}
    for name in sys.argv[1:] or CASES:
        out[name] = record(name)
        print(name, len(out[name]["rows"]), "hosts,", out[name]["n_status"], "lines:", HE.totals(out[name]["rows"]),
              flush=True)
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")


if __name__ == "__main__":
    main()
