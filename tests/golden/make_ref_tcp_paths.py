"""Fixture of the TCP path's path records (shd_tcp_path), from the reference's
own loop -- TEST INFRASTRUCTURE.  Runs each case through
oracle/_ref/libshdref_loop.so (the reference's worker.c, network_interface.c,
tcp.c ... compiled unmodified; oracle/Makefile `ref`) and stores what
tests/tcp_path_expect.py derives from its [STATUS] lines: per case the host
IPs, the number of status lines, of INET_SENT and of INET_DROPPED lines, and
the records (tcp_path_expect.FIELDS, one row per record, sorted by the key).
Rows only, no lines.  Nothing stored comes from the oracle's restatement.

    python tests/golden/make_ref_tcp_paths.py [case ...]   # -> tests/golden/ref_tcp_paths.json
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "shadow-1_amd")]

import ref_loop_ffi as R  # noqa: E402
import tcp_cases as TC  # noqa: E402
import tcp_hub_cases as TH  # noqa: E402
import tcp_path_expect as PE  # noqa: E402

CASES = ["lossy_2pct", "geo_pairs", "shared_hosts_rr", "loopback_mixed", "mixed_hosts", "mixed_slow_rr", "hub12_fifo",
         "hub40_slow"]


def build(name):
    """(case dict, model) of a fixture case, from whichever module defines it"""
    return TC.build(name) if name in TC.CASES else TH.build(name)


def record(name):
    """one case through the reference's loop: its fixture entry"""
    c, m = build(name)
    r = R.run(m, c["graph"], procs=c["procs"], tcp=TC.tcp_arg(c))
    st = TC.status_lines(r["lines"])
    recs = PE.derive(st, TC.ip_ints(r["ip"]), c["hv"])
    ns, nd = PE.counted(st)
    return dict(ips=r["ip"], n_status=len(st), n_inet_sent=ns, n_inet_dropped=nd, fields=list(PE.FIELDS),
                rows=PE.rows(recs))


def main():
    path = os.path.join(HERE, "ref_tcp_paths.json")
    out = json.load(open(path)) if os.path.exists(path) else {}
    for name in sys.argv[1:] or CASES:
        out[name] = f = record(name)
        print(name, len(f["rows"]), "records", f["n_inet_sent"], "sent", f["n_inet_dropped"], "dropped", flush=True)
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")


if __name__ == "__main__":
    main()
