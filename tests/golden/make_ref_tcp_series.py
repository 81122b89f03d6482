"""Fixture of the TCP path's flow time series (shd_tcp_sample), from the
reference's own loop -- TEST INFRASTRUCTURE.  Runs each case through
oracle/_ref/libshdref_loop.so (the reference's worker.c, network_interface.c,
tcp.c ... compiled unmodified; oracle/Makefile `ref`) and stores what
tests/tcp_series_expect.py derives from its [STATUS] lines at each of the
case's intervals: per case the host IPs, the end time, the number of flow
records and, per interval (in microseconds), the full rows
(tcp_series_expect.FIELDS) and the number of lines exactly on a boundary.
Nothing stored comes from the oracle's restatement.

    python tests/golden/make_ref_tcp_series.py [case ...]   # -> tests/golden/ref_tcp_series.json
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
import tcp_series_expect as SE  # noqa: E402

# case -> the intervals (us) its series is recorded at
CASES = {
    "lossy_2pct": [250000, 1000],
    "heavy_loss": [250000],
    "geo_pairs": [250000],
    "loopback_pair": [1000],
    "mixed_hosts": [250000],
    "shared_hosts_rr": [100000],
    "hub12_fifo": [250000],
}


def build(name):
    """(case dict, model) of a fixture case, from whichever module defines it"""
    return TC.build(name) if name in TC.CASES else TH.build(name)


def record(name):
    """one case through the reference's loop: its fixture entry"""
    c, m = build(name)
    r = R.run(m, c["graph"], procs=c["procs"], tcp=TC.tcp_arg(c))
    st = TC.status_lines(r["lines"])
    end_ns = int(m.struct.end_time)
    series = {}
    for us in CASES[name]:
        series[str(us)] = dict(rows=SE.derive(st, us * 1000, end_ns), n_boundary_lines=SE.boundary_lines(st, us * 1000))
    return dict(ips=r["ip"], end_ns=end_ns, n_status=len(st), n_flows=len(FE.derive(st)), fields=list(SE.FIELDS),
                series=series)


def main():
    path = os.path.join(HERE, "ref_tcp_series.json")
    out = json.load(open(path)) if os.path.exists(path) else {}
    for name in sys.argv[1:] or CASES:
        out[name] = record(name)
        for us, s in out[name]["series"].items():
            print(name, us, "us:", len(s["rows"]), "samples,", s["n_boundary_lines"], "of", out[name]["n_status"],
                  "lines on a boundary", flush=True)
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")


if __name__ == "__main__":
    main()
