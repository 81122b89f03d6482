#!/usr/bin/env python3
"""The host records' cost on bench.py's TCP model (workloads.tcp_echo_model,
65 536 hosts, 500 000 B each way, 20 s simulated) through tcp.run, one variant
per process (profiles/hosts/ab.txt):

    python scripts/tcp_hosts_ab.py off [runs]        this tree, option off
    python scripts/tcp_hosts_ab.py on [runs]         this tree, host records on
    SHDGPU_LIB=<the parent commit's libshdgpu.so> python scripts/tcp_hosts_ab.py parent [runs]

One warm-up run, then `runs` timed ones (default 3) with the workspace kept, as
the bench runs them.  Prints per run the events, rounds, device time of the
rounds, M events/s, device time per round and the call's host times (setup,
results, teardown: shd_tcp_result's); SHD_TCP_HOST_TIMING=1 adds the
size and host wall time of the records' copy on stderr.  AB_HOSTS: another
host count."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "shadow-1_amd")]

import shdgpu as S  # noqa: E402
import tcp as T  # noqa: E402
import workloads as W  # noqa: E402


def main():
    variant = sys.argv[1]
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    assert variant in ("parent", "off", "on")
    if variant == "parent":   # a library from before the host records: it has no such symbol
        del S._SIGS["shd_tcp_result_hosts"]
    H = int(os.environ.get("AB_HOSTS", "65536"))
    g, m, ips, procs, peers, nb = W.tcp_echo_model(H, 1000, seed=1, end_s=20, nbytes=500000, loss_max=0.0)
    S.lib().shd_tcp_keep_workspace(1)
    kw = dict(hosts=True) if variant == "on" else {}

    def run1():
        return T.run(m, g, ips, procs, peers, nbytes=nb, trace=False, packets_per_host=2048, **kw)

    run1()
    for i in range(runs):
        r = run1()
        extra = ""
        if variant == "on":
            h = r["hosts"]
            extra = " records=%d enqueued=%d dropped=%d depth_max=%d sojourn_max_ns=%d" % (
                len(h), int(h["router_enqueued"].sum()), int(h["router_dropped"].sum()), int(h["depth_max"].max()),
                int(h["sojourn_max"].max()))
        print("%s run%d events=%d rounds=%d device_ms=%.3f Mev/s=%.3f us/round=%.3f setup_ms=%.1f results_ms=%.1f "
              "teardown_ms=%.1f%s" % (
                  variant, i, r["events"], r["rounds"], r["device_ms"], r["events"] / r["device_ms"] / 1e3,
                  r["device_ms"] * 1e3 / r["rounds"], r["host_ms"]["setup"], r["host_ms"]["results"],
                  r["host_ms"]["teardown"], extra), flush=True)
    S.lib().shd_tcp_keep_workspace(0)


if __name__ == "__main__":
    main()
