#!/usr/bin/env python3
"""The cost of the host records' series on bench.py's TCP model
(workloads.tcp_echo_model, 65 536 hosts, 500 000 B each way, 20 s simulated)
through tcp.run, one variant per process (profiles/hseries_tcp/ab.txt):

    python scripts/tcp_hseries_ab.py off [runs]       this tree, no option
    python scripts/tcp_hseries_ab.py hosts [runs]     this tree, host records without the series
    python scripts/tcp_hseries_ab.py s100 [runs]      this tree, the series at 100 ms
    python scripts/tcp_hseries_ab.py s1 [runs]        this tree, the series at 1 ms
    SHDGPU_LIB=<the parent commit's libshdgpu.so> python scripts/tcp_hseries_ab.py parent [runs]
    SHDGPU_LIB=<the same> python scripts/tcp_hseries_ab.py parent_hosts [runs]

One warm-up run, then `runs` timed ones (default 3) with the workspace kept, as
the bench runs them.  Prints per run the events, rounds, device time of the
rounds, M events/s, device time per round and the call's host times; the
series variants add the samples, the drains, the fullest drain and the
capacity, and SHD_TCP_SERIES_TIMING=1 the drains' host wall time on stderr.
AB_HOSTS: another host count; AB_CAP: the sample array's records (default: the
library's at 100 ms, 2^24 at 1 ms, where a batch of 64 rounds spans a second of
simulated time and a busy host crosses a boundary with most of its events)."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "shadow-1_amd")]

import shdgpu as S  # noqa: E402
import tcp as T  # noqa: E402
import workloads as W  # noqa: E402

VARIANTS = {"parent": {}, "parent_hosts": dict(hosts=True), "off": {}, "hosts": dict(hosts=True),
            "s100": dict(hosts=True, host_series_us=100000), "s1": dict(hosts=True, host_series_us=1000)}


def main():
    variant = sys.argv[1]
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    kw = dict(VARIANTS[variant])
    if variant.startswith("parent"):
        # a library from before the series has no such symbol.  shdgpu.lib() binds every entry of
        # _SIGS when it first loads the library, so the entry goes before the first lib() call
        # (tcp_hosts_ab.py does the same); nothing below calls the accessor for these variants
        del S._SIGS["shd_tcp_result_host_series"]
    if "host_series_us" in kw:
        kw["host_series_cap"] = int(os.environ.get("AB_CAP", str(1 << 24 if variant == "s1" else 0)))
    H = int(os.environ.get("AB_HOSTS", "65536"))
    g, m, ips, procs, peers, nb = W.tcp_echo_model(H, 1000, seed=1, end_s=20, nbytes=500000, loss_max=0.0)
    S.lib().shd_tcp_keep_workspace(1)

    def run1():
        return T.run(m, g, ips, procs, peers, nbytes=nb, trace=False, packets_per_host=2048, **kw)

    run1()
    for i in range(runs):
        r = run1()
        extra = ""
        if "hosts" in r:
            h = r["hosts"]
            extra = " records=%d enqueued=%d depth_max=%d" % (len(h), int(h["router_enqueued"].sum()),
                                                              int(h["depth_max"].max()))
        if "host_series" in r:
            s, info = r["host_series"], r["host_series_info"]
            extra += " samples=%d hosts_sampled=%d drains=%d peak=%d capacity=%d" % (
                len(s), len(set(s["rec"]["host"].tolist())), info["drains"], info["peak"], info["capacity"])
        print("%s run%d events=%d rounds=%d device_ms=%.3f Mev/s=%.3f us/round=%.3f setup_ms=%.1f results_ms=%.1f "
              "teardown_ms=%.1f%s" % (
                  variant, i, r["events"], r["rounds"], r["device_ms"], r["events"] / r["device_ms"] / 1e3,
                  r["device_ms"] * 1e3 / r["rounds"], r["host_ms"]["setup"], r["host_ms"]["results"],
                  r["host_ms"]["teardown"], extra), flush=True)
    S.lib().shd_tcp_keep_workspace(0)


if __name__ == "__main__":
    main()
