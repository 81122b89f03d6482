"""Fixture of the TCP path's host-record series (shd_host_sample with
SHD_TCP_OPT_HOST_SERIES), from the reference's own loop -- TEST INFRASTRUCTURE.
Runs the cases of tests/golden/make_ref_tcp_hosts.py through
oracle/_ref/libshdref_loop.so (the reference's sources compiled unmodified;
oracle/Makefile `ref`) and stores what tests/eng_series_expect.py derives from
its [STATUS] lines at the (case, interval) pairs below: per pair the sample
count, each host's count, the SHA-256 of the canonical rows
(eng_series_expect.digest), the counted lines that fall exactly on a boundary,
and -- at 100 ms only -- the full rows of host 0 and of the host with the
deepest queue.  The counts are the issue's table, asserted here.  Recorded
results only.

    python tests/golden/make_ref_tcp_hseries.py   # -> tests/golden/ref_tcp_hseries.json
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "shadow-1_amd")]

import eng_series_expect as SE  # noqa: E402
import ref_loop_ffi as R  # noqa: E402
import tcp_cases as TC  # noqa: E402
import tcp_host_expect as HE  # noqa: E402
import tcp_hub_cases as TH  # noqa: E402

MS = 1000   # interval in us
# (case, interval in us): samples, the fewest and the most of a host, counted lines on a boundary
PAIRS = {("hub40_slow", 100 * MS): (416, 6, 33, 78), ("hub40_slow", 1 * MS): (3260, 38, 1352, 4245),
         ("slow_links", 10 * MS): (521, 260, 261, 560), ("slow_links", 1 * MS): (1806, 901, 905, 4799),
         ("slow_links", 60000 * MS): (0, 0, 0, None),
         ("mixed_slow_rr", 100 * MS): (107, 1, 39, 26), ("mixed_slow_rr", 1 * MS): (1784, 3, 847, 1932),
         ("hub12_fifo", 100 * MS): (111, 3, 13, 8), ("geo_pairs", 100 * MS): (521, 2, 70, 8),
         ("geo_pairs", 1000 * MS): (94, 1, 17, 2), ("loopback_pair", 10 * MS): (7, 7, 7, 45),
         ("lossy_2pct", 100 * MS): (160, 79, 81, 24), ("lossy_2pct", 1 * MS): (419, 208, 211, 4699)}


def key(name, us):
    return "%s@%d" % (name, us)


def build(name):
    """(case dict, model) of a fixture case, from whichever module defines it"""
    return TC.build(name) if name in TC.CASES else TH.build(name)


def entry(st, H, us, end):
    rows = SE.derive(st, H, 1000 * us, end)
    e = dict(interval_us=us, n=len(rows), per_host=SE.per_host(rows, H), sha256=SE.digest(rows),
             on_boundary=SE.on_boundary(st, 1000 * us))
    if us == 100 * MS:
        final = HE.derive(st, H)
        deep = max(range(H), key=lambda h: (final[h]["depth_max"], -h))
        e["hosts"] = {str(h): [r for r in rows if r[1] == h] for h in sorted({0, deep})}
        e["deepest"] = deep
    return e


def entries(pairs=None):
    """the fixture's entries of `pairs` (all of PAIRS), each case run once through the reference's loop"""
    out, lines = {}, {}
    for name, us in pairs or PAIRS:
        c, m = build(name)
        if name not in lines:
            r = R.run(m, c["graph"], procs=c["procs"], tcp=TC.tcp_arg(c))
            lines[name] = TC.status_lines(r["lines"])
        out[key(name, us)] = entry(lines[name], len(c["hv"]), us, int(m.struct.end_time))
    return out


def main():
    out = {"fields": list(SE.FIELDS)}
    out.update(entries())
    for (name, us), (n, lo, hi, onb) in PAIRS.items():
        e = out[key(name, us)]
        print(key(name, us), e["n"], "samples, per host", min(e["per_host"]), "-", max(e["per_host"]), "on a boundary",
              e["on_boundary"], flush=True)
        assert e["n"] == n, (name, us, e["n"], n)
        assert (min(e["per_host"]), max(e["per_host"])) == (lo, hi), (name, us)
        assert onb is None or e["on_boundary"] == onb, (name, us, e["on_boundary"], onb)
    assert out["hub40_slow@100000"]["deepest"] == 0 and out["hub40_slow@100000"]["per_host"][0] == 33
    path = os.path.join(HERE, "ref_tcp_hseries.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
