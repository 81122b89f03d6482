"""Fixture of the packet engine's host-record series (shd_host_sample with
SHD_QF_HOST_SERIES), from the reference's own loop -- TEST INFRASTRUCTURE.
Runs cases of tests/ref_loop_cases.py through oracle/_ref/libshdref_loop.so
(the reference's sources compiled unmodified; oracle/Makefile `ref`) and stores
what tests/eng_series_expect.py derives from its [STATUS] lines at the (case,
interval) pairs below: per pair the sample count, each host's count, the
SHA-256 of the canonical rows (eng_series_expect.digest), the counted lines
that fall exactly on a boundary, and -- at 100 ms only -- the full rows of host
0 and of the host with the deepest queue.  The counts are the issue's table,
asserted here.  Recorded results only.

    python tests/golden/make_ref_eng_hseries.py   # -> tests/golden/ref_eng_hseries.json
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "shadow-1_amd")]

import eng_series_expect as SE  # noqa: E402
import ref_loop_cases as RC  # noqa: E402
import ref_loop_ffi as R  # noqa: E402
import tcp_host_expect as HE  # noqa: E402

MS = 1000   # interval in us
# (case, interval in us): samples, and where the table gives them: samples of every host, lines on a boundary
PAIRS = {("codel", 100 * MS): (1140, 19, None), ("udp_echo_codel", 100 * MS): (737, None, None),
         ("udp_mix_codel", 100 * MS): (535, None, None), ("bootstrap", 100 * MS): (724, None, None),
         ("phold_v100", 100 * MS): (1900, None, None), ("codel", 1 * MS): (42965, None, 44432),
         ("udp_mix_codel", 1 * MS): (4737, None, 2868), ("bootstrap", 10 * MS): (3939, None, None),
         ("phold_v100", 1000 * MS): (100, 1, None), ("udp_echo_codel", 5000 * MS): (0, 0, None)}


def key(name, us):
    return "%s@%d" % (name, us)


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


def main():
    out, lines = {"fields": list(SE.FIELDS)}, {}
    for (name, us), (n, each, onb) in PAIRS.items():
        case = RC.CASES[name]()
        if name not in lines:
            r = R.run(case["model"], case["graph"], procs=RC.procs_of(case), echo=case["model"].app_peer)
            lines[name] = RC.split_lines(r["lines"])[0]
        H, end = int(case["model"].n_hosts), int(case["model"].params["end_time"])
        e = out[key(name, us)] = entry(lines[name], H, us, end)
        print(key(name, us), e["n"], "samples, per host", min(e["per_host"]), "-", max(e["per_host"]), "on a boundary",
              e["on_boundary"], flush=True)
        assert e["n"] == n, (name, us, e["n"], n)
        assert each is None or set(e["per_host"]) == {each}, (name, us)
        assert onb is None or e["on_boundary"] == onb, (name, us, e["on_boundary"], onb)
    path = os.path.join(HERE, "ref_eng_hseries.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
