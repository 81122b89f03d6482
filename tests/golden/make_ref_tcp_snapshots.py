"""Fixture of the five snapshot values of a TCP socket (state, cwnd, ssthresh,
srtt, rttvar), from the reference's own loop -- TEST INFRASTRUCTURE.  Runs each
case through oracle/_ref/libshdref_loop.so (the reference's worker.c,
network_interface.c, tcp.c ... compiled unmodified; oracle/Makefile `ref`) and
stores what its tcp_getInfo (tcp.c, the source of getsockopt(TCP_INFO)) gave
for every TCP descriptor an echo process held, each time the process ran,
after its connect call and before each of its closes
(oracle/ref_harness/ref_loop.c tcp_observe): per case the host IPs and every
observation row in tests/tcp_snapshot_expect.py's packing.  Nothing stored
comes from the oracle's restatement.

The file is kept no larger than the largest other tests/golden/ref_tcp_*.json
(ref_tcp_series.json, 36283 bytes) by leaving whole cases out, never rows of a
case.  Of the 14 cases of ref_tcp_flows.json five are left out, with their row
counts: hub40_slow (1864), fan_out20 (532) and mixed_slow_rr (920) first, then
geo_pairs (484) and hub12_fifo (346), the two largest of the rest but for
slow_links (766), which stays as the one remaining case whose congestion
window is seen both rising and falling.  The oracle gave the reference's rows
on each of the five when this fixture was made (`--all` prints the comparison
for every case and writes nothing); on the device they are checked against the
oracle's log only.  Two small cases are the fixture's own
(tcp_cases.SNAPSHOT_CASES): hub3_slow, the one kept case where a process finds
its socket in CLOSEWAIT, and rto_reset, the one case where a process observes
the srtt reset after three back-offs.  An entry's rows are in
tcp_snapshot_expect.OBS_FIELDS' order.

    python tests/golden/make_ref_tcp_snapshots.py [case ...]   # -> tests/golden/ref_tcp_snapshots.json
    python tests/golden/make_ref_tcp_snapshots.py --all        # every case against the oracle, nothing written
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "shadow-1_amd")]

import oracle_ffi as O  # noqa: E402
import ref_loop_ffi as R  # noqa: E402
import tcp_cases as TC  # noqa: E402
import tcp_hub_cases as TH  # noqa: E402
import tcp_snapshot_expect as XE  # noqa: E402

ECHO = ["ref_epoll_lossy", "lossy_2pct", "slow_links", "heavy_loss", "geo_pairs", "shared_hosts_rr", "server_first",
        "loopback_pair", "loopback_mixed", "mixed_hosts", "mixed_slow_rr"]
HUB = ["hub12_fifo", "hub40_slow", "fan_out20"]
DROPPED = ["hub40_slow", "fan_out20", "mixed_slow_rr", "geo_pairs", "hub12_fifo"]
CASES = [n for n in ECHO + HUB if n not in DROPPED] + ["hub3_slow", "rto_reset"]


def build(name):
    """(case dict, model) of a fixture case, from whichever module defines it"""
    return TH.build(name) if name in TH.CASES else TC.build(name)


def record(name):
    """one case through the reference's loop: (its fixture entry, the run)"""
    c, m = build(name)
    assert R.observes(), "oracle/_ref/libshdref_loop.so is older than the observation: make -C oracle ref"
    r = R.run(m, c["graph"], procs=c["procs"], tcp=TC.tcp_arg(c), observe=True)
    assert R.OBS_FIELDS == XE.OBS_FIELDS
    e = dict(ips=r["ip"], n_status=len(TC.status_lines(r["lines"])))
    e.update(XE.pack(r["obs"]))
    assert XE.unpack(e) == r["obs"]
    return e, r


def against_oracle(name):
    c, m = build(name)
    e, r = record(name)
    o = O.tcp_run(m, c["graph"], TC.ip_ints(r["ip"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                  qdisc=c.get("qdisc", 0), udp=TC.udp_arg(c), snapshots=True)
    same = [x[:12] for x in o["obs"]] == r["obs"]
    print(name, "rows", len(r["obs"]), "oracle rows", len(o["obs"]), "equal", same, "log rows", len(o["log"]),
          "bytes", len(json.dumps(e, separators=(",", ":"))), flush=True)
    return same


def main():
    if sys.argv[1:] == ["--all"]:
        ok = [against_oracle(n) for n in ECHO + HUB + ["hub3_slow", "rto_reset"]]
        sys.exit(0 if all(ok) else 1)
    path = os.path.join(HERE, "ref_tcp_snapshots.json")
    out = json.load(open(path)) if os.path.exists(path) else {}
    for name in sys.argv[1:] or CASES:
        out[name], _ = record(name)
        print(name, len(out[name]["rows"]), "rows", len(out[name]["sockets"]), "sockets", len(out[name]["values"]),
              "value tuples", flush=True)
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
