#!/usr/bin/env python3
"""One rank of a TCP-path group run with packet capture -- TEST INFRASTRUCTURE
(tests/test_tcp_pcap_gpu.py starts `world` of these as child processes;
tcp_group_worker.py has no capture argument).

Each rank builds the same case of tests/tcp_cases.py, creates a host-memory
communicator, runs its share of the hosts through shd_tcp_run_group with the
given capture hosts and writes the records of those it owns to
<out>/rank<r>.npz (pcap_hosts, pcap_<host> per captured host)."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(os.path.dirname(HERE), "shadow-1_amd"), HERE]

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--name", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--case", required=True, help="a tcp_cases name (echo processes only)")
    ap.add_argument("--hosts", required=True, help="capture hosts, comma-separated model indices")
    ap.add_argument("--ring", type=int, default=0)
    a = ap.parse_args()
    import sim
    import tcp as TCPGPU
    import tcp_cases as TC
    fix = json.load(open(os.path.join(HERE, "golden", "ref_tcp.json")))[a.case]
    c, m = TC.build(a.case)
    comm = sim.Comm.host(a.name, a.world, a.rank, 0)
    r = TCPGPU.run(m, c["graph"], TC.ip_ints(fix["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                   qdisc=c.get("qdisc", 0), comm=comm, mode="tables",
                   pcap=dict(hosts=[int(x) for x in a.hosts.split(",")], ring=a.ring))
    comm.close()
    caps = r["pcap_records"]
    np.savez(os.path.join(a.out, f"rank{a.rank}.npz"), pcap_hosts=np.array(sorted(caps), dtype=np.int64),
             pcap_drains=r["pcap_drains"], pcap_ring_peak=r["pcap_ring_peak"], rng_probe=r["rng_probe"],
             first_host=r["first_host"], n_local_hosts=r["n_local_hosts"],
             **{"pcap_%d" % h: v for h, v in caps.items()})
    print(f"rank {a.rank}: hosts [{r['first_host']}, {r['first_host'] + r['n_local_hosts']}) captured "
          f"{ {h: len(v) for h, v in caps.items()} } drains {r['pcap_drains']}", flush=True)


if __name__ == "__main__":
    main()
