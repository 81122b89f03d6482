#!/usr/bin/env python3
"""One rank of a TCP-path group run with the host records' series -- TEST
INFRASTRUCTURE (tests/test_tcp_hseries_gpu.py starts `world` of these as child
processes).

Each rank builds the same case of tests/tcp_cases.py or tests/tcp_hub_cases.py,
creates a host-memory communicator, runs its share of the hosts untraced
through shd_tcp_run_group with SHD_TCP_OPT_HOSTS | SHD_TCP_OPT_HOST_SERIES and
writes its records and samples to <out>/rank<r>.npz."""
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
    ap.add_argument("--case", required=True)
    ap.add_argument("--us", type=int, required=True)
    ap.add_argument("--mode", default="tables", choices=["tables", "device"])
    a = ap.parse_args()
    import sim
    import tcp as TCPGPU
    import tcp_cases as TC
    import tcp_hub_cases as TH
    fix = json.load(open(os.path.join(HERE, "golden", "ref_tcp_hosts.json")))[a.case]
    c, m = TC.build(a.case) if a.case in TC.CASES else TH.build(a.case)
    comm = sim.Comm.host(a.name, a.world, a.rank, 0)
    r = TCPGPU.run(m, c["graph"], TC.ip_ints(fix["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                   qdisc=c.get("qdisc", 0), udp=TC.udp_arg(c), comm=comm, mode=a.mode, trace=False, hosts=True,
                   host_series_us=a.us)
    comm.close()
    np.savez(os.path.join(a.out, f"rank{a.rank}.npz"), hosts=r["hosts"], host_series=r["host_series"],
             first_host=r["first_host"], n_local_hosts=r["n_local_hosts"])
    print(f"rank {a.rank}: hosts [{r['first_host']}, {r['first_host'] + r['n_local_hosts']}) "
          f"{len(r['host_series'])} host samples", flush=True)


if __name__ == "__main__":
    main()
