#!/usr/bin/env python3
"""One rank of a group run of a tests/tcp_hub_cases.py case -- TEST
INFRASTRUCTURE (tests/test_tcp_hub_gpu.py starts `world` of these as child
processes).

Each rank builds the same model, creates a host-memory communicator (several
ranks on one GPU), runs its share of the hosts through shd_tcp_run_group
(shadow-1_amd/tcp.py with comm) -- its own hosts' socket slots, processes and
interface queues sized from the whole model -- and writes its hosts' lines,
end state and shape to <out>/rank<r>.npz.
"""
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
    ap.add_argument("--case", required=True, help="a tcp_hub_cases name")
    ap.add_argument("--mode", default="tables", choices=["tables", "device"])
    a = ap.parse_args()
    import sim
    import tcp as TCPGPU
    import tcp_cases as TC
    import tcp_hub_cases as TH
    fix = json.load(open(os.path.join(HERE, "golden", "ref_tcp_hub.json")))[a.case]
    c, m = TH.build(a.case)
    comm = sim.Comm.host(a.name, a.world, a.rank, 0)
    r = TCPGPU.run(m, c["graph"], TC.ip_ints(fix["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"], node=True,
                   qdisc=c.get("qdisc", 0), udp=TC.udp_arg(c), comm=comm, mode=a.mode)
    comm.close()
    np.savez(os.path.join(a.out, f"rank{a.rank}.npz"), lines=json.dumps(r["lines"]),
             node_lines=json.dumps(r["node_lines"]), next_event_id=r["next_event_id"],
             next_packet_id=r["next_packet_id"], rng_probe=r["rng_probe"], first_host=r["first_host"],
             n_local_hosts=r["n_local_hosts"], rounds=r["rounds"], events=r["events"], first_touch=r["first_touch"],
             max_host_sockets=r["max_host_sockets"], max_host_procs=r["max_host_procs"], sock_bytes=r["sock_bytes"])
    print(f"rank {a.rank}: hosts [{r['first_host']}, {r['first_host'] + r['n_local_hosts']}) rounds {r['rounds']} "
          f"events {r['events']} sockets {r['max_host_sockets']}", flush=True)


if __name__ == "__main__":
    main()
