#!/usr/bin/env python3
"""Cost of SHD_QF_HOST_RECORDS on the bench's packet-engine models
(profiles/enghosts/ab.txt): one run of one variant, one line out.

    python scripts/eng_hosts_ab.py <c3|c5> <lean|general|records> [steps] [warmup]

The model is bench.py's (C3: 10 000 hosts on the 10 000-vertex geometric graph,
load 16, 1-B payloads, no loss; C5: 100 hosts per vertex of that graph with
edge loss U[0, 0.01], 1500-B payloads, 512 KiB/s receive buckets), `steps`
timed steps of one simulated second after `warmup` of them.  Variants:
  lean     no optional feature: the LEAN round kernels (what bench.py times)
  general  SHD_QF_HEARTBEATS alone: the general instantiations, nothing counted
           -- the comparison point that separates the cost of leaving the lean
           kernels from the cost of counting
  records  SHD_QF_HOST_RECORDS alone: the general instantiations, counting
Prints: label, M packet events/s over the timed steps (host clock around
run_until, which ends in a device synchronise), ms per step, device ms of the
launches per step, rounds, packet events, and for `records` the records' totals
and the time of the copy.
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(os.path.dirname(HERE), "shadow-1_amd")]

import numpy as np  # noqa: E402

import shdgpu as S  # noqa: E402
import workloads as W  # noqa: E402
from sim import Engine, PathCache  # noqa: E402


def main():
    wl, variant = sys.argv[1], sys.argv[2]
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    warmup = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    flags = {"lean": 0, "general": S.SHD_QF_HEARTBEATS, "records": S.SHD_QF_HOST_RECORDS}[variant]
    step, V = 1000 * S.SHD_MS, 10000
    end = (warmup + steps) * step
    if wl == "c5":
        g = W.geometric_graph(V, seed=1, loss_max=0.01)
        hv = W.hosts_on_vertices(V, 100)
        m = W.phold_model(hv, end_time=end, seed=1, load=16, payload=1500, bw_down=512, bw_up=10240, codelq_cap=256,
                          queue_flags=flags)
    else:
        g = W.geometric_graph(V, seed=1, loss_max=0.0)
        hv = W.hosts_on_vertices(V, 1)
        m = W.phold_model(hv, end_time=end, seed=1, load=16, payload=1, queue_flags=flags)
    pc = PathCache(g, W.attached_vertices(hv))
    eng = Engine(m, pc)
    eng.run_until(warmup * step)
    pkt = rounds = 0
    dev_ms = 0.0
    t0 = time.perf_counter()
    for k in range(steps):
        st = eng.run_until((warmup + k + 1) * step)
        pkt += st.n_pkt_events
        rounds += st.n_rounds
        dev_ms += st.device_ms_launches
    wall = time.perf_counter() - t0
    line = (f"{wl} {variant} Mpkt/s={pkt / wall / 1e6:.2f} ms_per_step={1e3 * wall / steps:.3f} "
            f"device_ms_per_step={dev_ms / steps:.3f} rounds={rounds} pkt_events={pkt} "
            f"us_per_round={1e3 * dev_ms / max(rounds, 1):.3f}")
    if variant == "records":
        t1 = time.perf_counter()
        a = eng.host_records()
        ms = 1e3 * (time.perf_counter() - t1)
        line += (f" records={len(a)} bytes={a.nbytes} copy_ms={ms:.2f} enqueued={int(a['router_enqueued'].sum())} "
                 f"dropped={int(a['router_dropped'].sum())} depth_max={int(a['depth_max'].max())} "
                 f"sojourn_max_ns={int(a['sojourn_max'].max())} if_sent={int(a['if_sent'].sum())}")
    dg = eng.digest()
    line += f" digest_sent={int(dg['n_sent'].sum())} digest_recv={int(dg['n_recv'].sum())}"
    print(line, flush=True)
    eng.close()


if __name__ == "__main__":
    main()
