#!/usr/bin/env python3
"""Cost of SHD_QF_HOST_SERIES on the bench's packet-engine models
(profiles/hseries/ab.txt): one run of one variant, one line out.

    python scripts/eng_hseries_ab.py <c3|c5> <lean|records|series> [steps] [warmup] [interval_us]

The models and the timing are scripts/eng_hosts_ab.py's (C3: 10 000 hosts on the
10 000-vertex geometric graph; C5: the 1 M-host shard, 100 hosts per vertex,
1500-B payloads into 512 KiB/s receive buckets; `steps` timed steps of one
simulated second after `warmup` of them, host clock around run_until).
Variants:
  lean     no optional feature (what bench.py times)
  records  SHD_QF_HOST_RECORDS alone
  series   the records and SHD_QF_HOST_SERIES at interval_us (default 100 000)
`lean` and `records` are scripts/eng_hosts_ab.py's variants of the same names:
a checkout of the parent commit runs that script for the comparison, one
process per run, alternating in one session.  Prints: label, M packet events/s, ms per step, device ms of the launches per step,
rounds, packet events, and for `series` the samples, the drains, the fullest
drain, the capacity, the chunks and the time of the read.
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(os.path.dirname(HERE), "shadow-1_amd")]

import shdgpu as S  # noqa: E402
import workloads as W  # noqa: E402
from sim import Engine, PathCache  # noqa: E402


def main():
    wl, variant = sys.argv[1], sys.argv[2]
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    warmup = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    us = int(sys.argv[5]) if len(sys.argv) > 5 else 100000
    opts = {"lean": {}, "records": dict(hosts=True), "series": dict(hosts=True, host_series_us=us)}[variant]
    step, V = 1000 * S.SHD_MS, 10000
    end = (warmup + steps) * step
    if wl == "c5":
        g = W.geometric_graph(V, seed=1, loss_max=0.01)
        hv = W.hosts_on_vertices(V, 100)
        m = W.phold_model(hv, end_time=end, seed=1, load=16, payload=1500, bw_down=512, bw_up=10240, codelq_cap=256,
                          **opts)
    else:
        g = W.geometric_graph(V, seed=1, loss_max=0.0)
        hv = W.hosts_on_vertices(V, 1)
        m = W.phold_model(hv, end_time=end, seed=1, load=16, payload=1, **opts)
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
    line = (f"{wl} {variant} Mpkt/s={pkt / wall / 1e6:.2f} "
            f"ms_per_step={1e3 * wall / steps:.3f} device_ms_per_step={dev_ms / steps:.3f} rounds={rounds} "
            f"pkt_events={pkt}")
    if variant == "series":
        t1 = time.perf_counter()
        a = eng.host_series()
        ms = 1e3 * (time.perf_counter() - t1)
        info = eng.host_series_info()
        line += (f" interval_us={us} samples={len(a)} bytes={a.nbytes} read_ms={ms:.1f} drains={info['drains']} "
                 f"peak={info['peak']} capacity={info['capacity']} chunks={info['chunks']}")
    dg = eng.digest()
    line += f" digest_sent={int(dg['n_sent'].sum())} digest_recv={int(dg['n_recv'].sum())}"
    print(line, flush=True)
    eng.close()


if __name__ == "__main__":
    main()
