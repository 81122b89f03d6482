"""TCP models with a bootstrap period (<shadow bootstraptime>) and per-host
heartbeat intervals (<host heartbeatfrequency>) -- TEST INFRASTRUCTURE.

Each case is a case of tests/tcp_cases.py (or the scaled echo model,
workloads.tcp_echo_model) with one or both options set on the model; the
reference's own loop (oracle/_ref/libshdref_loop.so, app 1) runs them for
tests/golden/ref_tcp_options.json (tests/golden/make_ref_tcp_options.py), and
the GPU's TCP path must reproduce that (tests/test_tcp_options_gpu.py).

What each case crosses:
  boot_lossy           lossy_2pct, 2.5 s: only the buckets differ before the end
                       of the period (as many drops as without, other lines)
  boot_whole_run       lossy_2pct, 4 s: the transfer ends inside the period: no
                       drop, no bucket ever consumed
  boot_slow_links      slow_links, 2.5 s: the CoDel queues start filling when the
                       period ends in mid-transfer
  boot_geo_pairs       geo_pairs, 2.5 s: ten pairs, multi-hop paths, device first
                       touches; the first drop right after the period
  boot_mixed_slow_rr   mixed_slow_rr, 2.5 s: both transports, rr qdisc; datagrams
                       unthrottled during the period
  boot_loopback_mixed  loopback_mixed, 2.2 s: loopback +1 ns tasks and routed
                       packets sharing a send bucket across the boundary
  hb_geo_pairs         geo_pairs, host h beats every (1 + h % 3) * 0.5 s: the
                       [STATUS] lines are geo_pairs's own, the [node] lines and
                       the event-ID counters are not; half-second hosts print 0
  hb_boot_geo_pairs    both of the above
  boot_echo64 / 96     the scaled echo model on 512 KiB/s links with 2 % loss,
                       2.3 s: a full wave, and a wave and a half, of lanes;
                       connection setup inside the period, the transfer outside
"""
import numpy as np

import shdgpu as S
import tcp_cases as TC
import workloads as W

SEC = S.SHD_SEC
MS = S.SHD_MS


def _hb_thirds(H):
    return [(1 + h % 3) * 500 * MS for h in range(H)]


def _echo(hosts):
    g, m, _, procs, peers, nb = W.tcp_echo_model(hosts, 40, end_s=12, nbytes=60000, loss_max=0.02, bw_down=512,
                                                 bw_up=512)
    hv = np.ctypeslib.as_array(m.struct.host_vertex, shape=(int(m.struct.n_hosts),)).copy()
    return dict(graph=g, hv=list(hv), procs=procs, peers=peers, nbytes=nb, end=12, bw=dict(bw_down=512, bw_up=512))


# name -> (base case of tcp_cases.CASES or a constructor, bootstrap end in ns, heartbeat rule or None)
OPTION_CASES = {
    "boot_lossy": ("lossy_2pct", 2500 * MS, None),
    "boot_whole_run": ("lossy_2pct", 4 * SEC, None),
    "boot_slow_links": ("slow_links", 2500 * MS, None),
    "boot_geo_pairs": ("geo_pairs", 2500 * MS, None),
    "boot_mixed_slow_rr": ("mixed_slow_rr", 2500 * MS, None),
    "boot_loopback_mixed": ("loopback_mixed", 2200 * MS, None),
    "hb_geo_pairs": ("geo_pairs", 0, _hb_thirds),
    "hb_boot_geo_pairs": ("geo_pairs", 2500 * MS, _hb_thirds),
    "boot_echo64": (lambda: _echo(64), 2300 * MS, None),
    "boot_echo96": (lambda: _echo(96), 2300 * MS, None),
}

# the cases the CPU test reruns through the reference's loop (a few seconds together)
CHEAP = ["boot_lossy", "boot_slow_links", "hb_geo_pairs"]


def base_of(name):
    """the tcp_cases name a case starts from (None: the scaled echo model)"""
    b = OPTION_CASES[name][0]
    return b if isinstance(b, str) else None


def build(name):
    """(case dict as tcp_cases.CASES makes them, model with the options set)"""
    base, boot, hb = OPTION_CASES[name]
    c = TC.CASES[base]() if isinstance(base, str) else base()
    hv = np.asarray(c["hv"], dtype=np.int32)
    m = W.phold_model(hv, end_time=c["end"] * SEC, trace=True, queue_flags=S.SHD_QF_TRACE_STATUS, load=0,
                      payload=c.get("payload", 1), bootstrap_end=int(boot),
                      host_heartbeat=None if hb is None else np.asarray(hb(len(hv)), dtype=np.uint64), **c["bw"])
    return c, m


def first_time(lines, status):
    """(count, time of the first) of the [STATUS] lines that name a status, as
    the line's own or in the packet's status list (-1: none)"""
    ts = [t for t, _, body in lines if status in body]
    return len(ts), (min(ts) if ts else -1)
