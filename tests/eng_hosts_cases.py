"""Models and runs of the packet engine's host-record tests -- TEST
INFRASTRUCTURE (tests/test_eng_hosts_ref_cpu.py, tests/test_eng_hosts_gpu.py,
tests/eng_hosts_worker.py: the test processes and their child processes build
the same model from the same name).

The reference-pinned cases are those of tests/ref_loop_cases.py, rebuilt with
other trace / queue_flags values (with_flags); `backlog` is the rollback and
replay model: 2 hosts on each vertex of a 200-vertex geometric graph, 3 s,
1500-B datagrams into 512 KiB/s receive buckets, so the router queues build.
"""
import numpy as np

import ref_loop_cases as RC
import shdgpu as S
import workloads as W

HR = S.SHD_QF_HOST_RECORDS
# the five cases of tests/golden/ref_eng_hosts.json
CASES = ["codel", "udp_echo_codel", "udp_mix_codel", "bootstrap", "phold_v100"]


def with_flags(m, trace, queue_flags):
    """the same model with another `trace` and `queue_flags`"""
    s, p = m.struct, m.params
    specs = None if m.app_specs is None else [(a.send, a.dest, a.n_start, a.per_read) for a in m.app_specs]
    return S.ModelArrays(m.host_vertex, m.host_rng, m.bw_down, m.bw_up, m.dest_cum, end_time=p["end_time"],
                         app_start=p["app_start"], load=p["load"], payload=p["payload"],
                         heartbeat_interval=p["heartbeat_interval"], bootstrap_end=p["bootstrap_end"], trace=trace,
                         evq_cap=int(s.evq_cap), inbox_cap=int(s.inbox_cap), codelq_cap=int(s.codelq_cap),
                         txq_cap=int(s.txq_cap), queue_flags=int(queue_flags), host_class=m.host_class,
                         host_heartbeat=m.host_heartbeat, app_peer=m.app_peer, app_specs=specs, host_app=m.host_app)


def ref_case(name, trace, queue_flags):
    """(graph, model, pushes) of a tests/ref_loop_cases.py case with the given flags"""
    case = RC.CASES[name]()
    return case["graph"], with_flags(case["model"], trace, queue_flags), case.get("pushes")


def backlog(trace, queue_flags):
    """(graph, model) of the rollback and replay model"""
    g = W.geometric_graph(200, seed=4)
    m = W.phold_model(W.hosts_on_vertices(200, 2), end_time=3 * S.SHD_SEC, trace=trace, payload=1500, bw_down=512,
                      codelq_cap=512, queue_flags=queue_flags)
    return g, m


def engine_records(g, m, pushes=None, steps=1, rounds=False):
    """one engine's run of the model: (records -- None without the flag --,
    digest, sorted trace, engine, summed statistics).  steps: run_until in that many unequal steps; rounds:
    the host drives every round (shd_eng_run_round)."""
    from sim import Engine, PathCache, sort_trace
    pc = PathCache(g, W.attached_vertices(m.host_vertex))
    eng = Engine(m, pc)
    end = int(m.params["end_time"])
    tot = dict(n_events=0, n_pkt_events=0, n_rounds=0, n_rounds_rerun=0, n_rounds_replayed=0, n_rounds_protected=0,
               n_batches=0, n_batches_persistent=0, n_batches_sparse=0, n_batches_ticketless=0)
    if pushes is not None or rounds:
        eng.boot()
    if pushes is not None:
        eng.push_events(pushes)
    if rounds:
        w, nxt = eng.window, eng.next_time()
        while nxt < end:
            r = eng.run_round(nxt, min(nxt + w, end))
            tot["n_events"] += r.n_events
            tot["n_pkt_events"] += r.n_pkt_events
            tot["n_rounds"] += 1
            nxt = r.next_time
    else:
        # unequal steps: three end at 1/5, 1/2 and the whole of the run
        cuts = [end] if steps == 1 else [end * (k * k + 1) // (steps * steps + 1) for k in range(1, steps)] + [end]
        for t in cuts:
            st = eng.run_until(t) if steps > 1 else eng.run()
            for k in tot:
                tot[k] += int(getattr(st, k))
    recs = eng.host_records() if int(m.params["queue_flags"]) & HR else None
    return recs, eng.digest(), sort_trace(eng.trace()), eng, tot


def array_of(rows):
    """fixture rows (tcp_host_expect.FIELDS order) as a TCP_HOSTREC_DTYPE array"""
    import tcp_host_expect as HE
    a = np.zeros(len(rows), dtype=S.TCP_HOSTREC_DTYPE)
    for j, k in enumerate(HE.SCALARS):
        a[k] = [r[j] for r in rows]
    a["sojourn_hist"] = [r[-1] for r in rows]
    return a
