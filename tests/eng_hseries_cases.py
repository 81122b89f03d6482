"""Models and runs of the packet engine's host-record series tests -- TEST
INFRASTRUCTURE (tests/test_eng_hseries_gpu.py and its child processes,
tests/eng_hseries_worker.py: both build the same model from the same name).

The cases are those of tests/eng_hosts_cases.py (the reference-pinned cases of
tests/ref_loop_cases.py and `backlog`), rebuilt with the series' flag and an
interval.
"""
import numpy as np

import eng_hosts_cases as EC
import ref_loop_cases as RC
import shdgpu as S
import workloads as W

HS = S.SHD_QF_HOST_RECORDS | S.SHD_QF_HOST_SERIES
STAT_KEYS = ("n_events", "n_pkt_events", "n_rounds", "n_rounds_rerun", "n_rounds_replayed", "n_rounds_protected",
             "n_batches", "n_batches_persistent", "n_batches_sparse", "n_batches_ticketless")


def with_series(m, trace, queue_flags, interval_us):
    """the same model with another `trace`, `queue_flags` and series interval"""
    s, p = m.struct, m.params
    specs = None if m.app_specs is None else [(a.send, a.dest, a.n_start, a.per_read) for a in m.app_specs]
    return S.ModelArrays(m.host_vertex, m.host_rng, m.bw_down, m.bw_up, m.dest_cum, end_time=p["end_time"],
                         app_start=p["app_start"], load=p["load"], payload=p["payload"],
                         heartbeat_interval=p["heartbeat_interval"], bootstrap_end=p["bootstrap_end"], trace=trace,
                         evq_cap=int(s.evq_cap), inbox_cap=int(s.inbox_cap), codelq_cap=int(s.codelq_cap),
                         txq_cap=int(s.txq_cap), queue_flags=int(queue_flags), host_class=m.host_class,
                         host_heartbeat=m.host_heartbeat, app_peer=m.app_peer, app_specs=specs, host_app=m.host_app,
                         hostrec_interval_us=int(interval_us))


def case(name, interval_us, trace=False, queue_flags=HS):
    """(graph, model, pushes): a case of ref_loop_cases.py, or `backlog`, with the series"""
    if name == "backlog":
        g, m = EC.backlog(trace, 0)
        return g, with_series(m, trace, queue_flags, interval_us), None
    c = RC.CASES[name]()
    return c["graph"], with_series(c["model"], trace, queue_flags, interval_us), c.get("pushes")


def cuts(end, steps):
    """run_until stops: three end at 1/5, 1/2 and the whole of the run"""
    return [end] if steps == 1 else [end * (k * k + 1) // (steps * steps + 1) for k in range(1, steps)] + [end]


def run(g, m, pushes=None, steps=1, rounds=False, stop_on_error=False):
    """one engine's run: dict(samples, records, digest, trace, info, tot, reads, engine, error).
    steps: run_until in that many unequal steps, reading the series after each
    (reads: [(stop, samples)]); rounds: the host drives every round
    (shd_eng_run_round); stop_on_error: a round's error ends the run (error: its bits)."""
    from sim import Engine, PathCache, sort_trace
    pc = PathCache(g, W.attached_vertices(m.host_vertex))
    eng = Engine(m, pc)
    end = int(m.params["end_time"])
    tot = dict.fromkeys(STAT_KEYS, 0)
    reads, error = [], 0
    if pushes is not None or rounds:
        eng.boot()
    if pushes is not None:
        eng.push_events(pushes)
    if rounds:
        w, nxt = eng.window, eng.next_time()
        while nxt < end:
            r = S.RoundSummary()
            rc = S.lib().shd_eng_run_round(eng.ptr, int(nxt), int(min(nxt + w, end)), S.C.byref(r))
            if rc and stop_on_error:
                error = int(r.error)
                break
            S.check(rc, f"shd_eng_run_round (error bits {r.error:#x})")
            tot["n_events"] += r.n_events
            tot["n_pkt_events"] += r.n_pkt_events
            tot["n_rounds"] += 1
            nxt = r.next_time
    else:
        for t in cuts(end, steps):
            st = eng.run_until(t) if steps > 1 else eng.run()
            for k in tot:
                tot[k] += int(getattr(st, k))
            if steps > 1:
                reads.append((t, eng.host_series()))
    series = bool(int(m.params["queue_flags"]) & S.SHD_QF_HOST_SERIES)
    return dict(samples=eng.host_series() if series else None, info=eng.host_series_info() if series else None,
                records=eng.host_records(), digest=eng.digest(), trace=sort_trace(eng.trace()), tot=tot, reads=reads,
                engine=eng, error=error)


def sample_array(rows):
    """rows ([t] + tcp_host_expect.FIELDS) as an S.HOST_SAMPLE_DTYPE array"""
    import tcp_host_expect as HE
    a = np.zeros(len(rows), dtype=S.HOST_SAMPLE_DTYPE)
    a["t"] = [r[0] for r in rows]
    for j, k in enumerate(HE.SCALARS):
        a["rec"][k] = [r[1 + j] for r in rows]
    a["rec"]["sojourn_hist"] = [r[-1] for r in rows] if rows else np.zeros((0, 16))
    return a
