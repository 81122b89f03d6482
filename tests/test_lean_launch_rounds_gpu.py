"""Whole untraced models on the launch-per-round kernels, against the oracle.

An engine runs its rounds as persistent launches where it can, so at small
sizes k_round_tl<true> -- the launch-per-round lean kernel, which the C4
benchmark runs throughout and every engine runs outside its persistent
batches -- sees a handful of 64-round batches, and the ticketed launch-per-
round kernels see fewer still.  SHD_NO_PS=1 keeps an engine off the persistent
kernels and SHD_NO_TL=1 off the ticketless ones; both are read once a process,
so each case here runs in a child (lean_rounds_worker.py) with a time limit.
The cases are those of lean_cases.py: trace off, no heartbeats, no bootstrap
period.  Every run's host digests and event counts must be the oracle's, and
the batch counters must say that the kernels meant ran the whole model.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from lean_cases import check_tor_inputs, make_case, oracle_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def run_child(name, tmp_path, timeout=120, **env_set):
    env = {k: v for k, v in os.environ.items()
           if k not in ("SHD_NO_PS", "SHD_NO_TL", "SHD_SP_HOSTS", "SHD_PS_BATCH", "SHDGPU_LIB")}
    env.update(env_set)
    p = subprocess.run([sys.executable, "-u", os.path.join(HERE, "lean_rounds_worker.py"), name, str(tmp_path)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-3000:]
    st = json.loads(out.strip().splitlines()[-1])
    print(out.strip().splitlines()[-1])
    return np.load(os.path.join(tmp_path, f"{name}.npz"))["digest"], st


def check(name, dg, st):
    g, m = make_case(name)
    odg, ost = oracle_of(name, g, m)
    assert st["error"] == 0 and st["hosts"] == m.n_hosts
    assert st["n_events"] == ost["n_events"]
    assert st["n_pkt_events"] == ost["n_pkt_events"] > 0
    assert np.array_equal(dg, odg)
    # what the case is for, on the oracle's output
    assert int(odg["n_inet_drop"].sum()) > 0
    if name == "codel":
        assert int(odg["n_codel_drop"].sum()) > 0
    if name == "threebins":
        width = 1 << (int(st["window_ns"]).bit_length() - 1)    # the calendar's bin width
        assert st["window_ns"] % 1_000_000 == 0 and st["window_ns"] > 1.9 * width
    if name == "tor":
        check_tor_inputs(m, odg)
    assert st["n_batches"] > 0 and st["n_batches_fused"] == 0    # (one engine: never a fused group batch)


@pytest.mark.parametrize("name", ["hosts65", "hosts300", "codel", "threebins", "tor"])
def test_ticketless_launch_per_round(name, tmp_path):
    """SHD_NO_PS=1: k_round_tl<true> runs the model (and the ticketed kernels
    the batches in which first touches come thick)."""
    dg, st = run_child(name, tmp_path, SHD_NO_PS="1")
    assert st["no_ps"] and not st["no_tl"]
    check(name, dg, st)
    assert st["n_batches_persistent"] == 0 and st["n_batches_sparse"] == 0
    assert st["n_batches_ticketless"] > 0


@pytest.mark.parametrize("name", ["hosts300", "codel"])
def test_ticketed_launch_per_round(name, tmp_path):
    """SHD_NO_PS=1 SHD_NO_TL=1: every batch on the ticketed launch-per-round kernels, untraced."""
    dg, st = run_child(name, tmp_path, SHD_NO_PS="1", SHD_NO_TL="1")
    assert st["no_ps"] and st["no_tl"]
    check(name, dg, st)
    assert st["n_batches_persistent"] == 0
    assert st["n_batches_ticketless"] == 0
