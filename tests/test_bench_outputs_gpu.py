"""bench.py's plain run and --dump-outputs: a plain run (no --full) prints the
result line with the legs beside the headline left out (null), and
--dump-outputs writes what the timed steps left: every host's end state
(shd_eng_digest's columns as float64) and the timed call's counts.  The dumped
end state is checked against the serial oracle on the model bench.py builds
from the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_ffi as O
import shdgpu as S
import workloads as W

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_the_end_state_the_oracle_computes(tmp_path):
    V, steps, warmup = 500, 1, 1
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--hosts-per-gpu", str(V), "--vertices", str(V), "--dump-outputs", str(out)]
    p = subprocess.run(cmd, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    lines = p.stdout.decode().strip().splitlines()
    assert len(lines) == 1, lines          # the JSON line is the only thing on stdout
    line = json.loads(lines[0])
    assert line["metric"] == "simulated packet events/sec" and line["unit"] == "packet events/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == steps and line["value"] > 0 and line["ms_per_step"] > 0
    # the legs that take runs of their own wait for --full
    assert line["cpu_baseline"] is None and line["lossy_c3"] is None and line["parity"] is None
    assert line["roofline"]["achieved"] > 0 and line["apsp"]["build_ms"] > 0

    # the same model, as bench.py builds it from these arguments, through the serial oracle
    g = W.geometric_graph(V, seed=1, loss_max=0.0)
    m = W.phold_model(W.hosts_on_vertices(V, 1), end_time=(warmup + steps) * S.SHD_SEC, seed=1, load=16, payload=1)
    _, odg, ost = O.engine_run(m, g)
    assert sorted(os.listdir(out)) == ["host_state.npy", "run_stats.npy"]
    hs = np.load(out / "host_state.npy")
    assert hs.dtype == np.float64 and hs.shape == (V, len(S.DIGEST_DTYPE.names))
    want = np.stack([odg[n].astype(np.float64) for n in S.DIGEST_DTYPE.names], axis=1)
    assert np.array_equal(hs, want)
    rs = np.load(out / "run_stats.npy")
    assert rs.dtype == np.float64 and rs.shape == (4,)
    n_events, n_pkt, n_rounds, final_time = rs
    # the timed call's share of the run: the steps after the warm-up
    assert 0 < n_pkt <= ost["n_pkt_events"] and n_pkt <= n_events and n_rounds > 0
    assert abs(n_pkt / (line["ms_per_step"] * steps * 1e-3) - line["value"]) <= 1e-3 * line["value"]
