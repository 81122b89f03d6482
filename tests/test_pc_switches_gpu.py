"""The path-cache kernels the library launches only behind an environment
switch, each against the oracle bit for bit.

Some switches are read once per process (SHD_PC_BF_PAIRS, SHD_PC_ONE_ROW), so
every case runs tests/pc_switch_worker.py as a child with the switch in the
child's environment: one child at a time, under its own time limit.  After a
child that ended on a signal or at its time limit nothing more is started on
the device: the remaining cases skip.
"""
import json
import os
import subprocess
import sys

import pytest

import shdgpu as S

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT_S = 240
_stopped_by = []   # the case whose child ended on a signal or its time limit

TIE_SWITCHES = ["SHD_PC_TIE_STG=0", "SHD_PC_TIE_KIND=st", "SHD_PC_TIE_SHEAP=1", "SHD_PC_TIE_HV8=1",
                "SHD_PC_TIE_NOGD=1", "SHD_PC_TIE_HC=64"]
FIRST_PASS_SWITCHES = ["SHD_PC_BF_PAIRS=1", "SHD_PC_ONE_ROW=1", "SHD_PC_LDS_OFF=1", "SHD_PC_RELABEL=1"]


def run_worker(graph, switch):
    if _stopped_by:
        pytest.skip(f"a child ended on a signal or its time limit before ({_stopped_by[0]}): no more device work")
    env = dict(os.environ)
    key, val = switch.split("=")
    env[key] = val
    p = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, "-u",
                        os.path.join(HERE, "pc_switch_worker.py"), graph],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env)
    out = p.stdout.decode(errors="replace")
    if p.returncode < 0 or p.returncode in (124, 137) or p.returncode > 128:
        _stopped_by.append(f"{graph} {switch}: exit status {p.returncode}")
    assert p.returncode == 0, f"exit status {p.returncode}\n{out[-3000:]}"
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert lines, out[-3000:]
    return json.loads(lines[-1])


@pytest.mark.parametrize("graph", ["grid30", "geo_half_ms_300"])
@pytest.mark.parametrize("switch", TIE_SWITCHES)
def test_tie_kernel_behind_a_switch_equals_the_oracle(graph, switch):
    # grid30: whole-number weights (4-byte heap values unless SHD_PC_TIE_HV8);
    # geo_half_ms_300: half milliseconds (the 8-byte heap values)
    r = run_worker(graph, switch)
    assert r["equal"], r
    assert r["all_rows"] and r["n_tie_rows"] > 0 and r["n_ties"] == r["oracle_ties"] > 0, r
    assert r["first_pass_kernel"] == S.SHD_PC_K_ROWS_LDS_256, r
    if switch == "SHD_PC_TIE_HC=64":
        assert r["n_tie_rows_global"] > 0, r   # a 64-entry heap overflows: the lane heaps in global scratch


@pytest.mark.parametrize("graph", ["geo2049", "grid30"])
@pytest.mark.parametrize("switch", FIRST_PASS_SWITCHES)
def test_first_pass_behind_a_switch_equals_the_oracle(graph, switch):
    r = run_worker(graph, switch)
    assert r["equal"], r
    if graph == "grid30":
        want = S.SHD_PC_K_ROWS_LDS_256
    else:
        want = S.SHD_PC_K_ROWS_LDS_1024 if switch == "SHD_PC_ONE_ROW=1" else S.SHD_PC_K_ROWS2_LDS
        assert r["n_tie_rows"] == 0 and r["n_ties"] == 0, r   # the first pass's own parents are the table's
    assert r["first_pass_kernel"] == want, r
