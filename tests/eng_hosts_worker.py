#!/usr/bin/env python3
"""One untraced run with host records on one engine, in a process of its own
-- TEST INFRASTRUCTURE (tests/test_eng_hosts_gpu.py).

The engine reads some of its switches once a process (SHD_NO_PS, SHD_NO_TL),
and the semantics-changing hooks (SHD_FORCE_AMBIG, SHD_PROTECT_ALL) exist only
in the test build libshdgpu_th.so, which only a child process loads
(SHDGPU_LIB), as in tests/hook_worker.py.  Usage:

    eng_hosts_worker.py <case> <steps> <out.npz>

<case>: a case of eng_hosts_cases.CASES, or `backlog`; the model runs untraced
with SHD_QF_HOST_RECORDS alone, in <steps> run_until steps (1: one run).
Writes the records and the host digests to <out.npz> and prints one JSON line
of run statistics.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(os.path.dirname(HERE), "shadow-1_amd"), HERE]

import numpy as np  # noqa: E402


def main():
    name, steps, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    import eng_hosts_cases as EC
    import shdgpu as S
    if name == "backlog":
        (g, m), pushes = EC.backlog(False, EC.HR), None
    else:
        g, m, pushes = EC.ref_case(name, False, EC.HR)
    recs, dg, tr, eng, tot = EC.engine_records(g, m, pushes, steps=steps)
    assert len(tr) == 0
    eng.close()
    np.savez(out, records=recs, digest=dg)
    tot.update(case=name, lib=os.path.basename(S.LIB_PATH))
    print(json.dumps(tot), flush=True)


if __name__ == "__main__":
    main()
