#!/usr/bin/env python3
"""One untraced run with the host-record series on one engine, in a process of
its own -- TEST INFRASTRUCTURE (tests/test_eng_hseries_gpu.py).

The engine reads some of its switches once a process (SHD_NO_PS, SHD_NO_TL),
and the semantics-changing hooks (SHD_FORCE_AMBIG, SHD_PROTECT_ALL) exist only
in the test build libshdgpu_th.so, which only a child process loads
(SHDGPU_LIB), as in tests/eng_hosts_worker.py.  Usage:

    eng_hseries_worker.py <case> <interval_us> <steps> <out.npz>

<case>: a case of tests/ref_loop_cases.py, or `backlog`; the model runs
untraced with SHD_QF_HOST_RECORDS | SHD_QF_HOST_SERIES alone, in <steps>
run_until steps (1: one run).  Writes the samples, the records and the host
digests to <out.npz> and prints one JSON line of run statistics.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(os.path.dirname(HERE), "shadow-1_amd"), HERE]

import numpy as np  # noqa: E402


def main():
    name, us, steps, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    import eng_hseries_cases as SC
    import shdgpu as S
    g, m, pushes = SC.case(name, us)
    r = SC.run(g, m, pushes, steps=steps)
    assert len(r["trace"]) == 0
    r["engine"].close()
    np.savez(out, samples=r["samples"], records=r["records"], digest=r["digest"])
    tot = dict(r["tot"], case=name, lib=os.path.basename(S.LIB_PATH), **r["info"])
    print(json.dumps(tot), flush=True)


if __name__ == "__main__":
    main()
