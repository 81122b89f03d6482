#!/usr/bin/env python3
"""One untraced case on one engine, in a process of its own -- TEST
INFRASTRUCTURE (tests/test_lean_launch_rounds_gpu.py).

The engine reads SHD_NO_PS and SHD_NO_TL once a process (engine.hip,
shd_eng_run_until), so a run that must stay off the persistent kernels, or off
the ticketless ones, needs a fresh process with the variable set from the
start.  Usage: lean_rounds_worker.py <case> <out-dir>.  Builds
lean_cases.make_case(<case>), runs it on one engine with the product library,
writes the host digests to <out-dir>/<case>.npz and prints one JSON line: the
run statistics and a hash of the digest.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(os.path.dirname(HERE), "shadow-1_amd"), HERE]

import numpy as np  # noqa: E402

FIELDS = ("n_rounds", "n_events", "n_pkt_events", "window_ns", "error", "n_batches", "n_batches_persistent",
          "n_batches_sparse", "n_batches_ticketless", "n_batches_fused", "n_rounds_protected", "n_rounds_rerun",
          "n_rounds_replayed")


def main():
    name, out = sys.argv[1], sys.argv[2]
    import lean_cases
    import shdgpu as S
    import workloads as W
    from sim import Engine, PathCache
    assert os.path.basename(S.LIB_PATH) == "libshdgpu.so", S.LIB_PATH
    g, m = lean_cases.make_case(name)
    lean_cases.check_lean(m)
    pc = PathCache(g, W.attached_vertices(m.host_vertex))
    eng = Engine(m, pc)
    st = eng.run()
    dg = eng.digest()
    assert len(eng.trace()) == 0
    eng.close()
    pc.close()
    np.savez(os.path.join(out, f"{name}.npz"), digest=dg)
    res = {k: int(getattr(st, k)) for k in FIELDS}
    res.update(case=name, hosts=int(m.n_hosts), digest_sha256=hashlib.sha256(dg.tobytes()).hexdigest(),
               no_ps="SHD_NO_PS" in os.environ, no_tl="SHD_NO_TL" in os.environ)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
