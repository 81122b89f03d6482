#!/usr/bin/env python3
"""One path-cache build against the oracle, in a process of its own -- TEST
INFRASTRUCTURE.

The library selects some kernels only behind an environment switch (SHD_PC_*),
and reads some switches once per process: tests/test_pc_switches_gpu.py runs
this worker as a child with the switch in the child's environment.  The worker
builds the cache of one named graph (pc_graphs.SWITCH_GRAPHS), compares the
tables with the oracle's bit for bit and prints one JSON line; a difference is
reported in that line, not by the exit status.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(os.path.dirname(HERE), "shadow-1_amd"), HERE]

import numpy as np  # noqa: E402


def main(name):
    import pc_graphs as G
    from pc_helpers import PathCache, oracle_table
    g, rows = G.SWITCH_GRAPHS[name]()
    V = g.n_vertices
    att = np.arange(V, dtype=np.int32)
    rows = list(range(V)) if rows is None else list(rows)
    pc = PathCache(g, att)
    info = pc.info()
    lat, rel = pc.rows()
    lat, rel = lat[rows], rel[rows]
    olat, orel, _, _, ties = oracle_table(g, att, rows)
    bad = np.argwhere((lat.view(np.uint64) != olat.view(np.uint64)) | (rel.view(np.uint64) != orel.view(np.uint64)))
    out = dict(graph=name, equal=len(bad) == 0, n_differ=int(len(bad)),
               first_diff=None if not len(bad) else [int(rows[bad[0][0]]), int(bad[0][1])],
               rows_compared=len(rows), all_rows=len(rows) == V, oracle_ties=int(ties), n_ties=int(info.n_ties),
               n_tie_rows=int(info.n_tie_rows), n_tie_rows_global=int(info.n_tie_rows_global),
               first_pass_kernel=int(info.first_pass_kernel))
    pc.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
