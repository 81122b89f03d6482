"""A run on a kept workspace (shd_tcp_keep_workspace(1): bench.py's and the
A/B scripts' way to run the driver) is the run on a fresh one: the second run
reuses every device buffer as the first left it, larger or smaller than it
needs, and must re-initialise what it reads.

Model A is workloads.tcp_echo_model at 96 hosts with 2 % loss, model B the same
at 64 hosts without loss; both traced with node lines and with flows, paths,
series and hosts on, so that every option's buffers are in the workspace.  In
one process: A then B kept (B inherits A's larger buffers), B again after the
workspace's release, then B and A kept (the workspace must grow)."""
import numpy as np
import pytest

import shdgpu as S
import tcp as TCPGPU
import workloads as W

pytestmark = pytest.mark.gpu

SCALARS = ("rounds", "events", "deliveries", "max_host_sockets")
PER_HOST = ("next_event_id", "next_packet_id", "rng_probe")
RECORDS = ("flows", "paths", "series", "hosts")


def _run(hosts, loss):
    g, m, ips, procs, peers, nb = W.tcp_echo_model(hosts, 30, seed=3, end_s=8, nbytes=40000, loss_max=loss)
    return TCPGPU.run(m, g, ips, procs, peers, nbytes=nb, trace=True, node=True, flows=True, paths=True,
                      series_us=250000, hosts=True)


def _same(kept, fresh, what):
    assert kept["first_touch"] == fresh["first_touch"], what
    assert len(fresh["lines"]) > 0 and kept["lines"] == fresh["lines"], (what, "lines")
    assert len(fresh["node_lines"]) > 0 and kept["node_lines"] == fresh["node_lines"], (what, "node_lines")
    for k in SCALARS:
        assert kept[k] == fresh[k], (what, k)
    for k in PER_HOST:
        assert kept[k].tolist() == fresh[k].tolist(), (what, k)
    for k in RECORDS:
        assert len(fresh[k]) > 0 and kept[k].dtype == fresh[k].dtype, (what, k)
        assert np.array_equal(kept[k], fresh[k]) and kept[k].tobytes() == fresh[k].tobytes(), (what, k)


def test_a_kept_workspace_changes_nothing():
    lib = S.lib()
    lib.shd_tcp_keep_workspace(0)   # (whatever an earlier test kept)
    try:
        lib.shd_tcp_keep_workspace(1)
        a_first = _run(96, 0.02)        # on an empty workspace: A fresh
        b_kept = _run(64, 0.0)          # in A's buffers
        lib.shd_tcp_keep_workspace(0)
        b_fresh = _run(64, 0.0)
        lib.shd_tcp_keep_workspace(1)
        b_again = _run(64, 0.0)         # on an empty workspace, kept for A
        a_kept = _run(96, 0.02)         # the workspace grows
    finally:
        lib.shd_tcp_keep_workspace(0)
    assert a_first["events"] > b_fresh["events"] > 0 and len(a_first["hosts"]) == 96 and len(b_fresh["hosts"]) == 64
    _same(b_kept, b_fresh, "B after A, kept")
    _same(b_again, b_fresh, "B kept, first")
    _same(a_kept, a_first, "A after B, kept")
