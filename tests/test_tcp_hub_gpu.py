"""The TCP path on the GPU with hub hosts -- one host that many others talk to,
its socket slots, processes and interface queue sized from the model
(include/shdtcp.h) -- against the reference's own loop: every case of
tests/tcp_hub_cases.py, each host's [STATUS] lines in its own order, the
tracker's [node] lines and every host's event-ID counter, packet counter and
RNG state equal to tests/golden/ref_tcp_hub.json (tests/test_tcp_hub_ref_cpu.py
shows the fixture is the reference's and which of it the oracle reproduces).
The shape the result reports (max_host_sockets, max_host_procs, sock_bytes) is
the rule's, so a build that keeps fixed arrays at some larger constant does
not pass."""
import functools
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import shdgpu as S
import tcp as TCPGPU
import tcp_cases as TC
import tcp_hub_cases as TH

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "ref_tcp_hub.json")))
BASE = json.load(open(os.path.join(HERE, "golden", "ref_tcp.json")))


@functools.lru_cache(maxsize=None)
def run_case(name, mode="device"):
    """one run of a case (computed once per argument set, never changed)"""
    c, m = TH.build(name)
    return TCPGPU.run(m, c["graph"], TC.ip_ints(FIX[name]["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                      node=True, qdisc=c.get("qdisc", 0), mode=mode, udp=TC.udp_arg(c))


def check_run(r, f):
    got = r["lines"]
    assert len(got) == f["n_status"], (len(got), f["n_status"])
    assert TC.digest(got) == f["status_by_host_sha256"]
    assert len(r["node_lines"]) == f["n_heartbeat"]
    assert TC.digest(r["node_lines"]) == f["heartbeat_sha256"]
    assert r["next_event_id"].tolist() == f["next_event_id"]
    assert r["next_packet_id"].tolist() == f["next_packet_id"]
    assert r["rng_probe"].tolist() == f["rng_probe"]


def check_shape(r, procs, peers, apps=None, hosts=None):
    """the result's shape against the rule, over `hosts` (default: all)"""
    slots = TH.slots_by_rule(procs, peers, apps)
    per = TH.procs_per_host(procs)
    if hosts is not None:
        slots = {h: n for h, n in slots.items() if h in hosts}
        per = {h: n for h, n in per.items() if h in hosts}
    assert r["sock_bytes"] == sum(slots.values()) * S.TCP_SOCK_BYTES
    assert r["max_host_procs"] == max(per.values(), default=0)


# the most socket slots one host used: a hub's listeners and children,
# fan_out20's clients.  hub12_mixed's hub also holds its datagram process's
# socket; its per-datagram sockets are released when the interface has sent
# their datagram, and a child created later takes the slot one of them left,
# so how many more slots it used depends on when the interface drains them:
# none at least, the 15 others the rule allows the process at most
SOCKETS = {"hub12_fifo": 24, "hub40_rr": 80, "hub40_slow": 80, "fan_out20": 20}


@pytest.mark.parametrize("mode", ["device", "tables"])
@pytest.mark.parametrize("name", list(TH.CASES))
def test_tcp_hub_gpu_equals_reference(name, mode):
    """mode "device": the path cache's first-touch rule on the device;
    "tables": path tables resolved by the driver.

    hub40_slow is also the case where the order of a GHashTable shows: at
    t = 3.043136240 s a child socket of the hub closes with three segments
    (sequences 12, 14, 15) still in its retransmit queue, and the reference's
    full clear (_tcp_clearRetransmit with -1, tcp.c:876-897) drops them in its
    table's order (14, 15, 12); the library puts those lines into that order
    (csrc/ght_order.h), which the oracle does not (its file comment)."""
    r = run_case(name, mode)
    assert r["rounds"] > 0 and r["events"] > 0
    assert r["first_touch"] == mode
    c = TH.CASES[name]()
    check_shape(r, c["procs"], c["peers"], c.get("apps"))
    if name in SOCKETS:
        assert r["max_host_sockets"] == SOCKETS[name]
    else:
        assert 24 + 1 <= r["max_host_sockets"] <= 24 + 16
    assert r["max_host_procs"] == {"hub12_fifo": 12, "hub40_rr": 40, "hub40_slow": 40, "fan_out20": 20,
                                   "hub12_mixed": 13}[name]
    check_run(r, FIX[name])


def run_ranks(world, case, tmp_path, mode, limit=120):
    """`world` ranks of tests/tcp_hub_group_worker.py on one GPU over the
    host-memory communicator, each under its own time limit"""
    name = "shdtcph_" + uuid.uuid4().hex[:16]
    procs = [subprocess.Popen(["timeout", "-k", "10", str(limit), sys.executable, "-u",
                               os.path.join(HERE, "tcp_hub_group_worker.py"), "--rank", str(r), "--world",
                               str(world), "--name", name, "--out", str(tmp_path), "--case", case, "--mode", mode],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(world)]
    outs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=limit + 20)
            outs.append(out.decode(errors="replace"))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} exited {p.returncode}:\n{outs[r][-3000:]}"
    return [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(world)]


@pytest.mark.parametrize("name,world,mode", [("hub12_fifo", 2, "device"), ("hub12_fifo", 3, "tables"),
                                             ("hub40_rr", 2, "tables"), ("hub40_rr", 3, "device")])
def test_tcp_hub_group_equals_reference(name, world, mode, tmp_path):
    """two and three engines, one process each: each rank sizes its own hosts
    from the whole model (the hub's children come from clients on the other
    ranks); the ranks' union is the fixture, and each rank's shape the rule's
    over its hosts"""
    f = FIX[name]
    c = TH.CASES[name]()
    H = len(f["ips"])
    res = run_ranks(world, name, tmp_path, mode)
    assert [int(x["first_host"]) for x in res] == [r * H // world for r in range(world)]
    assert sum(int(x["n_local_hosts"]) for x in res) == H
    lines = [tuple(x) for r in res for x in json.loads(str(r["lines"]))]
    node = sorted((tuple(x) for r in res for x in json.loads(str(r["node_lines"]))), key=lambda x: (x[0], x[1]))
    assert len(lines) == f["n_status"] and TC.digest(lines) == f["status_by_host_sha256"]
    assert len(node) == f["n_heartbeat"] and TC.digest(node) == f["heartbeat_sha256"]
    for k in ("next_event_id", "next_packet_id", "rng_probe"):
        got = np.concatenate([r[k] for r in res]).tolist()
        for h, (x, y) in enumerate(zip(got, f[k])):
            assert x == y, (k, "host", h, x, y)
        assert len(got) == len(f[k])
    assert {str(r["first_touch"]) for r in res} == {mode}
    for x in res:
        h0, n = int(x["first_host"]), int(x["n_local_hosts"])
        check_shape({k: int(x[k]) for k in ("sock_bytes", "max_host_procs")}, c["procs"], c["peers"],
                    hosts=set(range(h0, h0 + n)))
    assert int(res[0]["max_host_sockets"]) == SOCKETS[name]   # the hub is rank 0's
    assert all(int(x["max_host_sockets"]) == 1 for x in res[1:])


def test_tcp_hub_scaled_model_equals_oracle():
    """workloads.tcp_hub_model at 100 hosts (two blocks of lanes, four hubs of
    48 sockets and 24 processes, three in one block and one in the other):
    every host's [STATUS] lines and end state equal the oracle's; the oracle's
    run has no ROUTER_DROPPED line (asserted on the CPU as well,
    tests/test_tcp_hub_ref_cpu.py), so it is the reference's there"""
    g, m, ips, procs, peers, nb = TH.hub100()
    o = TH.hub100_oracle()
    assert not any("ROUTER_DROPPED" in body for _, _, body in o["lines"])
    want = TC.by_host(o["lines"])
    r = TCPGPU.run(m, g, ips, procs, peers, nbytes=nb)
    assert len(r["lines"]) == len(want) and r["lines"] == want
    assert r["next_event_id"].tolist() == o["next_event_id"].tolist()
    assert r["next_packet_id"].tolist() == o["next_packet_id"].tolist()
    assert r["rng_probe"].tolist() == o["rng_probe"].tolist()
    assert r["events"] == o["events"]
    check_shape(r, procs, peers)
    assert r["max_host_sockets"] == 48 and r["max_host_procs"] == 24
    assert r["sock_bytes"] == (4 * 48 + 96) * S.TCP_SOCK_BYTES


def test_tcp_small_case_takes_the_slots_it_needs():
    """geo_pairs (tests/tcp_cases.py) through the ranges: the reference's
    fixture still, with one slot per client host and two per server host"""
    c, m = TC.build("geo_pairs")
    f = BASE["geo_pairs"]
    r = TCPGPU.run(m, c["graph"], TC.ip_ints(f["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"], node=True)
    check_run(r, f)
    check_shape(r, c["procs"], c["peers"])
    assert r["sock_bytes"] == (10 * 1 + 10 * 2) * S.TCP_SOCK_BYTES
    assert r["max_host_sockets"] == 2 and r["max_host_procs"] == 1
