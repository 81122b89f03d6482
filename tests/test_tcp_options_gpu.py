"""The TCP path on the GPU with a bootstrap period (<shadow bootstraptime>:
shd_tcp_model.bootstrap_end) and per-host heartbeat intervals (<host
heartbeatfrequency>: shd_tcp_model.host_heartbeat) against the reference's own
loop: every case of tests/tcp_option_cases.py, each host's [STATUS] lines in
its own order, the tracker's [node] lines and every host's event-ID counter,
packet counter and RNG state equal to tests/golden/ref_tcp_options.json.  The
oracle (oracle/o_tcp.c) has no bootstrap period: the fixtures are the checker
(tests/test_tcp_options_ref_cpu.py shows they are the reference's)."""
import functools
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import pcap_expect as PE
import tcp as TCPGPU
import tcp_cases as TC
import tcp_option_cases as TO

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "ref_tcp_options.json")))


@functools.lru_cache(maxsize=None)
def run_case(name, mode="device", trace=True, pcap_hosts=None):
    """one run of a case (computed once per argument set, never changed)"""
    c, m = TO.build(name)
    return TCPGPU.run(m, c["graph"], TC.ip_ints(FIX[name]["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                      node=True, qdisc=c.get("qdisc", 0), mode=mode, udp=TC.udp_arg(c), trace=trace,
                      pcap=None if pcap_hosts is None else dict(hosts=list(pcap_hosts)))


def check_end_state(r, f):
    assert r["next_event_id"].tolist() == f["next_event_id"]
    assert r["next_packet_id"].tolist() == f["next_packet_id"]
    assert r["rng_probe"].tolist() == f["rng_probe"]


def check_run(r, f):
    got = r["lines"]
    assert len(got) == f["n_status"], (len(got), f["n_status"])
    assert TC.digest(got) == f["status_by_host_sha256"]
    assert len(r["node_lines"]) == f["n_heartbeat"]
    assert TC.digest(r["node_lines"]) == f["heartbeat_sha256"]
    check_end_state(r, f)
    assert TO.first_time(got, "INET_DROPPED") == (f["n_inet_dropped"], f["first_inet_dropped"])
    assert TO.first_time(got, "ROUTER_DROPPED") == (f["n_router_dropped"], f["first_router_dropped"])


@pytest.mark.parametrize("mode", ["device", "tables"])
@pytest.mark.parametrize("name", list(TO.OPTION_CASES))
def test_tcp_options_gpu_equals_reference(name, mode):
    """mode "device": the path cache's first-touch rule on the device;
    "tables": path tables resolved by the driver.  Without the two options the
    run is the base case's, whose digests differ (test_tcp_options_ref_cpu.py)."""
    r = run_case(name, mode)
    check_run(r, FIX[name])
    assert r["rounds"] > 0 and r["events"] > 0
    assert r["first_touch"] == mode


def test_tcp_options_half_second_hosts_print_zero():
    """hb_geo_pairs: host 0 beats every 0.5 s (the [node] line's first field is
    the interval in whole seconds: 0), host 1 every second, host 2 every 1.5 s (1)"""
    r = run_case("hb_geo_pairs")
    first = {}
    for t, h, body in r["node_lines"]:
        if body.startswith("[shadow-heartbeat] [node] ") and t > 0 and h not in first:
            first[h] = (t, body.split("[node] ")[1].split(",")[0])
    assert first[0] == (500_000_000, "0") and first[1] == (1_000_000_000, "1") and first[2] == (1_500_000_000, "1")


def test_tcp_options_untraced_run_keeps_end_state_and_node_lines():
    """boot_geo_pairs with no [STATUS] lines written (the bench's mode): the end
    state and the [node] lines are still the reference's"""
    f = FIX["boot_geo_pairs"]
    r = run_case("boot_geo_pairs", trace=False)
    assert r["lines"] == []
    check_end_state(r, f)
    assert len(r["node_lines"]) == f["n_heartbeat"] and TC.digest(r["node_lines"]) == f["heartbeat_sha256"]
    assert r["events"] == run_case("boot_geo_pairs")["events"]


def run_ranks(world, case, tmp_path, mode, limit=120):
    """`world` ranks of tests/tcp_options_group_worker.py on one GPU over the
    host-memory communicator, each under its own time limit"""
    name = "shdtcpo_" + uuid.uuid4().hex[:16]
    procs = [subprocess.Popen(["timeout", "-k", "10", str(limit), sys.executable, "-u",
                               os.path.join(HERE, "tcp_options_group_worker.py"), "--rank", str(r), "--world",
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


@pytest.mark.parametrize("name,mode", [("boot_geo_pairs", "device"), ("hb_boot_geo_pairs", "tables")])
def test_tcp_options_group_equals_reference(name, mode, tmp_path):
    """two engines, one process each (with this one: three hold the GPU): each
    rank runs its hosts with its slice of the intervals and the same period;
    compared host by host with the fixture"""
    f = FIX[name]
    res = run_ranks(2, name, tmp_path, mode)
    assert [int(x["first_host"]) for x in res] == [0, len(f["ips"]) // 2]
    assert sum(int(x["n_local_hosts"]) for x in res) == len(f["ips"])
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


def test_tcp_options_capture_during_and_after_the_period():
    """boot_lossy with both hosts captured: the run is still the fixture's, and
    the records are what its lines say the interfaces sent and received, before
    and after the end of the period"""
    f = FIX["boot_lossy"]
    r = run_case("boot_lossy", pcap_hosts=(0, 1))
    check_run(r, f)
    assert sorted(r["pcap_records"]) == [0, 1]
    PE.check(r["pcap_records"], r["lines"])
    boot = TO.OPTION_CASES["boot_lossy"][1]
    for h in (0, 1):
        t = r["pcap_records"][h]["time"]
        assert (t < boot).any() and (t >= boot).any(), h
