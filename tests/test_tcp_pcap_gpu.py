"""Packet capture of the TCP path on the GPU (shd_tcp_model.pcap_host,
csrc/tcp.hip pcap_capture): a capture host's records against the expectation
tests/pcap_expect.py derives from [STATUS] lines that are themselves pinned
to the reference's loop (tests/golden/ref_tcp.json; oracle/o_tcp.c on the
CPU).  Record content and per-direction order are checked that way; the
interleaving of directions within one nanosecond follows from where the two
capture points sit (network_interface.c:415-418, 571-574), one instance of
which is asserted below; the file's byte layout is tests/test_pcap_cpu.py's."""
import functools
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import oracle_ffi as O
import pcap_expect as PE
import shdgpu as S
import tcp as TCPGPU
import tcp_cases as TC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "ref_tcp.json")))


@functools.lru_cache(maxsize=None)
def oracle_lines(name):
    """the case's lines from the oracle, each host's in its own order (computed once, never changed)"""
    f = FIX[name]
    c, m = TC.build(name)
    o = O.tcp_run(m, c["graph"], TC.ip_ints(f["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                  qdisc=c.get("qdisc", 0))
    lines = tuple(TC.by_host(o["lines"]))
    assert TC.digest(lines) == f["status_by_host_sha256"]   # the expectation's source is the reference's
    return lines


def run_case(name, mode="device", hosts=None, ring=0, trace=True):
    f = FIX[name]
    c, m = TC.build(name)
    ips = TC.ip_ints(f["ips"])
    hosts = list(range(len(ips))) if hosts is None else hosts
    return TCPGPU.run(m, c["graph"], ips, c["procs"], c["peers"], nbytes=c["nbytes"], qdisc=c.get("qdisc", 0),
                      mode=mode, trace=trace, pcap=dict(hosts=hosts, ring=ring))


@functools.lru_cache(maxsize=None)
def geo_all():
    """geo_pairs, every host captured, the default ring: shared by the tests below"""
    return run_case("geo_pairs")


def same_records(a, b):
    return a.dtype == b.dtype and len(a) == len(b) and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("mode", ["device", "tables"])
@pytest.mark.parametrize("name", ["ref_epoll_lossless", "lossy_2pct", "bulk_2mb", "loopback_mixed", "shared_hosts_rr"])
def test_pcap_every_host_equals_the_lines(name, mode):
    """Every host a capture host: retransmissions and SACK (lossy_2pct), the
    widest windows of a long transfer (bulk_2mb; this reference counts a
    window in segments, so the fixtures' stay below 16 bits -- the widest is
    loopback_mixed's 4387 -- and the writer's cut to 16 bits is checked on
    hand-made records in test_pcap_cpu.py), loopback and routed packets on one
    interface (loopback_mixed), the round-robin qdisc (shared_hosts_rr).  The
    run itself is still the fixture's."""
    f = FIX[name]
    r = run_case(name, mode)
    assert TC.digest(r["lines"]) == f["status_by_host_sha256"] and len(r["lines"]) == f["n_status"]
    assert r["next_event_id"].tolist() == f["next_event_id"]
    assert r["next_packet_id"].tolist() == f["next_packet_id"]
    assert r["rng_probe"].tolist() == f["rng_probe"]
    assert r["first_touch"] == mode
    assert sorted(r["pcap_records"]) == list(range(len(f["ips"])))
    PE.check(r["pcap_records"], oracle_lines(name))
    # ... and against the run's own lines (the same thing, given the digest)
    PE.check(r["pcap_records"], r["lines"])
    assert all(len(v) > 0 for v in r["pcap_records"].values())
    assert r["pcap_drains"] >= 1 and 0 < r["pcap_ring_peak"] <= 65536
    if name == "loopback_mixed":
        h0 = r["pcap_records"][0]
        own = h0["dst_ip"] == h0["src_ip"]
        assert own.any() and not own.all()
        # a loopback packet is captured twice by its host: out, and in 1 ns later
        assert (h0["dir"][own] == S.PCAP_OUT).sum() == (h0["dir"][own] == S.PCAP_IN).sum() > 0


def test_pcap_synack_precedes_the_syn_in_the_servers_file():
    """ref_epoll_lossless: the server's first two records share one nanosecond,
    and the SYN+ACK (out) comes before the client's SYN (in).  The SYN is
    captured after socket_pushInPacket returns (network_interface.c:408,
    416-418); inside that call the listener multiplexes a child whose reply
    goes out at once (tcp.c:1823-1852 sets responseFlags = SYN|ACK, sent by
    _tcp_sendControlPacket -> _tcp_flush -> socket_addToOutputBuffer ->
    networkinterface_wantsSend -> _networkinterface_sendPackets, :604, which
    captures at :572-574).  The [STATUS] lines are in the other order."""
    r = run_case("ref_epoll_lossless")
    srv = r["pcap_records"][0]
    a, b = srv[0], srv[1]
    assert a["time"] == b["time"] == 2_050_000_000
    assert a["dir"] == S.PCAP_OUT and a["flags"] == S.PCAP_SYN | S.PCAP_ACK
    assert b["dir"] == S.PCAP_IN and b["flags"] == S.PCAP_SYN
    first = [ln[2] for ln in r["lines"] if ln[1] == 0 and ln[2].startswith(("[SND_INTERFACE_SENT]",
                                                                          "[RCV_INTERFACE_RECEIVED]"))][:2]
    assert first[0].startswith("[RCV_") and first[1].startswith("[SND_")
    # the client's file starts with its SYN going out; its ACK flag is clear, its ack field is not
    cli = r["pcap_records"][1]
    assert cli[0]["dir"] == S.PCAP_OUT and cli[0]["flags"] == S.PCAP_SYN and cli[0]["time"] == 2_000_000_000


def test_pcap_subset_of_hosts():
    """geo_pairs capturing hosts {1, 4} only: the other hosts return nothing,
    and the two hosts' records are those of the all-hosts capture"""
    sub = run_case("geo_pairs", hosts=[1, 4])
    assert sorted(sub["pcap_records"]) == [1, 4]
    every = geo_all()["pcap_records"]
    for h in (1, 4):
        assert len(sub["pcap_records"][h]) > 0
        assert same_records(sub["pcap_records"][h], every[h]), h
    PE.check(sub["pcap_records"], oracle_lines("geo_pairs"))
    PE.check(every, oracle_lines("geo_pairs"))
    f = FIX["geo_pairs"]
    assert TC.digest(sub["lines"]) == f["status_by_host_sha256"]
    assert sub["rng_probe"].tolist() == f["rng_probe"]


def test_pcap_untraced_run():
    """The bench's mode (no lines, no status lists on the device) with three
    capture hosts out of 64: the records equal the expectation from the
    oracle's lines, and the end state equals the run with no capture."""
    import workloads as W
    g, m, ips, procs, peers, nb = W.tcp_echo_model(64, 40, end_s=12, nbytes=60000)
    hosts = [0, 33, 63]
    r = TCPGPU.run(m, g, ips, procs, peers, nbytes=nb, trace=False, pcap=dict(hosts=hosts, ring=0))
    plain = TCPGPU.run(m, g, ips, procs, peers, nbytes=nb, trace=False)
    o = O.tcp_run(m, g, ips, procs, peers, nbytes=nb)
    assert r["lines"] == []
    assert sorted(r["pcap_records"]) == hosts and all(len(r["pcap_records"][h]) > 50 for h in hosts)
    PE.check(r["pcap_records"], TC.by_host(o["lines"]))
    for k in ("next_event_id", "next_packet_id", "rng_probe"):
        assert r[k].tolist() == plain[k].tolist() == o[k].tolist(), k
    assert r["events"] == plain["events"] == o["events"] and r["rounds"] == plain["rounds"]
    assert "pcap_records" not in plain


def test_pcap_ring_and_drain():
    """The rings are emptied between batches of rounds: the busiest host's
    capture is at least twice the most any ring held at a drain, so it cannot
    have fitted without one.  A ring of exactly that peak gives the same
    records; one record less fills it inside a batch, which fails the run with
    SHD_TCP_ERR_PCAP instead of truncating."""
    name, base = None, None
    for cand in ("geo_pairs", "heavy_loss", "lossy_2pct"):
        base = geo_all() if cand == "geo_pairs" else run_case(cand)
        P, T = base["pcap_ring_peak"], max(len(v) for v in base["pcap_records"].values())
        print(f"{cand}: pcap_ring_peak {P}, busiest host's records {T}, drains {base['pcap_drains']}")
        if T >= 2 * P:
            name = cand
            break
    assert name is not None
    P, T = base["pcap_ring_peak"], max(len(v) for v in base["pcap_records"].values())
    assert T >= 2 * P > 0
    tight = run_case(name, ring=P)
    assert tight["pcap_drains"] >= 2 and tight["pcap_ring_peak"] == P
    for h, v in base["pcap_records"].items():
        assert same_records(tight["pcap_records"][h], v), h
    with pytest.raises(S.ShdError) as e:
        run_case(name, ring=P - 1)
    bits = int(str(e.value).rsplit("error bits ", 1)[1], 16)
    assert bits & S.TCP_ERR_PCAP, str(e.value)


def test_pcap_refuses_datagram_processes():
    """the reference's capture asserts on a datagram (network_interface.c:348,
    packet.c:485-489): a capture host in a model with datagram processes is -22"""
    f = FIX["mixed_hosts"]
    c, m = TC.build("mixed_hosts")
    with pytest.raises(S.ShdError, match="-22"):
        TCPGPU.run(m, c["graph"], TC.ip_ints(f["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                   udp=TC.udp_arg(c), mode="tables", pcap=dict(hosts=[0], ring=0))


def test_pcap_group_of_two(tmp_path):
    """geo_pairs on two engines (processes sharing the GPU over the host-memory
    transport), one capture host on each rank: each rank returns its host's
    records, equal to the one-engine run's"""
    name = "shdpcap_" + uuid.uuid4().hex[:16]
    hosts = [3, 14]   # rank 0 runs hosts [0, 10), rank 1 [10, 20)
    procs = [subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "tcp_pcap_group_worker.py"), "--rank", str(r),
                               "--world", "2", "--name", name, "--out", str(tmp_path), "--case", "geo_pairs",
                               "--hosts", ",".join(map(str, hosts))],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=240)
            outs.append(out.decode(errors="replace"))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} exited {p.returncode}:\n{outs[r][-3000:]}"
    every = geo_all()["pcap_records"]
    f = FIX["geo_pairs"]
    probe = []
    for r in range(2):
        z = np.load(os.path.join(tmp_path, f"rank{r}.npz"))
        assert z["pcap_hosts"].tolist() == [hosts[r]]
        got = z["pcap_%d" % hosts[r]]
        assert len(got) > 0 and same_records(got, every[hosts[r]]), r
        assert int(z["pcap_drains"]) >= 1
        probe += z["rng_probe"].tolist()
    assert probe == f["rng_probe"]
