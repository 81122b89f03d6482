"""The fixtures of the TCP path's hub models (tests/golden/ref_tcp_hub.json)
are the reference's own loop's, the oracle's restatement (oracle/o_tcp.c)
reproduces them, and the result's new fields sit where the header puts them.

Every case of tests/tcp_hub_cases.py but hub40_slow: the oracle's [STATUS]
lines hash to the fixture, and every host's event-ID counter, packet counter
and RNG state end where the reference's do.  hub40_slow: the counters and the
RNG state only -- there the oracle prints 34 234 lines against the reference's
34 372 (69 ROUTER_DROPPED lines and their PDS_DESTROYED lines are missing, the
first at 2.343 s on the hub) while every counter agrees, so the drops happen in
the oracle and only their lines are lost; the GPU is compared with the
reference's fixture alone in that case (tests/test_tcp_hub_gpu.py).  Where the
reference's loop is built (oracle/Makefile `ref`), two cases run through it
again and must reproduce the committed fixture."""
import functools
import json
import os

import pytest

import oracle_ffi as O
import ref_loop_ffi as R
import shdgpu as S
import tcp_cases as TC
import tcp_hub_cases as TH
import tcp_option_cases as TO
import workloads as W

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "ref_tcp_hub.json")))


@functools.lru_cache(maxsize=None)
def _oracle(name):
    c, m = TH.build(name)
    return O.tcp_run(m, c["graph"], TC.ip_ints(FIX[name]["ips"]), c["procs"], c["peers"], nbytes=c["nbytes"],
                     qdisc=c.get("qdisc", 0), udp=TC.udp_arg(c))


def _check_counters(o, f):
    assert o["next_event_id"].tolist() == f["next_event_id"]
    assert o["next_packet_id"].tolist() == f["next_packet_id"]
    assert o["rng_probe"].tolist() == f["rng_probe"]


def test_every_case_has_a_fixture():
    assert sorted(FIX) == sorted(TH.CASES)
    assert sorted(TH.ORACLE_LINES + TH.ORACLE_COUNTERS) == sorted(TH.CASES)
    for name, f in FIX.items():
        c, _ = TH.build(name)
        assert len(f["ips"]) == len(c["hv"]) == len(f["next_event_id"]) == len(f["rng_probe"]), name


def test_fixture_cases_cross_the_old_shape():
    """what each case is there for: more than 8 processes and more than 16
    sockets on one host, the hub's CoDel queue dropping, both transports"""
    want = {"hub12_fifo": (24, 12), "hub40_rr": (80, 40), "hub40_slow": (80, 40), "fan_out20": (20, 20),
            "hub12_mixed": (24 + 16, 13)}
    for name, (slots, procs) in want.items():
        c = TH.CASES[name]()
        assert max(TH.slots_by_rule(c["procs"], c["peers"], c.get("apps")).values()) == slots, name
        assert max(TH.procs_per_host(c["procs"]).values()) == procs, name
    assert FIX["hub40_slow"]["n_router_dropped"] == 2 * 199   # each drop's own line and its PDS_DESTROYED line
    assert FIX["hub40_slow"]["n_retransmitted"] == 224
    assert FIX["hub12_mixed"]["n_datagram"] > 0
    assert [FIX[n]["n_status"] for n in ("hub12_fifo", "hub40_rr", "hub40_slow", "fan_out20")] == \
        [13221, 24945, 34372, 17755]
    assert FIX["hub40_rr"]["status_sha256"] != FIX["hub40_slow"]["status_sha256"]


@pytest.mark.parametrize("name", TH.ORACLE_LINES)
def test_tcp_oracle_equals_hub_fixture(name):
    f = FIX[name]
    o = _oracle(name)
    assert len(o["lines"]) == f["n_status"]
    assert TC.digest(o["lines"]) == f["status_sha256"]
    assert TC.digest(TC.by_host(o["lines"])) == f["status_by_host_sha256"]
    _check_counters(o, f)


@pytest.mark.parametrize("name", TH.ORACLE_COUNTERS)
def test_tcp_oracle_equals_hub_fixture_counters(name):
    _check_counters(_oracle(name), FIX[name])


@pytest.mark.skipif(not R.available(), reason="oracle/_ref/libshdref_loop.so not built (needs the reference tree)")
@pytest.mark.parametrize("name", TH.LIVE)
def test_reference_loop_reproduces_the_hub_fixture(name):
    f = FIX[name]
    c, m = TH.build(name)
    r = R.run(m, c["graph"], procs=c["procs"], tcp=TC.tcp_arg(c))
    st, hb = TC.status_lines(r["lines"]), TC.node_lines(r["lines"])
    assert r["ip"] == f["ips"]
    assert len(st) == f["n_status"] and TC.digest(st) == f["status_sha256"]
    assert TC.digest(TC.by_host(st)) == f["status_by_host_sha256"]
    assert len(hb) == f["n_heartbeat"] and TC.digest(hb) == f["heartbeat_sha256"]
    assert r["next_event_id"].tolist() == f["next_event_id"]
    assert r["next_packet_id"].tolist() == f["next_packet_id"]
    assert r["rng_probe"].tolist() == f["rng_probe"]
    assert TO.first_time(st, "ROUTER_DROPPED") == (f["n_router_dropped"], f["first_router_dropped"])


def test_hub_model_shape_and_starts():
    """workloads.tcp_hub_model: hubs first in their groups, every client a
    second or more after its server, no two clients at one time; the rule
    gives a hub 2 * clients_per_hub slots and a client host one"""
    g, m, ips, procs, peers, nb = W.tcp_hub_model(4, 24, 40, nbytes=20000, loss_max=0.02)
    assert int(m.struct.n_hosts) == len(ips) == 100 and len(procs) == 192 and nb == 20000
    hubs = sorted({procs[k][0] for k in range(len(procs)) if peers[k] < 0})
    assert hubs == [0, 25, 50, 75] and len({h // 64 for h in hubs}) == 2
    starts = [procs[k][1] for k in range(len(procs)) if peers[k] >= 0]
    assert len(set(starts)) == len(starts)
    for k, p in enumerate(peers):
        if p >= 0:
            assert procs[k][1] >= procs[p][1] + S.SHD_SEC and procs[k][0] != procs[p][0]
    slots = TH.slots_by_rule(procs, peers)
    assert [slots[h] for h in hubs] == [48] * 4 and sum(slots.values()) == 4 * 48 + 96
    assert TH.procs_per_host(procs)[25] == 24


def test_hub_model_runs_without_router_drops():
    """the scaled model the GPU test compares line for line with the oracle
    must not reach the ground where the oracle loses ROUTER_DROPPED lines"""
    o = TH.hub100_oracle()
    assert len(o["lines"]) > 0
    assert not any("ROUTER_DROPPED" in body for _, _, body in o["lines"])


def test_tcp_result_layout_appends_the_three_fields():
    """the new fields follow pcap_ring_peak / _pad11: every earlier offset keeps its place"""
    T = S.TcpResult
    assert T.pcap_ring_peak.offset == T.pcap_drains.offset + 8
    assert T.max_host_sockets.offset == T.pcap_ring_peak.offset + 8
    assert T.max_host_procs.offset == T.max_host_sockets.offset + 4
    assert T.sock_bytes.offset == T.max_host_sockets.offset + 8
    assert S.C.sizeof(T) == T.sock_bytes.offset + 8
    # (test_abi.py compares the mirror's size and offsets with the header's)
    assert T.deliveries.offset == 80 and T.max_round_deliveries.offset == 128


def test_sock_slot_bytes_mirror_the_header():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "shdtcp.h")).read()
    assert f"#define SHD_TCP_SOCK_BYTES {S.TCP_SOCK_BYTES}\n" in hdr


GLIB = "/usr/lib/x86_64-linux-gnu/libglib-2.0.so.0"


@pytest.mark.skipif(not os.path.exists(GLIB), reason="no GLib to compare the table's order with")
def test_hash_table_order_equals_glib(tmp_path):
    """shadow-1_amd/csrc/ght_order.h (the order in which the reference's
    retransmit queue, a GHashTable keyed by sequence, hands out its entries)
    against the system's GLib: tests/ght_check.cpp runs random histories of
    inserts, removals, steals and iterator clears over a sliding window of
    keys through both and compares every iteration"""
    import subprocess
    exe = tmp_path / "ght_check"
    repo = os.path.dirname(HERE)
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(repo, "shadow-1_amd", "csrc"),
                    os.path.join(HERE, "ght_check.cpp"), "-o", str(exe), "-l:libglib-2.0.so.0"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) > 10000
