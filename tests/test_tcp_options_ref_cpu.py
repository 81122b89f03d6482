"""The fixtures of the TCP path's bootstrap period and per-host heartbeat
intervals (tests/golden/ref_tcp_options.json) are the reference's own loop's,
and the driver hands both options to the library.

Where the reference's loop is built (oracle/Makefile `ref`), three cheap cases
run through it again and must reproduce the committed fixture: the fixture is
the reference's, not the code under test's.  Every case must also differ from
its base case in tests/golden/ref_tcp.json where its option says it does, so
that a run which drops the option cannot pass.  The config test follows
<shadow bootstraptime> and <host heartbeatfrequency> from the XML into the
shd_tcp_model the driver fills (tcp.fill_model), without a device."""
import json
import os

import numpy as np
import pytest

import ref_loop_ffi as R
import shdgpu as S
import tcp as TCPGPU
import tcp_cases as TC
import tcp_option_cases as TO
import workloads as W

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "ref_tcp_options.json")))
BASE = json.load(open(os.path.join(HERE, "golden", "ref_tcp.json")))


def test_every_case_has_a_fixture():
    assert sorted(FIX) == sorted(TO.OPTION_CASES)
    for name, f in FIX.items():
        c, m = TO.build(name)
        assert len(f["ips"]) == len(c["hv"]) == len(f["next_event_id"]) == len(f["rng_probe"]), name


@pytest.mark.parametrize("name", [n for n in TO.OPTION_CASES if TO.base_of(n)])
def test_option_changes_what_the_base_case_pins(name):
    """a bootstrap period changes the [STATUS] lines; per-host intervals change
    the [node] lines and the event-ID counters (and leave the [STATUS] lines)"""
    f, b = FIX[name], BASE[TO.base_of(name)]
    _, boot, hb = TO.OPTION_CASES[name]
    assert f["ips"] == b["ips"]
    if boot:
        assert f["status_sha256"] != b["status_sha256"]
        assert f["status_by_host_sha256"] != b["status_by_host_sha256"]
        assert f["first_inet_dropped"] < 0 or f["first_inet_dropped"] >= boot
    else:
        assert f["status_sha256"] == b["status_sha256"]
    if hb:
        assert f["heartbeat_sha256"] != b["heartbeat_sha256"] and f["n_heartbeat"] > b["n_heartbeat"]
        assert f["next_event_id"] != b["next_event_id"]
    assert f["status_sha256"] != b["status_sha256"] or f["heartbeat_sha256"] != b["heartbeat_sha256"]


def test_whole_run_inside_the_period_drops_nothing():
    f = FIX["boot_whole_run"]
    assert f["n_inet_dropped"] == 0 and f["n_router_dropped"] == 0
    assert FIX["boot_lossy"]["n_inet_dropped"] > 0 and FIX["boot_slow_links"]["n_router_dropped"] > 0


@pytest.mark.skipif(not R.available(), reason="oracle/_ref/libshdref_loop.so not built (needs the reference tree)")
@pytest.mark.parametrize("name", TO.CHEAP)
def test_reference_loop_reproduces_the_option_fixture(name):
    f = FIX[name]
    c, m = TO.build(name)
    r = R.run(m, c["graph"], procs=c["procs"], tcp=TC.tcp_arg(c))
    st, hb = TC.status_lines(r["lines"]), TC.node_lines(r["lines"])
    assert r["ip"] == f["ips"]
    assert len(st) == f["n_status"] and TC.digest(st) == f["status_sha256"]
    assert TC.digest(TC.by_host(st)) == f["status_by_host_sha256"]
    assert len(hb) == f["n_heartbeat"] and TC.digest(hb) == f["heartbeat_sha256"]
    assert r["next_event_id"].tolist() == f["next_event_id"]
    assert r["next_packet_id"].tolist() == f["next_packet_id"]
    assert r["rng_probe"].tolist() == f["rng_probe"]
    assert TO.first_time(st, "INET_DROPPED") == (f["n_inet_dropped"], f["first_inet_dropped"])
    assert TO.first_time(st, "ROUTER_DROPPED") == (f["n_router_dropped"], f["first_router_dropped"])


def _config():
    with open(os.path.join(HERE, "golden", "example_shadow.config.xml"), "rb") as fh:
        xml = fh.read()
    xml = xml.replace(b'<shadow stoptime="3600">', b'<shadow stoptime="30" bootstraptime="2">')
    xml = xml.replace(b'<host id="server">', b'<host id="server" heartbeatfrequency="3">')
    xml = xml.replace(b'<host id="client">', b'<host id="client" heartbeatfrequency="7">')
    assert xml.count(b"heartbeatfrequency") == 2 and b"bootstraptime" in xml
    return xml


def test_config_options_reach_the_tcp_model():
    """bootstraptime="2" and two hosts with heartbeatfrequency 3 and 7: the
    model config_model builds carries them, and so does the shd_tcp_model the
    driver fills from it, on tables and with a path cache alike"""
    g, m, _, names, ips = W.config_model(_config())
    assert names == ["server", "client"]
    assert int(m.struct.bootstrap_end) == 2 * S.SHD_SEC
    assert m.host_heartbeat.tolist() == [3 * S.SHD_SEC, 7 * S.SHD_SEC]
    procs, peers = [(0, S.SHD_SEC), (1, 2 * S.SHD_SEC)], [-1, 0]
    hvi = np.zeros(2, dtype=np.int32)
    tm, keep = TCPGPU.fill_model(m, ips, procs, peers, np.full((1, 1), 50.0), np.full((1, 1), 0.99), hvi, 20000)
    assert int(tm.bootstrap_end) == 2 * 10**9
    assert [int(tm.host_heartbeat[i]) for i in range(2)] == [3 * 10**9, 7 * 10**9]
    assert int(tm.n_hosts) == 2 and int(tm.n_procs) == 2 and int(tm.end_time) == 30 * S.SHD_SEC
    assert keep["hb"].dtype == np.uint64


def test_model_without_options_leaves_both_unset():
    c, m = TC.build("lossy_2pct")
    tm, _ = TCPGPU.fill_model(m, TC.ip_ints(BASE["lossy_2pct"]["ips"]), c["procs"], c["peers"], np.full((1, 1), 50.0),
                              np.full((1, 1), 0.98), np.zeros(2, dtype=np.int32), c["nbytes"])
    assert int(tm.bootstrap_end) == 0 and not tm.host_heartbeat


def test_zero_heartbeat_interval_is_refused():
    """a zero entry of host_heartbeat is an invalid model (-22), as on the
    packet engine; the check comes before anything touches a device"""
    c, m = TC.build("lossy_2pct")
    m.host_heartbeat = np.array([S.SHD_SEC, 0], dtype=np.uint64)
    tm, keep = TCPGPU.fill_model(m, TC.ip_ints(BASE["lossy_2pct"]["ips"]), c["procs"], c["peers"],
                                 np.full((1, 1), 50.0), np.full((1, 1), 0.98), np.zeros(2, dtype=np.int32), c["nbytes"])
    res = S.C.POINTER(S.TcpResult)()
    assert S.lib().shd_tcp_run(S.C.byref(tm), 0, S.C.byref(res)) == -22
    assert not res


def test_tcp_model_layout_appends_the_two_fields():
    """the new fields follow pcap_ring / _pad10: every earlier offset keeps its place"""
    T = S.TcpModel
    assert T.bootstrap_end.offset == T.pcap_ring.offset + 8
    assert T.host_heartbeat.offset == T.bootstrap_end.offset + 8
    assert S.C.sizeof(T) == T.host_heartbeat.offset + 8
