"""Every model shd_tcp_run refuses, with the code it refuses it with, without a
device: the driver's plan (tcp_plan in csrc/tcp.hip) decides all of them from
the model alone, in a fixed order, before anything touches a device.

Each row starts from a valid model -- tests/tcp_cases.py's lossy_2pct (two
hosts on one vertex, a server and its client) through tcp.fill_model, or that
plus a datagram process on each host -- changes one thing and names the code.
Two rows break two rules and pin the order of the checks: the unroutable pair
(-113) comes after the heartbeat check and before the queueing discipline's.

The rows marked NEEDS_DEVICE_BEFORE were checked after the device was opened
until the driver got its plan phase: a library from before that returns -5 for
them on a machine without a device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import shdgpu as S
import tcp as TCPGPU
import tcp_cases as TC

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = json.load(open(os.path.join(HERE, "golden", "ref_tcp.json")))
SEC, MS = S.SHD_SEC, S.SHD_MS
EINVAL, EHOSTUNREACH = -22, -113
DGRAM_MAX = 65507   # CONFIG_DATAGRAM_MAX_SIZE


def echo(**kw):
    """lossy_2pct as the driver fills it: one vertex, 50 ms, so the window is 50 ms"""
    c, m = TC.build("lossy_2pct")
    return TCPGPU.fill_model(m, TC.ip_ints(BASE["lossy_2pct"]["ips"]), c["procs"], c["peers"], np.full((1, 1), 50.0),
                             np.full((1, 1), 0.98), np.zeros(2, dtype=np.int32), c["nbytes"], **kw)


def dgram(**kw):
    """the same with a datagram process on each host (processes 2 and 3), both of
    application 0: a listener that sends to its host's app_peer"""
    c, m = TC.build("lossy_2pct")
    udp = dict(apps=[-1, -1, 0, 0], specs=[(S.SHD_SEND_LISTENER, S.SHD_DEST_PEER, 2, 1)], app_peer=[1, 0], payload=512)
    return TCPGPU.fill_model(m, TC.ip_ints(BASE["lossy_2pct"]["ips"]), c["procs"] + [(0, SEC), (1, SEC)],
                             c["peers"] + [-1, -1], np.full((1, 1), 50.0), np.full((1, 1), 0.98),
                             np.zeros(2, dtype=np.int32), c["nbytes"], udp=udp, **kw)


def run(tm):
    res = C.POINTER(S.TcpResult)()
    rc = S.lib().shd_tcp_run(C.byref(tm), 0, C.byref(res))
    got = bool(res)
    if got:
        S.lib().shd_tcp_result_free(res)
    return rc, got


def _set(field, value):
    return lambda tm, keep: setattr(tm, field, value)


def _put(key, index, value):
    def f(tm, keep):
        keep[key].reshape(-1)[index] = value
    return f


def _both(*fs):
    def f(tm, keep):
        for g in fs:
            g(tm, keep)
    return f


def _classes(tm, keep):
    keep["cls"] = np.array([0, 2], dtype=np.uint8)
    tm.host_class = S.as_ptr(keep["cls"], C.c_uint8)
    tm.n_classes = 2


def _zero_heartbeat(tm, keep):
    keep["hb"] = np.array([SEC, 0], dtype=np.uint64)
    tm.host_heartbeat = S.as_ptr(keep["hb"], C.c_uint64)


REQUIRED = ["host_ip", "host_seed", "bw_down_kibps", "bw_up_kibps", "path_lat_ms", "path_rel", "host_vertex",
            "proc_host", "proc_start", "proc_peer"]
SERIES = S.TCP_OPT_SERIES | S.TCP_OPT_FLOWS
NEEDS_DEVICE_BEFORE = {"qdisc 2"}

# (name, base, base's keywords, the one change, the code)
ROWS = [
    ("n_hosts 0", echo, {}, _set("n_hosts", 0), EINVAL),
    ("n_hosts above 2^26", echo, {}, _set("n_hosts", (1 << 26) + 1), EINVAL),
    ("n_procs negative", echo, {}, _set("n_procs", -1), EINVAL),
] + [("%s null" % f, echo, {}, _set(f, None), EINVAL) for f in REQUIRED] + [
    ("series without flows", echo, dict(series_us=1000), _set("options", S.TCP_OPT_SERIES), EINVAL),
    ("series with interval 0", echo, {}, _set("options", SERIES), EINVAL),
    ("series_cap above 2^26", echo, dict(flows=True, series_us=1000), _set("series_cap", (1 << 26) + 1), EINVAL),
    ("proc_host past the hosts", echo, {}, _put("ph", 1, 2), EINVAL),
    ("proc_host negative", echo, {}, _put("ph", 1, -1), EINVAL),
    ("proc_peer past the processes", echo, {}, _put("pp", 1, 2), EINVAL),
    ("a client of a client", echo, {}, _put("pp", 0, 1), EINVAL),
    ("a client of a datagram process", dgram, {}, _put("pp", 1, 2), EINVAL),
    ("a datagram process with a peer", dgram, {}, _put("pp", 2, 0), EINVAL),
    ("datagram: no app_spec", dgram, {}, _set("app_spec", None), EINVAL),
    ("datagram: n_app_specs 0", dgram, {}, _set("n_app_specs", 0), EINVAL),
    ("datagram: payload 0", dgram, {}, _set("udp_payload", 0), EINVAL),
    ("datagram: payload above the maximum", dgram, {}, _set("udp_payload", DGRAM_MAX + 1), EINVAL),
    ("datagram: app index past n_app_specs", dgram, {}, _put("pa", 3, 1), EINVAL),
    ("datagram: two on one host", dgram, {}, _put("ph", 3, 0), EINVAL),
    ("datagram: spec send out of range", dgram, {}, _put("sp", 0, 3), EINVAL),
    ("datagram: spec dest out of range", dgram, {}, _put("sp", 1, 3), EINVAL),
    ("datagram: spec per_read out of range", dgram, {}, _put("sp", 3, 2), EINVAL),
    ("datagram: weighted destinations without dest_cum", dgram, {},
     _both(_put("sp", 1, 0), _set("dest_cum", None)), EINVAL),
    ("datagram: peer destinations without app_peer", dgram, {}, _set("app_peer", None), EINVAL),
    ("datagram: app_peer past the hosts", dgram, {}, _put("ap", 1, 2), EINVAL),
    ("datagram: app_peer negative", dgram, {}, _put("ap", 0, -1), EINVAL),
    ("datagram: host_class past n_classes", dgram, {}, _classes, EINVAL),
    ("capture with a datagram process", dgram, dict(pcap=dict(hosts=[1])), lambda tm, keep: None, EINVAL),
    ("pcap_ring above 2^24", echo, dict(pcap=dict(hosts=[0])), _set("pcap_ring", (1 << 24) + 1), EINVAL),
    ("host_vertex past the vertices", echo, {}, _put("hv", 1, 1), EINVAL),
    ("host_vertex negative", echo, {}, _put("hv", 0, -1), EINVAL),
    ("packets_per_host above 2^24", echo, {}, _set("packets_per_host", (1 << 24) + 1), EINVAL),
    ("a zero latency between two hosts", echo, {}, _put("lat", 0, 0.0), EINVAL),
    ("a client starting inside its server's window", echo, {}, _put("ps", 1, SEC + 10 * MS), EINVAL),
    ("a client starting with its server", echo, {}, _put("ps", 1, SEC), EINVAL),
    ("qdisc 2", echo, {}, _set("qdisc", 2), EINVAL),
    ("a connection's pair without a route", echo, {}, _put("lat", 0, -1.0), EHOSTUNREACH),
    # two rules at once: the checks' order
    ("no route and qdisc 2", echo, {}, _both(_put("lat", 0, -1.0), _set("qdisc", 2)), EHOSTUNREACH),
    ("no route and a zero heartbeat", echo, {}, _both(_put("lat", 0, -1.0), _zero_heartbeat), EINVAL),
]


def test_row_names_are_distinct():
    names = [r[0] for r in ROWS]
    assert len(set(names)) == len(names) and NEEDS_DEVICE_BEFORE <= set(names)


@pytest.mark.parametrize("base", [echo, dgram], ids=["echo", "dgram"])
def test_the_bases_are_not_refused(base):
    """what every row starts from passes the plan: the run then needs a device
    (-5 without one, a result with one), so a row's code is its one change's"""
    tm, keep = base()
    rc, got = run(tm)
    del keep
    assert rc in (0, -5) and got == (rc == 0)


@pytest.mark.parametrize("name,base,kw,change,code", ROWS, ids=[r[0].replace(" ", "_") for r in ROWS])
def test_refused(name, base, kw, change, code):
    tm, keep = base(**kw)
    change(tm, keep)
    rc, got = run(tm)
    del keep
    assert rc == code, name
    assert not got, name


def test_null_model_and_null_result_are_refused():
    tm, keep = echo()
    res = C.POINTER(S.TcpResult)()
    assert S.lib().shd_tcp_run(None, 0, C.byref(res)) == EINVAL and not res
    assert S.lib().shd_tcp_run(C.byref(tm), 0, None) == EINVAL
    del keep
