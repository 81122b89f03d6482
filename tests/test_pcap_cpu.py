"""The pcap writer (shadow-1_amd/host/shd_pcap.c: shd_pcap_format,
shd_pcap_write_host) and the config front-end's logpcap / pcapdir attributes,
on the CPU.

The byte layout is utility/pcap_writer.c:19-137 restated: here a second time,
independently, with struct.pack, over hand-made records.  It is not compared
against a file the reference wrote (the reference harness never sets
logPcap)."""
import itertools
import os
import struct

import numpy as np
import pytest

import shdgpu as S

MAC = bytes([0x01, 0x23, 0x45, 0x67, 0x89, 0xAB, 0xA1, 0xB2, 0xC3, 0xD4, 0xE5, 0xF6])
GLOBAL = struct.pack("=IHHiIII", 0xA1B2C3D4, 2, 4, 0, 0, 65535, 1)


def rec(time, sip, dip, sport, dport, seq, ack, win, length, flags, d):
    return (time, sip, dip, seq, ack, win, sport, dport, length, flags, d, 0)


def records():
    """every flag combination; ACK clear with a non-zero ack; a window past 16
    bits; payloads 0 and 1434 (one MSS); a time whose nanoseconds below 1 us
    are non-zero; both directions"""
    out = []
    for i, fl in enumerate(itertools.product((0, 1), repeat=4)):
        flags = (S.PCAP_RST * fl[0]) | (S.PCAP_SYN * fl[1]) | (S.PCAP_ACK * fl[2]) | (S.PCAP_FIN * fl[3])
        out.append(rec(2 * S.SHD_SEC + 50_000_000 + i * 1001, 0x0B000001, 0x0B000002, 61271, 58745, 1000 + i,
                       77 + i, 121 + i, 1434 if i % 3 == 0 else (0 if i % 3 == 1 else 700), flags, i & 1))
    out.append(rec(3 * S.SHD_SEC + 999, 0x0B000002, 0x0B000001, 58745, 61271, 0, 1, 121, 0, S.PCAP_SYN, S.PCAP_IN))
    out.append(rec(3 * S.SHD_SEC + 123_456_789, 0xC0A80001, 0x0B0000FE, 80, 65535, 0xFFFFFFFF, 0xFFFFFFFE, 70000, 1434,
                   S.PCAP_ACK, S.PCAP_OUT))
    out.append(rec(299 * S.SHD_SEC + 999_999_999, 0x0B000001, 0x0B000001, 10000, 10001, 5, 0, 65536 + 914, 1,
                   S.PCAP_ACK | S.PCAP_FIN, S.PCAP_IN))
    return np.array(out, dtype=S.PCAP_DTYPE)


def restate(r, headers_only=False):
    """pcap_writer.c:45-137 for one record, written from the reference's text"""
    orig = 66 + int(r["len"])
    incl = 66 if headers_only else orig
    t = int(r["time"])
    ack_set = bool(r["flags"] & S.PCAP_ACK)
    tcp_flags = ((0x04 if r["flags"] & S.PCAP_RST else 0) | (0x02 if r["flags"] & S.PCAP_SYN else 0) |
                 (0x10 if ack_set else 0) | (0x01 if r["flags"] & S.PCAP_FIN else 0))
    b = struct.pack("=IIII", t // 10**9, (t % 10**9) // 1000, incl, orig)
    b += MAC + b"\x08\x00"
    b += bytes([0x45, 0x00]) + struct.pack("!H", orig - 14) + b"\x00\x00" + b"\x40\x00" + bytes([64, 6]) + b"\x00\x00"
    b += struct.pack("!II", int(r["src_ip"]), int(r["dst_ip"]))
    b += struct.pack("!HHII", int(r["src_port"]), int(r["dst_port"]), int(r["seq"]), int(r["ack"]) if ack_set else 0)
    b += bytes([0x80, tcp_flags]) + struct.pack("!H", int(r["win"]) & 0xFFFF) + b"\x00\x00" + bytes(14)
    if not headers_only:
        b += bytes(int(r["len"]))
    return b


def test_record_mirror_matches_the_header(tmp_path):
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "r.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s/include/shdtcp.h"\n'
                   'int main(void){printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\\n", sizeof(shd_pcap_rec),'
                   ' offsetof(shd_pcap_rec, win), offsetof(shd_pcap_rec, len), offsetof(shd_pcap_rec, dir),'
                   ' offsetof(shd_tcp_model, pcap_host), offsetof(shd_tcp_model, pcap_ring),'
                   ' offsetof(shd_tcp_result, pcap_records), offsetof(shd_tcp_result, pcap_ring_peak));'
                   'return 0;}\n' % repo)
    exe = tmp_path / "r"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    d = S.PCAP_DTYPE
    assert got == [d.itemsize, d.fields["win"][1], d.fields["len"][1], d.fields["dir"][1],
                   S.TcpModel.pcap_host.offset, S.TcpModel.pcap_ring.offset, S.TcpResult.pcap_records.offset,
                   S.TcpResult.pcap_ring_peak.offset]
    assert 32 <= d.itemsize <= 40


@pytest.mark.parametrize("headers_only", [False, True])
def test_writer_bytes_equal_the_restatement(headers_only):
    r = records()
    flags = S.PCAP_HEADERS_ONLY if headers_only else 0
    got = S.pcap_bytes(r, flags)
    want = GLOBAL + b"".join(restate(x, headers_only) for x in r)
    assert len(got) == len(want)
    assert got == want
    # record by record, without the global header
    for x in r:
        assert S.pcap_bytes(x.reshape(1), flags, header=False) == restate(x, headers_only)
    assert S.pcap_bytes(r[:0], flags) == GLOBAL and len(GLOBAL) == 24


def test_writer_truncates_win_and_zeroes_ack_without_the_flag():
    r = records()
    syn = S.pcap_bytes(r[16:17], header=False)   # SYN alone, ack = 1 in the packet
    assert r[16]["ack"] == 1 and not r[16]["flags"] & S.PCAP_ACK
    assert syn[16 + 14 + 20 + 8:16 + 14 + 20 + 12] == bytes(4)
    assert syn[:8] == struct.pack("=II", 3, 0)   # 999 ns: below one microsecond
    wide = S.pcap_bytes(r[17:18], header=False)
    assert wide[16 + 14 + 20 + 14:16 + 14 + 20 + 16] == struct.pack("!H", 70000 & 0xFFFF)
    assert wide[:8] == struct.pack("=II", 3, 123456)


@pytest.mark.parametrize("headers_only", [False, True])
def test_generic_walk_ends_at_eof(headers_only):
    """a reader that knows pcap only: records by incl_len end exactly at EOF,
    each an Ethernet/IPv4/TCP frame whose IP total length is orig_len - 14"""
    r = records()
    b = S.pcap_bytes(r, S.PCAP_HEADERS_ONLY if headers_only else 0)
    magic, vmaj, vmin, zone, sig, snap, net = struct.unpack("=IHHiIII", b[:24])
    assert (magic, vmaj, vmin, zone, sig, snap, net) == (0xA1B2C3D4, 2, 4, 0, 0, 65535, 1)
    at, n = 24, 0
    while at < len(b):
        sec, usec, incl, orig = struct.unpack("=IIII", b[at:at + 16])
        at += 16
        frame = b[at:at + incl]
        assert len(frame) == incl and incl <= orig and usec < 10**6
        assert frame[12:14] == b"\x08\x00"
        assert struct.unpack("!H", frame[16:18])[0] == orig - 14
        if not headers_only:
            assert struct.unpack("!H", frame[16:18])[0] == incl - 14
        assert frame[14] == 0x45 and frame[23] == 6
        assert frame[14 + 20 + 12] >> 4 == 8   # TCP data offset: 32 bytes
        assert orig == 66 + int(r[n]["len"]) and incl == (66 if headers_only else orig)
        at += incl
        n += 1
    assert at == len(b) and n == len(r)


def test_files_and_names(tmp_path, monkeypatch):
    r = records()
    caps = {0: r[:5], 2: r[5:]}
    names, ips = ["server", "idle", "client7"], [0x0B000001, 0x0B000002, 0xC0A80164]
    d = tmp_path / "caps"
    d.mkdir()
    paths = S.write_pcap_files(caps, names, ips, directory=str(d))
    assert sorted(os.listdir(d)) == sorted(["server-11.0.0.1.pcap", "server-127.0.0.1.pcap",
                                           "client7-192.168.1.100.pcap", "client7-127.0.0.1.pcap"])
    assert [os.path.basename(p) for p in paths] == ["server-11.0.0.1.pcap", "client7-192.168.1.100.pcap"]
    assert (d / "server-11.0.0.1.pcap").read_bytes() == S.pcap_bytes(r[:5])
    assert (d / "client7-192.168.1.100.pcap").read_bytes() == S.pcap_bytes(r[5:])
    # the loopback interface's file: the global header only
    assert (d / "server-127.0.0.1.pcap").read_bytes() == GLOBAL
    assert (d / "client7-127.0.0.1.pcap").read_bytes() == GLOBAL
    # a trailing slash is not doubled; headers-only files
    S.write_pcap_files({0: r[:5]}, names, ips, directory=str(d) + "/", flags=S.PCAP_HEADERS_ONLY)
    assert (d / "server-11.0.0.1.pcap").read_bytes() == S.pcap_bytes(r[:5], S.PCAP_HEADERS_ONLY)
    # no directory: data/pcapdata/ under the working directory
    monkeypatch.chdir(tmp_path)
    os.makedirs("data/pcapdata")
    S.write_pcap_files({1: r[:0]}, names, ips)
    assert sorted(os.listdir("data/pcapdata")) == ["idle-11.0.0.2.pcap", "idle-127.0.0.1.pcap"]
    assert open("data/pcapdata/idle-11.0.0.2.pcap", "rb").read() == GLOBAL


def test_a_file_that_cannot_be_opened_is_an_error(tmp_path):
    with pytest.raises(S.ShdError):
        S.write_pcap_files({0: records()[:1]}, ["h"], [0x0B000001], directory=str(tmp_path / "missing"))
    assert S.lib().shd_pcap_write_host(str(tmp_path / "missing").encode(), b"h", 0x0B000001, None, 0, 0) == -2
    assert S.lib().shd_pcap_write_host(None, None, 0x0B000001, None, 0, 0) == -22


def test_config_logpcap_and_pcapdir():
    xml = (b'<shadow stoptime="10"><topology path="t.graphml"/>'
           b'<host id="a" logpcap="TRUE" pcapdir="caps/a"><process plugin="p" starttime="1"/></host>'
           b'<host id="b" LogPcap="false" quantity="2"/>'
           b'<host id="c"/>'
           b'<host id="d" logpcap="true"/>'
           b'<host id="e" logpcap="yes" PCAPDIR="/tmp/x/"/>'
           b'</shadow>')
    hosts, ips, stop, topo = S.load_config(xml)
    assert [h["name"] for h in hosts] == ["a", "b1", "b2", "c", "d", "e"]
    assert [h["logpcap"] for h in hosts] == [True, False, False, False, True, False]
    assert [h["pcapdir"] for h in hosts] == ["caps/a", None, None, None, None, "/tmp/x/"]
    # the fields around them are where they were
    assert hosts[0]["process_start_s"] == [1] and hosts[1]["process_start_s"] == []
    assert len(set(ips.tolist())) == 6 and stop == 10
