"""Fixture of the packet engine's host records (shd_tcp_hostrec with
SHD_QF_HOST_RECORDS), from the reference's own loop -- TEST INFRASTRUCTURE.
Runs cases of tests/ref_loop_cases.py through oracle/_ref/libshdref_loop.so
(the reference's worker.c, router.c, router_queue_codel.c, network_interface.c
... compiled unmodified; oracle/Makefile `ref`) and stores what
tests/tcp_host_expect.py derives from its [STATUS] lines, whose datagram form
it reads as it reads the TCP form: per case the host IPs, the number of
[STATUS] lines, the field names and one row per host
(tcp_host_expect.FIELDS: the scalars, then the histogram's 16 buckets).
Recorded results only; nothing stored comes from the oracle's restatement.

    python tests/golden/make_ref_eng_hosts.py [case ...]   # -> tests/golden/ref_eng_hosts.json
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "shadow-1_amd")]

import ref_loop_cases as RC  # noqa: E402
import ref_loop_ffi as R  # noqa: E402
import tcp_host_expect as HE  # noqa: E402

CASES = ["codel", "udp_echo_codel", "udp_mix_codel", "bootstrap", "phold_v100"]


def record(name):
    """one case through the reference's loop: its fixture entry"""
    case = RC.CASES[name]()
    r = R.run(case["model"], case["graph"], procs=RC.procs_of(case), echo=case["model"].app_peer)
    st, _ = RC.split_lines(r["lines"])
    H = int(case["model"].n_hosts)
    return dict(ips=r["ip"], n_status=len(st), fields=list(HE.FIELDS), rows=HE.rows(HE.derive(st, H)))


def main():
    path = os.path.join(HERE, "ref_eng_hosts.json")
    out = json.load(open(path)) if os.path.exists(path) else {}
    for name in sys.argv[1:] or CASES:
        out[name] = record(name)
        i = HE.SCALARS.index("if_sent")
        print(name, len(out[name]["rows"]), "hosts,", out[name]["n_status"], "lines:", HE.totals(out[name]["rows"]),
              "if_sent", sum(r[i] for r in out[name]["rows"]), flush=True)
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")


if __name__ == "__main__":
    main()
