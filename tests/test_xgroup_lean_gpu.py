"""The engine group across processes, UNTRACED, against the serial oracle.

Tracing, heartbeats, a bootstrap period or path counters switch off the lean
instantiations of the round kernels (engine.hip lean_model), and every other
multi-rank comparison with the oracle is traced: it runs k_round_px<false> and
k_round_spx<false>, while every benchmark and production-style run is untraced
and launches <true> (eng_group.h x_enqueue_fused), whose put, region-take and
ingest path then carries the ranks' remote traffic.  Here `world` child
processes (xgroup_worker.py --case) run the untraced cases of lean_cases.py in
a group, with the worker's stops and resumes (but for the 4160-host pair); the concatenated host digests
and the summed event counts must be the oracle's, every rank must have run
packet events, and all ranks the same number of rounds.  There is no trace to
compare, so the per-host digests carry the comparison.

The group leaves the fused schedule by itself when its regions keep spilling
(eng_group.h: g->fused = false), so every test also asserts which schedule ran,
from the batch counters the worker sums (n_batches_fused, n_batches_sparse):
a test meant for k_round_px must not pass on k_round_xtl.

The ranks share one GPU here; the fused schedule then needs all their blocks
resident at once, one per compute unit.  The largest row (4160 hosts over two
ranks) has 66 blocks of 64 hosts.

What each case's input must show (drops, CoDel drops, a window over three
bins, both classes sending) is asserted on the oracle's output alone.
"""
import numpy as np
import pytest

from lean_cases import check_tor_inputs, make_case, oracle_of
from test_xgroup_procs_gpu import run_ranks

pytestmark = pytest.mark.gpu

# the worker's stats array: its seven sums, then the batch counters and the window of --case
PKT, EV, ROUNDS, FALLBACK, BATCHES, SPARSE, FUSED, WINDOW = 0, 1, 3, 6, 7, 8, 9, 10


def run_case(name, world, tmp_path, p2p=True, sp_hosts=None, one_run=False):
    """The case over `world` processes, checked against the oracle: (per-rank results, oracle digest, model)."""
    env = {"SHD_SP_HOSTS": str(sp_hosts)} if sp_hosts else None
    res = run_ranks(world, tmp_path, extra=["--case", name] + (["--p2p"] if p2p else []) +
                    (["--one-run"] if one_run else []), env_extra=env)
    g, m = make_case(name)
    odg, ost = oracle_of(name, g, m)
    st = np.stack([r["stats"] for r in res]).astype(np.int64)
    print(f"{name} x{world} {'p2p' if p2p else 'all-to-all'} sp_hosts {sp_hosts}: rounds {st[:, ROUNDS].tolist()} "
          f"batches {st[:, BATCHES].tolist()} fused {st[:, FUSED].tolist()} sparse {st[:, SPARSE].tolist()} "
          f"packet events {st[:, PKT].tolist()} of {ost['n_pkt_events']}, events {int(st[:, EV].sum())} of "
          f"{ost['n_events']}")
    assert all(len(r["trace"]) == 0 for r in res)
    assert (st[:, FALLBACK] == 0).all()                       # the transport asked for is the one that ran
    assert np.array_equal(np.concatenate([r["digest"] for r in res]), odg)
    assert int(st[:, EV].sum()) == ost["n_events"]
    assert int(st[:, PKT].sum()) == ost["n_pkt_events"]
    assert (st[:, PKT] > 0).all()
    assert len(set(st[:, ROUNDS].tolist())) == 1             # every rank ran the same rounds
    assert (st[:, BATCHES] > 0).all()
    return st, odg, m


def assert_fused_dense(st):
    """k_round_px<true> ran, and nothing else took over"""
    assert (st[:, FUSED] > 0).all() and (st[:, SPARSE] == 0).all()
    assert (st[:, FUSED] == st[:, BATCHES]).all()             # the group never left the fused schedule


def assert_fused_sparse(st):
    """k_round_spx<true> ran (forced: every fused batch is sparse)"""
    assert (st[:, SPARSE] > 0).all()
    assert (st[:, FUSED] == st[:, BATCHES]).all() and (st[:, SPARSE] == st[:, FUSED]).all()


@pytest.mark.parametrize("world", [2, 3, 4])
def test_fused_rounds_untraced(world, tmp_path):
    """k_round_px<true>: 300 hosts over 2 ranks (150 hosts: 3 blocks, the last
    with 22 lanes), 3 ranks (100 hosts: the second block partly filled) and 4
    ranks (75 hosts)."""
    st, odg, _ = run_case("hosts300", world, tmp_path)
    assert int(odg["n_inet_drop"].sum()) > 0
    assert_fused_dense(st)


def test_two_launch_rounds_untraced(tmp_path):
    """The all-to-all transport: k_round_xtl with the host-side exchange, untraced."""
    st, _, _ = run_case("hosts300", 2, tmp_path, p2p=False)
    assert (st[:, FUSED] == 0).all() and (st[:, SPARSE] == 0).all()


def test_fused_sparse_rounds_untraced_many_blocks(tmp_path):
    """k_round_spx<true> with SHD_SP_HOSTS=256 on 4160 hosts over 2 ranks: 2080
    hosts a rank in 9 sparse blocks, about ten hosts per vertex.  The same
    case without the variable runs the dense fused kernel over 33 blocks a rank
    and must take the same number of rounds.

    Both run to the end in one call, as an untraced production run does.  A
    round's next time is a lower bound where it comes from a calendar bin (the
    bin's start, cal_lower_bound), and the two kernels need not arrive at the
    same bound, so after a window that a stop cuts short they may start the
    next one at different times, both no later than its first event: with the
    worker's stop 3 ns into the application start's burst the sparse run opens
    its next window at 1 000 341 504 ns (a bin's start) and the dense one at
    1 001 000 000 ns (a timer), and the runs take 1844 and 1843 rounds, both
    with the oracle's digests.  In one call both take 1843, as one engine does."""
    sp = tmp_path / "sp"
    plain = tmp_path / "plain"
    sp.mkdir()
    plain.mkdir()
    st, odg, _ = run_case("hosts4160", 2, sp, sp_hosts=256, one_run=True)
    assert int(odg["n_inet_drop"].sum()) > 0
    assert_fused_sparse(st)
    pst, _, _ = run_case("hosts4160", 2, plain, one_run=True)
    assert_fused_dense(pst)
    assert int(st[0, ROUNDS]) == int(pst[0, ROUNDS])


def test_fused_sparse_rounds_untraced_small_blocks(tmp_path):
    """SHD_SP_HOSTS=64 on 300 hosts over 3 ranks: sparse blocks of 64 hosts, the second of 36."""
    st, _, _ = run_case("hosts300", 3, tmp_path, sp_hosts=64)
    assert_fused_sparse(st)


@pytest.mark.parametrize("sp_hosts", [None, 64], ids=["dense", "sparse64"])
def test_codel_with_remote_arrivals_untraced(sp_hosts, tmp_path):
    """CoDel queues building, lean kernels, arrivals from other ranks: the
    combination of the 1 M-host C5 run, at 50 hosts a rank."""
    st, odg, _ = run_case("codel", 3, tmp_path, sp_hosts=sp_hosts)
    assert int(odg["n_codel_drop"].sum()) > 0
    (assert_fused_sparse if sp_hosts else assert_fused_dense)(st)


@pytest.mark.parametrize("sp_hosts", [None, 64], ids=["dense", "sparse64"])
def test_window_spanning_three_bins_untraced(sp_hosts, tmp_path):
    """Whole-millisecond latencies: the window is 1.9 calendar bins wide, so it
    spans three, and every row of the path table ties."""
    st, _, m = run_case("threebins", 2, tmp_path, sp_hosts=sp_hosts)
    (assert_fused_sparse if sp_hosts else assert_fused_dense)(st)
    window = int(st[0, WINDOW])
    assert (st[:, WINDOW] == window).all()
    width = 1 << (int(window).bit_length() - 1)               # the calendar's bin width
    assert window % 1_000_000 == 0 and window > 1.9 * width


@pytest.mark.parametrize("p2p", [False, True], ids=["alltoall", "p2p"])
def test_tor_classes_untraced(p2p, tmp_path):
    """The relay/client model over 3 processes, untraced: two host classes
    with a destination row each, the relays -- most of the traffic -- all on
    rank 0, so the exchange is lopsided."""
    st, odg, m = run_case("tor", 3, tmp_path, p2p=p2p)
    check_tor_inputs(m, odg)
    assert m.n_classes == 2 and int(np.asarray(m.host_class)[:m.n_hosts // 3].min()) == 0
    assert (np.asarray(m.host_class)[m.n_hosts // 3:] == 1).all()   # ranks 1 and 2 hold clients only
    if p2p:
        assert_fused_dense(st)
    else:
        assert (st[:, FUSED] == 0).all()
