"""The second fill of a speculative batch walks its own reads (GsswParams::refill_walk), on the device.

With the field set the wavefront that filled a missed read pair again also walks it back, at the end of the fill kernel, and no
gssw_walk_missed_kernel follows.  The form was measured slower on the MI355X and ships off: VGAMD_REFILL_WALK=1, read when a batch is packed, sets the
field; VGAMD_NO_REFILL_WALK=1 leaves it 0 and the same library runs the separate kernel.  Every batch here is packed twice, once with either switch, so
that both forms run whatever the default is: results and ops must be byte-identical between the two forms and equal
the oracle's, refill_stats() the same in both with no walk left of its read's start — wavefronts, missed and bounded reads; not the wavefronts' summed
steps: on the device the miss list fills in the order the first walk's lanes arrive, which reads share a second-fill wavefront differs from run to run
of one form already, and with it the maximum each wavefront runs to (a step or two in a few hundred).

The batches: miss lists of M reads with M mod 16 = 0, 1 and 15 (a last pair with one read, a last wavefront with one pair: indels planted in
exactly M reads of an otherwise error-free batch) and M = 0 (no wavefront of the second-fill grid has work); 5 % indels (nearly every read
misses); windows with a SNP bubble (the walks read boundary columns their own wavefront has just written to the scratch); local and pinned reads
mixed; an op window too small for the reads with indels (the same reads must report VGK_EOPS); read lengths that take the second fill through each
of its instantiations (12 and 64 bases: 16 rows per lane, the former with one lane per pair and 128 reads per wavefront; 150: 19; 100: 20, twelve
pairs per wavefront; 96: 24); a batch on the second launch lane; one resident batch run speculative, plain, speculative."""
import numpy as np
import pytest

from test_refill_bound import linear_problem, same
from test_refill_layout_lanes import N, SC, bubble_batch, chain_batch, mixed_batch, oracle_of, run_batch
from util import ENGINE_LIB
from vg_amd import capi

pytestmark = pytest.mark.gpu


def stable(st):
    """refill_stats() without the one figure that depends on the order the miss list filled in"""
    return {k: v for k, v in st.items() if k != "steps"}


def both_forms(monkeypatch, problems, packer="pack_windows", orders=(1,), ops_per=0):
    """-> [(results, ops, stats)] per run of the batch packed with the walks in the fill, after holding it to the batch packed without"""
    monkeypatch.setenv("VGAMD_REFILL_WALK", "1")
    try:
        on = run_batch(ENGINE_LIB, problems, packer, orders=orders, ops_per=ops_per)
    finally:
        monkeypatch.delenv("VGAMD_REFILL_WALK")
    monkeypatch.setenv("VGAMD_NO_REFILL_WALK", "1")
    try:
        off = run_batch(ENGINE_LIB, problems, packer, orders=orders, ops_per=ops_per)
    finally:
        monkeypatch.delenv("VGAMD_NO_REFILL_WALK")
    for k, ((r, o, st), (r2, o2, st2)) in enumerate(zip(on, off)):
        assert r.tobytes() == r2.tobytes(), (k, [f for f in r.dtype.names if (r[f] != r2[f]).any()])
        assert o.tobytes() == o2.tobytes(), k
        assert stable(st) == stable(st2) and st["broken"] == 0, (k, st, st2)
        assert (st["steps"] > 0) == (st["waves"] > 0) == (st2["steps"] > 0), (k, st, st2)
    return on


def checked(monkeypatch, problems, what, **kw):
    ro, oo = oracle_of(problems)
    runs = both_forms(monkeypatch, problems, **kw)
    for k, (r, o, st) in enumerate(runs):
        same(r, o, ro, oo, (what, k))
    return runs


def planted(m, seed):
    """an error-free batch whose miss list has exactly m reads.  The first read of a batch of 150-base reads is always on it (walk_diag_one fetches the 160
    bytes that end with a read's end cell, and before the arena's first read there are none): a three-column deletion planted in m - 1 others.
    m = 0: reads of 160 bases, none with a deletion."""
    rng = np.random.default_rng(seed)
    if m == 0:
        return [linear_problem(rng, 0.0, sub=0.0, read_len=160) for _ in range(N)]
    at = set(1 + int(k) for k in rng.choice(N - 1, m - 1, replace=False))
    return [linear_problem(rng, 0.0, sub=0.0, deletion=3 if k in at else 0) for k in range(N)]


@pytest.mark.parametrize("m", [0, 32, 33, 47])
def test_miss_lists_that_end_inside_a_pair_and_inside_a_wavefront(monkeypatch, m):
    (r, o, st), = checked(monkeypatch, planted(m, 31 + m), "planted %d" % m)
    print(m, st)
    assert st["missed"] == m and st["waves"] == (m + 15) // 16 and st["bounded"] == m, st


def test_nearly_every_read_misses(monkeypatch):
    rng = np.random.default_rng(32)
    (r, o, st), = checked(monkeypatch, [linear_problem(rng, 0.05, sub=0.05) for _ in range(N)], "5 % indels")
    assert st["missed"] > 0.9 * N, st


@pytest.mark.parametrize("packer", ["pack", "pack_windows"])
def test_bubble_windows_walk_over_the_scratch_of_their_own_fill(monkeypatch, packer):
    (r, o, st), = checked(monkeypatch, bubble_batch(33), "bubbles", packer=packer)
    assert st["missed"] > 100 and st["bounded"] == 0, st


def test_local_and_pinned_reads_mixed(monkeypatch):
    problems, n_other = mixed_batch(34, "pinned")
    (r, o, st), = checked(monkeypatch, problems, "local + pinned", packer="pack")
    assert st["bounded"] > 0 and st["missed"] - st["bounded"] >= n_other, st


def test_op_windows_too_small_for_some_reads(monkeypatch):
    """two ops per read: M alone, or M and one soft clip — a read with an indel needs three at least and must report VGK_EOPS in both forms (both_forms
    holds the statuses to each other byte for byte); every read's score is the oracle's, and every read that fits has the oracle's alignment"""
    problems = chain_batch(35)
    ro, oo = oracle_of(problems)
    (r, o, st), = both_forms(monkeypatch, problems, ops_per=2)
    eops = r["status"] == capi.VGK_EOPS
    assert st["missed"] > 100 and eops.sum() > 50 and (r["status"][~eops] == 0).all(), (st, int(eops.sum()))
    assert (ro["n_ops"][eops] > 2).all() and (ro["n_ops"][~eops] <= 2).all()
    for f in ("score", "end_node", "end_offset", "end_read"):
        assert (r[f] == ro[f]).all(), f
    for i in np.nonzero(~eops)[0]:
        assert r["n_ops"][i] == ro["n_ops"][i] and capi.cigar_string(r[i], o) == capi.cigar_string(ro[i], oo), i


@pytest.mark.parametrize("read_len", [12, 64, 150, 100, 96])
def test_each_instantiation_of_the_second_fill(monkeypatch, read_len):
    rng = np.random.default_rng(36 + read_len)
    width = 96 if read_len == 12 else None
    problems = [linear_problem(rng, 0.0 if read_len == 12 else 0.02, sub=0.01, read_len=read_len, width=width,
                               start=int(rng.integers(30, 70)) if read_len == 12 else None, deletion=1 if read_len == 12 else 0) for _ in range(N)]
    (r, o, st), = checked(monkeypatch, problems, "%d-base reads" % read_len)
    assert st["missed"] > 100 and st["bounded"] > 0, st


def test_a_batch_on_the_second_launch_lane(monkeypatch):
    problems = chain_batch(37)
    ro, oo = oracle_of(problems)
    for no_walk in (False, True):
        monkeypatch.setenv("VGAMD_NO_REFILL_WALK" if no_walk else "VGAMD_REFILL_WALK", "1")
        eng = capi.Engine(SC, lib=ENGINE_LIB)
        eng.set_speculation(1)
        ps = capi.ProblemSet.from_lists(problems)
        with eng.pack(ps, 0) as b0, eng.pack(ps, 0) as b1:                  # (consecutive batches of a context alternate between its two lanes)
            assert b0.lane() == 0 and b1.lane() == 1
            b0.run(); b1.run(); b1.sync(); b0.sync()
            assert b1.speculated() and b0.speculated()
            st0, st1 = b0.refill_stats(), b1.refill_stats()
            for b in (b1, b0):
                r, o = b.fetch()
                same(r, o, ro, oo, ("lane", b.lane(), no_walk))
        assert stable(st0) == stable(st1) and st1["broken"] == 0 and st1["missed"] > 100, (st0, st1)
        monkeypatch.delenv("VGAMD_NO_REFILL_WALK" if no_walk else "VGAMD_REFILL_WALK")


def test_speculative_plain_speculative_on_one_resident_batch(monkeypatch):
    runs = checked(monkeypatch, chain_batch(38), "spec, plain, spec", orders=(1, 2, 1))
    assert runs[1][2]["missed"] == 0 and stable(runs[0][2]) == stable(runs[2][2]) and runs[0][2]["bounded"] > 0
