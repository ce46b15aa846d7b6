"""The second fill of a speculative batch starts each missed read where its traceback can first be (gssw_device.hpp: refill_col0).

The rule, for a LOCAL read with a traceback in a window that is a chain: with the end cell (r_e, c_e) and the score S of the first fill, m the
largest match score, B the two full-length bonuses and gx = min(go, ge), a path to the end cell deletes at most
D_max = 1 + floor((m (r_e + 1) + B - S - go) / gx) columns (0 when the numerator is negative) and so lies in columns
[c_e - r_e - D_max, c_e]; the fill starts at that column rounded down to a multiple of 4.  No bound for gx = 0, windows with branches, and the
pinned and X-drop modes.

Everything here runs the engine's own lane code on the CPU emulator, speculation forced on, against the oracle — field by field, op by op —
and against itself with VGAMD_NO_REFILL_BOUND=1.  Batch.refill_stats() says how many missed reads really started right of column 0 (so that a
bound quietly switched off cannot pass) and how many walks asked for a code left of their start (never)."""
import subprocess

import numpy as np
import pytest

from util import EMU_LIB, ORACLE_LIB, ROOT
from vg_amd import capi

BASES = "ACGT"
NODE = 32
FIELDS = ("status", "score", "end_node", "end_offset", "end_read", "first_offset", "n_ops")
LOCAL_TB = capi.VGK_GSSW_LOCAL | capi.VGK_GSSW_TRACEBACK


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "emu"], cwd=ROOT)
    return EMU_LIB


def rand_seq(rng, n):
    return "".join(BASES[i] for i in rng.integers(0, 4, n))


def chain(ref, node=NODE):
    nodes = [ref[k:k + node] for k in range(0, len(ref), node)]
    return nodes, [[]] + [[v - 1] for v in range(1, len(nodes))]


def mutate(rng, tmpl, length, sub, indel):
    out, i = [], 0
    while len(out) < length and i < len(tmpl):
        r = rng.random()
        if r < indel / 2:
            i += int(rng.geometric(0.5)); continue
        if r < indel:
            out.extend(rand_seq(rng, int(rng.geometric(0.5))))
        out.append(BASES[int(rng.integers(0, 4))] if rng.random() < sub else tmpl[i]); i += 1
    while len(out) < length:
        out.append(BASES[int(rng.integers(0, 4))])
    return "".join(out[:length])


def linear_problem(rng, indel, sub=0.01, read_len=150, width=None, start=None, deletion=0):
    width = int(rng.choice([384, 416])) if width is None else width
    ref = rand_seq(rng, width)
    lo = int(rng.integers(96, width - read_len - 48)) if start is None else start      # (as the flagship workload: reads lie a flank away from the window's edges; the left edge has a test of its own)
    tmpl = ref[lo:]
    if deletion:
        at = int(rng.integers(read_len // 5, 4 * read_len // 5))
        tmpl = tmpl[:at] + tmpl[at + deletion:]
    nodes, preds = chain(ref)
    return {"read": mutate(rng, tmpl, read_len, sub, indel), "nodes": nodes, "preds": preds, "flags": LOCAL_TB, "pinning": None}


def rule_col0(res, ops, problem, sc):
    """refill_col0 restated, from a result (the oracle's): -> (col0, D_max, first column of the path, deleted columns), or None without a traceback"""
    if res["score"] <= 0 or res["n_ops"] == 0:
        return None
    starts = np.concatenate([[0], np.cumsum([len(s) for s in problem["nodes"]])])
    c_e = int(starts[res["end_node"]] + res["end_offset"]); r_e = int(res["end_read"])
    mine = ops[res["ops_begin"]:res["ops_begin"] + res["n_ops"]]
    n_m = int(sum(o["len"] for o in mine if o["op"] == capi.OP_M)); n_d = int(sum(o["len"] for o in mine if o["op"] == capi.OP_D))
    m = max(0, max(sc.matrix)); gx = min(sc.gap_open, sc.gap_extend)
    if gx == 0:
        return 0, None, c_e - n_m - n_d + 1, n_d
    num = m * (r_e + 1) + 2 * sc.full_length_bonus - int(res["score"]) - sc.gap_open
    d_max = 0 if num < 0 else 1 + num // gx
    return max(0, c_e - r_e - d_max) & ~3, d_max, c_e - n_m - n_d + 1, n_d


def run(lib, ps, sc, bound=True, monkeypatch=None, orders=(1,)):
    """one resident batch, run once per entry of `orders` (1 = speculate, 2 = plain) -> [(results, ops, stats)]"""
    if not bound:
        monkeypatch.setenv("VGAMD_NO_REFILL_BOUND", "1")
    try:
        eng = capi.Engine(sc, lib=lib)
        out = []
        with eng.pack(ps, 0) as b:
            for mode in orders:
                eng.set_speculation(mode)
                b.run(); b.sync()
                assert b.speculated() == (mode == 1)
                st = b.refill_stats()
                r, o = b.fetch()
                out.append((r.copy(), o.copy(), st))
        return out
    finally:
        if not bound:
            monkeypatch.delenv("VGAMD_NO_REFILL_BOUND")


def same(r, o, ro, oo, what):
    for f in FIELDS:
        assert (r[f] == ro[f]).all(), (what, f, np.nonzero(r[f] != ro[f])[0][:8])
    tot = int(ro["n_ops"].sum())
    for i in range(len(r)):
        a = o[r["ops_begin"][i]:r["ops_begin"][i] + r["n_ops"][i]]; b = oo[ro["ops_begin"][i]:ro["ops_begin"][i] + ro["n_ops"][i]]
        assert (a.view(np.uint64) == b.view(np.uint64)).all(), (what, i)
    return tot


def check(emu_lib, monkeypatch, problems, sc, what, min_share=None, max_bounded=None, orders=(1,), rule=True):
    """engine == oracle == engine with the switch, no walk left of its start; -> the bounded run's stats and the rule's col0 per read (oracle's alignments)"""
    ps = capi.ProblemSet.from_lists(problems)
    ro, oo = capi.Engine(sc, lib=ORACLE_LIB).align(ps, 0)
    col0 = []
    for i, p in enumerate(problems):                                   # first: the oracle's own alignments lie inside the rule's range
        q = rule_col0(ro[i], oo, p, sc) if (rule and p["flags"] == LOCAL_TB) else None
        col0.append(q[0] if q else 0)
        if q and q[1] is not None:
            assert q[3] <= q[1] and q[2] >= q[0], (what, i, q)
    on = run(emu_lib, ps, sc, orders=orders)
    off = run(emu_lib, ps, sc, bound=False, monkeypatch=monkeypatch, orders=orders)
    for k, ((r, o, st), (r2, o2, st2)) in enumerate(zip(on, off)):
        same(r, o, ro, oo, (what, "bound", k)); same(r2, o2, ro, oo, (what, "switch", k))
        assert st["broken"] == 0 and st2["broken"] == 0 and st2["bounded"] == 0, (what, st, st2)
        if orders[k] == 1:
            assert st["missed"] == st2["missed"] > 0 and st["waves"] == st2["waves"] and st["steps"] <= st2["steps"], (what, st, st2)
            share = st["bounded"] / st["missed"]
            print("%s run %d: %d of %d missed reads started right of column 0 (%.1f %%); steps per second-fill wavefront %.1f, unbounded %.1f"
                  % (what, k, st["bounded"], st["missed"], 100 * share, st["steps"] / st["waves"], st2["steps"] / st2["waves"]))
            if min_share is not None:
                assert share > min_share, (what, st)
            if max_bounded is not None:
                assert st["bounded"] <= max_bounded, (what, st)
            if rule:                                                    # only reads the rule gives a start to can have one
                assert st["bounded"] <= int((np.array(col0) > 0).sum()), (what, st)
        else:
            assert st["missed"] == 0 and st["bounded"] == 0
    return on[0][2], np.array(col0)


@pytest.mark.parametrize("indel", [0.001, 0.01, 0.05])
def test_linear_windows_at_three_indel_rates(emu_lib, monkeypatch, indel):
    rng = np.random.default_rng(int(indel * 1e4))
    problems = [linear_problem(rng, indel) for _ in range(1100)]
    st, col0 = check(emu_lib, monkeypatch, problems, capi.Scoring.simple(1, 4, 6, 1, 5), "linear %g" % indel, min_share=0.9)
    # the starts fall inside nodes and exactly on nodes' first columns
    assert ((col0 > 0) & (col0 % NODE == 0)).sum() > 20 and ((col0 > 0) & (col0 % NODE != 0)).sum() > 200
    assert st["steps"] / st["waves"] < 260                              # (unbounded: close to 400)


def test_planted_deletions_up_to_and_beyond_the_bound(emu_lib, monkeypatch):
    """A clean read with one deletion of D columns scores 160 - 5 - D: the rule's D_max is exactly D, the tightest case.  Beyond about 25 columns
    the soft clip wins and the oracle's alignment is another one; either way the engine's is the oracle's."""
    rng = np.random.default_rng(11)
    problems = [linear_problem(rng, 0.0, sub=0.0 if k % 2 else 0.01, deletion=1 + k % 40) for k in range(1120)]
    check(emu_lib, monkeypatch, problems, capi.Scoring.simple(1, 4, 6, 1, 5), "planted deletions", min_share=0.9)


def test_end_cells_near_the_left_edge_start_at_column_0(emu_lib, monkeypatch):
    rng = np.random.default_rng(12)
    problems = [linear_problem(rng, 0.01, start=int(rng.integers(0, 4))) for _ in range(1100)]
    # (reads that start in the window's first four columns: the diagonal through the end cell meets row 0 left of column 4 unless the alignment
    # clips the read's start or ends early — a handful of reads may, and those the rule bounds; check() holds the engine to the rule's count)
    st, col0 = check(emu_lib, monkeypatch, problems, capi.Scoring.simple(1, 4, 6, 1, 5), "left edge")
    assert (col0 == 0).mean() > 0.99 and st["bounded"] < 0.01 * st["missed"]


def test_reads_shorter_than_one_lane_block(emu_lib, monkeypatch):
    rng = np.random.default_rng(13)
    problems = [linear_problem(rng, 0.0, sub=0.0, read_len=12, width=96, start=int(rng.integers(30, 70)), deletion=1) for _ in range(1100)]
    check(emu_lib, monkeypatch, problems, capi.Scoring.simple(1, 4, 6, 1, 5), "12-base reads", min_share=0.9)


def test_windows_with_snp_bubbles_run_unbounded(emu_lib, monkeypatch):
    rng = np.random.default_rng(14)
    problems = []
    for _ in range(1100):
        p = linear_problem(rng, 0.01)
        nodes, v = p["nodes"], int(rng.integers(2, 9))
        # node v becomes: its first 15 bases, a SNP bubble of two one-base nodes, the rest
        a, alt = nodes[v][15], BASES[(BASES.index(nodes[v][15]) + 1) % 4]
        nodes = nodes[:v] + [nodes[v][:15], a, alt, nodes[v][16:]] + nodes[v + 1:]
        preds = [[]] + [[k - 1] for k in range(1, len(nodes))]
        preds[v + 2] = [v]; preds[v + 3] = [v + 1, v + 2]
        problems.append(dict(p, nodes=nodes, preds=preds))
    check(emu_lib, monkeypatch, problems, capi.Scoring.simple(1, 4, 6, 1, 5), "SNP bubbles", max_bounded=0, rule=False)


def test_scorings_without_a_bound_and_with_a_larger_match(emu_lib, monkeypatch):
    rng = np.random.default_rng(15)
    problems = [linear_problem(rng, 0.01) for _ in range(1100)]
    check(emu_lib, monkeypatch, problems, capi.Scoring.simple(1, 4, 6, 0, 5), "gap extension 0", max_bounded=0)
    check(emu_lib, monkeypatch, problems, capi.Scoring.simple(2, 4, 6, 1, 5), "match 2", min_share=0.9)
    check(emu_lib, monkeypatch, problems, capi.Scoring.simple(1, 4, 2, 3, 5), "open below extend", min_share=0.9)


def test_pinned_and_xdrop_reads_of_a_batch_run_unbounded(emu_lib, monkeypatch):
    rng = np.random.default_rng(16)
    problems = [linear_problem(rng, 0.01) for _ in range(1100)]
    n_other = 0
    for k in range(0, 1100, 6):
        p = problems[k]; n_other += 1
        if k % 12:
            problems[k] = dict(p, flags=capi.VGK_GSSW_PINNED | capi.VGK_GSSW_TRACEBACK, pinning=[0] * (len(p["nodes"]) - 1) + [1])
        else:
            problems[k] = dict(p, flags=capi.VGK_XDROP_PINNED | capi.VGK_GSSW_TRACEBACK, max_gap=16)
    st, _ = check(emu_lib, monkeypatch, problems, capi.Scoring.simple(1, 4, 6, 1, 5), "mixed modes")
    assert st["missed"] - st["bounded"] >= n_other and st["bounded"] > 0


def test_speculative_plain_speculative_on_one_resident_batch(emu_lib, monkeypatch):
    """the plain run must find every read back at column 0 (refill_restore_one), the third run its bounds again"""
    rng = np.random.default_rng(17)
    problems = [linear_problem(rng, 0.01) for _ in range(1100)]
    check(emu_lib, monkeypatch, problems, capi.Scoring.simple(1, 4, 6, 1, 5), "spec, plain, spec", min_share=0.9, orders=(1, 2, 1))
