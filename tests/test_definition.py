"""Kernels, emulator and oracle against the DEFINITION of what they compute (refdp.py), and every alignment they return
re-scored from its own op list.  The other randomized tests compare engine and oracle with each other; a rule both misread
passes there.  Here the reference is the plain dynamic program of the problem statement: exact integers, no tolerance.

Per driver: the optimum is asserted for EVERY problem of the families that have one (gssw LOCAL / PINNED, un-pruned X-drop,
banded with a band that excludes nothing, WFA connects that come back ok), validity and the re-score for every alignment
returned with status 0 and score > 0; what a driver could not assert the optimum of is counted and the share asserted.
The k-best entry points (banded and pinned alternates) are held to refdp's k-best programs (f) and (g) in the same way: further down.

Boundary reads (L * match + 2 * bonus = 990 / 991 / 2046 / 2047, the limits of the packed kernels' key and score ranges):
a read of exactly 1 024 bases reaches none of these sums: a context refuses a negative full_length_bonus (VGK_EUNSUPPORTED), and with
0 <= bonus <= 127 the sum 1024 * match + 2 * bonus is 1024 .. 1278 (match 1) or at least 2048 — so the factorizations stop at 1 023 rows and
1 024-base reads are covered by the read-length sweep instead."""
import contextlib
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import refdp
import util
from gen import BASES, problem_set, random_banded_problem, random_dag, random_problem
from util import EMU_LIB, ENGINE_LIB, ORACLE_LIB, ROOT
from vg_amd import capi

LOCAL, PINNED, XDROP = capi.VGK_GSSW_LOCAL, capi.VGK_GSSW_PINNED, capi.VGK_XDROP_PINNED
TB = capi.VGK_GSSW_TRACEBACK
VGK_ENOBAND, VGK_ETOOBIG, VGK_EUNSUPPORTED = -8, -7, -9
# every scoring the suite uses that the packed kernels take for short reads ...
SCORINGS = [(1, 4, 6, 1, 5), (2, 3, 5, 2, 7), (1, 4, 6, 1, 0), (3, 5, 7, 2, 9), (1, 1, 1, 1, 5), (2, 3, 5, 2, 0), (1, 1, 1, 1, 0), (2, 2, 3, 1, 0),
            (5, 4, 9, 3, 11)]
WIDE_SCORING = (20, 9, 12, 3, 10)          # ... and the one whose scores leave 11 bits (the wide route of align_call)


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "emu"], cwd=ROOT)
    return EMU_LIB


def ops_of(row, ops):
    return ops[int(row["ops_begin"]):int(row["ops_begin"]) + int(row["n_ops"])]


def rand_seq(rng, n):
    return "".join(BASES[i] for i in rng.integers(0, 4, n))


def sinks_of(preds):
    has_succ = [False] * len(preds)
    for pr in preds:
        for q in pr:
            has_succ[q] = True
    return [0 if h else 1 for h in has_succ]


def as_mode(p, mode, max_gap=40):
    q = dict(p, flags=mode | TB, pinning=sinks_of(p["preds"]) if mode == PINNED else None)
    if mode == XDROP:
        q["max_gap"] = p.get("max_gap", max_gap)
    return q


# ---- the gssw entry points ---------------------------------------------------------------------------------------------

def run_route(eng, problems, route):
    if route == "windows":                                       # the problems' graphs behind each other as ONE resident graph
        nodes, preds, first = [], [], []
        for p in problems:
            first.append(len(nodes))
            preds += [[q + len(nodes) for q in pr] for pr in p["preds"]]; nodes += p["nodes"]
        node_len = np.array([len(s) for s in nodes], dtype=np.uint32)
        seq = np.frombuffer("".join(nodes).encode(), dtype=np.uint8).copy()
        pred_off = np.concatenate([[0], np.cumsum([len(p) for p in preds])]).astype(np.uint32)
        pred_idx = np.array([q for p in preds for q in p] or [0], dtype=np.uint32)
        graph = eng.graph(node_len, seq, pred_off, pred_idx)
        reads = np.frombuffer("".join(p["read"] for p in problems).encode(), dtype=np.uint8).copy()
        read_off = np.concatenate([[0], np.cumsum([len(p["read"]) for p in problems])])
        ws = capi.WindowSet(reads, read_off, first, [len(p["nodes"]) for p in problems], [p["flags"] for p in problems],
                            [p.get("max_gap", 40) for p in problems], cols=[sum(len(s) for s in p["nodes"]) for p in problems])
        return eng.align_windows(graph, ws)
    ps = problem_set(problems)
    return eng.align(ps) if route == "align" else eng.align_call(ps)


def check_results(problems, sc, res, ops, qual_adj=None, cache=None):
    """every problem: status 0 and the definition's optimum; every alignment: valid, and re-scored to the reported score"""
    aligned = 0
    for i, p in enumerate(problems):
        mode = p["flags"] & 15
        ctx = "problem %d: %r -> %r" % (i, p, res[i])
        assert res["status"][i] == 0, ctx
        key = (id(p), mode)
        if cache is not None and key in cache:
            opt = cache[key]
        else:
            opt = refdp.optimum(p, sc, mode, qual_adj)
            if cache is not None:
                cache[key] = opt
        assert res["score"][i] == opt, "optimum %d: %s" % (opt, ctx)
        if res["score"][i] > 0 and p["flags"] & TB:
            try:
                refdp.check_alignment(p, sc, mode, res[i], ops_of(res[i], ops), qual_adj, expect_optimum=opt)
            except AssertionError as e:
                raise AssertionError("%s: %s ops %s" % (e, ctx, capi.cigar_string(res[i], ops))) from e
            aligned += 1
    return aligned


def gssw_against_definition(lib, problems, scoring, routes=("align", "align_call"), qual_adj=None):
    sc = capi.Scoring.simple(*scoring)
    cache, aligned = {}, 0
    for route in routes:
        eng = capi.Engine(sc, lib=lib, qual_adj=qual_adj)
        res, ops = run_route(eng, problems, route)
        aligned += check_results(problems, sc, res, ops, qual_adj, cache)
    return aligned


def random_family(seed, n_per_mode, with_qual=False):
    rng = np.random.default_rng(seed)
    out = []
    for mode in (LOCAL, PINNED, XDROP):
        for k in range(n_per_mode):
            if k % 4 == 3:
                p = random_problem(rng, max_nodes=12, max_node_len=24, max_read=150, mode=mode, with_n=0.05)
            else:
                p = random_problem(rng, max_nodes=8, max_node_len=12, max_read=40, mode=mode, with_n=0.1)
            if with_qual:
                p["qual"] = rng.choice(np.array([2, 5, 10, 20, 30, 40], dtype=np.uint8), size=len(p["read"]))
            out.append(p)
    return out


def not_pinned(problems):                  # the window route takes LOCAL and X-drop
    return [p for p in problems if p["flags"] & 15 != PINNED]


def random_gssw(lib, n_per_mode, routes=("align", "align_call"), seed=100):
    """n_per_mode problems of each mode under every scoring together (the problems differ from scoring to scoring)"""
    per = -(-n_per_mode // len(SCORINGS))
    aligned = 0
    for k, s in enumerate(SCORINGS):
        aligned += gssw_against_definition(lib, random_family(seed + k, per), s, routes)
    aligned += gssw_against_definition(lib, random_family(seed + 50, 60), WIDE_SCORING, ("align_call",))
    return aligned


def quality_adjusted(lib, n_per_mode, seed=300):
    from qualadj import qual_adj_tables
    tables = qual_adj_tables(1, 4, 5)
    return gssw_against_definition(lib, random_family(seed, n_per_mode, with_qual=True), (1, 4, 6, 1, 5), qual_adj=tables)


def long_and_bubble_problems(seed, n):
    from test_gssw_wide import bubble_chain_problem, long_problem
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        mode = (LOCAL, PINNED, XDROP)[k % 3]
        if k % 2:
            out.append(long_problem(rng, mode, int(rng.integers(200, 700)), 24, 60, with_n=0.05))
        else:
            out.append(bubble_chain_problem(rng, mode, int(rng.integers(150, 500)), 30, 24))
    return out


READ_LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 2049, 4096, 4097]


def read_length_sweep(lib, lengths=READ_LENGTHS, seed=7):
    from test_gssw_wide import long_problem
    rng = np.random.default_rng(seed)
    problems = []
    for L in lengths:
        for mode in (LOCAL, PINNED, XDROP):
            p = long_problem(rng, mode, L, L // 40 + 4, 80, with_n=0.02)
            assert len(p["read"]) == L
            problems.append(p)
    return gssw_against_definition(lib, problems, (1, 4, 6, 1, 5), ("align_call",))


def edge_graphs(seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for mode in (LOCAL, PINNED, XDROP):
        out += [random_problem(rng, max_nodes=30, max_node_len=1, max_read=25, mode=mode) for _ in range(60)]        # single-base nodes
        for _ in range(20):                                                                                        # sources that are sinks
            a, b = rand_seq(rng, int(rng.integers(1, 30))), rand_seq(rng, int(rng.integers(1, 30)))
            read = (a if rng.random() < 0.5 else b)[int(rng.integers(0, 3)):] + rand_seq(rng, int(rng.integers(0, 4)))
            out.append(as_mode(dict(read=read or "A", nodes=[a, b], preds=[[], []]), mode))
        for _ in range(20):                                                   # a sink (pinning node) that is not last in topological order
            a, b, c = (rand_seq(rng, int(rng.integers(2, 20))) for _ in range(3))
            read = a[int(rng.integers(0, 2)):] + (b if rng.random() < 0.7 else c)
            out.append(as_mode(dict(read=read, nodes=[a, b, c], preds=[[], [0], [0]]), mode))
        big = rand_seq(rng, 65535)                                                                                  # the longest node an op can span
        at = 0 if mode == XDROP else 65535 - 70
        out.append(as_mode(dict(read=big[at:at + 30] + "T" + big[at + 31:at + 70], nodes=[big, "ACGT"], preds=[[], [0]]), mode))
    for max_gap in (0, 1, 7, 8, 9, 16, 17, 200):                 # leading insertions around the limit, reads that need one
        for k in (0, 1, 2, 7, 8, 9, 10, 16, 17, 24, 25):
            src = rand_seq(rng, 40)
            out.append(dict(read=rand_seq(rng, k) + src[:30], nodes=[src, rand_seq(rng, 8)], preds=[[], [0]], flags=XDROP | TB, pinning=None, max_gap=max_gap))
    return out


# Reads whose achieved LOCAL score is exactly L * match + 2 * bonus at the packed kernels' limits: 990 keeps the three-input key maximum,
# 991 must leave it off; 2046 stays on the packed kernels, 2047 goes the wide route.
BOUNDARY = {990: [(980, 1, 5), (490, 2, 5), (330, 3, 0), (196, 5, 5), (140, 7, 5), (165, 6, 0)],
            991: [(981, 1, 5), (327, 3, 5), (109, 9, 5), (991, 1, 0)],
            2046: [(1023, 2, 0), (1018, 2, 5), (682, 3, 0), (680, 3, 3)],
            2047: [(681, 3, 2), (409, 5, 1), (157, 13, 3), (89, 23, 0)]}


def boundary_graph(rng, L, bubbles):
    """a graph that holds a walk of exactly L bases (returned) with a few bases of flank either side: a chain, or a chain with SNP / indel bubbles"""
    nodes, preds, walk, last = [], [], [], []
    need = L + 12
    while sum(len(s) for s in walk) < need:
        seg = rand_seq(rng, int(rng.integers(8, 40)))
        nodes.append(seg); preds.append(list(last)); walk.append(seg)
        s = len(nodes) - 1
        if bubbles:
            a1, a2 = rand_seq(rng, 1), rand_seq(rng, int(rng.integers(1, 4)))
            nodes += [a1, a2]; preds += [[s], [s]]
            last = [s + 1, s + 2] if rng.random() < 0.8 else [s + 2, s + 1, s]
            walk.append(a1 if rng.random() < 0.5 else a2)
        else:
            last = [s]
    return nodes, preds, "".join(walk)[5:5 + L]


def boundary_problems(rng, L, n_distinct):
    """-> (exact reads, neighbours: one substitution / one inserted base / one deleted base away)"""
    exact, near = [], []
    for k in range(n_distinct):
        nodes, preds, read = boundary_graph(rng, L, bubbles=bool(k % 2))
        base = dict(nodes=nodes, preds=preds, flags=LOCAL | TB, pinning=None)
        exact.append(dict(base, read=read))
        m = L // 2
        near.append(dict(base, read=read[:m] + BASES[(BASES.index(read[m]) + 1) % 4] + read[m + 1:]))
        if L > 1:
            near.append(dict(base, read=read[:m] + read[m + 1:]))
        near.append(dict(base, read=read[:m] + BASES[(BASES.index(read[m]) + 2) % 4] + read[m:]))
    return exact, near


def pack_accepts(problems, match, bonus):
    maxL = max(len(p["read"]) for p in problems)
    return maxL <= 1024 and maxL * match + 2 * bonus <= 2046


def boundary_reads(lib, n_distinct=2, copies=1, speculation=None, seed=990, max_len=None):
    """every factorization: the exact reads (achieved score asserted = the sum) and their neighbours, through align where the pack takes the
    batch and through align_call always; sums above 2046 must have gone the wide route.  speculation = 1 / 2: the exact batch (copies of
    its problems, one geometry) packed and run with the speculative first fill forced on / off."""
    rng = np.random.default_rng(seed)
    done = 0
    for total, facts in BOUNDARY.items():
        for (L, match, bonus) in facts:
            assert L * match + 2 * bonus == total
            if max_len is not None and L > max_len:
                continue
            scoring = (match, 4, 6, 1, bonus)
            sc = capi.Scoring.simple(*scoring)
            exact, near = boundary_problems(rng, L, n_distinct)
            for p in exact:
                assert refdp.gssw_optimum(p, sc, refdp.MODE_LOCAL) == total, (L, match, bonus)
            for batch in (exact * copies, near):
                cache = {}
                if lib == ORACLE_LIB or pack_accepts(batch, match, bonus):          # (the oracle has no packed range)
                    eng = capi.Engine(sc, lib=lib)
                    if speculation is not None and batch is not near:
                        eng.set_speculation(speculation)
                        with eng.pack(problem_set(batch)) as b:
                            b.run(); b.sync()
                            assert b.speculated() == (speculation == 1), (L, match, bonus, len(batch))
                            res, ops = b.fetch()
                    else:
                        res, ops = eng.align(problem_set(batch))
                    done += check_results(batch, sc, res, ops, cache=cache)
                else:
                    with pytest.raises(capi.VgkError):
                        capi.Engine(sc, lib=lib).pack(problem_set(batch))
                if speculation is None or batch is near:
                    eng = capi.Engine(sc, lib=lib)
                    res, ops = eng.align_call(problem_set(batch))
                    done += check_results(batch, sc, res, ops, cache=cache)
                    if lib != ORACLE_LIB:
                        assert (eng.wide_last(4) > 0) == (not pack_accepts(batch, match, bonus)), (L, match, bonus)
    return done


# ---- banded global ---------------------------------------------------------------------------------------------------------

def banded_problems(seed, n_wide, n_narrow):
    from test_banded import mixed_band_problems
    rng = np.random.default_rng(seed)
    wide = [random_banded_problem(rng, wide=True) for _ in range(n_wide - n_wide // 5)]
    wide += [random_banded_problem(rng, max_nodes=10, max_node_len=30, max_read=200, p_empty=0.1, wide=True) for _ in range(n_wide // 5)]
    narrow = [random_banded_problem(rng) for _ in range(n_narrow // 2)] + mixed_band_problems(seed + 1, n_narrow - n_narrow // 2, 0, 40, max_read=120, max_node_len=20)
    return wide, narrow


def banded_against_definition(lib, n_wide, n_narrow, seed=500):
    """-> (alignments checked, narrow-band problems whose optimum could not be asserted)"""
    from qualadj import qual_adj_tables
    checked = unasserted = 0
    runs = [(s, None) for s in SCORINGS] + [((1, 4, 6, 1, 5), qual_adj_tables(1, 4, 5))]       # every scoring, and a quality-adjusted context
    for k, (scoring, qa) in enumerate(runs):
        sc = capi.Scoring.simple(*scoring)
        wide, narrow = banded_problems(seed + 10 * k, -(-n_wide // len(runs)), -(-n_narrow // len(runs)))
        problems = wide + narrow
        if qa is not None:
            rng = np.random.default_rng(seed + 5)
            for p in problems:
                p["qual"] = rng.choice(np.array([2, 5, 10, 20, 30, 40], dtype=np.uint8), size=len(p["read"]))
        res, ops = capi.Engine(sc, lib=lib, qual_adj=qa).banded_align(capi.BandedSet.from_lists(problems))
        for i, p in enumerate(problems):
            is_wide = i < len(wide)
            ctx = "problem %d: %r -> %r" % (i, p, res[i])
            opt = refdp.banded_global_optimum(p, sc, qa)
            if is_wide:
                assert res["status"][i] == 0 and res["score"][i] == opt, "optimum %d: %s" % (opt, ctx)
            else:
                unasserted += 1
                assert res["status"][i] in (0, VGK_ENOBAND), ctx
                if res["status"][i] != 0:
                    continue
                assert res["score"][i] <= opt, "optimum %d: %s" % (opt, ctx)
            try:
                refdp.check_alignment(p, sc, refdp.MODE_BANDED, res[i], ops_of(res[i], ops), qa)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (e, ctx)) from e
            checked += 1
    return checked, unasserted


def xdrop_band_against_definition(lib, n, seed=700):
    """the pruned X-drop is a heuristic: every alignment valid and re-scored, no score above the un-pruned optimum; -> (checked, equal to the optimum)"""
    rng = np.random.default_rng(seed)
    problems = [random_problem(rng, max_nodes=10, max_node_len=24, max_read=150, mode=XDROP, with_n=0.05) for _ in range(n)]
    from qualadj import qual_adj_tables
    for p in problems:
        p["qual"] = rng.choice(np.array([2, 5, 10, 20, 30, 40], dtype=np.uint8), size=len(p["read"]))
    checked = equal = 0
    for scoring, qa in [(s, None) for s in SCORINGS] + [((1, 4, 6, 1, 5), qual_adj_tables(1, 4, 5))]:
        sc = capi.Scoring.simple(*scoring)
        res, ops, _ = capi.Engine(sc, lib=lib, qual_adj=qa).xdrop_band_align(problem_set(problems))
        for i, p in enumerate(problems):
            ctx = "problem %d: %r -> %r" % (i, p, res[i])
            assert res["status"][i] == 0, ctx
            opt = refdp.xdrop_optimum(p, sc, qa)
            assert 0 <= res["score"][i] <= opt, "optimum %d: %s" % (opt, ctx)
            equal += int(res["score"][i] == opt)
            if res["score"][i] > 0:
                try:
                    refdp.check_alignment(p, sc, refdp.MODE_XDROP, res[i], ops_of(res[i], ops), qa)
                except AssertionError as e:
                    raise AssertionError("%s: %s ops %s" % (e, ctx, capi.cigar_string(res[i], ops))) from e
                checked += 1
    return checked, equal


# ---- WFA --------------------------------------------------------------------------------------------------------------

def thread_walks(threads):
    walks = []
    for t in threads:
        t = [int(x) for x in t]
        walks += [t, [x ^ 1 for x in reversed(t)]]
    return walks


def is_subwalk(path, walks):
    n = len(path)
    return any(w[i:i + n] == path for w in walks for i in range(len(w) - n + 1))


# The default error model and one with a low cap (two mismatches, two gaps, four gap bases).  Both keep the default DISTANCE event: the distance band
# drops wavefront points that fall behind, a pruning rule and not part of the definition — with a tight one (test_wfa.MODELS[1]: at most 4) an ok = 1
# connect need not be the cheapest, so the optimum is only asserted where the band is wide against these sequences (at most ~60 bases).
WFA_MODELS = [None, ((0.0, 2, 2), (0.0, 2, 2), (0.0, 4, 4), (0.1, 10, 200))]


def wfa_against_definition(lib, seeds, n_problems=60, form=None):
    """Every random result with ok = 1: the reference's validity checker (test_wfa.check_alignment, which re-scores the edits), and the path a
    sub-walk of ONE thread.  Connects, with best = refdp.wfa_connect_optimum (the cheapest gap-affine global alignment of the sequence to the
    bases between `from` and any later `to` on one thread, either orientation; None: no thread holds the pair) and cap = refdp.wfa_penalty_cap:
      ok = 1  =>  best <= cap and the alignment's penalty, match * (graph bases + sequence bases) - 2 score, is best;
      best is None or best > cap  =>  ok = 0.
    Not asserted, and counted: ok = 0 although best <= cap (the distance band may exclude the path; a rule, not part of the definition) and
    VGK_ETOOBIG (a kernel table limit).  -> (valid alignments, connects, connects not asserted, connects beyond the cap that came back ok = 0)"""
    import test_wfa
    S = test_wfa.SCORES
    eng = capi.Engine(lib=lib)
    if form is not None:
        eng.lib.vgk_wfa_set_form.argtypes = [ctypes.c_void_p, ctypes.c_int]
        assert eng.lib.vgk_wfa_set_form(eng.h, form) == 0
    valid = connects = unasserted = beyond = 0
    for s in seeds:
        nodes, threads, problems = test_wfa.random_wfa_case(np.random.default_rng(s), n_problems)
        index_of = {k: k for k in range(len(nodes))}
        walks = thread_walks(threads)
        model = WFA_MODELS[s % 2]
        out = eng.wfa_extend(eng.haplo_index(nodes, threads), problems, model)
        for i, p in enumerate(problems):
            r, path, ed = test_wfa.unpack(*out, i)
            connect = p["mode"] == "connect"
            connects += int(connect)
            try:
                assert r["status"] in (0, VGK_ETOOBIG), "status"
                best = cap = None
                if connect and r["status"] == 0:
                    if max(p["from"][0], p["to"][0]) < 2 * len(nodes):
                        best = refdp.wfa_connect_optimum(nodes, threads, p["seq"], p["from"], p["to"], S["match"], S["mismatch"], S["gap_open"], S["gap_extend"])
                    cap = refdp.wfa_penalty_cap(len(p["seq"]), S["match"], S["mismatch"], S["gap_open"], S["gap_extend"], model)
                    if best is None or best > cap:
                        assert not r["ok"], "ok = 1 with the optimum %s beyond the cap %d" % (best, cap)
                        beyond += int(best is not None)
                if r["status"] != 0 or not r["ok"]:
                    unasserted += int(connect and (r["status"] != 0 or (best is not None and best <= cap)))
                    continue
                pos = lambda q: None if q is None else (q[0] >> 1, q[0] & 1, q[1])
                case = {"sequence": p["seq"], "call": p["mode"], "from": pos(p.get("from")), "to": pos(p.get("to"))}
                test_wfa.check_alignment(case, r, path, ed, nodes, threads, index_of)
                if len(path) == 1 and not is_subwalk(path, walks):          # inside the caller's own node, which no thread need visit
                    assert path[0] in (p.get("from", (None,))[0], p.get("to", (None,))[0]), "a node of no thread"
                else:
                    assert is_subwalk(path, walks), "the path follows no single thread"
                if connect:
                    graph_len = sum(n for t, n in ed if t != capi.WFA_INSERTION)
                    assert S["match"] * (graph_len + len(p["seq"])) - 2 * int(r["score"]) == best <= cap, "smallest penalty %d, cap %d" % (best, cap)
            except AssertionError as e:
                raise AssertionError("%s: seed %d problem %d %r -> %r path %s edits %s" % (e, s, i, p, r, path, ed)) from e
            valid += 1
    return valid, connects, unasserted, beyond


# ---- the k-best entry points: vgk_banded_align_multi and vgk_gssw_align_multi ----------------------------------------------------
#
# Oracle, emulator, kernels and both host walkers restate ONE procedure (a stack of deflections); comparing them with each other passes a rule all
# of them misread.  Here the alternates are held to refdp's k-best dynamic programs, which know nothing of tracebacks: rules (f) and (g).  The
# families and their reference lists are made once (lru_cache) and shared by the oracle, emulator and HIP drivers.

@contextlib.contextmanager
def forced_host_walk(on):
    """VGAMD_MULTI_HOST_WALK=1: every problem's alternates are enumerated by the host walker instead of the kernel"""
    before = os.environ.get("VGAMD_MULTI_HOST_WALK")
    if on:
        os.environ["VGAMD_MULTI_HOST_WALK"] = "1"
    else:
        os.environ.pop("VGAMD_MULTI_HOST_WALK", None)
    try:
        yield
    finally:
        if before is None:
            os.environ.pop("VGAMD_MULTI_HOST_WALK", None)
        else:
            os.environ["VGAMD_MULTI_HOST_WALK"] = before


def alignment_key(o):
    return tuple((int(x["node"]), int(x["len"]), int(x["op"])) for x in o)


def walk_key(o):
    return tuple(dict.fromkeys(int(x["node"]) for x in o))


class Richness:
    """what keeps a k-best comparison from going quiet, counted per family on one library's output"""

    def __init__(self):
        self.n = self.many = self.ties = self.other_walk = self.short = 0

    def add(self, scores, walks, k):
        self.n += 1
        self.many += len(scores) >= 2
        self.ties += len(set(scores)) < len(scores)
        self.other_walk += len(set(walks)) > 1
        self.short += len(scores) < k

    def check(self, name):
        ctx = (name, vars(self))
        assert self.many >= 0.5 * self.n, ctx                          # at least half the problems return two alternates or more
        assert self.ties > 0 and self.other_walk > 0, ctx              # ties between ranks; an alternate on another walk than the first
        assert self.short > 0, ctx                                     # somewhere the count falls below k


_rescored = set()


def rescore_once(family, i, problem, sc, mode, row, o, qa, **kw):
    """refdp.check_alignment, once per distinct result of a family's problem: the kernel route and the forced host walk return the same op lists"""
    key = (family, mode, i, int(row["score"]), int(row["first_offset"]), int(row["end_node"]), int(row["end_offset"]), int(row["end_read"]), alignment_key(o), tuple(sorted(kw.items())))
    if key not in _rescored:
        refdp.check_alignment(problem, sc, mode, row, o, qa, **kw)
        _rescored.add(key)


LADDER_SCORING = (1, 20, 40, 1, 0)
TWO_ALIGNMENTS = dict(read="C", nodes=["C"], preds=[[]], band_padding=4, permissive=True)         # 1M and 1D1I (1I1D: exclusion 1): fewer than any k here


def ladder_problem(stem, rung, sink, depth):
    """Alternates that need one deflection more each.  Sources g_0 .. g_depth all spell `stem`; rungs w_1 .. w_depth of one base each, w_i behind
    [g_(i-1), w_(i-1)]; the sink behind [g_depth, w_depth]; the read is stem + sink.  The best alignment walks g_depth -> sink; the next best deletes
    w_depth coming from g_(depth-1), the next w_(depth-1) w_depth from g_(depth-2), ...: one gap_extend worse each, and each leaves the one before at a
    node boundary further left, which a traceback can only name as a further deflection.  Under LADDER_SCORING a second gap costs more than 30 bases of
    the first, so these are the best alternates and the 25th has more deflections than a device slot holds (BM_MAX_DEFL = 24)."""
    nodes, preds = [stem] * (depth + 1), [[] for _ in range(depth + 1)]
    for i in range(1, depth + 1):
        nodes.append(rung[(i - 1) % len(rung)]); preds.append([i - 1] + ([len(nodes) - 2] if i > 1 else []))
    nodes.append(sink); preds.append([depth, len(nodes) - 2])
    read = stem + sink
    return dict(read=read, nodes=nodes, preds=preds, band_padding=len(read) + sum(len(x) for x in nodes) + 2, permissive=True)


# name -> (k, scoring, kind).  kind "exact": no empty nodes, a band that excludes nothing: the score list IS (f).  "empty": the same with empty
# nodes: (f) for all but a counted share, the superset bound for all.  "narrow": random_banded_set's own bands: the superset bound only.
BANDED_KBEST = {"tiny": (6, (1, 4, 6, 1, 0), "exact"), "tiny-empty": (6, (1, 4, 6, 1, 0), "empty"),
                "default": (12, (1, 4, 6, 1, 0), "exact"), "default-empty": (12, (1, 4, 6, 1, 0), "empty"),
                "slot-pool": (63, (1, 4, 6, 1, 0), "exact"),           # the device's slot pool: free_slots is one 64-bit mask over max_alt + 1 slots
                "beyond-the-slot-pool": (80, (2, 3, 5, 2, 0), "exact"),
                "deflections": (63, LADDER_SCORING, "exact"),
                "narrow": (6, (1, 4, 6, 1, 0), "narrow"),
                "quality": (12, (1, 4, 6, 1, 5), "empty")}
# problems with a copy among their alternates ((f) DUPLICATES), as the oracle gives them; kernel, host walker and emulator must give the same.  The families
# without empty nodes have none.
BANDED_COPIES = {"tiny-empty": 3, "default-empty": 2, "narrow": 3, "quality": 2}
UNSTATED_SHARE = 0.02       # of an empty-node family: what (f) states no rule for (refdp.py (f), "what stays outside the definition")


@functools.lru_cache(maxsize=None)
def banded_kbest_family(name):
    """-> (problems, qual_adj tables or None)"""
    from test_banded import random_banded_set
    tiny = dict(max_nodes=5, max_node_len=4, max_read=9, wide=True)
    qa = None
    if name == "tiny":
        ps = random_banded_set(1, 300, p_empty=0, **tiny)
    elif name == "tiny-empty":
        ps = random_banded_set(2, 300, p_empty=0.2, **tiny)
    elif name == "default":
        ps = random_banded_set(4, 60, p_empty=0, wide=True)
    elif name == "default-empty":
        ps = random_banded_set(3, 200, p_empty=0.15, wide=True)
        ps = ps[:60] + [ps[163]]                  # 163: two chains of empty nodes in front of node 2 ((f) exclusion 2); six alternates before the rule was stated, twelve in the definition
    elif name == "slot-pool":
        ps = random_banded_set(5, 11, p_empty=0, wide=True) + [TWO_ALIGNMENTS]
    elif name == "beyond-the-slot-pool":
        ps = random_banded_set(6, 11, p_empty=0, wide=True) + [TWO_ALIGNMENTS]
    elif name == "deflections":
        ps = [ladder_problem(stem, rung, sink, depth) for stem, rung, sink, depth in
              [("CG", "A", "T", 30), ("CGT", "A", "TG", 28), ("C", "A", "G", 32), ("CGCG", "A", "T", 30), ("CG", "AT", "G", 27), ("GC", "T", "A", 26),
               ("C", "TA", "GC", 29), ("TGC", "A", "C", 31), ("G", "A", "CT", 33), ("CGG", "AAT", "T", 28)]] + [TWO_ALIGNMENTS]
    elif name == "narrow":
        ps = random_banded_set(7, 150)                                 # random_banded_set's defaults: paddings 0 .. 5, three in ten not permissive
    elif name == "quality":
        from qualadj import qual_adj_tables
        ps = random_banded_set(8, 60, p_empty=0.15, wide=True)
        rng = np.random.default_rng(9)
        for p in ps:
            p["qual"] = rng.choice(np.array([2, 5, 10, 20, 30, 40], dtype=np.uint8), size=len(p["read"]))
        qa = qual_adj_tables(1, 4, 5)
    return ps, qa


@functools.lru_cache(maxsize=None)
def banded_kbest_reference(name):
    """-> per problem ((f), (f) without its exclusions); the first only where the kind asserts it, the second only where it is not implied"""
    k, scoring, kind = BANDED_KBEST[name]
    ps, qa = banded_kbest_family(name)
    sc = capi.Scoring.simple(*scoring)
    return [(refdp.banded_kbest_scores(p, sc, k, qa) if kind != "narrow" else None,
             refdp.banded_kbest_scores(p, sc, k, qa, exclude_whole_read_lead_insertion=False) if kind != "exact" else None) for p in ps]


def banded_kbest_against_definition(lib, name, host_walk=False):
    """Every alternate: a valid global alignment whose re-score is the reported score (refdp.check_alignment); per problem: descending scores, no
    (walk, ops) twice (but see refdp (f) DUPLICATES), the list against (f) as the family's kind says.  -> (Richness, problems whose list is not (f),
    problems with a copy among their alternates, problems a host thread walked)"""
    k, scoring, kind = BANDED_KBEST[name]
    ps, qa = banded_kbest_family(name)
    ref = banded_kbest_reference(name)
    sc = capi.Scoring.simple(*scoring)
    eng = capi.Engine(sc, lib=lib, qual_adj=qa)
    with forced_host_walk(host_walk):
        res, cnt, ops = eng.banded_align_multi(capi.BandedSet.from_lists(ps), k)
    rich, unstated, copies = Richness(), 0, 0
    for i, p in enumerate(ps):
        ctx = "%s problem %d: %r" % (name, i, p)
        exact, superset = ref[i]
        if cnt[i] == 0:
            assert kind == "narrow" and res[i, 0]["status"] == VGK_ENOBAND, ctx
            continue
        rows = [res[i, a] for a in range(int(cnt[i]))]
        got = [int(r["score"]) for r in rows]
        keys = []
        for a, r in enumerate(rows):
            assert r["status"] == 0, ctx
            try:
                rescore_once(name, i, p, sc, refdp.MODE_BANDED, r, ops_of(r, ops), qa)
            except AssertionError as e:
                raise AssertionError("%s: alternate %d of %s" % (e, a, ctx)) from e
            keys.append(alignment_key(ops_of(r, ops)))
        ctx += " -> %s" % got
        assert got == sorted(got, reverse=True), ctx
        if len(set(keys)) != len(keys):                                  # refdp (f) DUPLICATES: only where two chains of empty nodes join two nodes of the walk, and no more copies than such walks
            assert refdp.ambiguous_empty_chains(p), "an alignment twice: %s %s" % (ctx, keys)
            for key in set(keys):
                assert keys.count(key) <= refdp.empty_chain_walks(p, walk_key(ops_of(rows[keys.index(key)], ops))), "more copies than walks: %s %s" % (ctx, key)
            copies += 1
        if superset is not None:
            assert len(got) <= len(superset) and all(g <= s for g, s in zip(got, superset)), "superset %s: %s" % (superset, ctx)
        if kind == "exact":
            assert got == exact, "definition %s: %s" % (exact, ctx)
        elif kind == "empty" and got != exact:
            unstated += 1
        rich.add(got, [walk_key(ops_of(r, ops)) for r in rows], k)
    if kind == "empty":
        assert unstated <= UNSTATED_SHARE * len(ps), (name, unstated, len(ps))
    assert copies == BANDED_COPIES.get(name, 0), (name, copies)
    return rich, unstated, copies, eng.multi_host_walks


def banded_kbest_on_an_engine(lib, name):
    """as enumerated by the kernel (a host thread for what it declines), and with every problem forced to the host walker"""
    for host_walk in (False, True):
        rich, unstated, copies, walked = banded_kbest_against_definition(lib, name, host_walk)
        n = len(banded_kbest_family(name)[0])
        if host_walk or name == "beyond-the-slot-pool":
            assert walked >= rich.n - 1, (name, host_walk, walked, rich.n)               # (all that reached the device)
        elif name == "deflections":
            assert walked == n - 1, (name, walked)                         # every ladder was more than a slot holds; the two-alignment problem was not
        elif BANDED_KBEST[name][2] == "exact":
            assert walked == 0, (name, walked)                              # nothing here for the kernel to decline
        assert rich.n > 0.6 * n, (name, rich.n)


# ---- pinned

def low_complexity_pinned_problem(rng):
    """a diamond of mostly-C nodes and a read off one of its walks: gaps slide along the runs, so the alternates outnumber any slot pool"""
    def low(n):
        return "".join(BASES[int(rng.integers(0, 4))] if rng.random() < 0.1 else "C" for _ in range(n))
    a, b, c, d = (low(int(rng.integers(6, 13))) for _ in range(4))
    read = list((a + (b if rng.random() < 0.5 else c) + d)[int(rng.integers(0, len(a))):])
    for _ in range(int(rng.integers(0, 3))):
        i = int(rng.integers(0, len(read) - 1))
        read[i:i + 1] = [] if rng.random() < 0.5 else [read[i], "C"]
    return dict(read="".join(read), nodes=[a, b, c, d], preds=[[], [0], [0], [1, 2]], flags=PINNED | TB, pinning=[0, 0, 0, 1])


def repetitive_pinned_problem(rng, max_nodes, max_node_len, max_read):
    """random_problem's graph shapes over mostly-C nodes, the read the last bases of a walk into a sink (one edit now and then): in a run a gap slides and
    two branches of a bubble spell the same, so a second alignment worth more than 0 is the rule.  The random reads of random_problem end anywhere, and a
    detour costs at least 5 under the scorings with match 1: most of them have one alignment worth more than 0, or none."""
    n_nodes = int(rng.integers(1, max_nodes + 1))
    _, preds = random_dag(rng, n_nodes, max_node_len)
    nodes = ["".join(BASES[int(rng.integers(0, 4))] if rng.random() < 0.08 else "C" for _ in range(int(rng.integers(1, max_node_len + 1)))) for _ in range(n_nodes)]
    pinning = sinks_of(preds)
    v = [u for u in range(n_nodes) if pinning[u]][int(rng.integers(0, sum(pinning)))]
    walk = nodes[v]
    while preds[v]:
        v = preds[v][int(rng.integers(0, len(preds[v])))]
        walk = nodes[v] + walk
    read = list(walk[-int(rng.integers(max(1, max_read // 2), max_read + 1)):])
    if len(read) > 3 and rng.random() < 0.3:
        i = int(rng.integers(1, len(read) - 1))
        read[i:i + 1] = [] if rng.random() < 0.5 else [read[i], "C"]
    return dict(read="".join(read[-max_read:]), nodes=nodes, preds=preds, flags=PINNED | TB, pinning=pinning)


ONE_ALIGNMENT = dict(read="ACGT", nodes=["ACGT"], preds=[[]], flags=PINNED | TB, pinning=[1])        # nothing else is worth more than 0: fewer than any k here

# name -> (k, scoring).  Every random family is the issue's random_problem(mode=PINNED) problems followed by as many repetitive_pinned_problem ones of the
# same sizes: by themselves the random ones return two alternates in a fifth to a third of the problems under the scorings with match 1 (59 of 300, 20 of
# 60, 7 of 30 on the oracle), and the comparison with the bound would mostly be of one score with one score.
PINNED_KBEST = {"tiny": (6, (1, 4, 6, 1, 5)), "default": (12, (1, 4, 6, 1, 5)),
                "slot-pool": (62, (1, 4, 6, 1, 0)),                    # the device holds max_alt + 2 <= 64 slots
                "beyond-the-slot-pool": (80, (1, 4, 6, 1, 0)),         # ... so these are walked by host threads
                "seventeen-predecessors": (20, (1, 4, 6, 1, 5)),       # more than a lane's source table (MT_MAX_PRED = 15): that problem goes to a host thread
                "quality": (12, (1, 4, 6, 1, 5))}
PINNED_KBEST.update(("scoring-%d" % n, (12, s)) for n, s in enumerate(SCORINGS[1:] + [WIDE_SCORING]))


@functools.lru_cache(maxsize=None)
def pinned_kbest_family(name):
    qa = None

    def pinned(seed, n, **kw):
        rng = np.random.default_rng(seed)
        ps = [random_problem(rng, mode=PINNED, **kw) for _ in range(n)]
        return ps + [repetitive_pinned_problem(rng, **kw) for _ in range(n)]
    if name == "tiny":
        ps = pinned(1, 300, max_nodes=5, max_node_len=5, max_read=10)
    elif name == "default":
        ps = pinned(2, 60, max_nodes=8, max_node_len=10, max_read=40)
    elif name in ("slot-pool", "beyond-the-slot-pool"):
        rng = np.random.default_rng(len(name))
        ps = [low_complexity_pinned_problem(rng) for _ in range(12)] + [ONE_ALIGNMENT]
    elif name == "seventeen-predecessors":
        wide = {"read": "ACGTACGTTG", "nodes": ["ACGTA", "ACGTT", "ACGAA", "ACTTA", "AGGTA", "CCGTA", "ACGTC", "ACGGA", "TCGTA", "ACGTG", "AAGTA",
                                                "ACCTA", "ACGCA", "GCGTA", "ACGTA", "ATGTA", "ACGAT", "CGTTG"],
                "preds": [[] for _ in range(17)] + [list(range(17))], "flags": PINNED | TB, "pinning": [0] * 17 + [1]}     # test_pinned_multi.declined_by_the_kernel_case
        ps = [wide, dict(wide, read="ACGTTCGTTG"), dict(wide, read="GTACGTTG")]
    elif name == "quality":
        from qualadj import qual_adj_tables
        ps = pinned(3, 30, max_nodes=8, max_node_len=10, max_read=40)
        rng = np.random.default_rng(4)
        for p in ps:
            p["qual"] = rng.choice(np.array([2, 5, 10, 20, 30, 40], dtype=np.uint8), size=len(p["read"]))
        qa = qual_adj_tables(1, 4, 5)
    else:
        ps = pinned(10 + int(name.split("-")[1]), 30, max_nodes=8, max_node_len=10, max_read=40)
    return ps, qa


@functools.lru_cache(maxsize=None)
def pinned_kbest_reference(name):
    """-> per problem (the PINNED optimum of (a), the bound (g))"""
    k, scoring = PINNED_KBEST[name]
    ps, qa = pinned_kbest_family(name)
    sc = capi.Scoring.simple(*scoring)
    return [(refdp.gssw_optimum(p, sc, refdp.MODE_PINNED, qa), refdp.pinned_kbest_bound(p, sc, k, qa)) for p in ps]


def pinned_kbest_against_definition(lib, name, host_walk=False):
    """Every alternate: a valid pinned alignment whose re-score is the reported score; per problem: the first is the definition's optimum, none exactly
    when that is <= 0; every score > 0; descending; no (first_offset, ops) twice; at every rank at most the bound (g).  -> (Richness, host walks)"""
    k, scoring = PINNED_KBEST[name]
    ps, qa = pinned_kbest_family(name)
    ref = pinned_kbest_reference(name)
    sc = capi.Scoring.simple(*scoring)
    eng = capi.Engine(sc, lib=lib, qual_adj=qa)
    with forced_host_walk(host_walk):
        res, cnt, ops = eng.align_multi(problem_set(ps), k)
    rich = Richness()
    for i, p in enumerate(ps):
        opt, bound = ref[i]
        rows = [res[i, a] for a in range(int(cnt[i]))]
        got = [int(r["score"]) for r in rows]
        ctx = "%s problem %d: %r -> %s" % (name, i, p, got)
        assert (not got) == (opt <= 0), "optimum %d: %s" % (opt, ctx)
        keys = []
        for a, r in enumerate(rows):
            assert r["status"] == 0, ctx
            try:
                rescore_once(name, i, p, sc, refdp.MODE_PINNED, r, ops_of(r, ops), qa, expect_optimum=opt if a == 0 else None)
            except AssertionError as e:
                raise AssertionError("%s: alternate %d (%s) of %s" % (e, a, capi.cigar_string(r, ops), ctx)) from e
            keys.append((int(r["first_offset"]), alignment_key(ops_of(r, ops))))
        assert all(g > 0 for g in got) and got == sorted(got, reverse=True), ctx
        assert len(set(keys)) == len(keys), "an alignment twice: %s" % ctx
        assert len(got) <= len(bound) and all(g <= b for g, b in zip(got, bound)), "bound %s: %s" % (bound, ctx)
        rich.add(got, [walk_key(ops_of(r, ops)) for r in rows], k)
    return rich, eng.multi_host_walks


def pinned_kbest_on_an_engine(lib, name):
    n = len(pinned_kbest_family(name)[0])
    rich, walked = pinned_kbest_against_definition(lib, name)
    assert rich.n == n
    assert walked == {"beyond-the-slot-pool": n, "seventeen-predecessors": n}.get(name, 0), (name, walked)               # k = 80: every problem is a host thread's
    rich, walked = pinned_kbest_against_definition(lib, name, host_walk=True)
    assert rich.n == n and walked > 0, (name, walked)


# ---- CPU half: oracle and emulator ----------------------------------------------------------------------------------------

def test_oracle_gssw_modes_reach_the_definitions_optimum():
    assert random_gssw(ORACLE_LIB, 2100, routes=("align",)) > 4000
    assert quality_adjusted(ORACLE_LIB, 300) > 600
    assert gssw_against_definition(ORACLE_LIB, long_and_bubble_problems(21, 60), (1, 4, 6, 1, 5), ("align",)) > 50


def test_emulated_gssw_modes_reach_the_definitions_optimum(emu_lib):
    assert random_gssw(emu_lib, 2100) > 8000
    assert quality_adjusted(emu_lib, 300) > 1200
    assert gssw_against_definition(emu_lib, long_and_bubble_problems(22, 30), (1, 4, 6, 1, 5)) >= 40
    assert gssw_against_definition(emu_lib, not_pinned(random_family(33, 200)), (1, 4, 6, 1, 5), ("windows",)) > 300       # LOCAL and X-drop as windows


def test_oracle_read_lengths_and_edge_graphs():
    assert read_length_sweep(ORACLE_LIB) >= 45
    assert gssw_against_definition(ORACLE_LIB, edge_graphs(), (1, 4, 6, 1, 5), ("align",)) > 300
    assert gssw_against_definition(ORACLE_LIB, edge_graphs(12), (2, 3, 5, 2, 7), ("align",)) > 300


def test_emulated_read_lengths_and_edge_graphs(emu_lib):
    assert read_length_sweep(emu_lib) >= 45
    assert gssw_against_definition(emu_lib, edge_graphs(), (1, 4, 6, 1, 5)) > 600
    assert gssw_against_definition(emu_lib, edge_graphs(12), (2, 3, 5, 2, 7)) > 600


def test_xdrop_optima_that_rest_on_the_unpinned_rounding_are_few_and_counted():
    """The leading insertion's limit is max_gap_length rounded up to dozeu's 8-row vectors — no reference vector decides it ([PARITY-UNPINNED] in
    refdp.py and oracle/vgo_xdrop.c).  How many X-drop optima of this file's problems would differ without the rounding: some of the edge graphs built
    around the limit (so the rule is exercised), none of the random families (max_gap 0..59 against reads that rarely start with an insertion)."""
    sc = capi.Scoring.simple(1, 4, 6, 1, 5)
    depends = lambda ps: sum(refdp.xdrop_optimum(p, sc) != refdp.xdrop_optimum(p, sc, round8=False) for p in ps if p["flags"] & 15 == XDROP)
    edge, rand = depends(edge_graphs()), depends(random_family(100, 234))
    print("X-drop optima that depend on the 8-rounding: %d of the edge graphs, %d of 234 random problems" % (edge, rand))
    assert edge > 0 and rand <= 2


def test_oracle_boundary_reads():
    assert boundary_reads(ORACLE_LIB) > 100


def test_emulated_boundary_reads(emu_lib):
    assert boundary_reads(emu_lib) > 100


@pytest.mark.parametrize("speculation", [1, 2])
def test_emulated_boundary_reads_with_and_without_the_speculative_fill(emu_lib, speculation):
    """key3 exists only in the speculative first fill, which needs a batch of 1 024: the factorizations with reads of at most 200 bases (what the
    emulator steps through in seconds), 990 among them with key3 on and 991 with it off; the longer ones run on the device only."""
    assert boundary_reads(emu_lib, n_distinct=2, copies=512, speculation=speculation, max_len=200) > 4000


def test_oracle_banded_reaches_the_global_optimum():
    checked, unasserted = banded_against_definition(ORACLE_LIB, 600, 1500)
    assert checked > 1800 and unasserted <= 1500


def test_emulated_banded_reaches_the_global_optimum(emu_lib):
    checked, unasserted = banded_against_definition(emu_lib, 200, 300, seed=600)
    assert checked > 400 and unasserted <= 300


def test_oracle_pruned_xdrop_stays_below_the_optimum():
    checked, equal = xdrop_band_against_definition(ORACLE_LIB, 600)
    assert checked > 600 and equal > checked // 2


def test_oracle_wfa_results_are_valid_and_connects_optimal():
    valid, connects, unasserted, beyond = wfa_against_definition(ORACLE_LIB, range(300, 400))
    assert valid > 2500 and connects >= 1000 and unasserted <= 0.1 * connects and beyond > 0, (valid, connects, unasserted, beyond)


def test_emulated_wfa_results_are_valid_and_connects_optimal(emu_lib):
    for form in (0, 1, 2):                                     # hybrid, one thread per problem, one wavefront per problem
        valid, connects, unasserted, beyond = wfa_against_definition(emu_lib, range(420, 440), form=form)
        assert valid > 500 and connects >= 200 and unasserted <= 0.1 * connects, (form, valid, connects, unasserted, beyond)


def test_the_kbest_references_agree_with_the_optimum_at_k_1():
    """(f) and (g) at k = 1 against (c) and (a) on every family's problems, and the first of every (g) list: the k-best programs share no line with
    the optimum programs, so this holds the new references to the old ones"""
    for name, (k, scoring, kind) in BANDED_KBEST.items():
        ps, qa = banded_kbest_family(name)
        sc = capi.Scoring.simple(*scoring)
        for p, (exact, superset) in zip(ps, banded_kbest_reference(name)):
            opt = refdp.banded_global_optimum(p, sc, qa)
            assert refdp.banded_kbest_scores(p, sc, 1, qa) == [opt] == refdp.banded_kbest_scores(p, sc, 1, qa, exclude_whole_read_lead_insertion=False), (name, p)
            for full in (exact, superset):
                assert full is None or (full[0] == opt and full == sorted(full, reverse=True)), (name, p, full)
            if exact is not None and superset is not None:
                assert len(exact) <= len(superset) and all(a <= b for a, b in zip(exact, superset)), (name, p, exact, superset)
    for name, (k, scoring) in PINNED_KBEST.items():
        ps, qa = pinned_kbest_family(name)
        sc = capi.Scoring.simple(*scoring)
        for p, (opt, bound) in zip(ps, pinned_kbest_reference(name)):
            assert refdp.pinned_kbest_bound(p, sc, 1, qa) == ([opt] if opt > 0 else []), (name, p)
            assert (bound[0] if bound else 0) == opt and bound == sorted(bound, reverse=True) and all(b > 0 for b in bound), (name, p, bound)


@pytest.mark.parametrize("name", list(BANDED_KBEST))
def test_oracle_banded_alternates_are_the_definitions_k_best(name):
    """Measured on the oracle: tiny-empty 1 of 300 lists is not (f) (problem 91, 0.3 %), default-empty 0 of 60, quality 1 of 60 (problem 3, 1.7 %); both
    are refdp (f)'s "what stays outside the definition".  Before (f)'s exclusions 2 and 3 were stated: 4 of the 300, and 1 of 200 seed-3 problems."""
    rich, unstated, copies, _ = banded_kbest_against_definition(ORACLE_LIB, name)
    print("%s: %d problems, %d not (f), %d with a copy among the alternates, %r" % (name, rich.n, unstated, copies, vars(rich)))
    # (a family built so that every problem has more alignments than k falls short of k in its two-alignment problem)
    rich.check(name)


@pytest.mark.parametrize("name", list(BANDED_KBEST))
def test_emulated_banded_alternates_are_the_definitions_k_best(emu_lib, name):
    banded_kbest_on_an_engine(emu_lib, name)


@pytest.mark.parametrize("name", list(PINNED_KBEST))
def test_oracle_pinned_alternates_stay_under_the_definitions_bound(name):
    rich, _ = pinned_kbest_against_definition(ORACLE_LIB, name)
    print("%s: %r" % (name, vars(rich)))
    rich.check(name)


@pytest.mark.parametrize("name", list(PINNED_KBEST))
def test_emulated_pinned_alternates_stay_under_the_definitions_bound(emu_lib, name):
    pinned_kbest_on_an_engine(emu_lib, name)


# ---- GPU half: the HIP engine against the definition directly ------------------------------------------------------------------

@pytest.mark.gpu
def test_hip_gssw_modes_reach_the_definitions_optimum():
    assert random_gssw(ENGINE_LIB, 2100, seed=1100) > 8000
    assert quality_adjusted(ENGINE_LIB, 300, seed=1300) > 1200
    assert gssw_against_definition(ENGINE_LIB, long_and_bubble_problems(1021, 60), (1, 4, 6, 1, 5)) > 100
    assert gssw_against_definition(ENGINE_LIB, not_pinned(random_family(1033, 700)), (1, 4, 6, 1, 5), ("windows",)) > 1000


@pytest.mark.gpu
def test_hip_read_lengths_and_edge_graphs():
    assert read_length_sweep(ENGINE_LIB) >= 45
    assert gssw_against_definition(ENGINE_LIB, edge_graphs(), (1, 4, 6, 1, 5)) > 600
    assert gssw_against_definition(ENGINE_LIB, edge_graphs(12), (2, 3, 5, 2, 7)) > 600


@pytest.mark.gpu
def test_hip_boundary_reads():
    assert boundary_reads(ENGINE_LIB) > 100


@pytest.mark.gpu
@pytest.mark.parametrize("speculation", [1, 2])
def test_hip_boundary_reads_with_and_without_the_speculative_fill(speculation):
    """batches of 1 024 (the smallest that speculate) of one geometry: with key3 on (990) / off (991 and above) and the speculative first fill
    on / off these are the four builds of the fill kernel"""
    assert boundary_reads(ENGINE_LIB, n_distinct=2, copies=512, speculation=speculation) > 10000


@pytest.mark.gpu
def test_hip_banded_reaches_the_global_optimum():
    checked, unasserted = banded_against_definition(ENGINE_LIB, 600, 1500, seed=1500)
    assert checked > 1800 and unasserted <= 1500


@pytest.mark.gpu
def test_hip_pruned_xdrop_stays_below_the_optimum():
    checked, equal = xdrop_band_against_definition(ENGINE_LIB, 600, seed=1700)
    assert checked > 600 and equal > checked // 2


@pytest.mark.gpu
def test_hip_wfa_results_are_valid_and_connects_optimal():
    for form in (0, 1, 2):
        valid, connects, unasserted, beyond = wfa_against_definition(ENGINE_LIB, range(1420, 1460), form=form)
        assert valid > 1000 and connects >= 400 and unasserted <= 0.1 * connects, (form, valid, connects, unasserted, beyond)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BANDED_KBEST))
def test_hip_banded_alternates_are_the_definitions_k_best(name):
    banded_kbest_on_an_engine(ENGINE_LIB, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PINNED_KBEST))
def test_hip_pinned_alternates_stay_under_the_definitions_bound(name):
    pinned_kbest_on_an_engine(ENGINE_LIB, name)
