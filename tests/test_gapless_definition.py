"""Gapless extension held to its rule and to its kernels' table limits.

The rule is tests/refgapless.py: the haplotypes as oriented sequences, everything counted over copies — no GBWT records, no ranges as data.
The oracle (oracle/vgo_gapless.c), the emulated kernels and the HIP kernels (as they come, with VGAMD_GAPLESS_SLAB_ONLY, and with merged runs)
are held to it on two corpora made once and never changed: single-seed problems without trimming (the winner of a search is a top finished
entry of the reference's exhaustive search) and multi-seed problems (every returned extension is valid, every set keeps the set rules).  The
edge corpus puts one or a few reads on each of the limits gapless_device.hpp states — at the limit the result equals the oracle's and meets
the reference, one past it that read alone is declined — and the same calls run through a program of their own under the host sanitizers
(make gapless_san) before any of them goes to a GPU."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import refgapless as ref
import util
from vg_amd import capi

ETOOBIG = -7
BASES = "ACGT"
DEFAULT_SCORING = (1, 4, 5)


def comp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def rand_seq(rng, n):
    return "".join(BASES[i] for i in rng.integers(0, 4, int(n)))


def oriented_seq(nodes, t):
    return "".join(nodes[o // 2] if not o & 1 else comp(nodes[o // 2]) for o in t)


# ---- generators -----------------------------------------------------------------------------------------------------------------------
def sample_reads(rng, nodes, threads, n_reads, max_len=60, sub_rate=0.06, extra_seeds=None, max_mm=None):
    """reads from a thread (either strand) with substitutions; seeds at true positions plus a false one on a VISITED node now and then"""
    seen = sorted({o for t in threads for o in t} | {o ^ 1 for t in threads for o in t})
    problems = []
    for _ in range(n_reads):
        t = threads[int(rng.integers(0, len(threads)))]
        if rng.random() < 0.5:
            t = [o ^ 1 for o in reversed(t)]
        seq = oriented_seq(nodes, t)
        starts = np.cumsum([0] + [len(nodes[o // 2]) for o in t])
        L = int(rng.integers(5, min(max_len, len(seq)) + 1)); a = int(rng.integers(0, len(seq) - L + 1))
        read = list(seq[a:a + L])
        for k in range(L):
            r = rng.random()
            if r < sub_rate:
                read[k] = BASES[int(rng.integers(0, 4))]
            elif r < sub_rate + 0.01:
                read[k] = "N"
        seeds = []
        for _ in range(int(rng.integers(1, 6))):
            ro = int(rng.integers(0, L)); g = a + ro
            k = int(np.searchsorted(starts, g, side="right") - 1)
            seeds.append((t[k], ro - (g - int(starts[k]))))
            if extra_seeds:
                seeds += extra_seeds(rng, t[k], seeds[-1][1])
        if rng.random() < 0.3:                          # a false seed
            o = seen[int(rng.integers(0, len(seen)))]
            seeds.append((o, int(rng.integers(0, L)) - int(rng.integers(0, len(nodes[o // 2])))))
        if rng.random() < 0.15:                         # ... and one that puts the read's last base alone on a node: mostly a mismatch, trimmed away
            seeds.append((seen[int(rng.integers(0, len(seen)))], L - 1))
        seeds = list(dict.fromkeys(seeds))              # a cluster is a set
        problems.append(dict(read="".join(read), seeds=seeds, max_mismatches=int(rng.integers(0, 5)) if max_mm is None else max_mm,
                             overlap_threshold=float(rng.choice([0.1, 0.8, 0.9])), trim=bool(rng.random() < 0.8)))
    return problems


def bubble_graph(rng, n_haplotypes, chain_nodes=14, max_alleles=3, cyclic=0.0, snp=0.0, invert=0.0):
    """a bubble chain with n_haplotypes random threads; `cyclic`: the share of threads that run through a stretch of the chain twice; `invert`:
    how often a thread takes its allele on the other strand (an inversion: a node is then followed by both orientations of another, the one
    place where the order of the opposite-strand ranges differs from the order of the nodes)"""
    nodes, chain, bubbles = [], [], []
    for c in range(chain_nodes):
        nodes.append(rand_seq(rng, rng.integers(3, 12)))
        chain.append(len(nodes) - 1)
        if c + 1 < chain_nodes and rng.random() < 0.6:
            alts = []
            for _ in range(int(rng.integers(2, max_alleles + 1))):
                nodes.append(rand_seq(rng, 1 if rng.random() < snp else rng.integers(1, 4)))
                alts.append(len(nodes) - 1)
            if rng.random() < 0.3:
                alts.append(None)                      # a deletion allele: skip the bubble
            bubbles.append(alts)
        else:
            bubbles.append(None)
    threads = []
    for _ in range(n_haplotypes):
        first = int(rng.integers(0, 3)); last = chain_nodes - int(rng.integers(0, 3))
        cols = list(range(first, last))
        if rng.random() < cyclic:
            i = int(rng.integers(0, len(cols) - 2)); j = int(rng.integers(i + 1, min(i + 4, len(cols))))
            cols = cols[:j] + cols[i:j] + cols[j:]
        t = []
        for k, c in enumerate(cols):
            t.append(2 * chain[c])
            if k + 1 < len(cols) and cols[k + 1] == c + 1 and bubbles[c]:
                a = bubbles[c][int(rng.integers(0, len(bubbles[c])))]
                if a is not None:
                    t.append(2 * a + int(rng.random() < invert))
        threads.append(t)
    return nodes, threads


def tandem_graph(rng):
    """tandem copies of a short motif, each copy a node of its own (one of them a variant now and then), between two flanks; the haplotypes
    take different numbers of copies.  A read inside the array aligns full-length at several shifts: overlaps and sets of several members."""
    motif = rand_seq(rng, rng.integers(3, 7)); n_copies = int(rng.integers(4, 8))
    nodes = [rand_seq(rng, rng.integers(6, 12))]
    copies = []
    for _ in range(n_copies):
        m = list(motif)
        if rng.random() < 0.25:
            m[int(rng.integers(0, len(m)))] = BASES[int(rng.integers(0, 4))]
        nodes.append("".join(m)); copies.append(len(nodes) - 1)
    nodes.append(rand_seq(rng, rng.integers(6, 12)))
    threads = []
    for _ in range(int(rng.integers(3, 6))):
        keep = [c for c in copies if rng.random() < 0.8] or copies[:1]
        threads.append([0] + [2 * c for c in keep] + [2 * (len(nodes) - 1)])
    return nodes, threads, copies


def tandem_case(rng, n_reads):
    nodes, threads, copies = tandem_graph(rng)

    def shifted(rng, o, diff):                          # the same seed on other copies of the motif
        if o // 2 not in copies:
            return []
        return [(2 * c + (o & 1), diff) for c in copies if rng.random() < 0.5]

    inner = [t[1:-1] for t in threads if len(t) > 4]                                  # reads inside the array: full-length at several shifts
    problems = sample_reads(rng, nodes, threads, n_reads - n_reads // 2, max_len=40, sub_rate=0.03, extra_seeds=shifted)
    if inner:
        problems += sample_reads(rng, nodes, inner, n_reads // 2, max_len=20, sub_rate=0.02, extra_seeds=shifted)
    return nodes, threads, problems


def corpus_case(seed, n_reads, kind):
    rng = np.random.default_rng(seed)
    if kind == 0:
        nodes, threads = bubble_graph(rng, 4)
    elif kind == 1:
        nodes, threads = bubble_graph(rng, 8, max_alleles=6, cyclic=0.3, invert=0.15)
    elif kind == 2:
        nodes, threads = bubble_graph(rng, 5, snp=0.7, cyclic=0.2, invert=0.3)
    else:
        return tandem_case(rng, n_reads)
    return nodes, threads, sample_reads(rng, nodes, threads, n_reads)


@functools.lru_cache(maxsize=None)
def set_corpus():
    """multi-seed problems: about 700 sets"""
    return tuple(corpus_case(s, 30, s % 4) for s in range(1000, 1024))


@functools.lru_cache(maxsize=None)
def winner_corpus():
    """every seed of a set corpus as a problem of its own, without trimming, max_mismatches 0 ... 4: about 2 000 problems"""
    out = []
    for s in range(2000, 2024):                                      # (few tandem arrays here: their copies tie at the top by construction)
        kind = (0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 2, 2, 1, 1, 1, 3)[s % 16]
        nodes, threads, problems = corpus_case(s, 16 if kind == 3 else 32, kind)
        singles = [dict(read=p["read"], seeds=[sd], max_mismatches=(i + k) % 5, overlap_threshold=p["overlap_threshold"], trim=False)
                   for i, p in enumerate(problems) for k, sd in enumerate(p["seeds"])]
        out.append((nodes, threads, singles))
    return tuple(out)


# ---- running a corpus -------------------------------------------------------------------------------------------------------------------
def run_case(eng, nodes, threads, problems):
    idx = eng.haplo_index(nodes, threads)
    out = tuple(a.copy() for a in eng.gapless_extend(idx, problems))
    idx.close()
    return out


def run_corpus(lib, corpus, scoring=None, alter=None):
    eng = capi.Engine(scoring, lib=lib)
    return [run_case(eng, nodes, threads, [alter(p) for p in problems] if alter else problems) for nodes, threads, problems in corpus]


@functools.lru_cache(maxsize=None)
def oracle_outputs(which):
    return run_corpus(util.ORACLE_LIB, CORPORA[which]())


CORPORA = dict(sets=set_corpus, winners=winner_corpus)
_checked = {}


def as_bytes(outputs):
    return b"".join(a.tobytes() for out in outputs for a in out)


def check_against_reference(which, outputs):
    """the reference checks over a corpus's output; computed once per distinct output (an engine that equals the oracle byte for byte shares
    the oracle's verdict).  -> counts"""
    key = (which, hash(as_bytes(outputs)), len(as_bytes(outputs)))
    if key in _checked:
        return _checked[key]
    counts = dict(problems=0, extensions=0, on_visited=0, unvisited=0, tied_problems=0, notes={})
    for (nodes, threads, problems), out in zip(CORPORA[which](), outputs):
        hap = ref.Haplotypes(nodes, threads)
        for p, (status, full, exts) in zip(problems, ref.sets_of(out)):
            read = ref.mask(p["read"])
            counts["problems"] += 1; counts["extensions"] += len(exts)
            assert status == 0, "no read of the corpora is declined"
            counts["on_visited"] += ref.check_set(hap, read, p, status, full, exts)
            if which == "winners":
                w = ref.check_winner(hap, read, p, status, exts)
                if w is None:
                    counts["unvisited"] += 1
                    continue
                counts["tied_problems"] += w[0] > 1
                for n in w[1]:
                    counts["notes"][n] = counts["notes"].get(n, 0) + 1
            else:
                counts["unvisited"] += sum(not ref.visited(hap, e) for e in exts)
    _checked[key] = counts
    return counts


def assert_equal_outputs(got, want):
    for a, b in zip(got, want):
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and len(x) == len(y) and x.tobytes() == y.tobytes()


def build_emu():
    subprocess.check_call(["make", "-s", "-j8", "emu"], cwd=util.ROOT)


# ---- the oracle and the emulated kernels against the reference --------------------------------------------------------------------------
def test_oracle_winners_are_top_finished_entries_of_the_reference_search():
    c = check_against_reference("winners", oracle_outputs("winners"))
    print(c)
    assert c["problems"] >= 1800
    assert c["unvisited"] <= c["problems"] // 100                    # seeds on nodes no thread visits: outside the reference
    assert c["tied_problems"] <= c["problems"] // 10                 # ties at the top are accepted as any top entry: membership is not the whole test


def test_oracle_sets_are_valid_and_keep_the_set_rules():
    c = check_against_reference("sets", oracle_outputs("sets"))
    print(c)
    assert c["problems"] >= 600 and c["extensions"] >= 1000
    assert c["unvisited"] <= c["extensions"] // 100
    assert c["on_visited"] == c["extensions"] - c["unvisited"]


def launch_forms(lib, which, monkeypatch):
    """a corpus on an engine as it comes and with the slab kernel alone, then both again with merged runs: each equals the oracle byte for byte
    and meets the reference"""
    want = oracle_outputs(which)
    for merge in (False, True):
        if merge:
            monkeypatch.setenv("VGAMD_HAPLO_MERGE", "1")
        for slab_only in (False, True):
            if slab_only:
                monkeypatch.setenv("VGAMD_GAPLESS_SLAB_ONLY", "1")
            else:
                monkeypatch.delenv("VGAMD_GAPLESS_SLAB_ONLY", raising=False)
            got = run_corpus(lib, CORPORA[which]())
            check_against_reference(which, got)
            assert_equal_outputs(got, want)
    monkeypatch.delenv("VGAMD_GAPLESS_SLAB_ONLY", raising=False); monkeypatch.delenv("VGAMD_HAPLO_MERGE", raising=False)


def test_emulated_kernels_meet_the_reference_on_the_winner_corpus(monkeypatch):
    build_emu()
    launch_forms(util.EMU_LIB, "winners", monkeypatch)


def test_emulated_kernels_meet_the_reference_on_the_set_corpus(monkeypatch):
    build_emu()
    launch_forms(util.EMU_LIB, "sets", monkeypatch)


@pytest.mark.gpu
def test_hip_kernels_meet_the_reference_on_the_winner_corpus(monkeypatch):
    launch_forms(util.ENGINE_LIB, "winners", monkeypatch)


@pytest.mark.gpu
def test_hip_kernels_meet_the_reference_on_the_set_corpus(monkeypatch):
    launch_forms(util.ENGINE_LIB, "sets", monkeypatch)


# ---- the corpus reaches every rule --------------------------------------------------------------------------------------------------------
def contained(small, big):
    n = len(small.path)
    return big.r0 <= small.r0 and small.r1 <= big.r1 and any(big.path[i:i + n] == small.path for i in range(len(big.path) - n + 1))


def test_the_corpora_reach_every_rule():
    """counted on the oracle's output; the floors are what the corpora gave when they were made (a generator that changes has to keep them)"""
    w = check_against_reference("winners", oracle_outputs("winners"))
    s = check_against_reference("sets", oracle_outputs("sets"))
    reached = dict(ties_at_the_top=w["tied_problems"], right_closed_by_stuck_copies=w["notes"].get("stuck_right", 0),
                   left_step_drops_the_stuck_entry=w["notes"].get("dropped_left", 0), initial_node_mismatches=w["notes"].get("init_mm", 0),
                   half_branch_of_the_limit=w["notes"].get("half", 0))
    plain = oracle_outputs("sets")
    untrimmed = run_corpus(util.ORACLE_LIB, set_corpus(), alter=lambda p: dict(p, trim=False))
    all_kept = run_corpus(util.ORACLE_LIB, set_corpus(), alter=lambda p: dict(p, overlap_threshold=1.0))
    several = rejected = trimmed = removed = five_edges = cyclic = 0
    for (nodes, threads, problems), a, b, c in zip(set_corpus(), plain, untrimmed, all_kept):
        hap = ref.Haplotypes(nodes, threads)
        wide = {o for o in hap.at if len(hap.edges(o)) >= 5}; twice = hap.revisiting()
        for p, x, y, z in zip(problems, ref.sets_of(a), ref.sets_of(b), ref.sets_of(c)):
            if x[1]:
                several += len(x[2]) >= 2
                rejected += len(z[2]) - len(x[2])
            elif p["trim"]:
                keys = {e.key() for e in x[2]}
                trimmed += sum(e.key() not in keys for e in y[2])
                removed += sum(not any(contained(t, e) for t in x[2]) for e in y[2])
            for e in x[2]:
                five_edges += any(o in wide for o in e.path[:-1]) or any(o ^ 1 in wide for o in e.path[1:])
                cyclic += any(o >> 1 in twice for o in e.path)
    reached.update(full_length_sets_of_several=several, overlap_rejections=rejected, trimmed_members=trimmed, members_trimmed_to_nothing=removed,
                   records_of_five_edges=five_edges, cyclic_threads=cyclic)
    print(reached, w, s)
    for name, n in reached.items():
        assert n >= 10, (name, reached)
    for name, n in FLOORS.items():
        assert reached[name] >= n, (name, reached[name], n)
    assert w["problems"] == FLOORS_PROBLEMS["winners"] and s["problems"] == FLOORS_PROBLEMS["sets"]


# what the corpora gave when they were made
FLOORS = dict(ties_at_the_top=160, right_closed_by_stuck_copies=147, left_step_drops_the_stuck_entry=239, initial_node_mismatches=809,
              half_branch_of_the_limit=193, full_length_sets_of_several=97, overlap_rejections=437, trimmed_members=131, members_trimmed_to_nothing=28,
              records_of_five_edges=264, cyclic_threads=308)
FLOORS_PROBLEMS = dict(winners=2106, sets=720)


# ---- the edge corpus: one or a few reads on each limit, inside a batch of ordinary reads ------------------------------------------------------
# Every limit is taken from the line of vg_amd/csrc/gapless_device.hpp (or gapless_api.cpp) that states it, cited beside the case.  At a limit the
# read's set equals the oracle's and meets the reference; one past it that read alone is declined with VGK_ETOOBIG, and every other read of the
# batch is what it is without it.  These are the reasons behind the share of declined reads that test_gapless.py's many_haplotypes allows (up to
# 10 % VGK_ETOOBIG with 300 haplotypes): more haplotypes, more branching, and a few more searches outgrow G_POOL entries per seed, G_PATH nodes or
# G_MISM mismatches per extension — here one read at a time, with the status each limit's line predicts.
@functools.lru_cache(maxsize=None)
def ordinary_batch():
    rng = np.random.default_rng(4242)
    nodes, threads = bubble_graph(rng, 4, chain_nodes=30)
    return nodes, threads, sample_reads(rng, nodes, threads, 200)


class Edge:
    """nodes and threads of a component of its own (oriented nodes counted from the component's first node), the special reads, and per read
    the status the header line predicts"""

    def __init__(self, name, nodes, threads, problems, expect, scoring=DEFAULT_SCORING, n_ext=None):
        self.name, self.nodes, self.threads, self.problems, self.expect, self.scoring, self.n_ext = name, nodes, threads, problems, expect, scoring, n_ext
        assert len(problems) == len(expect)

    def placed(self):
        """-> nodes, threads, ordinary reads, special reads of the whole index (the component behind the ordinary graph)"""
        nodes, threads, ordinary = ordinary_batch()
        shift = 2 * len(nodes)
        return (nodes + self.nodes, threads + [[o + shift for o in t] for t in self.threads], ordinary,
                [dict(p, seeds=[(o + shift, d) for o, d in p["seeds"]]) for p in self.problems])


def problem(read, seeds, max_mm=0, trim=True, overlap=0.8):
    return dict(read=read, seeds=seeds, max_mismatches=max_mm, overlap_threshold=overlap, trim=trim)


def substituted(s, positions):
    s = list(s)
    for p in positions:
        s[p] = BASES[(BASES.index(s[p]) + 1) % 4]
    return "".join(s)


def edge_path_nodes():
    """G_PATH = 48 nodes per extension (gapless_device.hpp: `constexpr int G_PATH = 48`; g_path: `nf >= G_PATH`, `nb >= G_PATH` before a node is
    added, `nb + nf > G_PATH` for the two together): 48 fit, 49 do not — to the right alone, and grown on both sides (24 + 24 | 24 + 25 | 25 + 24)"""
    rng = np.random.default_rng(1)
    nodes = [rand_seq(rng, 1) for _ in range(60)]
    whole = "".join(nodes)
    cases = [(47, 0), (48, 0), (49, 0), (48, 24), (49, 24), (49, 25), (48, 47), (49, 48)]          # (nodes, of them in front of the seed's)
    problems = [problem(whole[5:5 + k], [(2 * (5 + front), front)]) for k, front in cases]
    return Edge("path_nodes", nodes, [[2 * i for i in range(60)]], problems, [0 if k <= 48 else ETOOBIG for k, _ in cases])


def edge_mismatches():
    """G_MISM = 48 mismatches per extension (`constexpr int G_MISM = 48`; gx_find_mismatches: `if (e.n_mism >= G_MISM) overflow` before one is
    stored): 48 fit, 49 do not — in a full-length set (max_mismatches 60) and in a partial one that is then trimmed (max_mismatches 40)"""
    rng = np.random.default_rng(2)
    nodes = [rand_seq(rng, 150)]
    problems, expect = [], []
    for m in (47, 48, 49):
        read = substituted(nodes[0][10:130], [2 + 2 * i + (i % 3 == 0) for i in range(m)])
        problems += [problem(read, [(0, -10)], max_mm=60), problem(read, [(0, -10)], max_mm=40, trim=True), problem(read, [(0, -10)], max_mm=40, trim=False)]
        expect += [0 if m <= 48 else ETOOBIG] * 3
    return Edge("mismatches", nodes, [[0]], problems, expect)


def edge_seeds():
    """G_SEEDS = 64 seeds per cluster (`constexpr int G_SEEDS = 64`; `pb.n_seeds > (uint32_t)G_SEEDS` declines): 64 are taken, 65 are not; and
    G_HOT = 8 winners in the hot slab (`constexpr int G_HOT = 8`; GRes: `i < G_HOT ? hot[i] : cold[i - G_HOT]`): 8 and 9 distinct partial winners"""
    rng = np.random.default_rng(3)
    nodes = [rand_seq(rng, 9) for _ in range(132)]
    problems, expect, n_ext = [], [], []
    for k in (8, 9, 63, 64, 65):
        read = "".join(nodes[2 * j][1:8] + "x" for j in range(k))
        problems.append(problem(read, [(2 * (2 * j), 8 * j - 1) for j in range(k)]))
        expect.append(0 if k <= 64 else ETOOBIG); n_ext.append(k if k <= 64 else None)
    return Edge("seeds", nodes, [[2 * i for i in range(132)]], problems, expect, n_ext=n_ext)


def gate_graph(rng, n_chain=12):
    nodes = [rand_seq(rng, 32) for _ in range(n_chain)] + [rand_seq(rng, 1), rand_seq(rng, 1)]
    a, b = 2 * n_chain, 2 * n_chain + 2
    threads = [[2 * i for i in range(n_chain)], [2 * i for i in range(5)] + [a] + [2 * i for i in range(5, n_chain)], [2 * i for i in range(5)] + [b] + [2 * i for i in range(5, n_chain)]]
    return nodes, threads


def edge_read_length():
    """the fast kernel takes reads of at most 255 bases (gapless_extend_one / gapless_search_lane: `pb.read_len > 255u` hands the read to the slab
    kernel: its LDS entries keep read offsets in 8 bits): 254, 255, 256, 257 over nodes of 32 bases — all accepted"""
    rng = np.random.default_rng(4)
    nodes, threads = gate_graph(rng)
    problems = []
    for L in (254, 255, 256, 257):
        for t in threads[:2]:
            seq = oriented_seq(nodes, t)
            problems.append(problem(substituted(seq[7:7 + L], [40, 41, 170]), [(t[0], -7), (t[4], 4 * 32 - 7)], max_mm=4))
            rc = comp(seq[7:7 + L])
            problems.append(problem(rc, [(t[0] ^ 1, L + 7 - 32)], max_mm=4))
    return Edge("read_length", nodes, threads, problems, [0] * len(problems))


def edge_node_length(longest):
    """the fast kernel takes indexes whose longest node has at most 255 bases (`P.index.max_node_len > 255u`: 8-bit node offsets)"""
    rng = np.random.default_rng(5)
    nodes = [rand_seq(rng, 20), rand_seq(rng, longest), rand_seq(rng, 20)]
    whole = "".join(nodes)
    problems = [problem(whole[10:80], [(0, -10)], max_mm=2), problem(substituted(whole[120:170], [5, 30]), [(2, -100)], max_mm=4),
                problem(comp(whole[longest - 20:longest + 35]), [(5, 15 - 20)], max_mm=1), problem(whole[20:20 + longest], [(2, 0)], max_mm=0)]
    return Edge("node_length_%d" % longest, nodes, [[0, 2, 4]], problems, [0] * 4)


def edge_visits(most):
    """the fast kernel takes indexes whose most-visited node has at most 254 visits (`P.index.max_visits > 254u`: 8-bit visit ranks, an empty
    range stored as [1, 0])"""
    rng = np.random.default_rng(6)
    nodes = [rand_seq(rng, 12), rand_seq(rng, 12), rand_seq(rng, 12)]
    threads = [[0, 2]] * (most - 3) + [[0, 4]] * 2 + [[0]]
    whole = nodes[0] + nodes[1]
    problems = [problem(whole[3:20], [(0, -3)], max_mm=1), problem((nodes[0] + nodes[2])[2:22], [(4, 10)], max_mm=1), problem(comp(whole[1:22]), [(3, 0)], max_mm=2),
                problem(nodes[0][4:], [(0, -4)])]
    return Edge("visits_%d" % most, nodes, threads, problems, [0] * 4)


def edge_bubble(alleles):
    """records of up to four edges are counted in one pass, 16 bits per edge (g_counts: "a record with at most four edges"; g_search_step:
    `ne <= 4`), the others walk their visits per edge: bubbles of 3, 4, 5 and 8 alleles whose first bases match, behind an upstream SNP (the state
    at the fork is a strict sub-range), a thread that ends at the fork (the edge to -1), reads of both orientations"""
    rng = np.random.default_rng(70 + alleles)
    U, F, J, T = rand_seq(rng, 8), rand_seq(rng, 6), rand_seq(rng, 8), rand_seq(rng, 6)
    al = []
    while len(al) < alleles:
        s = "A" + rand_seq(rng, 3)
        if s not in al:
            al.append(s)
    nodes = [U, "C", "G", F] + al + [J, T]
    j, t = 4 + alleles, 5 + alleles
    threads = [[0, 2 * p, 6, 2 * (4 + i), 2 * j, 2 * t] for i in range(alleles) for p in (1, 2)] + [[0, 2, 6]]
    problems = []
    for i in (0, 1, alleles - 1):
        for p in (1, 2):
            fwd = U[2:] + nodes[p] + F + al[i] + J[:5]
            for read in (fwd, substituted(fwd, [len(fwd) - 5 - 2])):               # exact, and a mismatch inside the allele: several alleles are entered
                problems.append(problem(read, [(0, -2)], max_mm=2, trim=False))
                problems.append(problem(comp(read), [(2 * j + 1, -3)], max_mm=2, trim=False))
                problems.append(problem(read, [(0, -2), (6, 7), (2 * j, len(fwd) - 5)], max_mm=1))
    problems.append(problem(U[1:] + "C" + F, [(0, -1)], max_mm=0))                  # to the end of the thread that ends at the fork
    problems.append(problem(U[1:] + "C" + F + "ACC", [(6, 8)], max_mm=3))
    return Edge("bubble_%d" % alleles, nodes, threads, problems, [0] * len(problems))


def fan(rng, branches, tail):
    S, J = rand_seq(rng, 8), rand_seq(rng, 8)
    nodes = [S] + ["ACGT"] * branches + [J]
    threads = [[0, 2 * (1 + i), 2 * (1 + branches)] for i in range(branches)]
    return nodes, threads, S[2:] + "ACGT" + J[:tail]


def edge_fast_queue(branches):
    """the fast kernel's queue holds G_FAST_QUEUE = 5 entries in LDS beside the held-back candidate (`#define VGK_GAPLESS_FAST_QUEUE 5`; GStoreLds::
    slot_take fails without a free slot and the read is handed to the slab kernel): a fan-out of 5, 6, 7 and 12 equally good branches gives the same
    set wherever the read ends up"""
    nodes, threads, read = fan(np.random.default_rng(8), branches, 6)
    return Edge("fast_queue_%d" % branches, nodes, threads, [problem(read, [(0, -2)], max_mm=1), problem(comp(read), [(2 * (1 + branches) + 1, -2)], max_mm=1)], [0, 0])


def edge_pool(branches):
    """G_POOL = 160 partial extensions per seed (`constexpr int G_POOL = 160`; g_search_step: `s.np >= ST::ENTRIES` before an entry is made): the
    initial entry and one per branch — every allele ends the read — so 159 branches fit and 160 do not"""
    nodes, threads, read = fan(np.random.default_rng(9), branches, 0)
    return Edge("pool_%d" % branches, nodes, threads, [problem(read, [(0, -2)])], [0 if 1 + branches <= 160 else ETOOBIG])


def edge_score_width(scoring):
    """the fast kernel's LDS entries keep a 16-bit score (GStoreLds::pool_set: `(uint16_t)(int16_t)e.score`).  A context takes a scoring only when
    match + max(1, mismatch) + 2 x bonus <= 255 (vgk_api.cpp create_ctx: the profile bytes), so match, mismatch and bonus of 127 each are refused
    before any kernel sees them (test_a_context_refuses_the_scoring_past_its_range); the extremes a context does take: 127 / 1 / 63, where a read
    of 255 bases that matches throughout scores 255 x 127 + 2 x 63 = 32 511, and 1 / 127 / 63, where one whose initial node mismatches throughout
    scores 255 - 255 x 128 + 2 x 63 = -32 259"""
    rng = np.random.default_rng(10)
    nodes, threads = gate_graph(rng)
    n0 = len(nodes)
    nodes = nodes + ["A" * 255]
    threads = threads + [[2 * n0]]
    seq = oriented_seq(nodes, threads[1])
    problems = [problem(seq[3:258], [(0, -3), (2 * 3, 96 - 3)], max_mm=4), problem(comp(seq[3:258]), [(2 * 0 + 1, 255 + 3 - 32)], max_mm=4),
                problem(substituted(seq[3:258], [100, 200]), [(0, -3), (2 * 3, 96 - 3)], max_mm=4),
                problem("C" * 255, [(2 * n0, 0)], max_mm=4, trim=False), problem("C" * 255, [(2 * n0, 0)], max_mm=4, trim=True),
                problem("C" * 100 + "A" * 155, [(2 * n0, 0)], max_mm=4, trim=False)]
    # (the reads of C run their search with the extreme score and are then declined by the set rules: 255 and 100 mismatches are past G_MISM)
    return Edge("score_width_%d_%d_%d" % scoring, nodes, threads, problems, [0, 0, 0, ETOOBIG, ETOOBIG, ETOOBIG], scoring=scoring)


@functools.lru_cache(maxsize=None)
def edge_cases():
    out = [edge_path_nodes(), edge_mismatches(), edge_seeds(), edge_read_length(), edge_node_length(255), edge_node_length(256),
           edge_visits(254), edge_visits(255), edge_visits(256)]
    out += [edge_bubble(a) for a in (3, 4, 5, 8)] + [edge_fast_queue(b) for b in (5, 6, 7, 12)] + [edge_pool(b) for b in (158, 159, 160)]
    out += [edge_score_width((127, 1, 63)), edge_score_width((1, 127, 63))]
    return {e.name: e for e in out}


EDGE_NAMES = ["path_nodes", "mismatches", "seeds", "read_length", "node_length_255", "node_length_256", "visits_254", "visits_255", "visits_256",
              "bubble_3", "bubble_4", "bubble_5", "bubble_8", "fast_queue_5", "fast_queue_6", "fast_queue_7", "fast_queue_12", "pool_158", "pool_159", "pool_160",
              "score_width_127_1_63", "score_width_1_127_63"]


def per_read(outputs):
    return [(status, full, [(e.key(), tuple(e.mism), e.state) for e in exts]) for status, full, exts in ref.sets_of(outputs)]


def engine_with(scoring, lib):
    return capi.Engine(capi.Scoring.simple(scoring[0], scoring[1], 6, 1, scoring[2]), lib=lib)


@functools.lru_cache(maxsize=None)
def edge_oracle(name):
    """the oracle's sets of a case's batch, the special reads held to the reference (the oracle has no table limits: it answers every read)"""
    e = edge_cases()[name]
    nodes, threads, ordinary, special = e.placed()
    out = run_case(engine_with(e.scoring, util.ORACLE_LIB), nodes, threads, ordinary + special)
    hap = ref.Haplotypes(nodes, threads)
    for p, (status, full, exts) in zip(special, ref.sets_of(out)[len(ordinary):]):
        ref.check_set(hap, ref.mask(p["read"]), p, status, full, exts, e.scoring)
    sets = per_read(out)
    if e.n_ext:
        for want, got in zip(e.n_ext, sets[len(ordinary):]):
            assert want is None or len(got[2]) == want
    return out, sets


def check_edge(lib, name, merged=False):
    e = edge_cases()[name]
    nodes, threads, ordinary, special = e.placed()
    want_out, want = edge_oracle(name)
    eng = engine_with(e.scoring, lib)
    idx = eng.haplo_index(nodes, threads)
    with_out = tuple(a.copy() for a in eng.gapless_extend(idx, ordinary + special))
    got = per_read(with_out)
    without = per_read(eng.gapless_extend(idx, ordinary))
    n = len(ordinary)
    assert got[:n] == without, "the other reads of the batch do not move"
    assert got[:n] == want[:n]
    for k, status in enumerate(e.expect):
        g = got[n + k]
        if merged and status == ETOOBIG and g[0] == 0:               # a run is one node: a read the plain index declines may fit
            assert g == want[n + k], (name, k)
            continue
        assert g[0] == status, (name, k, g[0], status)
        if status == 0:
            assert g == want[n + k], (name, k, g, want[n + k])       # (equal to a set that met the reference: edge_oracle)
        else:
            assert g[1:] == (0, [])
    if all(s == 0 for s in e.expect):
        for x, y in zip(with_out, want_out):
            assert x.tobytes() == y.tobytes()
    idx.close()


def edge_forms(lib, name, monkeypatch):
    for merge in (False, True):
        if merge:
            monkeypatch.setenv("VGAMD_HAPLO_MERGE", "1")
        for slab_only in (False, True):
            if slab_only:
                monkeypatch.setenv("VGAMD_GAPLESS_SLAB_ONLY", "1")
            else:
                monkeypatch.delenv("VGAMD_GAPLESS_SLAB_ONLY", raising=False)
            check_edge(lib, name, merged=merge)
    monkeypatch.delenv("VGAMD_GAPLESS_SLAB_ONLY", raising=False); monkeypatch.delenv("VGAMD_HAPLO_MERGE", raising=False)


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edge_corpus_on_the_oracle(name):
    """the oracle has no table limits: it answers every read of every case, and its sets of the special reads meet the reference"""
    out, sets = edge_oracle(name)
    assert all(s[0] == 0 for s in sets)


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edge_corpus_on_the_emulated_kernels(name, monkeypatch):
    build_emu()
    edge_forms(util.EMU_LIB, name, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edge_corpus_on_the_hip_kernels(name, monkeypatch):
    edge_forms(util.ENGINE_LIB, name, monkeypatch)


def refused_scoring(lib):
    with pytest.raises(capi.VgkError, match="outside the kernels' range"):
        engine_with((127, 127, 127), lib)


def test_a_context_refuses_the_scoring_past_its_range():
    """match, mismatch and bonus of 127 each: VGK_EUNSUPPORTED from vgk_create — the 16-bit score of the fast kernel's entries never meets them"""
    build_emu()
    refused_scoring(util.EMU_LIB)


@pytest.mark.gpu
def test_a_hip_context_refuses_the_scoring_past_its_range():
    refused_scoring(util.ENGINE_LIB)


def merged_runs_hand_out_more_nodes(lib, monkeypatch):
    monkeypatch.setenv("VGAMD_HAPLO_MERGE", "1")
    e = edge_cases()["path_nodes"]
    want = per_read(run_case(capi.Engine(lib=util.ORACLE_LIB), e.nodes, e.threads, e.problems))
    got = per_read(run_case(capi.Engine(lib=lib), e.nodes, e.threads, e.problems))
    assert got == want and all(g[0] == 0 for g in got)


def test_merged_runs_hand_out_more_original_nodes_than_a_path_holds(monkeypatch):
    """with merged runs an extension of one merged node may touch more than G_PATH original nodes: the device's room for nodes follows the caller's,
    not seeds x G_PATH (the batch here is the path-node reads alone, so nothing else pads the arrays)"""
    build_emu()
    merged_runs_hand_out_more_nodes(util.EMU_LIB, monkeypatch)


@pytest.mark.gpu
def test_merged_runs_hand_out_more_original_nodes_than_a_path_holds_on_the_gpu(monkeypatch):
    merged_runs_hand_out_more_nodes(util.ENGINE_LIB, monkeypatch)


# ---- the index builder's refusals (gapless_api.cpp vgk_haplo_from_tables: `ne > 255 || count[o] > 65535 || len[o] > 65535`: edge numbers are
# bytes, ranks and lengths 16 bits) — host-side, nothing is launched; the context then takes a valid index and a valid batch
def refusal_indexes():
    rng = np.random.default_rng(11)
    out = {}
    for n in (254, 255):                                 # successors of node 0 (the end of a thread is an edge too: 255 | 256 edges)
        nodes = ["ACGT"] + ["C" + BASES[i % 4] if i < 12 else "GT"[i % 2] + BASES[(i // 2) % 4] for i in range(n)]      # a dozen successors the read enters
        out["edges_%d" % (n + 1)] = (nodes, [[0, 2 * (1 + i)] for i in range(n)] + [[0]], n + 1 <= 255)
    node = rand_seq(rng, 10)
    for v in (65535, 65536):
        out["visits_%d" % v] = ([node], None, v <= 65535)     # (threads made where they are used: v lists of one node)
    for ln in (65535, 65536):
        out["length_%d" % ln] = ([rand_seq(rng, ln)], [[0]], ln <= 65535)
    return out


def check_index_refusals(lib):
    eng = capi.Engine(lib=lib); ora = capi.Engine(lib=util.ORACLE_LIB)
    o_nodes, o_threads, o_reads = ordinary_batch()
    for name, (nodes, threads, accepted) in refusal_indexes().items():
        if threads is None:
            threads = np.zeros((int(name.split("_")[1]), 1), dtype=np.uint32)
        if accepted:
            idx = eng.haplo_index(nodes, threads)
            rng = np.random.default_rng(12)
            whole = nodes[0] + (nodes[1] if len(nodes) > 1 else "")
            problems = [problem(whole[a:a + 8], [(0, -a)], max_mm=0) for a in (0, 1, 2)] + [problem(comp(nodes[0])[:9], [(1, 0)], max_mm=1)]
            if len(nodes[0]) > 1000:
                problems += [problem(substituted(nodes[0][65000:65100], [50]), [(0, -65000)], max_mm=2), problem(nodes[0][-30:], [(0, 30 - len(nodes[0]))])]
            got = per_read(run_case(eng, nodes, threads, problems)); want = per_read(run_case(ora, nodes, threads, problems))
            assert got == want and all(g[0] == 0 for g in got), name
            hap = None if len(threads) > 1000 else ref.Haplotypes(nodes, threads)          # (65 535 copies of one node: the ranks are the thread numbers)
            for p, (status, full, exts) in zip(problems, ref.sets_of(run_case(eng, nodes, threads, problems))):
                if hap:
                    ref.check_set(hap, ref.mask(p["read"]), p, status, full, exts)
                else:
                    assert all(x.state == (x.path[-1], 0, len(threads) - 1, x.path[0] ^ 1, 0, len(threads) - 1) for x in exts)
            idx.close()
        else:
            with pytest.raises(capi.VgkError, match="vgk_haplo_create"):
                eng.haplo_index(nodes, threads)
        got = per_read(run_case(eng, o_nodes, o_threads, o_reads[:40]))                        # the context goes on
        assert got == per_read(run_case(ora, o_nodes, o_threads, o_reads[:40])), name


def test_index_builder_refuses_past_its_field_widths_on_the_emulator():
    build_emu()
    check_index_refusals(util.EMU_LIB)


@pytest.mark.gpu
def test_index_builder_refuses_past_its_field_widths_on_the_gpu():
    check_index_refusals(util.ENGINE_LIB)


# ---- the lane code under the host sanitizers: every edge case as one call of a program of its own ------------------------------------------------
SAN = os.path.join(util.ROOT, "tests", "emu", "gapless_san")


def write_call(path, scoring, nodes, threads, problems):
    gs = capi.GaplessSet.from_lists(problems)
    sc = capi.Scoring.simple(scoring[0], scoring[1], 6, 1, scoring[2])
    toff = np.concatenate([[0], np.cumsum([len(t) for t in threads])]).astype("<u4")
    tn = np.concatenate([np.asarray(t, dtype="<u4") for t in threads]) if len(threads) else np.zeros(0, "<u4")
    with open(path, "wb") as f:
        f.write(b"VGKG"); f.write(bytes(sc))
        f.write(struct.pack("<I", len(nodes))); f.write(np.array([len(s) for s in nodes], dtype="<u4").tobytes()); f.write("".join(nodes).encode())
        f.write(struct.pack("<I", len(threads))); f.write(toff.tobytes()); f.write(tn.tobytes())
        f.write(struct.pack("<I", gs.n))
        for r in gs.array:
            f.write(struct.pack("<IIIId", int(r["read_len"]), int(r["n_seeds"]), int(r["max_mismatches"]), int(r["flags"]), float(r["overlap_threshold"])))
        f.write(gs.reads[:int(gs.read_off[-1])].tobytes()); f.write(gs.seeds[:int(gs.seed_off[-1])].tobytes())


def sanitized_call(tmp_path, name, scoring, nodes, threads, problems, env):
    call, out = str(tmp_path / (name + ".call")), str(tmp_path / (name + ".out"))
    write_call(call, scoring, nodes, threads, problems)
    clean = {k: v for k, v in os.environ.items() if k not in ("VGAMD_HAPLO_MERGE", "VGAMD_GAPLESS_SLAB_ONLY")}
    p = subprocess.run([SAN, call, out], env=dict(clean, **env), capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (name, env, p.returncode, p.stderr[-2000:])
    with open(out, "rb") as f:
        return f.read()


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edge_corpus_is_clean_under_the_host_sanitizers(name, tmp_path, monkeypatch):
    """AddressSanitizer and UBSan over vgk_haplo_create and vgk_gapless_extend on the emulated backend (make gapless_san), one child process per
    call: exit status 0, nothing on stderr, and the bytes the emulator library gives"""
    build_emu()
    subprocess.check_call(["make", "-s", "-j8", "gapless_san"], cwd=util.ROOT)
    e = edge_cases()[name]
    nodes, threads, ordinary, special = e.placed()
    problems = ordinary[:60] + special
    for env in ({}, {"VGAMD_GAPLESS_SLAB_ONLY": "1"}, {"VGAMD_HAPLO_MERGE": "1"}):
        for k in ("VGAMD_GAPLESS_SLAB_ONLY", "VGAMD_HAPLO_MERGE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        res, ext, nd, mm = run_case(engine_with(e.scoring, util.EMU_LIB), nodes, threads, problems)
        want = struct.pack("<iiQQQ", 0, 0, len(ext), len(nd), len(mm)) + res.tobytes() + ext.tobytes() + nd.tobytes() + mm.tobytes()
        assert sanitized_call(tmp_path, name, e.scoring, nodes, threads, problems, env) == want, (name, env)


def test_index_refusals_are_clean_under_the_host_sanitizers(tmp_path):
    build_emu()
    subprocess.check_call(["make", "-s", "-j8", "gapless_san"], cwd=util.ROOT)
    for name, (nodes, threads, accepted) in refusal_indexes().items():
        if threads is None:
            threads = np.zeros((int(name.split("_")[1]), 1), dtype=np.uint32)
        problems = [problem(nodes[0][:8], [(0, 0)], max_mm=1), problem(comp(nodes[0])[:9], [(1, 0)], max_mm=1)]
        got = sanitized_call(tmp_path, name, DEFAULT_SCORING, nodes, threads, problems, {})
        if not accepted:
            assert got == struct.pack("<iiQQQ", ETOOBIG, 0, 0, 0, 0), name
        else:
            res, ext, nd, mm = run_case(capi.Engine(lib=util.EMU_LIB), nodes, threads, problems)
            assert got == struct.pack("<iiQQQ", 0, 0, len(ext), len(nd), len(mm)) + res.tobytes() + ext.tobytes() + nd.tobytes() + mm.tobytes(), name
