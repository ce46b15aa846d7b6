"""Anchors for chaining from seeds and their gapless extensions (reference src/minimizer_mapper_from_chains.cpp:1380-1596): the host shim's restatement
(vg_amd/host/extension_anchors.cpp, vgh_extension_anchors), the serial statement of the device's rule (vg_amd/csrc/extension_anchors_device.hpp:
ea_problem_one, through tests/emu/extension_anchors_driver.cpp) and the device call (include/vgk_engine.h: vgk_extension_anchors).

References: the reference's own known answers for the seed anchors (src/unittest/minimizer_mapper.cpp:997-1003, :1050-1128, transcribed as data in
tests/golden/ref_extension_anchors.json); for find_anchor_intervals, of which the reference holds NO unit test, `intervals_restated`: an index-based
restatement from the function's contract (every bound is the best of its candidate cuts, counted over ranges instead of swept), held to the shim on every
extension of the corpus, with the contract of the function's comment (:464-479) asserted on the results; for the block as a whole `block_restated`, which
also counts which rules a problem reaches.  The corpus is made once, shared, never changed."""
import bisect
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import util

K = 7                       # the corpus' minimizer length
MATCH, MISMATCH, MAX_MM = 1, 4, 4
NONE = 0xffffffff


@functools.lru_cache(maxsize=None)
def capi():
    from vg_amd import capi as c
    return c


# ---- a graph for the rule: only oriented node lengths matter to it (the engine wants bases and a thread too)
@functools.lru_cache(maxsize=None)
def graph():
    rng = np.random.default_rng(41)
    lens = [int(x) for x in rng.integers(1, 13, 90)] + [int(x) for x in rng.integers(20, 60, 10)]
    nodes = ["".join("ACGT"[b] for b in rng.integers(0, 4, n)) for n in lens]
    return nodes, [[2 * i for i in range(len(nodes))]], np.repeat(np.array(lens, dtype=np.uint32), 2)


def walk_of(rng, olen, L):
    """a random walk of oriented nodes under a read of L bases that begins `first` bases into the first node -> per read base (walk step, oriented node, offset)"""
    walk, total = [], 0
    first = None
    while first is None or total < first + L:
        o = int(rng.integers(0, len(olen)))
        if first is None:
            first = int(rng.integers(0, olen[o]))
        walk.append(o); total += int(olen[o])
    step, node, off = [], [], []
    at = first
    for k, o in enumerate(walk):
        while at < olen[o] and len(step) < L:
            step.append(k); node.append(o); off.append(at); at += 1
        at = 0
    return walk, step, node, off


def extension_on(walk, step, off, rb, re_, mm, L):
    return dict(path=walk[step[rb]:step[re_ - 1] + 1], offset=off[rb], read_begin=rb, read_end=re_, mismatches=sorted(mm), left_full=int(rb == 0), right_full=int(re_ == L))


def random_problem(rng, n_seeds, n_ext, L=None, k=K, flavour=None, mismatches_on_seeds=False):
    """mismatches_on_seeds: a mismatch may fall on the stapled base of a seed.  No extension of real seeds has one there — the extension compares the very
    base the seed matched, on the seed's own diagonal.  Otherwise a third of the read's positions is set aside for mismatches and no seed is stapled there"""
    _, _, olen = graph()
    L = int(rng.integers(max(k + 4, 24), 161)) if L is None else L
    walk, step, node, off = walk_of(rng, olen, L)
    seeds = np.zeros(n_seeds, dtype=capi().ANCHOR_SEED_DT)
    for_mismatches = rng.random(L) < (0.0 if mismatches_on_seeds else 0.33)
    for_mismatches[:k] = False; for_mismatches[L - k:] = False      # (so that either orientation can be stapled near both ends)
    free = np.flatnonzero(~for_mismatches)
    for i in range(n_seeds):
        r = rng.random()
        if i and r < 0.04:                                          # the same seed again: equal diagonal and stapled base
            seeds[i] = seeds[int(rng.integers(0, i))]; continue
        rev = int(rng.random() < 0.5); st = -1
        while st < 0 or not (k - 1 <= st if rev else st + k <= L):
            st = int(free[int(rng.integers(0, len(free)))])
        if r > 0.97:                                                # a seed off the walk
            o = int(rng.integers(0, len(olen))); seeds[i] = (o, st - int(rng.integers(0, olen[o])), st, k, rev, int(rng.integers(0, 1 << 62)))
        else:
            seeds[i] = (node[st], st - off[st], st, k, rev, int(rng.integers(1, 1 << 62)) if rng.random() < 0.7 else 0xf)
    exts = []
    for _ in range(n_ext):
        r = rng.random()
        if exts and r < 0.12:                                       # an extension again: a tied score, and no seed left for it
            exts.append(dict(exts[int(rng.integers(0, len(exts)))])); continue
        if exts and r < 0.2:                                        # one of another walk: no seed of the problem lies on it
            w2, s2, _, o2 = walk_of(rng, olen, L)
            exts.append(extension_on(w2, s2, o2, 0, L, [], L)); exts[-1]["left_full"] = 0; continue
        if flavour == "full" or r > 0.9:
            rb, re_ = 0, L
        else:
            rb = int(rng.integers(0, L - 10)); re_ = int(rng.integers(rb + 8, L + 1))
        n_mm = int(rng.integers(0, 9)) if rng.random() < 0.8 else 0
        if flavour == "full":
            n_mm = int(rng.integers(0, 3))
        mm = set(int(x) for x in rng.integers(rb, re_, n_mm))
        for m in list(mm):                                          # runs of mismatches
            if rng.random() < 0.35 and m + 2 < re_:
                mm.add(m + 1 + int(rng.integers(0, 2)))
        if not mismatches_on_seeds:
            mm = set(m for m in mm if for_mismatches[m]) | set(m + 1 for m in mm if m + 1 < re_ and for_mismatches[m] and for_mismatches[m + 1])
        exts.append(extension_on(walk, step, off, rb, re_, mm, L))
    front = exts[0] if exts else None
    full = int(bool(front) and front["left_full"] and front["right_full"] and len(front["mismatches"]) <= 4)      # GaplessExtender::full_length_extensions over MAX_MISMATCHES
    return dict(seeds=seeds, extensions=exts, full_length=full)


@functools.lru_cache(maxsize=None)
def corpus():
    rng = np.random.default_rng(2027)
    problems = [random_problem(rng, 0, 3), random_problem(rng, 12, 0), random_problem(rng, 0, 0)]
    problems += [random_problem(rng, int(rng.integers(1, 201)), int(rng.integers(1, 9))) for _ in range(2400)]
    problems += [random_problem(rng, int(rng.integers(1, 40)), int(rng.integers(1, 4)), flavour="full") for _ in range(100)]
    problems += [random_problem(rng, int(rng.integers(150, 201)), int(rng.integers(20, 40)), L=160) for _ in range(20)]
    # what no real extension has, for the branch that only this reaches (an interval all of whose seeds are used: see the contract test)
    problems += [random_problem(rng, int(rng.integers(1, 201)), int(rng.integers(1, 9)), mismatches_on_seeds=True) for _ in range(200)]
    return problems


def packed(problems):
    c = capi()
    soff = np.zeros(len(problems) + 1, dtype=np.uint64); eoff = np.zeros(len(problems) + 1, dtype=np.uint64)
    exts, nodes, mism = [], [], []
    for p, q in enumerate(problems):
        soff[p + 1] = soff[p] + len(q["seeds"]); eoff[p + 1] = eoff[p] + len(q["extensions"])
        for e in q["extensions"]:
            exts.append((len(nodes), len(e["path"]), e["offset"], e["read_begin"], e["read_end"], len(mism), len(e["mismatches"]), 0, e["left_full"], e["right_full"], (0, 0), (0,) * 6))
            nodes += e["path"]; mism += e["mismatches"]
    seeds = np.concatenate([q["seeds"] for q in problems]) if problems else np.zeros(0, dtype=c.ANCHOR_SEED_DT)
    return dict(seed_off=soff, seeds=seeds, ext_off=eoff, extensions=np.array(exts, dtype=c.EXT_DT) if exts else np.zeros(0, dtype=c.EXT_DT),
                full_length=np.array([q["full_length"] for q in problems], dtype=np.uint32), nodes=np.array(nodes, dtype=np.uint32), mismatches=np.array(mism, dtype=np.uint32))


@functools.lru_cache(maxsize=None)
def corpus_packed():
    return packed(corpus())


@functools.lru_cache(maxsize=None)
def host_lib():
    subprocess.check_call(["make", "-s", "host"], cwd=util.ROOT)
    h = ctypes.CDLL(util.HOST_LIB)
    h.vgh_last_error.restype = ctypes.c_char_p
    return h


@functools.lru_cache(maxsize=None)
def serial_lib():
    subprocess.check_call(["make", "-s", "extanchors"], cwd=util.ROOT)
    return ctypes.CDLL(os.path.join(util.ROOT, "tests", "emu", "libvgamd_extanchors.so"))


def call(fn, head, P, from_seeds=False, tail=(), caps=None, match=MATCH, mismatch=MISMATCH, olen=None):
    c = capi()
    if head is None:
        olen = graph()[2] if olen is None else olen
        head = (ctypes.c_void_p(olen.ctypes.data), ctypes.c_uint64(len(olen)))
    return c.extension_anchors_call(fn, head, match, mismatch, c.VGK_ANCHORS_FROM_SEEDS if from_seeds else 0, MAX_MM, P["seed_off"], P["seeds"], P["ext_off"], P["extensions"],
                                    P["full_length"], P["nodes"], P["mismatches"], tail=tail, caps=caps)


def shim_raw(P, from_seeds=False, threads=4, **kw):
    rc, out = call(host_lib().vgh_extension_anchors, None, P, from_seeds, tail=(ctypes.c_int(threads),), **kw)
    assert rc == 0, host_lib().vgh_last_error()
    return out


def serial_raw(P, from_seeds=False, **kw):
    rc, out = call(serial_lib().vgt_extension_anchors_serial, None, P, from_seeds, **kw)
    assert rc == 0, rc
    return out


@functools.lru_cache(maxsize=None)
def shim_on_corpus(from_seeds=False):
    out = shim_raw(corpus_packed(), from_seeds)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


FIELDS = ("anchor_off", "anchors", "origins", "rep_off", "represented", "status")


def same(got, want, context):
    assert got["written"] == want["written"], context
    for name in FIELDS:
        assert len(got[name]) == len(want[name]) and got[name].tobytes() == want[name].tobytes(), (context, name)


# ---- the restatements
def seed_anchor_restated(s, olen, match=MATCH):
    k, offset = int(s["length"]), int(s["stapled"]) - int(s["diff"])
    if s["is_reverse"]:
        length = min(k, offset + 1)
        return dict(read_start=int(s["stapled"]) + 1 - length, length=length, margin_before=k - length, margin_after=0, score=match * k, start_hint_offset=length - 1,
                    end_hint_offset=1, base_seed_length=k, start_paths=int(s["paths"]), end_paths=int(s["paths"]))
    length = min(k, int(olen[s["node"]]) - offset)
    return dict(read_start=int(s["stapled"]), length=length, margin_before=0, margin_after=k - length, score=match * k, start_hint_offset=0, end_hint_offset=length,
                base_seed_length=k, start_paths=int(s["paths"]), end_paths=int(s["paths"]))


def intervals_restated(rb, re_, mm, pos, count=None):
    """find_anchor_intervals from its contract, index-based.  A stretch [x, y) of the extension is worth its matches minus 4 per mismatch.  The first
    interval begins at the read bound or just behind a mismatch before the first seed, wherever the stretch up to the last such mismatch is worth most (the
    latest such start among equals).  Mismatches a .. b between two seeds are split at mismatch a + (b - a + 1) // 2: the left interval ends at one of the
    mismatches a .. split, wherever the stretch from mismatch a is worth most (the earliest among equals); the right one begins just behind one of the
    mismatches split .. b, wherever the stretch up to mismatch b is worth most (the latest among equals).  Behind the last seed the left rule runs up to
    the read bound."""
    count = count if count is not None else {}
    def bump(name):
        count[name] = count.get(name, 0) + 1
    if not mm:
        return [(rb, re_)]
    def worth(x, y):                                                # matches minus 4 per mismatch in [x, y)
        n = bisect.bisect_left(mm, y) - bisect.bisect_left(mm, x)
        return (y - x - n) - 4 * n
    out = []
    before = bisect.bisect_left(mm, pos[0])                        # mismatches strictly before the first seed
    start = rb
    if before:
        last = mm[before - 1]
        cands = [mm[j] + 1 for j in range(before - 1, -1, -1)] + [rb]      # from the seed leftwards
        best = max(worth(c, last + 1) for c in cands)
        start = next(c for c in cands if worth(c, last + 1) == best)
        if start != rb:
            bump("first_trim_moves_start")
        if start not in (rb, last + 1):
            bump("first_trim_inside")
    for i in range(len(pos)):
        nxt = pos[i + 1] if i + 1 < len(pos) else None
        a = bisect.bisect_left(mm, pos[i])                         # the first mismatch at or behind this seed
        b = (bisect.bisect_left(mm, nxt) if nxt is not None else len(mm)) - 1      # the last one strictly before the next seed
        if b < a:
            if nxt is None:
                out.append((start, re_))
            continue
        if nxt is not None:
            split = a + (b - a + 1) // 2
            bump("split_odd" if (b - a + 1) % 2 else "split_even")
        else:
            split = len(mm)
        bound = lambda c: re_ if c == len(mm) else mm[c]
        cands = list(range(a, split + 1))
        best = max(worth(mm[a], bound(c)) for c in cands)
        cut = next(c for c in cands if worth(mm[a], bound(c)) == best)
        out.append((start, bound(cut)))
        if nxt is not None:
            cands = list(range(b, split - 1, -1))
            best = max(worth(mm[c] + 1, mm[b] + 1) for c in cands)
            rcut = next(c for c in cands if worth(mm[c] + 1, mm[b] + 1) == best)
            start = mm[rcut] + 1
            if cut != split:
                bump("left_cut_not_split")
            if rcut != split:
                bump("right_cut_not_split")
            if cut != split and rcut != split:
                bump("both_cuts_not_split")
    return out


def block_restated(q, olen, from_seeds=False, count=None, seen=None):
    """the whole block for one problem -> (status, listed extensions, [(anchor, origin)] sorted); count: the rules reached; seen: the (extension, unused seed
    positions) pairs find_anchor_intervals was asked about"""
    count = count if count is not None else {}
    def bump(name, n=1):
        count[name] = count.get(name, 0) + n
    seeds, exts = q["seeds"], q["extensions"]
    sa = [seed_anchor_restated(s, olen) for s in seeds]
    for s, a in zip(seeds, sa):
        bump("reverse_minimizers", int(s["is_reverse"])); bump("margin_before", int(a["margin_before"] > 0)); bump("margin_after", int(a["margin_after"] > 0))
    made = []
    if from_seeds:
        bump("seeds_only")
        for i, a in enumerate(sa):
            made.append((a, dict(seed_first=i, seed_last=i, n_seq=1, rep=[i], extension=NONE, read_begin=a["read_start"] - a["margin_before"], read_end=a["read_start"] + a["length"] + a["margin_after"])))
    else:
        bump("no_seeds", int(len(seeds) == 0)); bump("seeds_without_extensions", int(len(seeds) > 0 and not exts))
        if q["full_length"]:
            good = [x for x, e in enumerate(exts) if e["left_full"] and e["right_full"] and len(e["mismatches"]) <= MAX_MM]
            if good:
                bump("full_length_shortcut")
                return 1, good, []
        diagonals = {}
        for i, s in enumerate(seeds):
            diagonals.setdefault((int(s["node"]), int(s["diff"])), []).append((int(s["stapled"]), i))
        for d in diagonals.values():
            d.sort()
            bump("equal_diagonal_and_stapled", sum(1 for x, y in zip(d, d[1:]) if x[0] == y[0]))
        scores = [(e["read_end"] - e["read_begin"]) - 5 * len(e["mismatches"]) for e in exts]
        bump("tied_extension_scores", len(scores) - len(set(scores)))
        used = set()
        for x in sorted(range(len(exts)), key=lambda x: (-scores[x], x)):
            e = exts[x]
            bump("extension_over_three_nodes", int(len(e["path"]) >= 3))
            contained, at, node_offset = [], e["read_begin"], e["offset"]
            for o in e["path"]:
                n = min(int(olen[o]) - node_offset, e["read_end"] - at)
                contained += [i for st, i in diagonals.get((o, at - node_offset), []) if at <= st < at + n]
                at += n; node_offset = 0
            left = [i for i in contained if i not in used]
            if not left:
                bump("extension_without_seed_left")
                continue
            positions = [int(seeds[i]["stapled"]) for i in left]
            if seen is not None:
                seen.append((e["read_begin"], e["read_end"], e["mismatches"], positions))
            for a, b in intervals_restated(e["read_begin"], e["read_end"], e["mismatches"], positions, count):
                mine = [i for i in contained if a <= int(seeds[i]["stapled"]) < b and i not in used]
                if not mine:
                    bump("interval_all_seeds_used")
                    continue
                used.update(mine)
                n_mm = sum(1 for m in e["mismatches"] if a <= m < b)
                f, l = sa[mine[0]], sa[mine[-1]]
                w = dict(read_start=f["read_start"], length=l["read_start"] + l["length"] - f["read_start"],
                         margin_before=(f["margin_before"] + (f["read_start"] - f["margin_before"]) - a) & 0xffffffff,
                         margin_after=(l["margin_after"] + b - (l["read_start"] + l["length"] + l["margin_after"])) & 0xffffffff,
                         score=MATCH * (b - a - n_mm) - MISMATCH * n_mm, start_hint_offset=f["start_hint_offset"], end_hint_offset=l["end_hint_offset"],
                         base_seed_length=(f["base_seed_length"] + l["base_seed_length"]) // 2, start_paths=f["start_paths"], end_paths=l["end_paths"])
                n_seq = 2 if f["read_start"] + f["length"] <= l["read_start"] else 1
                bump("n_seq_%d" % n_seq)
                made.append((w, dict(seed_first=mine[0], seed_last=mine[-1], n_seq=n_seq, rep=mine, extension=x, read_begin=a, read_end=b)))
    order = sorted(range(len(made)), key=lambda k: (made[k][0]["read_start"], -(made[k][0]["read_start"] + made[k][0]["length"]), k))
    return 0, [], [made[k] for k in order]


def assert_restated_equals(out, problems, from_seeds, count=None, seen=None):
    olen = graph()[2]
    for p, q in enumerate(problems):
        status, listed, made = block_restated(q, olen, from_seeds, count, seen)
        a0, a1 = int(out["anchor_off"][p]), int(out["anchor_off"][p + 1]); r0, r1 = int(out["rep_off"][p]), int(out["rep_off"][p + 1])
        assert int(out["status"][p]) == status and a1 - a0 == len(made), p
        if status:
            assert [int(x) for x in out["represented"][r0:r1]] == listed, p
            continue
        for k, (w, o) in enumerate(made):
            got, org = out["anchors"][a0 + k], out["origins"][a0 + k]
            assert {name: int(got[name]) for name in w} == w, (p, k)
            assert [int(org[name]) for name in ("seed_first", "seed_last", "n_seq", "n_rep", "extension", "read_begin", "read_end")] \
                == [o["seed_first"], o["seed_last"], o["n_seq"], len(o["rep"]), o["extension"], o["read_begin"], o["read_end"]], (p, k)
            b = int(org["rep_begin"])
            assert r0 <= b and b + len(o["rep"]) <= r1 and [int(x) for x in out["represented"][b:b + len(o["rep"])]] == o["rep"], (p, k)
        assert sum(len(o["rep"]) for _, o in made) == r1 - r0, p


# ---- without a GPU
def golden():
    return util.load_golden("ref_extension_anchors.json")


def golden_problems():
    """-> (oriented node lengths, problems of one or four seeds each, expectations per problem)"""
    g = golden(); st = g["stick"]; c = capi()
    out = []
    for size in st["node_sizes"]:
        lens = [min(size, st["sequence_length"] - a) for a in range(0, st["sequence_length"], size)]
        olen = np.repeat(np.array(lens, dtype=np.uint32), 2)
        where = [(2 * n, i) for n, ln in enumerate(lens) for i in range(ln)]      # forward strand of the stick: (oriented node, offset) per base
        problems, expect = [], []
        for start in st["minimizer_starts"]:
            for rev in st["orientations"]:
                pin = start + st["minimizer_length"] - 1 if rev else start
                node, off = where[pin]
                problems.append(dict(seeds=np.array([(node, pin - off, pin, st["minimizer_length"], rev, 1)], dtype=c.ANCHOR_SEED_DT), extensions=[], full_length=0))
                expect.append([dict(score=st["expect_score"])])
        out.append((olen, problems, expect, st["match"]))
    geo = g["geometry"]
    olen = np.array([geo["node_length"]] * 2, dtype=np.uint32)
    problems, expect = [], []
    for case in geo["cases"]:
        # the read runs along the strand named; an offset on that strand is the read offset here
        seeds = [(case["graph_reverse_strand"], s["read_offset"] - s["graph_offset"], s["read_offset"], s["length"], s["is_reverse"], 1) for s in case["seeds"]]
        problems.append(dict(seeds=np.array(seeds, dtype=c.ANCHOR_SEED_DT), extensions=[], full_length=0))
        expect.append([dict(read_start=s["expect_read_start"], length=s["expect_length"]) for s in case["seeds"]])
    out.append((olen, problems, expect, 1))
    return out


def check_golden(run):
    """run(packed problems, oriented node lengths, match) -> the seeds-only answer, anchors sorted: looked up by their origin's seed"""
    n = 0
    for olen, problems, expect, match in golden_problems():
        out = run(packed(problems), olen, match)
        for p, want in enumerate(expect):
            a0, a1 = int(out["anchor_off"][p]), int(out["anchor_off"][p + 1])
            assert a1 - a0 == len(want)
            by_seed = {int(out["origins"][k]["seed_first"]): out["anchors"][k] for k in range(a0, a1)}
            for i, w in enumerate(want):
                for name, value in w.items():
                    assert int(by_seed[i][name]) == value, (p, i, name); n += 1
    assert n == 3 * 16 + 8 * 4 * 2


def test_the_references_known_answers():
    """src/unittest/minimizer_mapper.cpp:1050-1128 (every anchor scores 5 whatever the node size) and :997-1003 (read start, length): shim and serial lane code"""
    check_golden(lambda P, olen, match: shim_raw(P, True, olen=olen, match=match))
    check_golden(lambda P, olen, match: serial_raw(P, True, olen=olen, match=match))


REQUIRED = ("first_trim_moves_start", "first_trim_inside", "split_odd", "split_even", "left_cut_not_split", "right_cut_not_split", "both_cuts_not_split", "interval_all_seeds_used",
            "extension_without_seed_left", "reverse_minimizers", "margin_before", "margin_after", "extension_over_three_nodes", "equal_diagonal_and_stapled",
            "tied_extension_scores", "n_seq_1", "n_seq_2", "full_length_shortcut", "no_seeds", "seeds_without_extensions", "seeds_only")


@functools.lru_cache(maxsize=None)
def corpus_walked():
    """the block restated over the corpus, held to the shim problem by problem -> (the rules reached, find_anchor_intervals' inputs)"""
    count, seen = {}, []
    assert_restated_equals(shim_on_corpus(False), corpus(), False, count, seen)
    assert_restated_equals(shim_on_corpus(True), corpus(), True, count)
    return count, seen


def test_the_shim_equals_the_restatement_and_the_corpus_reaches_every_rule():
    count, _ = corpus_walked()
    print({name: count.get(name, 0) for name in REQUIRED})
    for name in REQUIRED:
        assert count.get(name, 0) > 0, name


def test_find_anchor_intervals_equals_its_restatement_and_keeps_its_contract():
    """the reference has no unit test of find_anchor_intervals: the shim's is held to intervals_restated on every extension of the corpus that still has
    seeds in its turn, and both to the function's comment (:464-479).  "A seed in each interval" presupposes what every real extension gives: no
    mismatch on a seed's stapled base (the seed matched that very base on that diagonal).  With a mismatch there the reference's own sweep ends the
    interval AT the seed — and only then can the block's branch "all seeds in the interval were used already" (:1549-1557) be reached: where the clause
    holds, the interval holds an unused seed.  So that clause is asserted wherever its premise holds, the premise computed from the extension itself, and
    the other clauses everywhere; the corpus' 200 problems with such mismatches are there for that branch."""
    h = host_lib()
    h.vgh_find_anchor_intervals.restype = ctypes.c_int64
    h.vgh_find_anchor_intervals.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]
    _, seen = corpus_walked()
    assert len(seen) > 3000
    premise = 0
    for rb, re_, mm, pos in seen:
        m = np.array(mm, dtype=np.uint64); s = np.array(pos, dtype=np.uint64); out = np.zeros(2 * len(pos) + 2, dtype=np.uint64)
        n = h.vgh_find_anchor_intervals(rb, re_, m.ctypes.data if len(m) else None, len(m), s.ctypes.data, len(s), out.ctypes.data, len(pos) + 1)
        got = [(int(out[2 * k]), int(out[2 * k + 1])) for k in range(n)]
        assert got == intervals_restated(rb, re_, mm, pos), (rb, re_, mm, pos)
        assert all(a <= b for a, b in got) and all(x[1] <= y[0] for x, y in zip(got, got[1:]))                # sorted, disjoint
        if not set(mm) & set(pos):
            assert all(a < b and any(a <= p < b for p in pos) for a, b in got)                                # a seed in each
            premise += 1
        assert all((a == rb or a - 1 in mm) and (b == re_ or b in mm) for a, b in got)                        # bounds: the extension's, or just outside a mismatch
        assert mm or got == [(rb, re_)]
    assert premise > 0.9 * len(seen)


def test_serial_lane_code_equals_the_shim():
    """ea_problem_one (the statement of the device's rule, the kernels' checker) through tests/emu/extension_anchors_driver.cpp, field for field"""
    for from_seeds in (False, True):
        same(serial_raw(corpus_packed(), from_seeds), shim_on_corpus(from_seeds), from_seeds)


def test_sizing_calls_of_shim_and_serial_lane_code():
    P = packed(corpus()[:40]); want = shim_raw(P)
    for fn, tail in ((host_lib().vgh_extension_anchors, (ctypes.c_int(2),)), (serial_lib().vgt_extension_anchors_serial, ())):
        rc, out = call(fn, None, P, tail=tail, caps=(0, 0))
        assert rc == capi().VGK_EOPS and out["written"] == want["written"]
        rc, out = call(fn, None, P, tail=tail, caps=want["written"])
        assert rc == 0
        same(out, want, "exact room")


def test_the_driver_as_a_program_under_the_host_sanitizers(tmp_path):
    """the stand-alone driver, built with -fsanitize=address,undefined, on a part of the corpus: a clean run and the shim's answer"""
    subprocess.check_call(["make", "-s", "extanchors_san"], cwd=util.ROOT)
    problems = corpus()[:400] + corpus()[-20:]
    P = packed(problems); want = shim_raw(P); olen = graph()[2]; n = len(problems)
    with open(tmp_path / "call.bin", "wb") as f:
        f.write(np.array([len(olen), MATCH, MISMATCH, 0, MAX_MM, n, len(P["seeds"]), len(P["extensions"]), len(P["nodes"]), len(P["mismatches"])], dtype=np.uint64).tobytes())
        for a in (olen, P["seed_off"], P["seeds"], P["ext_off"], P["extensions"], P["full_length"], P["nodes"], P["mismatches"]):
            f.write(a.tobytes())
    r = subprocess.run([os.path.join(util.ROOT, "tests", "emu", "extension_anchors_san"), str(tmp_path / "call.bin"), str(tmp_path / "answer.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    raw = open(tmp_path / "answer.bin", "rb").read(); c = capi()
    head = np.frombuffer(raw, dtype=np.uint64, count=3); na, nr = int(head[1]), int(head[2]); at = 24
    got = dict(written=(na, nr))
    for name, dt, k in (("anchor_off", np.uint64, n + 1), ("rep_off", np.uint64, n + 1), ("status", np.uint32, n), ("anchors", c.CHAIN_ANCHOR_DT, na), ("origins", c.ANCHOR_ORIGIN_DT, na),
                        ("represented", np.uint32, nr)):
        got[name] = np.frombuffer(raw, dtype=dt, count=k, offset=at); at += k * np.dtype(dt).itemsize
    assert int(head[0]) == 0 and at == len(raw)
    same(got, want, "sanitized driver")


def hand_over(chain_items, out, n):
    """every problem's anchors as vgk_chain_items' input with no candidate transitions"""
    c = capi()
    return chain_items(dict(max_chains=1), out["anchor_off"], out["anchors"], np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=c.CHAIN_CANDIDATE_DT))


def test_the_anchors_are_in_the_order_and_of_the_lengths_chaining_validates():
    """vgk_chain_items refuses anchors out of sort_anchor_indexes' order or of length 0 (chain_items_api.cpp): the same checks, on every problem of the corpus"""
    for from_seeds in (False, True):
        out = shim_on_corpus(from_seeds); a = out["anchors"]; n = 0
        for p in range(len(corpus())):
            a0, a1 = int(out["anchor_off"][p]), int(out["anchor_off"][p + 1])
            x = a[a0:a1]; start = x["read_start"].astype(np.int64); end = start + x["length"]
            assert (x["length"] > 0).all() and (np.diff(start) >= 0).all() and ((np.diff(start) > 0) | (np.diff(end) <= 0)).all(), p
            n += a1 - a0
        assert n == len(a) > 5000


def test_header():
    text = open(os.path.join(util.ROOT, "include", "vgk_engine.h")).read()
    for name in ("vgk_extension_anchors", "vgk_extension_anchors_limits", "vgk_extension_anchors_last_ms"):
        assert re.search(r"\b%s\(" % name, text), name
    assert "vgk_extension_anchors" not in open(os.path.join(util.ROOT, "include", "vgk.h")).read()      # the oracle has no counterpart


# ---- on the GPU
@functools.lru_cache(maxsize=None)
def engine():
    eng = capi().Engine(lib=util.ENGINE_LIB, device=0)
    nodes, threads, _ = graph()
    return eng, eng.haplo_index(nodes, threads)


def device_raw(P, from_seeds=False, eng=None, index=None, caps=None, **kw):
    e, i = engine()
    eng = eng or e; index = index or i
    return call(eng.lib.vgk_extension_anchors, (eng.h, index.h), P, from_seeds, caps=caps, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("from_seeds", (False, True))
def test_device_equals_the_shim_on_the_corpus(from_seeds):
    rc, got = device_raw(corpus_packed(), from_seeds)
    assert rc == 0
    same(got, shim_on_corpus(from_seeds), from_seeds)
    assert all(ms > 0.0 for ms in engine()[0].extension_anchors_last_ms()[:1 if from_seeds else 3])


@pytest.mark.gpu
def test_device_hands_over_to_chain_items():
    rc, got = device_raw(corpus_packed())
    assert rc == 0
    out = hand_over(engine()[0].chain_items, got, len(corpus()))
    assert len(out["chains"]) == len(corpus())


@pytest.mark.gpu
def test_more_seeds_than_the_lds_arrays_hold_and_more_extensions_than_lanes():
    lds_seeds, lanes, lds_ext, _ = engine()[0].extension_anchors_limits()
    rng = np.random.default_rng(77)
    problems = [random_problem(rng, lds_seeds + 300, 12, L=3000, mismatches_on_seeds=True), random_problem(rng, 150, lanes + 37, L=160, mismatches_on_seeds=True),
                random_problem(rng, 90, lds_ext + 5, L=120), random_problem(rng, 20, 3)]
    P = packed(problems); want = shim_raw(P)
    assert_restated_equals(want, problems, False)
    for from_seeds in (False, True):
        rc, got = device_raw(P, from_seeds)
        assert rc == 0
        same(got, shim_raw(P, from_seeds), from_seeds)


@pytest.mark.gpu
def test_device_reproduces_the_references_known_answers():
    eng = engine()[0]
    def run(P, olen, match):
        nodes = ["A" * int(n) for n in olen[::2]]
        index = eng.haplo_index(nodes, [[2 * i for i in range(len(nodes))]])
        rc, out = device_raw(P, True, index=index, match=match)
        assert rc == 0
        return out
    check_golden(run)


@pytest.mark.gpu
def test_a_context_reused_and_a_second_index():
    eng, index = engine(); nodes, threads, _ = graph()
    big = packed(corpus()[:300]); small = packed(corpus()[300:340])
    first = device_raw(big)[1]
    same(device_raw(small)[1], shim_raw(small), "smaller call on the same context")
    same(device_raw(big)[1], first, "the first call again")
    same(device_raw(big, index=eng.haplo_index(nodes, threads))[1], first, "a second index")
    other = capi().Engine(lib=util.ENGINE_LIB, device=0)
    same(device_raw(big, eng=other, index=other.haplo_index(nodes, threads))[1], first, "a second context")


@pytest.mark.gpu
def test_sizing_and_argument_errors():
    c = capi(); eng, index = engine()
    problems = corpus()[3:43]; P = packed(problems); want = shim_raw(P)
    rc, out = device_raw(P, caps=(0, 0))
    assert rc == c.VGK_EOPS and out["written"] == want["written"]
    rc, out = device_raw(P, caps=(want["written"][0], want["written"][1] - 1))
    assert rc == c.VGK_EOPS and out["written"] == want["written"]
    rc, out = device_raw(P, caps=want["written"])
    assert rc == 0
    same(out, want, "exact room")

    def changed(array, field, k, value):
        Q = dict(P); Q[array] = P[array].copy()
        if field is None:
            Q[array][k] = value
        else:
            Q[array][field][k] = value
        return Q
    e = P["extensions"]; has_mm = int(np.flatnonzero(e["n_mismatches"] >= 2)[0]); m0 = int(e["mism_begin"][has_mm])
    olen = graph()[2]
    bad = dict(seed_off_descends=changed("seed_off", None, 2, int(P["seed_off"][1]) - 1) if P["seed_off"][2] > P["seed_off"][1] else changed("seed_off", None, 0, 1),
               seed_off_not_from_0=changed("seed_off", None, 0, 1), ext_off_not_from_0=changed("ext_off", None, 0, 1),
               seed_outside_its_node=changed("seeds", "diff", 5, int(P["seeds"]["stapled"][5]) - int(olen[P["seeds"]["node"][5]])),
               seed_before_its_node=changed("seeds", "diff", 5, int(P["seeds"]["stapled"][5]) + 1),
               seed_node_outside_the_index=changed("seeds", "node", 5, len(olen)),
               length_0=changed("seeds", "length", 7, 0), is_reverse_2=changed("seeds", "is_reverse", 7, 2),
               path_leaves_the_array=changed("extensions", "path_begin", 3, len(P["nodes"])), mismatches_leave_the_array=changed("extensions", "mism_begin", has_mm, len(P["mismatches"]) - 1),
               mismatches_descend=changed("mismatches", None, m0 + 1, int(P["mismatches"][m0])), mismatch_outside_the_interval=changed("mismatches", None, m0, int(e["read_end"][has_mm])),
               empty_read_interval=changed("extensions", "read_end", 3, int(e["read_begin"][3])), node_outside_the_index=changed("nodes", None, 0, len(olen)))
    rev = int(np.flatnonzero(P["seeds"]["is_reverse"] == 1)[0])
    Q = changed("seeds", "stapled", rev, K - 2); Q["seeds"]["diff"][rev] = K - 2 - (int(P["seeds"]["stapled"][rev]) - int(P["seeds"]["diff"][rev]))
    bad["reverse_stapled_before_its_length"] = Q
    for what, Q in bad.items():
        assert device_raw(Q)[0] == c.VGK_EINVAL, what
    assert device_raw(P, match=-1)[0] == c.VGK_EINVAL
    assert device_raw(P)[0] == 0                                    # and the context still answers
    sc = c.Scoring.simple(1, 4, 6, 1, 5)
    qa = c.Engine(sc, lib=util.ENGINE_LIB, device=0, qual_adj=(np.zeros(256 * 25, dtype=np.int8), np.zeros(256, dtype=np.int8)))
    nodes, threads, _ = graph()
    assert device_raw(P, eng=qa, index=qa.haplo_index(nodes, threads))[0] == c.VGK_EUNSUPPORTED
    rc, out = c.extension_anchors_call(eng.lib.vgk_extension_anchors, (eng.h, index.h), 1, 4, 0, 4, np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=c.ANCHOR_SEED_DT), np.zeros(1, dtype=np.uint64))
    assert rc == 0 and out["written"] == (0, 0)                     # a call without problems


@pytest.mark.gpu
def test_the_pipeline_on_reads_with_substitutions():
    """pipeline.extension_anchors (vgk_gapless_extend, then the new call) on ExtensionAnchorsWorkload agrees with the shim run on the same extensions"""
    from vg_amd import pipeline, workloads
    wl = workloads.ExtensionAnchorsWorkload(60, seed=5, read_len=600, graph_bp=40000)
    eng = capi().Engine(lib=util.ENGINE_LIB, device=0)
    index = eng.haplo_index(wl.nodes, wl.threads)
    problems = wl.problems(eng, index)
    got = pipeline.extension_anchors(eng, index, problems)
    olen = np.repeat(np.array([len(s) for s in wl.nodes], dtype=np.uint32), 2)
    rc, want = capi().extension_anchors_call(host_lib().vgh_extension_anchors, (ctypes.c_void_p(olen.ctypes.data), ctypes.c_uint64(len(olen))), 1, 4, 0, 4, got["seed_off"], got["seeds"],
                                             got["ext_off"], got["extensions"], got["full_length"], got["nodes"], got["mismatches"], tail=(ctypes.c_int(4),))
    assert rc == 0, host_lib().vgh_last_error()
    same(got, want, "pipeline")
    # not a trivial batch: an anchor per read at least, extensions with mismatches, anchors that stand for several seeds
    assert len(got["anchors"]) >= 60 and (got["extensions"]["n_mismatches"] > 0).sum() > 20 and (got["origins"]["n_rep"] > 1).sum() > 20
