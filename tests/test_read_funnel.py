"""vgk_funnel_clusters, vgk_funnel_extension_sets and vgk_funnel_winners (include/vgk_engine.h): a short read's funnel on the device — which clusters are
extended, which extension sets are aligned, which alignments win and which minimizers count as explored (MinimizerMapper::map_from_extensions,
src/minimizer_mapper.cpp:650-1128, find_supplementaries == false).

The pins, from the outside in: a statement of the cited lines in this file, in another shape (sorted on a key, an explicit tie run, a loop over verdicts, its
own minstd_rand; score_cluster with sets and a boolean array; the estimate is vgh_score_extension_group, which tests/test_extension_scoring.py pins on its
quadratic recurrence) must equal the host shim (vgh_funnel_*: callbacks into one process_until_threshold_e) in every output field; the serial statement of
the device rule (rf_walk and the rf_*_one of vg_amd/csrc/read_funnel_device.hpp, behind tests/emu/read_funnel_driver.cpp) must equal the shim — every
integer, and both doubles bit for bit: the score is additions in one order, the coverage one division; the same driver runs as a program of its own under
the host sanitizers; and the engine must equal the shim in every field, the doubles bit for bit."""
import collections
import ctypes
import os
import subprocess

import numpy as np
import pytest

from vg_amd import capi, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = os.path.join(ROOT, "vg_amd", "libvgamd.so")
DRIVER = os.path.join(ROOT, "tests", "emu", "libvgamd_readfunnel.so")
GO, GE = 6, 1
EINVAL, OK, EOPS = capi.VGK_EINVAL, capi.VGK_OK, capi.VGK_EOPS


def limits():
    out = (ctypes.c_uint32 * 4)()
    assert ctypes.CDLL(ENGINE).vgk_funnel_limits(out) == 0
    return tuple(int(x) for x in out)


def policies():
    P = capi.FunnelPolicy.giraffe
    return collections.OrderedDict([
        ("main", P(0, capi.FUNNEL_OWN_LENGTH, cluster_score_threshold=4.0, pad_cluster_score_threshold=2.0, cluster_coverage_threshold=0.25)),
        ("zero thresholds", P(0, capi.FUNNEL_OWN_LENGTH, cluster_score_threshold=0.0, cluster_coverage_threshold=0.0, extension_set_score_threshold=0.0, max_multimaps=3)),
        ("small counts", P(0, capi.FUNNEL_OWN_LENGTH, cluster_score_threshold=4.0, cluster_coverage_threshold=0.0, max_extensions=3, min_extensions=1, max_alignments=2,
                           min_extension_sets=1, max_multimaps=2, extension_set_min_score=5)),
    ])


# ---- the statement in another shape ---------------------------------------------------------------------------------------------------------------------
class Minstd:
    def __init__(self, state, seq):
        self.x, self.seq = int(state), seq

    def __call__(self):
        if not self.x:
            s = 0
            for b in self.seq:
                s = (s * 13 + int(b)) & 0xffffffff
            self.x = s % 2147483647 or 1
        self.x = self.x * 48271 % 2147483647
        return self.x


def walk(n, key, score, threshold, at_least, at_most, rng, process, cover, what):
    """-> (order, better_or_equal per position, fate per item: taken / skipped / count / score)"""
    order = sorted(range(n), key=key)
    width = sum(1 for i in order if key(i) == key(order[0])) if n else 0
    if width >= 2:
        cover["a %d-wide top tie %s rng_state" % (min(width, 3), "with" if rng is not None else "without")] += 1
    if rng is not None:
        for i in range(1, width):
            j = rng() % (i + 1)
            order[j], order[i] = order[i], order[j]
    keys = [key(i) for i in order]
    boe = [sum(1 for q in keys if q <= k) for k in keys]
    if any(keys[i] == keys[i + 1] for i in range(width, n - 1)):
        cover["ties below the top left in index order"] += 1
    cutoff = score(order[0]) - threshold if n else 0.0
    if n and threshold == 0:
        cover["threshold 0: nothing fails"] += 1
    taken, fate = 0, {}
    for it in order:
        below = threshold != 0 and score(it) <= cutoff
        if below and score(it) == cutoff and taken >= at_least:
            cover["an item exactly at best - threshold fails"] += 1
        if below and taken >= at_least:
            fate[it] = "score"
        elif not below and taken >= at_most:
            fate[it] = "count"
            cover[what + ": fails by count"] += 1
        else:
            fate[it] = "taken" if process(it, below) else "skipped"
            if below and fate[it] == "taken":
                cover["the minimum filled by an item below the cutoff"] += 1
            if fate[it] == "skipped":
                cover["a skipped item that does not count towards the minimum"] += 1
            taken += fate[it] == "taken"
    return order, boe, fate


def own_clusters(pol, a, rng_state, cover):
    n = len(a["read_off"]) - 1
    out = np.zeros(len(a["cluster_seed_off"]) - 1, dtype=capi.FUNNEL_CLUSTER_DT); status = np.zeros(n, dtype=np.int32); kept = [[] for _ in range(n)]
    for r in range(n):
        L = int(a["read_off"][r + 1] - a["read_off"][r]); mlo, mhi = int(a["minimizer_off"][r]), int(a["minimizer_off"][r + 1]); M = mhi - mlo
        clo, chi = int(a["cluster_off"][r]), int(a["cluster_off"][r + 1])
        mins = a["minimizers"][mlo:mhi]; sc = a["minimizer_score"][mlo:mhi]
        length = mins["reserved"].astype(np.int64) if pol.flags & capi.FUNNEL_OWN_LENGTH else np.full(M, pol.k, dtype=np.int64)
        src = [a["sources"][int(a["cluster_seed_off"][c]):int(a["cluster_seed_off"][c + 1])] for c in range(clo, chi)]
        bad = (chi > clo and L == 0) or not np.isfinite(sc).all() or (mins["offset"].astype(np.int64) + length > L).any() or any((s >= M).any() for s in src)
        if bad:
            status[r] = EINVAL
            continue
        if chi == clo:
            cover["a read with no cluster"] += 1
        score, coverage = [], []
        for c, s in enumerate(src):
            present = sorted(set(int(x) for x in s))
            total = 0.0
            bases = np.zeros(L, dtype=bool)
            for j in present:
                total += float(sc[j])
                if bases[int(mins["offset"][j]):int(mins["offset"][j]) + int(length[j])].any():
                    cover["overlapping k-mers: a union"] += 1
                bases[int(mins["offset"][j]):int(mins["offset"][j]) + int(length[j])] = True
                if int(mins["offset"][j]) + int(length[j]) == L:
                    cover["a k-mer ending at the read's last base"] += 1
                for bit in (32, 64):
                    if int(mins["offset"][j]) < bit < int(mins["offset"][j]) + int(length[j]):
                        cover["a k-mer straddling bit %d of the bitmap" % bit] += 1
            if len(present) < len(s):
                cover["two seeds of one minimizer, counted once"] += 1
            if len(s) == 1:
                cover["a cluster of one seed"] += 1
            if M >= 65 and present and present[-1] >= 64 and present[0] < 64:
                cover["present bits that cross a word"] += 1
            covered = int(bases.sum())
            out[clo + c]["score"] = total; out[clo + c]["covered"] = covered; out[clo + c]["coverage"] = covered / L
            score.append(total); coverage.append(covered / L)
        best = max([0.0] + score); second = max([0.0] + sorted(score)[:-1]) if score else 0.0
        cutoff = best - pol.cluster_score_threshold
        if score and len(score) > 1:
            gap = cutoff - pol.pad_cluster_score_threshold
            if second < cutoff:
                cover["the second best " + ("inside the pad" if gap < second else "exactly on the pad" if gap == second else "outside the pad")] += 1
        if cutoff - pol.pad_cluster_score_threshold < second:
            cutoff = min(cutoff, second)
        if len(set(coverage)) < len(coverage) and len(set(zip(coverage, score))) > len(set(coverage)):
            cover["a tie in coverage broken by score"] += 1
        mine = kept[r]

        def process(c, below):
            if pol.cluster_score_threshold != 0 and score[c] < cutoff:
                if len(mine) >= pol.min_extensions:
                    cover["the cluster score filter fires"] += 1
                    return False
                cover["the cluster score filter waits for min_extensions"] += 1
            mine.append(clo + c)
            return True
        rng = None if rng_state is None else Minstd(rng_state[r], a["reads"][int(a["read_off"][r]):int(a["read_off"][r + 1])])
        order, boe, fate = walk(chi - clo, lambda c: (-coverage[c], -score[c]), lambda c: coverage[c], pol.cluster_coverage_threshold, pol.min_extensions, pol.max_extensions,
                                rng, process, cover, "max_extensions")
        if rng is not None:
            rng_state[r] = rng.x
        for at, c in enumerate(order):
            out[clo + c]["rank"] = at; out[clo + c]["better_or_equal"] = boe[at]
            out[clo + c]["verdict"] = {"taken": capi.FUNNEL_EXTEND, "skipped": capi.FUNNEL_FAIL_SCORE, "count": capi.FUNNEL_FAIL_MAX_EXTENSIONS, "score": capi.FUNNEL_FAIL_COVERAGE}[fate[c]]
    kept_off = np.concatenate([[0], np.cumsum([len(k) for k in kept])]).astype(np.uint64)
    return dict(clusters=out, status=status, kept_off=kept_off, kept=np.array([c for k in kept for c in k], dtype=np.uint32), written=int(kept_off[-1]))


def own_sets(pol, a, rng_state, cover):
    host = pipeline._host_lib()
    host.vgh_score_extension_group.restype = ctypes.c_int
    host.vgh_score_extension_group.argtypes = [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    n = len(a["read_off"]) - 1; n_clusters = len(a["cluster_seed_off"]) - 1
    out = np.zeros(len(a["results"]), dtype=capi.FUNNEL_SET_DT); status = np.zeros(n, dtype=np.int32); aligned = [[] for _ in range(n)]
    explored = np.zeros(int(a["minimizer_off"][-1]), dtype=np.uint8)
    for r in range(n):
        L = int(a["read_off"][r + 1] - a["read_off"][r]); mlo = int(a["minimizer_off"][r]); M = int(a["minimizer_off"][r + 1]) - mlo
        lo, hi = int(a["kept_off"][r]), int(a["kept_off"][r + 1])
        est, failed, src, bad = [], [], [], False
        for s in range(lo, hi):
            c = int(a["kept"][s]); g = a["results"][s]
            if c >= n_clusters:
                bad = True
                break
            src.append(a["sources"][int(a["cluster_seed_off"][c]):int(a["cluster_seed_off"][c + 1])])
            bad = bad or bool((src[-1] >= M).any())
            failed.append(g["status"] != 0)
            if failed[-1]:
                cover["a failed gapless result"] += 1
                est.append(0)
                continue
            if int(g["ext_begin"]) + int(g["n_ext"]) > len(a["extensions"]):
                bad = True
                break
            e = a["extensions"][int(g["ext_begin"]):int(g["ext_begin"]) + int(g["n_ext"])]
            if (e["read_begin"] >= e["read_end"]).any() or (e["read_end"] > L).any() or (np.diff(e["read_begin"].astype(np.int64)) < 0).any():
                bad = True
            iv = np.ascontiguousarray(np.stack([e["read_begin"], e["read_end"], e["score"]], axis=1).astype(np.int64))
            cover["a full-length set" if g["full_length"] and len(e) else "an empty set" if not len(e) else "a set to chain"] += 1
            est.append(0 if bad else host.vgh_score_extension_group(L, iv.ctypes.data if len(e) else None, len(e), int(g["full_length"]), GO, GE))
        if bad:
            status[r] = EINVAL
            continue
        out["estimate"][lo:hi] = est
        mine = aligned[r]

        def process(s, below):
            if failed[s]:
                return False
            if est[s] < pol.extension_set_min_score:
                if below:
                    cover["an estimate below extension_set_min_score admitted by the minimum and still discarded"] += 1
                return False
            mine.append(lo + s)
            explored[mlo + src[s].astype(np.int64)] = 1
            return True
        rng = None if rng_state is None else Minstd(rng_state[r], a["reads"][int(a["read_off"][r]):int(a["read_off"][r + 1])])
        if rng is not None and rng.x and hi - lo >= 2 and sorted(est)[-1] == sorted(est)[-2]:
            cover["rng_state carried from one call into the next"] += 1
        order, boe, fate = walk(hi - lo, lambda s: -est[s], lambda s: float(est[s]), pol.extension_set_score_threshold, pol.min_extension_sets, pol.max_alignments, rng, process,
                                cover, "max_alignments")
        if rng is not None:
            rng_state[r] = rng.x
        for at, s in enumerate(order):
            v = {"taken": capi.FUNNEL_SET_ALIGN, "count": capi.FUNNEL_SET_FAIL_MAX_ALIGNMENTS, "score": capi.FUNNEL_SET_FAIL_SCORE, "skipped": capi.FUNNEL_SET_FAIL_MIN_SCORE}[fate[s]]
            out[lo + s]["rank"] = at; out[lo + s]["better_or_equal"] = boe[at]; out[lo + s]["verdict"] = capi.FUNNEL_SET_FAILED if failed[s] else v
        in_aligned = collections.Counter(int(j) for s in range(hi - lo) if fate[s] == "taken" for j in set(src[s].tolist()))
        in_other = collections.Counter(int(j) for s in range(hi - lo) if fate[s] != "taken" for j in set(src[s].tolist()))
        if any(j not in in_aligned for j in in_other):
            cover["a minimizer only in a kept-but-not-aligned cluster is not explored"] += 1
        if any(j in in_aligned for j in in_other):
            cover["a minimizer in two clusters, one of them aligned, is explored"] += 1
    aligned_off = np.concatenate([[0], np.cumsum([len(k) for k in aligned])]).astype(np.uint64)
    return dict(sets=out, status=status, aligned_off=aligned_off, aligned=np.array([s for k in aligned for s in k], dtype=np.uint32), explored=explored, written=int(aligned_off[-1]))


def own_winners(pol, a, rng_state, cover):
    n = len(a["read_off"]) - 1
    scores, picks, n_reported, unmapped = [], [], np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
    for r in range(n):
        items = []                                                        # (score, set, alignment, mappings)
        for j in range(int(a["aligned_off"][r]), int(a["aligned_off"][r + 1])):
            lo, hi = int(a["aln_off"][j]), int(a["aln_off"][j + 1])
            for t in range(lo, hi):
                s = int(a["aln_score"][t])
                if s == 0:
                    cover["a zero score ends a set's alignments"] += 1
                if s == 0 or s < int(a["aln_score"][lo]) * 0.8:
                    if s and any(int(x) >= int(a["aln_score"][lo]) * 0.8 for x in a["aln_score"][t + 1:hi]):
                        cover["just below 0.8: dropped, and a later higher one is not looked at"] += 1
                    break
                if t > lo and s == int(a["aln_score"][lo]) * 0.8:
                    cover["a second alignment at exactly 0.8 of the first is kept"] += 1
                items.append((s, j, t - lo, int(a["aln_mappings"][t])))
        if not items:
            cover["nothing kept: one unaligned entry"] += 1
            items = [(0, capi.FUNNEL_NONE, capi.FUNNEL_NONE, 0)]
        if len(items) > pol.max_multimaps:
            cover["more kept than max_multimaps"] += 1
        rng = None if rng_state is None else Minstd(rng_state[r], a["reads"][int(a["read_off"][r]):int(a["read_off"][r + 1])])
        order, _, fate = walk(len(items), lambda i: -items[i][0], lambda i: float(items[i][0]), 0.0, 1, pol.max_multimaps, rng, lambda i, below: True, cover, "max_multimaps")
        if rng is not None:
            rng_state[r] = rng.x
        scores.append([items[i][0] for i in order]); picks.append([items[i][1:3] for i in order])
        n_reported[r] = sum(1 for i in order if fate[i] == "taken"); unmapped[r] = items[order[0]][3] == 0
    score_off = np.concatenate([[0], np.cumsum([len(s) for s in scores])]).astype(np.uint64)
    reported = np.zeros(int(score_off[-1]), dtype=capi.FUNNEL_PICK_DT)
    flat = [p for ps in picks for p in ps]
    reported["set"] = [p[0] for p in flat]; reported["alignment"] = [p[1] for p in flat]
    return dict(score_off=score_off, scores=np.array([s for ss in scores for s in ss], dtype=np.int32), reported=reported, n_reported=n_reported, unmapped=unmapped,
                written=int(score_off[-1]))


# ---- the corpus -----------------------------------------------------------------------------------------------------------------------------------------
def read_of(L, mins, clusters, rng, **hints):
    return dict(L=L, seq=rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), L), mins=mins, clusters=clusters, **hints)


def edge_reads(rng, lim):
    flat8 = [(0, 10, s) for s in (6.0, 4.0, 5.0, 0.5, 3.0, 1.0, 3.5, 2.5)]        # eight minimizers over the same ten bases: equal coverage, chosen scores
    e = []
    e.append(read_of(100, [(0, 11, 1.5), (5, 11, 2.0), (89, 11, 1.25)], [[0, 0, 1], [2], [1, 2, 2]], rng))                     # one minimizer twice; overlap; the last base
    e.append(read_of(120, [(28, 11, 1.5), (60, 11, 2.0), (100, 20, 1.0)], [[0], [1], [0, 1, 2]], rng))                       # bits 32 and 64
    e.append(read_of(400, [(6 * j, 11, 1.0 + j / 64) for j in range(65)], [[3, 64], [64], [0, 63]], rng))                    # 65 minimizers
    e.append(read_of(60, [(3, 11, 1.0)], [], rng)); e.append(read_of(50, [], [], rng))                                      # no cluster
    for _ in range(3):                                                                                                      # beyond every limit
        M = lim[0] + 5
        e.append(read_of(3 * M + 20, [(3 * j, 11, 1.0 + (j % 7) / 8) for j in range(M)], [[0, M - 1], [5, 6, 7], [M - 2]], rng))
        L = lim[1] + 37
        e.append(read_of(L, [(0, 11, 1.0), (L - 11, 11, 2.0), (L // 2, 31, 1.5)], [[0, 1], [2], [1, 2]], rng))
        C = lim[2] + 3
        e.append(read_of(200, [(5 * j, 11, 1.0 + (j % 5) / 4) for j in range(30)], [[j % 30, (7 * j + 1) % 30] for j in range(C)], rng, big_set=lim[3] + 4))
    e.append(read_of(40, [(0, 15, 1.0), (15, 15, 1.0), (0, 10, 1.0), (20, 10, 1.0)], [[0, 1], [1, 0], [2, 3]], rng))        # 0.75, 0.75, 0.5: exactly at the cutoff, fails
    e.append(read_of(40, [(0, 15, 1.0), (15, 15, 1.0), (0, 10, 1.0), (20, 10, 1.0)], [[0, 1], [2, 3]], rng))                # 0.75, 0.5: the minimum takes it
    for second in ([2, 3], [4], [1]):                                                                                       # best 10; second 5.5 inside, 3 outside, 4 on the pad
        e.append(read_of(40, flat8, [[0, 1], second, [4], [5], [3]], rng))
    e.append(read_of(40, flat8, [[0, 1], [2, 6], [2, 4], [5]], rng))                                                         # second 8.5 above the cutoff
    e.append(read_of(80, [(0, 10, 3.0)] * 10, [[j] for j in range(10)], rng, ext_score=40))                                  # ten equal clusters, ten good sets: the ninth fails by count
    e.append(read_of(80, [(0, 10, 3.0)] * 3, [[0], [1], [2]], rng, ext_score=30))                                             # a three-wide tie all the way down
    e.append(read_of(80, [(0, 10, 3.0), (20, 10, 3.0)], [[0], [0, 1]], rng))
    # refused, each for its own reason
    e.append(read_of(60, [(3, 11, 1.0)], [[0, 1]], rng, refused=True))                                                       # a source beyond the read's minimizers
    e.append(read_of(60, [(50, 11, 1.0)], [[0]], rng, refused=True))                                                         # a k-mer that leaves the read
    e.append(read_of(0, [], [[]], rng, refused=True))                                                                       # length 0 with a cluster
    e.append(read_of(60, [(3, 11, float("nan"))], [[0]], rng, refused=True)); e.append(read_of(60, [(3, 11, float("inf"))], [], rng, refused=True))
    return e


def random_reads(rng, count):
    out = []
    for _ in range(count):
        L = int(rng.integers(30, 401))
        offs = np.sort(rng.choice(L - 11, size=min(L - 11, int(rng.integers(0, max(2, L // 10)))), replace=False)) if L > 12 else []
        style = rng.integers(0, 3)
        mins = []
        for o in offs:
            length = int(min(L - o, rng.choice([11, 11, 11, 17, 29])))
            score = float(rng.choice([1.0, 1.5, 2.25, 3.0])) if style == 0 else 1.0 + float(np.log(500.0)) - float(np.log(float(rng.integers(1, 500)))) if style == 1 else 2.0
            mins.append((int(o), length, score))
        clusters = []
        for _ in range(int(rng.integers(0, 7)) if mins else 0):
            if clusters and rng.random() < 0.3:
                clusters.append(list(clusters[int(rng.integers(0, len(clusters)))]))                     # a twin: tied in coverage and score
            else:
                clusters.append([int(x) for x in rng.integers(0, len(mins), size=int(rng.integers(1, 7)))])
        out.append(read_of(L, mins, clusters, rng))
    return out


def flatten(reads):
    n = len(reads)
    a = dict(read_off=np.zeros(n + 1, dtype=np.uint64), minimizer_off=np.zeros(n + 1, dtype=np.uint64), cluster_off=np.zeros(n + 1, dtype=np.uint64))
    mins, seed_off, sources = [], [0], []
    for r, rd in enumerate(reads):
        a["read_off"][r + 1] = a["read_off"][r] + rd["L"]; a["minimizer_off"][r + 1] = a["minimizer_off"][r] + len(rd["mins"]); a["cluster_off"][r + 1] = a["cluster_off"][r] + len(rd["clusters"])
        mins += rd["mins"]
        for c in rd["clusters"]:
            sources += c; seed_off.append(len(sources))
    a["reads"] = np.concatenate([rd["seq"] for rd in reads]).astype(np.uint8)
    a["minimizers"] = np.zeros(len(mins), dtype=capi.READ_MINIMIZER_DT)
    a["minimizers"]["offset"] = [m[0] for m in mins]; a["minimizers"]["reserved"] = [m[1] for m in mins]; a["minimizers"]["hits"] = 1
    a["minimizers"]["key"] = np.arange(len(mins))
    a["minimizer_score"] = np.array([m[2] for m in mins], dtype=np.float64)
    a["cluster_seed_off"] = np.array(seed_off, dtype=np.uint64); a["sources"] = np.array(sources, dtype=np.uint32)
    return a


def make_sets(rng, reads, a, kept_off, kept, lim):
    """a gapless result per kept cluster: mostly a few extensions in read order, some full-length, empty or failed; five reads spoilt, each in its own way"""
    res = np.zeros(len(kept), dtype=capi.GAPLESS_RESULT_DT); ext = []
    spoil = {}
    candidates = [r for r in range(len(reads)) if kept_off[r + 1] > kept_off[r] and reads[r]["L"] > 40 and "ext_score" not in reads[r] and "big_set" not in reads[r]]
    for what, r in zip(("kept beyond", "range beyond", "leaves the read", "empty", "unsorted"), candidates[7::41]):
        spoil[r] = what
    read_of_set = np.repeat(np.arange(len(reads)), np.diff(kept_off.astype(np.int64)))
    for s, r in enumerate(read_of_set):
        L = reads[r]["L"]; first = s == int(kept_off[r])
        res[s]["ext_begin"] = len(ext)
        roll = rng.random()
        if r in spoil and first:
            mine = [(2, 20, 9), (10, 30, 9)]
        elif "ext_score" in reads[r]:
            mine = [(0, 30, reads[r]["ext_score"])]
        elif "big_set" in reads[r] and first:
            mine = [(3 * j, 3 * j + 8, 5 + j % 4) for j in range(reads[r]["big_set"])]
        elif roll < 0.08:
            res[s]["status"] = -3; res[s]["n_ext"] = 7; res[s]["ext_begin"] = 0xfffffff0
            continue
        elif roll < 0.16:
            mine = []
        elif roll < 0.26:
            res[s]["full_length"] = 1
            mine = [(0, L, L - 4 * int(rng.integers(0, 4))), (0, L, L - 16)][:int(rng.integers(1, 3))]
        else:
            begins = np.sort(rng.integers(0, L - 1, size=int(rng.integers(1, 5))))
            mine = [(int(b), int(rng.integers(b + 1, L + 1)), 0) for b in begins]
            mine = [(b, e, int(rng.integers(1, e - b + 6)) if rng.random() < 0.8 else 25) for b, e, _ in mine]
        if spoil.get(r) and first and len(mine) >= (2 if spoil[r] == "unsorted" else 1) and not res[s]["full_length"]:
            b, e, sc = mine[0]
            if spoil[r] == "leaves the read":
                mine[0] = (b, L + 1, sc)
            elif spoil[r] == "empty":
                mine[0] = (b, b, sc)
            elif spoil[r] == "unsorted":
                mine = [(mine[-1][0] + 1, L, 9)] + mine[1:]
            spoil[r] += " (done)"
        res[s]["n_ext"] = len(mine)
        ext += mine
    extensions = np.zeros(len(ext), dtype=capi.EXT_DT)
    extensions["read_begin"] = [x[0] for x in ext]; extensions["read_end"] = [x[1] for x in ext]; extensions["score"] = [x[2] for x in ext]
    kept = kept.copy()
    for r, what in spoil.items():
        if what.startswith("kept beyond"):
            kept[int(kept_off[r])] = len(a["cluster_seed_off"]) + 3
        if what.startswith("range beyond"):
            res[int(kept_off[r])]["status"] = 0; res[int(kept_off[r])]["ext_begin"] = len(ext) - 1; res[int(kept_off[r])]["n_ext"] = 3; res[int(kept_off[r])]["full_length"] = 0
    return dict(results=res, extensions=extensions, kept=kept, spoilt=sorted(r for r, w in spoil.items() if w.endswith("(done)")))


def make_alignments(rng, aligned_off, lim):
    menu = [(50, 40), (50, 39, 45), (0,), (50, 0, 45), (60, 59), (33,), (), (45, 45)]
    off, score = [0], []
    for j in range(int(aligned_off[-1])):
        pick = menu[int(rng.integers(0, len(menu)))] if rng.random() < 0.5 else tuple(sorted((int(x) for x in rng.integers(20, 90, size=int(rng.integers(1, 3)))), reverse=True))
        score += pick; off.append(len(score))
    score = np.array(score, dtype=np.int32)
    return dict(aln_off=np.array(off, dtype=np.uint64), aln_score=score, aln_mappings=(rng.random(len(score)) < 0.9).astype(np.uint32) * 3)


CLUSTER_ARGS = ("reads", "read_off", "minimizer_off", "minimizers", "minimizer_score", "cluster_off", "cluster_seed_off", "sources")
SET_ARGS = ("reads", "read_off", "set_off", "results", "extensions", "kept_off", "kept", "cluster_seed_off", "sources", "minimizer_off")
WINNER_ARGS = ("reads", "read_off", "aligned_off", "aln_off", "aln_score", "aln_mappings")


def args(a, names):
    return [a[k] for k in names]


@pytest.fixture(scope="module")
def corpus():
    """per policy and with / without generators: the three calls' inputs, chained through this file's own statement, with its answers; the cover counts"""
    lim = limits()
    rng = np.random.default_rng(20261020)
    reads = edge_reads(rng, lim) + random_reads(rng, 2000)
    base = flatten(reads)
    n = len(reads)
    cover = collections.Counter()
    runs = []
    for name, pol in policies().items():
        for with_rng in (True, False):
            a = dict(base)
            state = np.zeros(n, dtype=np.uint32) if with_rng else None
            before1 = None if state is None else state.copy()
            want1 = own_clusters(pol, a, state, cover)
            a.update(kept_off=want1["kept_off"], set_off=want1["kept_off"], **make_sets(np.random.default_rng(5), reads, a, want1["kept_off"], want1["kept"], lim))
            before2 = None if state is None else state.copy()
            want2 = own_sets(pol, a, state, cover)
            a.update(aligned_off=want2["aligned_off"], **make_alignments(np.random.default_rng(6), want2["aligned_off"], lim))
            before3 = None if state is None else state.copy()
            want3 = own_winners(pol, a, state, cover)
            runs.append(dict(name="%s, %s generators" % (name, "with" if with_rng else "without"), pol=pol, a=a, before=(before1, before2, before3),
                             after=None if state is None else state.copy(), want=(want1, want2, want3)))
    refused = np.array([bool(rd.get("refused")) for rd in reads])
    return dict(reads=reads, runs=runs, cover=cover, refused=refused, lim=lim)


def same(got, want, what):
    """every field of every output, the doubles by their bits"""
    for key, w in want.items():
        g = got[key]
        if isinstance(w, np.ndarray):
            assert len(g) == len(w) and g.tobytes() == np.ascontiguousarray(w, dtype=g.dtype).tobytes(), (what, key, np.nonzero(g != np.ascontiguousarray(w, dtype=g.dtype))[0][:5])
        else:
            assert g == w, (what, key, g, w)


def three_calls(run, clusters, sets, winners, what):
    """the three calls of one run through one implementation, each from the states the statement entered it with -> nothing; asserts against run['want']"""
    a, pol, before = run["a"], run["pol"], run["before"]
    state = None if before[0] is None else before[0].copy()
    rc, got = clusters(pol, a, state)
    assert rc == OK and got["sizing_rc"] in (OK, EOPS), (what, rc)
    same(got, run["want"][0], what + ": clusters")
    assert state is None or (state == before[1]).all(), what
    rc, got = sets(pol, a, state)
    assert rc == OK, (what, rc)
    same(got, run["want"][1], what + ": sets")
    assert state is None or (state == before[2]).all(), what
    rc, got = winners(pol, a, state)
    assert rc == OK, (what, rc)
    same(got, run["want"][2], what + ": winners")
    assert state is None or (state == run["after"]).all(), what


def shim_calls():
    h = pipeline._host_lib()
    t = (ctypes.c_int(4),)
    return (lambda pol, a, st: capi.funnel_clusters_call(h.vgh_funnel_clusters, (), pol, *args(a, CLUSTER_ARGS), rng_state=st, tail=t),
            lambda pol, a, st: capi.funnel_extension_sets_call(h.vgh_funnel_extension_sets, (), pol, *args(a, SET_ARGS), rng_state=st, between=(ctypes.c_int(GO), ctypes.c_int(GE)), tail=t),
            lambda pol, a, st: capi.funnel_winners_call(h.vgh_funnel_winners, (), pol, *args(a, WINNER_ARGS), rng_state=st, tail=t))


def serial_calls():
    d = ctypes.CDLL(DRIVER)
    return (lambda pol, a, st: capi.funnel_clusters_call(d.vgt_funnel_clusters_serial, (), pol, *args(a, CLUSTER_ARGS), rng_state=st),
            lambda pol, a, st: capi.funnel_extension_sets_call(d.vgt_funnel_extension_sets_serial, (), pol, *args(a, SET_ARGS), rng_state=st, between=(ctypes.c_int32(GO), ctypes.c_int32(GE))),
            lambda pol, a, st: capi.funnel_winners_call(d.vgt_funnel_winners_serial, (), pol, *args(a, WINNER_ARGS), rng_state=st))


def engine_calls(eng):
    return (lambda pol, a, st: capi.funnel_clusters_call(eng.lib.vgk_funnel_clusters, (eng.h,), pol, *args(a, CLUSTER_ARGS), rng_state=st),
            lambda pol, a, st: capi.funnel_extension_sets_call(eng.lib.vgk_funnel_extension_sets, (eng.h,), pol, *args(a, SET_ARGS), rng_state=st),
            lambda pol, a, st: capi.funnel_winners_call(eng.lib.vgk_funnel_winners, (eng.h,), pol, *args(a, WINNER_ARGS), rng_state=st))


COVERED = """two seeds of one minimizer, counted once|overlapping k-mers: a union|a k-mer ending at the read's last base|a k-mer straddling bit 32 of the bitmap
a k-mer straddling bit 64 of the bitmap|present bits that cross a word|a cluster of one seed|a read with no cluster|an item exactly at best - threshold fails
threshold 0: nothing fails|the minimum filled by an item below the cutoff|a skipped item that does not count towards the minimum|max_alignments: fails by count
max_extensions: fails by count|max_multimaps: fails by count|a 2-wide top tie with rng_state|a 2-wide top tie without rng_state|a 3-wide top tie with rng_state
a 3-wide top tie without rng_state|a tie in coverage broken by score|ties below the top left in index order|rng_state carried from one call into the next
the second best inside the pad|the second best outside the pad|the second best exactly on the pad|the cluster score filter fires
the cluster score filter waits for min_extensions|a full-length set|an empty set|a failed gapless result|a set to chain
an estimate below extension_set_min_score admitted by the minimum and still discarded|a minimizer only in a kept-but-not-aligned cluster is not explored
a minimizer in two clusters, one of them aligned, is explored|a second alignment at exactly 0.8 of the first is kept
just below 0.8: dropped, and a later higher one is not looked at|a zero score ends a set's alignments|nothing kept: one unaligned entry|more kept than max_multimaps"""


def test_the_corpus_holds_every_case(corpus):
    for case in COVERED.replace("\n", "|").split("|"):
        assert corpus["cover"][case] >= 1, case
    lim, reads = corpus["lim"], corpus["reads"]
    assert sum(len(rd["mins"]) > lim[0] for rd in reads) >= 3 and sum(rd["L"] > lim[1] for rd in reads) >= 3 and sum(len(rd["clusters"]) > lim[2] for rd in reads) >= 3
    main = corpus["runs"][0]
    assert (np.diff(main["a"]["kept_off"].astype(np.int64)) > lim[2]).sum() >= 3                       # a set walk beyond the limit
    assert ((main["a"]["results"]["status"] == 0) & (main["a"]["results"]["n_ext"] > lim[3])).sum() >= 3      # an estimate beyond the limit
    ninth = [r for r, rd in enumerate(reads) if rd.get("ext_score") == 40][0]
    v = main["want"][1]["sets"][int(main["a"]["kept_off"][ninth]):int(main["a"]["kept_off"][ninth + 1])]["verdict"]
    assert len(v) == 10 and (v == capi.FUNNEL_SET_ALIGN).sum() == 8 and (v == capi.FUNNEL_SET_FAIL_MAX_ALIGNMENTS).sum() == 2      # the ninth good set fails by count
    # one read per refusal, and only those; the spoilt sets likewise
    assert corpus["refused"].sum() == 5 and ((main["want"][0]["status"] == EINVAL) == corpus["refused"]).all()
    assert len(main["a"]["spoilt"]) == 5 and (np.nonzero(main["want"][1]["status"] == EINVAL)[0] == main["a"]["spoilt"]).all()
    with_rng, without = corpus["runs"][0], corpus["runs"][1]
    assert (with_rng["after"] != 0).sum() > 50 and (with_rng["want"][0]["clusters"]["rank"] != without["want"][0]["clusters"]["rank"]).any()


def test_the_shim_equals_the_statement_in_another_shape(corpus):
    for run in corpus["runs"]:
        three_calls(run, *shim_calls(), what="shim, " + run["name"])


def test_the_serial_device_rule_equals_the_shim(corpus):
    """through the statement both are held to: every integer, and both doubles bit for bit"""
    for run in corpus["runs"]:
        three_calls(run, *serial_calls(), what="serial, " + run["name"])


def winners_beyond_the_limit(lim):
    """three reads whose kept alignments outnumber the walk's LDS items, one with nothing aligned"""
    rng = np.random.default_rng(12)
    sets = [lim[2] // 2 + 3, 0, lim[2] + 1, lim[2] // 2 + 9]
    aligned_off = np.concatenate([[0], np.cumsum(sets)]).astype(np.uint64)
    score = np.stack([rng.integers(60, 70, size=int(aligned_off[-1])), rng.integers(50, 60, size=int(aligned_off[-1]))], axis=1).astype(np.int32).reshape(-1)
    return dict(reads=rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 4 * 50), read_off=np.arange(5, dtype=np.uint64) * 50, aligned_off=aligned_off,
                aln_off=np.arange(int(aligned_off[-1]) + 1, dtype=np.uint64) * 2, aln_score=score, aln_mappings=np.ones(len(score), dtype=np.uint32))


def test_a_winner_walk_beyond_the_limit(corpus):
    a = winners_beyond_the_limit(corpus["lim"]); pol = policies()["zero thresholds"]
    want = own_winners(pol, a, np.zeros(4, dtype=np.uint32), collections.Counter())
    assert (np.diff(want["score_off"].astype(np.int64)) > corpus["lim"][2]).sum() == 3
    for calls in (shim_calls(), serial_calls()):
        rc, got = calls[2](pol, a, np.zeros(4, dtype=np.uint32))
        assert rc == OK
        same(got, want, "winners beyond the limit")


def malformed_calls(a, pol):
    """(name, which call, changed arguments, policy, states given without reads) -> each must answer VGK_EINVAL, the last VGK_ETOOBIG"""
    bad = lambda key: {key: np.concatenate([a[key][:2][::-1], a[key][2:]]) if a[key][1] else np.concatenate([[1], a[key][1:]]).astype(np.uint64)}
    out = [("read_off that does not ascend", 0, bad("read_off"), pol), ("minimizer_off", 0, bad("minimizer_off"), pol), ("cluster_off from 1", 0, dict(cluster_off=a["cluster_off"] + np.uint64(1)), pol),
           ("cluster_seed_off", 0, bad("cluster_seed_off"), pol)]
    for field in ("cluster_score_threshold", "pad_cluster_score_threshold", "cluster_coverage_threshold", "extension_set_score_threshold"):
        p = capi.FunnelPolicy.from_buffer_copy(pol); setattr(p, field, float("nan") if field[0] == "c" else float("inf"))
        out.append((field + " not finite", 0, {}, p))
    p = capi.FunnelPolicy.from_buffer_copy(pol); p.flags = 2
    out.append(("unknown flags", 1, {}, p))
    shifted = a["set_off"].copy(); shifted[1] += 1
    out.append(("set_off that disagrees with kept_off", 1, dict(set_off=shifted), pol))
    out.append(("generators without reads", 2, dict(reads=None), pol))
    p = capi.FunnelPolicy.from_buffer_copy(pol); p.max_multimaps = 0
    out.append(("no mapping allowed", 2, {}, p))
    return out


def hold_malformed(run, calls, n_reads):
    a, pol = run["a"], run["pol"]
    names = (CLUSTER_ARGS, SET_ARGS, WINNER_ARGS)
    for name, which, changed, p in malformed_calls(a, pol):
        b = dict(a); b.update(changed)
        rc, _ = calls[which](p, b, np.zeros(n_reads, dtype=np.uint32) if "generators" in name else None)
        assert rc == EINVAL, (name, rc)
    huge = dict(a, read_off=np.array([0, 1 << 32], dtype=np.uint64), minimizer_off=np.zeros(2, dtype=np.uint64), cluster_off=np.zeros(2, dtype=np.uint64))
    rc, _ = calls[0](pol, huge, None)
    assert rc == capi.VGK_ETOOBIG
    del names


def test_malformed_calls_are_refused_by_the_serial_rule_s_checks(corpus):
    hold_malformed(corpus["runs"][1], serial_calls(), len(corpus["reads"]))


def frame(path, which, arrays):
    with open(path, "wb") as f:
        f.write(np.array([which, len(arrays)], dtype=np.uint64).tobytes())
        for x in arrays:
            raw = b"" if x is None else np.ascontiguousarray(x).tobytes()
            f.write(np.array([x is not None, len(raw)], dtype=np.uint64).tobytes()); f.write(raw + b"\0" * (-len(raw) % 8))


def unframe(path):
    raw = open(path, "rb").read()
    count = int(np.frombuffer(raw[8:16], dtype=np.uint64)[0]); at = 16; out = []
    for _ in range(count):
        size = int(np.frombuffer(raw[at + 8:at + 16], dtype=np.uint64)[0])
        out.append(raw[at + 16:at + 16 + size]); at += 16 + size + (-size % 8)
    return out


def test_the_serial_rule_under_the_host_sanitizers(corpus, tmp_path):
    """the driver as a program of its own under -fsanitize=address,undefined over the corpus' edge reads, the refused ones among them, and the winner walk beyond
    the limit: sized with capacity 0, run with exactly the capacity asked for — the statement's answers, nothing reported"""
    subprocess.check_call(["make", "-s", "readfunnel_san"], cwd=ROOT)
    program = os.path.join(ROOT, "tests", "emu", "read_funnel_san")
    reads = [rd for rd in corpus["reads"][:len(edge_reads(np.random.default_rng(0), corpus["lim"])) + 150]]
    a = flatten(reads); n = len(reads); pol = policies()["main"]; word = lambda *v: np.array(v, dtype=np.uint64)

    def run(which, arrays):
        frame(tmp_path / "call.bin", which, arrays)
        done = subprocess.run([program, str(tmp_path / "call.bin"), str(tmp_path / "answer.bin")], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "", done.stderr[-2000:]
        return unframe(tmp_path / "answer.bin")
    for with_rng in (True, False):
        state = np.zeros(n, dtype=np.uint32) if with_rng else None
        entering = None if state is None else state.copy()
        want = own_clusters(pol, a, state, collections.Counter())
        got = run(0, [bytes(pol), word(n)] + args(a, CLUSTER_ARGS) + [entering])
        rcs = np.frombuffer(got[0], dtype=np.int64)
        assert rcs[0] == EOPS and rcs[1] == OK and rcs[2] == want["written"]
        assert got[1] == want["clusters"].tobytes() and got[2] == want["status"].tobytes() and got[3] == want["kept_off"].tobytes() and got[4] == want["kept"].tobytes()
        assert state is None or got[5] == state.tobytes()
        a.update(kept_off=want["kept_off"], set_off=want["kept_off"], **make_sets(np.random.default_rng(5), reads, a, want["kept_off"], want["kept"], corpus["lim"]))
        entering = None if state is None else state.copy()
        want = own_sets(pol, a, state, collections.Counter())
        got = run(1, [bytes(pol), word(n, GO, GE, len(a["extensions"]), len(a["cluster_seed_off"]) - 1, int(a["minimizer_off"][-1]))] + args(a, SET_ARGS[:7])
                  + [a["cluster_seed_off"], a["sources"], a["minimizer_off"], entering])
        rcs = np.frombuffer(got[0], dtype=np.int64)
        assert rcs[1] == OK and rcs[2] == want["written"] and (want["status"] == EINVAL).sum() >= 1
        assert got[1] == want["sets"].tobytes() and got[2] == want["status"].tobytes() and got[3] == want["aligned_off"].tobytes() and got[4] == want["aligned"].tobytes()
        assert got[5] == want["explored"].tobytes() and (state is None or got[6] == state.tobytes())
        a.update(aligned_off=want["aligned_off"], **make_alignments(np.random.default_rng(6), want["aligned_off"], corpus["lim"]))
        for b in (a, winners_beyond_the_limit(corpus["lim"])):
            m = len(b["read_off"]) - 1
            st = None if state is None else (state.copy() if b is a else np.zeros(m, dtype=np.uint32))
            entering = None if st is None else st.copy()
            want = own_winners(pol, b, st, collections.Counter())
            got = run(2, [bytes(pol), word(m)] + args(b, WINNER_ARGS) + [entering])
            rcs = np.frombuffer(got[0], dtype=np.int64)
            assert rcs[0] == EOPS and rcs[1] == OK and rcs[2] == want["written"]
            assert got[1] == want["score_off"].tobytes() and got[2] == want["scores"].tobytes() and got[3] == want["reported"].tobytes()
            assert got[4] == want["n_reported"].tobytes() and got[5] == want["unmapped"].tobytes() and (st is None or got[6] == st.tobytes())
    # a call refused as a whole: the program answers its verdict and touches nothing
    got = run(0, [bytes(pol), word(n)] + args(dict(a, cluster_off=a["cluster_off"] + np.uint64(1)), CLUSTER_ARGS) + [None])
    assert np.frombuffer(got[0], dtype=np.int64)[1] == EINVAL


def test_the_entry_points_are_the_engine_library_s_own():
    engine_h = open(os.path.join(ROOT, "include", "vgk_engine.h")).read(); vgk_h = open(os.path.join(ROOT, "include", "vgk.h")).read()
    lib = ctypes.CDLL(ENGINE)
    for name in ("vgk_funnel_clusters", "vgk_funnel_extension_sets", "vgk_funnel_winners", "vgk_funnel_limits", "vgk_funnel_last_ms", "vgk_funnel_last_launches"):
        assert name + "(" in engine_h and name + "(" not in vgk_h and hasattr(lib, name), name
    assert all(hasattr(pipeline._host_lib(), name) for name in ("vgh_funnel_clusters", "vgh_funnel_extension_sets", "vgh_funnel_winners"))
    lib.vgk_abi_version.restype = ctypes.c_int
    assert lib.vgk_abi_version() == 6 and min(limits()) >= 1
    assert "PARITY-UNPINNED" in engine_h[engine_h.index("a short read's funnel"):engine_h.index("vgk_funnel_last_launches")]


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    return capi.Engine(capi.Scoring.simple(1, 4, GO, GE, 5), lib=ENGINE, device=0)


@pytest.mark.gpu
def test_the_engine_equals_the_shim_in_every_field(corpus, gpu):
    """through the statement both are held to, the doubles bit for bit (covered compared exactly among them); both launches of every pair used"""
    for run in corpus["runs"]:
        three_calls(run, *engine_calls(gpu), what="engine, " + run["name"])
    run = corpus["runs"][0]; a, pol = run["a"], run["pol"]
    rc, got = engine_calls(gpu)[0](pol, a, None)
    in_lds, over_slab, refused = gpu.funnel_last_launches()
    assert rc == OK and in_lds > 1000 and over_slab >= 9 and refused == 5 and gpu.funnel_last_ms()[0] > 0
    rc, got = engine_calls(gpu)[1](pol, a, None)
    in_lds, over_slab, refused = gpu.funnel_last_launches()
    assert rc == OK and in_lds > 1000 and over_slab >= 3 and refused == 5 and gpu.funnel_last_ms()[1] > 0


@pytest.mark.gpu
def test_the_engine_s_winner_walk_beyond_the_limit_and_its_sizing(corpus, gpu):
    a = winners_beyond_the_limit(corpus["lim"]); pol = policies()["zero thresholds"]
    state = np.zeros(4, dtype=np.uint32)
    want = own_winners(pol, a, state.copy(), collections.Counter())
    rc, got = engine_calls(gpu)[2](pol, a, state)
    assert rc == OK and got["sizing_rc"] == EOPS and gpu.funnel_last_launches() == (1, 3, 0) and gpu.funnel_last_ms()[2] > 0
    same(got, want, "winners beyond the limit")
    # the sizing calls with capacity 0 answer the same written[] as the calls that fill
    run = corpus["runs"][0]
    for which, names, key in ((0, CLUSTER_ARGS, "kept"), (1, SET_ARGS, "aligned")):
        fn = (capi.funnel_clusters_call, capi.funnel_extension_sets_call)[which]
        lib_fn = (gpu.lib.vgk_funnel_clusters, gpu.lib.vgk_funnel_extension_sets)[which]
        rc, sized = fn(lib_fn, (gpu.h,), run["pol"], *args(run["a"], names), cap=0)
        assert rc == EOPS and sized["written"] == run["want"][which]["written"] > 0 and (sized[key + "_off"] == run["want"][which][key + "_off"]).all()


@pytest.mark.gpu
def test_the_engine_refuses_malformed_calls_and_takes_an_empty_one(corpus, gpu):
    hold_malformed(corpus["runs"][1], engine_calls(gpu), len(corpus["reads"]))
    run = corpus["runs"][1]; a = run["a"]
    empty = {k: (v[:1] if k.endswith("_off") else v[:0]) for k, v in a.items() if isinstance(v, np.ndarray)}
    for which, names in enumerate((CLUSTER_ARGS, SET_ARGS, WINNER_ARGS)):
        rc, got = engine_calls(gpu)[which](run["pol"], empty, None)
        assert rc == OK and got["written"] == 0, which


class ShimFunnel:
    """the host shim in the engine's place for the three funnel calls of pipeline.read_funnel"""

    def __init__(self):
        self.h, self.t = pipeline._host_lib(), (ctypes.c_int(4),)

    def funnel_clusters(self, policy, *rest, cap=None):
        return capi.funnel_clusters_call(self.h.vgh_funnel_clusters, (), policy, *rest[:-1], rng_state=rest[-1], tail=self.t, cap=cap)

    def funnel_extension_sets(self, policy, *rest, cap=None):
        return capi.funnel_extension_sets_call(self.h.vgh_funnel_extension_sets, (), policy, *rest[:-1], rng_state=rest[-1], between=(ctypes.c_int(GO), ctypes.c_int(GE)), tail=self.t, cap=cap)

    def funnel_winners(self, policy, *rest, cap=None):
        return capi.funnel_winners_call(self.h.vgh_funnel_winners, (), policy, *rest[:-1], rng_state=rest[-1], tail=self.t, cap=cap)


def clusters_by_diagonal(wl, seeded, n, apart=60):
    """any partition will do: a read's seeds sorted by (strand, diagonal on the concatenated nodes), cut where two neighbours lie more than `apart` apart"""
    node_start = np.concatenate([[0], np.cumsum([len(s) for s in wl.nodes])]).astype(np.int64)
    seeds = seeded["seeds"]; moff = seeded["minimizer_off"].astype(np.int64); soff = seeded["seed_off"].astype(np.int64)
    diagonal = node_start[seeds["node"].astype(np.int64) >> 1] - seeds["diff"].astype(np.int64)
    strand = seeds["node"].astype(np.int64) & 1
    cluster_off, cluster_seed_off, cluster_seeds = [0], [0], []
    for r in range(n):
        lo, hi = int(soff[moff[r]]), int(soff[moff[r + 1]])
        mine = sorted(range(lo, hi), key=lambda j: (int(strand[j]), int(diagonal[j])))
        count = 0
        for at, j in enumerate(mine):
            if at and (strand[j] != strand[mine[at - 1]] or diagonal[j] - diagonal[mine[at - 1]] > apart):
                cluster_seed_off.append(len(cluster_seeds)); count += 1
            cluster_seeds.append(j)
        if mine:
            cluster_seed_off.append(len(cluster_seeds)); count += 1
        cluster_off.append(cluster_off[-1] + count)
    return np.array(cluster_off, dtype=np.uint64), np.array(cluster_seed_off, dtype=np.uint64), np.array(cluster_seeds, dtype=np.int64)


@pytest.mark.gpu
def test_end_to_end_the_route_with_clusters_given_equals_the_same_chain_over_the_shim():
    """500 reads on a 20 kbp graph through pipeline.read_funnel, clusters cut by diagonal: verdicts, explored, scores and vgk_read_mapq's quality are those of
    the same chain with the host shim answering the three funnel calls; and the route matters: some read's explored minimizers are not the all-seeds guess"""
    import util
    from vg_amd import workloads
    h = util.host(); h.vgh_log_base.restype = ctypes.c_double; h.vgh_log_base.argtypes = [ctypes.c_void_p]
    aligner = util.HostAligner(util.ORACLE_LIB)                       # (kept: the scorer lives as long as this object)
    log_base = h.vgh_log_base(aligner.ptr)
    wl = workloads.GaplessWorkload(500, seed=33, graph_bp=20000, inserted_reads=0.3)
    n = wl.gs.n
    rng = np.random.default_rng(4)
    quality = rng.integers(10, 40, len(wl.gs.reads)).astype(np.uint8)
    eng = capi.Engine(capi.Scoring.simple(1, 4, GO, GE, 5), lib=ENGINE, device=0)
    index = eng.haplo_index(wl.nodes, wl.threads); mindex = eng.minimizer_index(wl.nodes, wl.threads, k=29, w=11)
    seeded = pipeline.seed_long_reads(eng, mindex, wl.gs.reads, wl.gs.read_off, 29, choice="device")
    cluster_off, cluster_seed_off, cluster_seeds = clusters_by_diagonal(wl, seeded, n)
    assert (np.diff(cluster_off.astype(np.int64)) >= 2).sum() > 20
    pol = capi.FunnelPolicy.giraffe(29)
    got_state, want_state = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    common = (eng, index, wl.gs.reads, wl.gs.read_off, seeded, cluster_off, cluster_seed_off, cluster_seeds, pol, quality, 29, 11, log_base)
    got = pipeline.read_funnel(*common, rng_state=got_state)
    want = pipeline.read_funnel(*common, rng_state=want_state, funnel=ShimFunnel())
    for key in ("clusters", "cluster_status", "kept_off", "kept", "sets", "set_status", "aligned_off", "aligned", "explored", "score_off", "scores", "reported", "n_reported", "unmapped"):
        assert got[key].tobytes() == want[key].tobytes(), key
    assert (got_state == want_state).all() and got["mapq"].tobytes() == want["mapq"].tobytes() and (got["mapq"]["status"] == 0).all()
    guess = ((np.asarray(seeded["take"]) != 0) & (seeded["minimizers"]["hits"] > 0)).astype(np.uint8)
    print("clusters %d, kept %d, aligned %d; explored %d against the all-seeds guess' %d; mapq 60: %d, below: %d" % (
        len(got["clusters"]), len(got["kept"]), len(got["aligned"]), got["explored"].sum(), guess.sum(), (got["mapq"]["mapq"] == 60).sum(), (got["mapq"]["mapq"] < 60).sum()))
    assert (got["clusters"]["verdict"] != capi.FUNNEL_EXTEND).any() and len(got["aligned"]) >= n // 2
    assert (guess != got["explored"]).any()
