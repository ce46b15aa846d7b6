"""vgk_pair_mapq (include/vgk_engine.h): a pair's mapping qualities on the device — the candidate pairings' scores, their order with the max_multimaps cut, the
multiplicities of rescued pairs, the pair's uncapped quality, the fragment-cluster cap, the two mates' explored caps summed, the unpaired cap, the halving for
unreachable mates and max(min(capped, 120) / 2, 0) (MinimizerMapper::map_paired, src/minimizer_mapper.cpp:2476-2765; score_alignment_pair :6017-6028).

The pins, from the outside in: a plain Python statement of the rule, written here from those lines, against the host shim (vgh_pair_mapq: the reference's loop
shape over vectors, MappingQualityCalculator, read_mapq's cap for the mates); the serial statement of the device rule (pm_candidate_score / pm_pair_one of
vg_amd/csrc/pair_mapq_device.hpp, behind tests/emu/pair_mapq_driver.cpp) against the shim byte for byte in every output; the shim's quality of a single candidate
against vgh_compute_mapping_quality; and the engine against the shim: status, n_chosen and the pair scores bit for bit, the order equal, the caps to 1e-12 (the
device library's log10), the integers equal except on the pairs the shim's own doubles put within reach of a truncation boundary (set_aside), where they may
differ by 1.

set_aside reads "capped / 2 within 1e-6 of an integer" for the values a library can move: those whose capped quality came from a cap (a double made with
log10).  Where the capped quality is the pair's integer-valued uncapped quality itself (halved or not), the clamp at 120 or a zero, capped / 2 is exact in
both libraries — it sits ON an integer by construction and truncates alike — and such a pair is set aside only through its uncapped quality's own boundary."""
import collections
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import util
from vg_amd import capi, pipeline, workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = os.path.join(ROOT, "vg_amd", "libvgamd.so")
DRIVER = os.path.join(ROOT, "tests", "emu", "libvgamd_pairmapq.so")
INT32_MAX, INT64_MAX = capi.INT32_MAX, capi.INT64_MAX
QUALITY_SCALE = 10.0 / math.log(10.0)
LOWEST = -sys.float_info.max


# ---- the plain statement of the rule --------------------------------------------------------------------------------------------------------------------
def add_log(x, y):
    return x + math.log1p(math.exp(y - x)) if x > y else y + math.log1p(math.exp(x - y))


def max_mapping_quality(scaled, mult=None):
    """MappingQualityCalculator::maximum_mapping_quality_exact (src/mapping_quality_calculator.cpp:26-139) and compute_max_mapping_quality's (int32_t)"""
    log_sum_exp = to_score = LOWEST
    for i in reversed(range(len(scaled))):
        score = scaled[i]
        if score >= to_score:
            to_score = score
        if mult is not None and mult[i] > 1.0:
            score += math.log(mult[i])
        log_sum_exp = add_log(log_sum_exp, score)
    if len(scaled) == 1 and (mult is None or mult[0] <= 1.0):
        log_sum_exp = add_log(log_sum_exp, 0.0)
    p = math.exp(to_score - log_sum_exp)
    if p >= 1.0:
        return INT32_MAX                                              # log1p(-1): infinite
    return int(-QUALITY_SCALE * math.log1p(-p))


def python_rule(scheme, a, caps, mate_stopped):
    """The rule of include/vgk_engine.h over a call's arrays.  caps: the 2 n explored caps; mate_stopped: bool per read -> (results, pair_score, order)"""
    coff = a["cand_off"].astype(np.int64); cands = a["candidates"]; n = len(coff) - 1
    out = np.zeros(n, dtype=capi.PAIR_MAPQ_RESULT_DT); pair_score = np.zeros(len(cands)); order = np.zeros(len(cands), dtype=np.uint32)
    lb, mean, sd = scheme.log_base, scheme.fragment_mean, scheme.fragment_sd
    uoff = a["unpaired_off"].astype(np.int64)
    for j, c in enumerate(cands.tolist()):
        (s0, s1), distance, _, _, t, aligned, _ = c
        if t > 3:
            continue
        if t in (2, 3) and not (aligned >> (1 if t == 2 else 0)) & 1:
            pair_score[j] = float(s0 if t == 2 else s1)
            continue
        dev = float(INT64_MAX if t == 1 else distance) - mean
        ll = (-dev * dev / (2.0 * sd * sd)) / lb
        pair_score[j] = max(float(s0 + s1) + ll, float(min(s0, s1)))
    for p in range(n):
        lo, hi = int(coff[p]), int(coff[p + 1]); C = hi - lo
        cs = cands[lo:hi].tolist(); counts = a["counts"][p]
        order[lo:hi] = np.arange(C)
        attempts = [min(int(counts["rescued_count"][r]), scheme.max_rescue_attempts) for r in (0, 1)]
        bad = mate_stopped[2 * p] or mate_stopped[2 * p + 1]
        for (_, distance, _, _, t, aligned, _) in cs:
            bad = bad or t > 3 or (t in (2, 3) and (attempts[t - 2] == 0 or (not (aligned >> (3 - t)) & 1 and distance != INT64_MAX)))
        if bad:
            out["status"][p] = capi.VGK_EINVAL
            continue
        s = pair_score[lo:hi]
        ranked = sorted(range(C), key=lambda i: -s[i])                # (sorted is stable: ties in candidate order)
        order[lo:hi] = ranked
        o = out[p]
        o["n_chosen"] = min(C, scheme.max_multimaps)
        o["explored_cap"] = caps[2 * p:2 * p + 2]
        o["fragment_cluster_cap"] = math.inf; o["score_group"] = INT32_MAX
        if not C:
            continue
        types = [cs[i][4] for i in ranked]
        found_pair = 0 in types
        est = lambda r: int(counts["unpaired_count"][r]) / attempts[r] if counts["unpaired_count"][r] > 0 else 1.0
        mult = None if found_pair else [est(t - 2) if t in (2, 3) else 1.0 for t in types]
        scores = [s[i] for i in ranked]
        uncapped = 0 if scores[0] == 0 else max_mapping_quality([lb * x for x in scores], mult)
        win = cs[ranked[0]]
        if win[3] > 1:
            o["fragment_cluster_cap"] = -10.0 * math.log10(1.0 - 1.0 / win[3])
        unreachable = win[4] == 1 or win[1] == INT64_MAX
        for r in (0, 1):
            if found_pair:
                group = [scores[0]]
                if win[4] == 0:
                    group += [s[j] for j in range(C) if j != ranked[0] and cs[j][4] == 0 and cs[j][2][r] == win[2][r]]
                o["score_group"][r] = max_mapping_quality([lb * x for x in group])
            bonus = 2.0 if uncapped == INT32_MAX else 1.0
            cap = min(o["fragment_cluster_cap"], (caps[2 * p] + caps[2 * p + 1]) * bonus)
            if win[4] == 1:
                alone = a["unpaired_scores"][int(uoff[2 * p + r]):int(uoff[2 * p + r + 1])]
                cap = min(cap, max_mapping_quality([lb * float(x) for x in alone]))
            o["applied_cap"][r] = cap
            capped = min(cap, uncapped)
            if unreachable:
                capped = capped / 2.0
            o["mapq"][r] = int(max(min(capped, 120.0) / 2.0, 0.0)) if (win[5] >> r) & 1 else 0
        o["uncapped"] = uncapped
    return out, pair_score, order


# ---- the corpus and the three statements ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_aligner():
    h = util.host()
    h.vgh_log_base.restype = ctypes.c_double; h.vgh_log_base.argtypes = [ctypes.c_void_p]
    h.vgh_compute_mapping_quality.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_int, ctypes.c_int]
    h.vgh_read_mapq_direct.restype = ctypes.c_double
    h.vgh_read_mapq_direct.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    al = util.HostAligner(util.ORACLE_LIB)
    return h, al, h.vgh_log_base(al.ptr)


def shim_pairs(scheme, a):
    return capi.pair_mapq_call(pipeline._host_lib().vgh_pair_mapq, (), scheme, tail=(ctypes.c_int(4),), **a)


def serial_pairs(scheme, a):
    return capi.pair_mapq_call(ctypes.CDLL(DRIVER).vgt_pair_mapq_serial, (), scheme, **a)


def shim_mate_caps(wl, quality=True):
    """the mates' explored caps and verdicts by the shim of vgk_read_mapq (no scores: the unmapped byte)"""
    m = wl.mates; n = len(m["read_off"]) - 1
    a = dict(score_off=np.zeros(n + 1, dtype=np.uint64), scores=np.zeros(0, dtype=np.int32), minimizer_off=m["minimizer_off"], minimizers=m["minimizers"], regions=m["regions"],
             explored=m["explored"], read_off=m["read_off"], quality=m["quality"] if quality else None, unmapped=np.ones(n, dtype=np.uint8))
    rc, out = capi.read_mapq_call(pipeline._host_lib().vgh_read_mapq, (), capi.ReadMapqScheme(wl.log_base, 1.0, 0, wl.k, 0, 0), tail=(ctypes.c_int(4),), **a)
    assert rc == 0
    return a, out


@pytest.fixture(scope="module")
def corpus(host_aligner):
    """PairMapqWorkload with the scorer's log base, and per variant the shim's answer"""
    wl = workloads.PairMapqWorkload(log_base=host_aligner[2])
    per_variant = []
    for v in wl.variants:
        rc, want, score, order = shim_pairs(wl.scheme(v), wl.arrays(v))
        assert rc == 0, v
        per_variant.append((v, want, score, order))
    return wl, per_variant


def same_bytes(got, want):
    return all(np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes() for g, w in zip(got, want))


def multiplicities(wl, scheme):
    """per candidate its multiplicity under :2660-2685, and per pair whether they are used (no PAIRED candidate)"""
    cands = wl.candidates; pair_of = np.repeat(np.arange(wl.n), np.diff(wl.cand_off.astype(np.int64)))
    attempts = np.minimum(wl.counts["rescued_count"], scheme.max_rescue_attempts).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        est = np.where(wl.counts["unpaired_count"] > 0, wl.counts["unpaired_count"] / attempts, 1.0)
    t = cands["type"].astype(np.int64)
    mult = np.where((t == 2) | (t == 3), est[pair_of, np.clip(t - 2, 0, 1)], 1.0)
    has_paired = np.bincount(pair_of, weights=(t == 0), minlength=wl.n) > 0
    return mult, ~has_paired


BY_SCORE = {}                                                         # per workload: the pairs at a boundary of the uncapped quality


def set_aside(h, wl, v, want, score, order):
    """The pairs whose integers may differ by 1 between two correct libraries, from the shim's own doubles alone: the pre-truncation uncapped quality within
    1e-3 of an integer below 121, the sum of exp(other - best) in [5e-15, 5e-14] (the edge of the infinite case) — or, for either mate, capped / 2 within 1e-6
    of an integer where a cap made it (see the module's docstring).  -> (aside, the share under the literal reading of the third condition)"""
    scheme = wl.scheme(v)
    key = (id(wl), scheme.max_rescue_attempts)
    cache = BY_SCORE
    if key not in cache:                                              # the quality's own boundaries do not depend on the variant
        mult, used = multiplicities(wl, scheme)
        coff = wl.cand_off.astype(np.int64); by_score = np.zeros(wl.n, dtype=bool)
        for p in range(wl.n):
            lo, hi = int(coff[p]), int(coff[p + 1])
            if hi == lo or p in wl.refusals:
                continue
            ranked = order[lo:hi].astype(np.int64)
            s = np.ascontiguousarray(wl.log_base * score[lo:hi][ranked])
            if s[0] == 0:
                continue
            m = np.ascontiguousarray(mult[lo:hi][ranked]) if used[p] else None
            others = ctypes.c_double()
            direct = h.vgh_read_mapq_direct(s.ctypes.data, len(s), None if m is None else m.ctypes.data, 0, ctypes.byref(others))
            by_score[p] = (direct < 121 and abs(direct - round(direct)) < 1e-3) or 5e-15 <= others.value <= 5e-14
        cache[key] = by_score
    aside = cache[key].copy()
    ok = (want["status"] == 0) & (want["n_chosen"] > 0)
    winner = order[wl.cand_off[:-1].astype(np.int64).clip(max=len(order) - 1)].astype(np.int64) + wl.cand_off[:-1].astype(np.int64)
    win = wl.candidates[winner.clip(max=len(wl.candidates) - 1)]
    unreachable = (win["type"] == 1) | (win["distance"] == INT64_MAX)
    literal = aside.copy()
    for r in (0, 1):
        cap = want["applied_cap"][:, r]; capped = np.minimum(cap, want["uncapped"])
        capped = np.where(unreachable, capped / 2.0, capped)
        pre = np.maximum(np.minimum(capped, 120.0) / 2.0, 0.0)
        at_integer = ok & np.isfinite(pre) & (np.abs(pre - np.round(pre)) < 1e-6)
        literal |= at_integer
        aside |= at_integer & (cap < want["uncapped"]) & (capped > 0) & (capped < 120)
        # ... and where a cap lies within a library's reach of the uncapped quality, which of the two is applied is the library's to say
        with np.errstate(invalid="ignore"):
            aside |= at_integer & np.isfinite(cap) & (cap != np.round(cap)) & (np.abs(cap - want["uncapped"]) <= 1e-9 * np.maximum(np.abs(want["uncapped"]), 1.0))
    return aside & (want["status"] == 0), float((literal & (want["status"] == 0)).mean())


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_shim_equals_a_plain_statement_of_the_rule(corpus):
    wl, per_variant = corpus
    _, mate = shim_mate_caps(wl)
    for v, want, score, order in per_variant:
        scheme = wl.scheme(v); a = wl.arrays(v)
        stopped = np.zeros(2 * wl.n, dtype=bool)
        if scheme.flags & capi.PAIR_MAPQ_NO_EXPLORED_CAP or (v["caps"] == "computed" and not v.get("quality", True)):
            caps = np.full(2 * wl.n, np.inf)
        elif v["caps"] == "given":
            caps = wl.given_cap
        else:
            caps = mate["explored_cap"]; stopped = mate["status"] != 0
        got, got_score, got_order = python_rule(scheme, a, caps, stopped)
        assert (got_score == score).all(), v["name"]                  # IEEE basic operations only: Python's doubles are the shim's
        assert (got_order == order).all(), (v["name"], np.nonzero(got_order != order)[0][:5])
        for name in ("status", "n_chosen", "mapq"):
            assert (got[name] == want[name]).all(), (v["name"], name, np.nonzero(got[name] != want[name])[0][:5])
        for name in ("uncapped", "fragment_cluster_cap", "explored_cap", "score_group", "applied_cap"):
            g, w = got[name], want[name]
            with np.errstate(invalid="ignore"):                       # (infinity - infinity, where both are infinite and equal)
                same = (g == w) | (np.abs(g - w) <= 1e-9 * np.maximum(np.abs(w), 1.0))
            assert same.all() and (np.signbit(g) == np.signbit(w))[g == 0].all(), (v["name"], name, np.nonzero(~same)[0][:5])
        refused = wl.stops(v)
        assert sorted(np.nonzero(want["status"])[0]) == sorted(refused) and (want["status"][sorted(refused)] == capi.VGK_EINVAL).all(), v["name"]
        blank = want[sorted(refused)].copy(); blank["status"] = 0
        assert blank.tobytes() == bytes(len(blank.tobytes())), v["name"]


def test_the_serial_statement_equals_the_shim_byte_for_byte(corpus):
    wl, per_variant = corpus
    for v, want, score, order in per_variant:
        rc, got, got_score, got_order = serial_pairs(wl.scheme(v), wl.arrays(v))
        assert rc == 0 and got_score.tobytes() == score.tobytes() and got_order.tobytes() == order.tobytes(), v["name"]
        assert got.tobytes() == want.tobytes(), (v["name"], np.nonzero([x.tobytes() != y.tobytes() for x, y in zip(got, want)])[0][:5])


def test_the_corpus_reaches_what_the_rule_must_reach(corpus):
    wl, per_variant = corpus
    by_name = {v["name"]: (v, want, score, order) for v, want, score, order in per_variant}
    assert 19000 <= wl.n <= 21000
    reach = collections.Counter()
    coff = wl.cand_off.astype(np.int64); C = np.diff(coff); limit = 64
    v, want, score, order = by_name["given caps, four mappings"]
    ok = want["status"] == 0
    for c in list(range(9)) + [limit - 1, limit, limit + 1]:
        reach["%d candidates" % c] = int((ok & (C == c)).sum())
    reach["several hundred candidates"] = int((ok & (C >= 300)).sum())
    cands = wl.candidates
    first = np.clip(coff[:-1], 0, len(cands) - 1)
    winner = first + order[first].astype(np.int64)
    win = cands[winner]; has = ok & (C > 0)
    for t, name in enumerate(("PAIRED", "UNPAIRED", "RESCUED_FROM_FIRST", "RESCUED_FROM_SECOND")):
        reach["a winner of type " + name] = int((has & (win["type"] == t)).sum())
    pair_of = np.repeat(np.arange(wl.n), C)
    n_paired = np.bincount(pair_of, weights=cands["type"] == 0, minlength=wl.n); n_rescued = np.bincount(pair_of, weights=cands["type"] >= 2, minlength=wl.n)
    mult, used = multiplicities(wl, wl.scheme(v))
    big = np.bincount(pair_of, weights=mult > 1.0, minlength=wl.n) > 0
    reach["rescued candidates only, a multiplicity above 1 in use"] = int((has & (n_rescued == C) & big).sum())
    reach["mixed: multiplicities ignored"] = int((has & (n_paired > 0) & (n_rescued > 0) & big).sum())
    floor = (cands["type"] != 1) & (cands["distance"] != INT64_MAX) & (cands["aligned"] == 3) & (score == cands["score"].min(axis=1)) & (cands["score"].min(axis=1) > 0)
    reach["the likelihood pushes the sum below the worse mate's score"] = int(floor.sum())
    reach["a distance exactly at the mean"] = int((cands["distance"] == int(wl.mean)).sum())
    reach["a distance of INT64_MAX"] = int((cands["distance"] == INT64_MAX).sum())
    reach["an unreachable winner: the halving"] = int((has & (win["distance"] == INT64_MAX)).sum())
    rescued_mate_bit = np.where(cands["type"] == 2, 2, 1)
    unaligned = (cands["type"] >= 2) & (cands["type"] <= 3) & ((cands["aligned"] & rescued_mate_bit) == 0)
    is_winner = np.zeros(len(cands), dtype=bool); is_winner[winner[has]] = True
    reach["an unaligned rescued mate as winner"] = int((unaligned & is_winner & ok[pair_of]).sum())
    reach["an unaligned rescued mate as loser"] = int((unaligned & ~is_winner & ok[pair_of]).sum())
    assert (want["mapq"][pair_of[unaligned & is_winner & ok[pair_of]]].min(axis=1) == 0).all()
    ties = cut_ties = cut_ties_1 = 0
    for p in np.nonzero(has & (C >= 2))[0]:
        s = score[coff[p]:coff[p + 1]][order[coff[p]:coff[p + 1]]]
        ties += bool((s[1:] == s[:-1]).any())
        cut_ties += bool(C[p] > 4 and s[3] == s[4]); cut_ties_1 += bool(s[0] == s[1])
    reach["equal pair scores"] = ties
    reach["a tie at the cut of four mappings"] = cut_ties; reach["a tie at the cut of one mapping"] = cut_ties_1
    reach["a first score of 0"] = int((has & (score[winner] == 0) & (want["uncapped"] == 0)).sum())
    infinite = has & (want["uncapped"] == INT32_MAX)
    reach["an uncapped quality of INT32_MAX"] = int(infinite.sum())
    doubled = infinite & np.isinf(want["fragment_cluster_cap"]) & (win["type"] != 1) & np.isfinite(want["explored_cap"]).all(axis=1)
    reach["the escape bonus of 2"] = int(doubled.sum())
    assert (want["applied_cap"][doubled, 0] == 2.0 * want["explored_cap"][doubled].sum(axis=1)).all()
    reach["a finite uncapped quality above 0"] = int((has & (want["uncapped"] > 0) & (want["uncapped"] < INT32_MAX)).sum())
    for b in (0, 1, 2, 1000):
        reach["better_cluster_count %d" % b] = int((has & (win["better_cluster_count"] == b)).sum())
    assert np.isinf(want["fragment_cluster_cap"][has & (win["better_cluster_count"] <= 1)]).all()
    assert np.allclose(want["fragment_cluster_cap"][has & (win["better_cluster_count"] == 2)], -10 * math.log10(0.5))
    reach["the fragment-cluster cap applied"] = int((has & (want["applied_cap"][:, 0] == want["fragment_cluster_cap"]) & np.isfinite(want["fragment_cluster_cap"])).sum())
    reach["the unpaired cap applied"] = int((has & (win["type"] == 1) & (want["applied_cap"][:, 0] != want["applied_cap"][:, 1])).sum())
    reach["a score group of more than the winner"] = int((has & (want["score_group"] < INT32_MAX).any(axis=1) & (win["type"] == 0) & (C > 1)).sum())
    reach["a winner with an unaligned mate"] = int((has & (win["aligned"] != 3)).sum())
    reach["a quality of 60"] = int((want["mapq"] == 60).any(axis=1).sum()); reach["a quality strictly between 0 and 60"] = int(((want["mapq"] > 0) & (want["mapq"] < 60)).any(axis=1).sum())
    assert ((want["mapq"] >= 0) & (want["mapq"] <= 60)).all()
    for why in ("type above 3", "no rescue attempts", "unaligned rescued mate with a distance"):
        reach["refused: " + why] = sum(1 for p, w in wl.refusals.items() if w == why and want["status"][p] == capi.VGK_EINVAL)
    v, want, score, order = by_name["caps in the call"]
    reach["refused: a mate the sweep stops on"] = sum(1 for p in wl.mate_stops if p not in wl.refusals and want["status"][p] == capi.VGK_EINVAL)
    ok = want["status"] == 0
    nothing = (want["explored_cap"] == 0) & np.signbit(want["explored_cap"])
    reach["nothing explored on one mate: -0.0"] = int((ok & (nothing.sum(axis=1) == 1)).sum()); reach["nothing explored on both mates: -0.0"] = int((ok & nothing.all(axis=1)).sum())
    assert (want["mapq"][ok & nothing.all(axis=1)] == 0).all()
    reach["caps computed in the call"] = int((ok & np.isfinite(want["explored_cap"]).all(axis=1) & (want["explored_cap"] > 0).all(axis=1)).sum())
    v, want, _, _ = by_name["caps in the call, no qualities"]
    reach["without qualities: +infinity"] = int(np.isinf(want["explored_cap"][want["status"] == 0]).all() and v["max_multimaps"] == 1)
    v, want, _, _ = by_name["no explored cap"]
    reach["NO_EXPLORED_CAP: +infinity"] = int(np.isinf(want["explored_cap"][want["status"] == 0]).all())
    v, want, _, _ = by_name["given caps, one mapping"]
    reach["max_multimaps of 1 and of 4"] = int((want["n_chosen"] <= 1).all() and (want["n_chosen"] == 1).any() and (by_name["given caps, four mappings"][1]["n_chosen"] == 4).any())
    print(dict(reach))
    assert [what for what, count in reach.items() if count == 0] == [] and len(reach) == 52


def test_a_single_candidate_s_quality_is_the_calculator_s(corpus, host_aligner):
    wl, per_variant = corpus
    h, al, log_base = host_aligner
    v, want, score, order = per_variant[0]
    coff = wl.cand_off.astype(np.int64)
    singles = np.nonzero((np.diff(coff) == 1) & (want["status"] == 0))[0]
    _, used = multiplicities(wl, wl.scheme(v))
    checked = 0
    for p in singles:
        s = float(score[coff[p]])
        if s == 0 or (used[p] and wl.candidates["type"][coff[p]] >= 2):      # (vgh_compute_mapping_quality takes no multiplicities)
            continue
        assert h.vgh_compute_mapping_quality(al.ptr, (ctypes.c_double * 1)(s), 1, 0, 0) == want["uncapped"][p], p
        checked += 1
    assert checked > 1000


def test_few_pairs_lie_at_a_truncation_boundary(corpus, host_aligner):
    """a condition on the corpus, from the shim's doubles alone: at most 2 % of the pairs of any variant are set aside (by uniformity about 0.3 %)"""
    wl, per_variant = corpus
    for v, want, score, order in per_variant:
        aside, literal = set_aside(host_aligner[0], wl, v, want, score, order)
        print(v["name"], "set aside: %.4f; with every capped / 2 that sits on an integer, exact ones included: %.4f" % (aside.mean(), literal))
        assert aside.mean() <= 0.02, (v["name"], aside.mean())


def write_call(path, scheme, a):
    n = len(a["cand_off"]) - 1
    given, q = a.get("given_cap"), a.get("quality")
    empty_off = np.zeros(2 * n + 1, dtype=np.uint64)
    moff = a.get("minimizer_off", empty_off); roff = a.get("read_off", empty_off); mins = a.get("minimizers", np.zeros(0, dtype=capi.READ_MINIMIZER_DT))
    head = np.array([n, len(a["candidates"]), len(a["unpaired_scores"]), len(mins), int(roff[-1]), scheme.max_multimaps, scheme.max_rescue_attempts, scheme.k, scheme.flags, 1,
                     given is not None, q is not None], dtype=np.uint64)
    with open(path, "wb") as f:
        f.write(head.tobytes()); f.write(np.array([scheme.log_base, scheme.fragment_mean, scheme.fragment_sd], dtype=np.float64).tobytes())
        for arr, dt in ((a["cand_off"], np.uint64), (a["candidates"], capi.PAIR_CANDIDATE_DT), (a["counts"], capi.PAIR_COUNTS_DT), (a["unpaired_off"], np.uint64),
                        (a["unpaired_scores"], np.int32), (given, np.float64), (moff, np.uint64), (mins, capi.READ_MINIMIZER_DT),
                        (a.get("regions", np.zeros(0, dtype=capi.MINIMIZER_REGION_DT)), capi.MINIMIZER_REGION_DT), (a.get("explored", np.zeros(0, dtype=np.uint8)), np.uint8),
                        (roff, np.uint64), (q, np.uint8)):
            if arr is not None:
                f.write(np.ascontiguousarray(arr, dtype=dt).tobytes())


def test_the_serial_statement_under_the_host_sanitizers(corpus, tmp_path):
    """the driver as a program of its own under -fsanitize=address,undefined on the corpus: the driver library's bytes, nothing reported"""
    wl, per_variant = corpus
    subprocess.check_call(["make", "-s", "pairmapq_san"], cwd=ROOT)
    for v, want, score, order in per_variant:
        scheme = wl.scheme(v); a = wl.arrays(v)
        write_call(tmp_path / "call.bin", scheme, a)
        done = subprocess.run([os.path.join(ROOT, "tests", "emu", "pair_mapq_san"), str(tmp_path / "call.bin"), str(tmp_path / "answer.bin")], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "", done.stderr[-2000:]
        raw = open(tmp_path / "answer.bin", "rb").read()
        rc, out, got_score, got_order = serial_pairs(scheme, a)
        assert int(np.frombuffer(raw[:8], dtype=np.int64)[0]) == rc == 0
        assert raw[8:] == out.tobytes() + got_score.tobytes() + got_order.tobytes(), v["name"]
        assert out.tobytes() == want.tobytes()


def test_the_entry_points_are_the_engine_library_s_own():
    engine_h = open(os.path.join(ROOT, "include", "vgk_engine.h")).read(); vgk_h = open(os.path.join(ROOT, "include", "vgk.h")).read()
    lib = ctypes.CDLL(ENGINE)
    for name in ("vgk_pair_mapq", "vgk_pair_mapq_limits", "vgk_pair_mapq_last_ms", "vgk_pair_mapq_last_launches", "vgk_pair_mapq_last_kernel_launches"):
        assert name + "(" in engine_h and name + "(" not in vgk_h and hasattr(lib, name), name
    assert hasattr(pipeline._host_lib(), "vgh_pair_mapq")
    out = (ctypes.c_uint32 * 4)()
    assert lib.vgk_pair_mapq_limits(out) == 0 and out[0] >= 8 and out[1] == 1 and out[2] == 1


def test_the_kernels_use_no_scratch():
    """what DESIGN.md section 36 says of the kernels, read off the built library (tools/kernel_registers.py): no scratch memory, no spills, and LDS that leaves
    three workgroups of the pair kernel per CU (160 KiB / 3) — the three pair kernels and the two of the mates' cap-only sweep"""
    rows = []
    for pattern, count in (("pair_", 3), ("explored_cap", 2)):
        done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_registers.py"), ENGINE, pattern], capture_output=True, text=True)
        assert done.returncode == 0, done.stderr[-1000:]
        found = [line.split() for line in done.stdout.splitlines() if pattern in line]
        assert len(found) == count, found
        rows += found
    assert sorted(row[0].split("::")[-1] for row in rows[:3]) == ["pair_mapq_kernel", "pair_mapq_slab_kernel", "pair_score_kernel"]
    for row in rows:
        spills, scratch, lds = int(row[row.index("spills") + 1]), int(row[row.index("scratch") + 1]), int(row[row.index("lds") + 1])
        assert spills == 0 and scratch == 0 and lds <= 160 * 1024 // 3, row


def test_the_emulated_backend_says_unsupported(corpus):
    wl, per_variant = corpus
    if not os.path.exists(util.EMU_LIB):
        subprocess.check_call(["make", "-s", "emu"], cwd=ROOT)
    eng = capi.Engine(lib=util.EMU_LIB)
    for v in (wl.variants[0], wl.variants[2]):
        rc, _, _, _ = capi.pair_mapq_call(eng.lib.vgk_pair_mapq, (eng.h,), wl.scheme(v), **wl.arrays(v, [1, 2, 3]))
        assert rc == capi.VGK_EUNSUPPORTED, v["name"]


def test_the_candidates_made_from_a_paired_stage_answer():
    """pipeline.pair_mapq_inputs on hand cases: nodes of 10 columns each (node v begins at column 10 v), reads of 50 bases.  A mate's outer end is the column
    its first base lies at: forward on node v at offset o, 10 v + o; reverse (oriented node 2 v + 1), the node's end less the offset, 10 (v + 1) - o.  A
    rescued mate lies on the forward strand of its subgraph from (first node, first offset) over its aligned bases: its outer end is the alignment's end when
    its partner reads forward (it was aligned as its reverse complement), else its start."""
    class Graph:
        col = np.arange(0, 1010, 10, dtype=np.int64)

    class Wl:
        graph = Graph()
    res_dt = np.dtype([("status", "<i4"), ("n_ext", "<u4"), ("ext_begin", "<u4")]); ext_dt = np.dtype([("path_begin", "<u4"), ("path_len", "<u4"), ("offset", "<u4")])
    # reads:      0: fwd node 2 +3   1: rev node 40 +4   2: fwd node 5 +0   3: none   4: fwd node 10 +7   5: lost, rescued   6: lost, rescued   7: rev node 60 +1
    #             8: fwd node 3 +0   9: lost, rescue failed, no score of its own
    res = np.zeros(10, dtype=res_dt); ext = np.zeros(6, dtype=ext_dt); nodes = np.array([2 * 2, 2 * 40 + 1, 2 * 5, 2 * 10, 2 * 60 + 1, 2 * 3], dtype=np.uint32)
    for read, e in ((0, 0), (1, 1), (2, 2), (4, 3), (7, 4), (8, 5)):
        res["n_ext"][read] = 1; res["ext_begin"][read] = e
    res["status"][3] = -1
    ext["path_begin"] = np.arange(6); ext["path_len"] = 1; ext["offset"] = [3, 4, 0, 7, 1, 0]
    read_score = np.array([140, 150, 120, 0, 130, 20, 0, 145, 110, 0], dtype=np.int64)
    stage = dict(res=res, ext=ext, nodes=nodes, read_score=read_score, mapped=np.array([4, 7, 8]), rescued=np.array([5, 6, 9]),
                 rescue=np.array([[90, 0, 50, 2, 3, 48], [95, 0, 20, 5, 2, 50], [0, -1, -1, 0, 0, 0]], dtype=np.int64))      # score, status, first node, first offset, mappings, aligned bases
    a = pipeline.pair_mapq_inputs(stage, Wl())
    c = a["candidates"]
    assert (a["cand_off"] == np.arange(6)).all() and len(c) == 5
    # pair 0: both mates through the stage: 23 and 10 * 41 - 4 = 406
    assert c["type"][0] == capi.PAIR_PAIRED and c["distance"][0] == 406 - 23 and tuple(c["score"][0]) == (140, 150) and c["aligned"][0] == 3
    # pair 1: the second mate has nothing: no distance, not aligned
    assert c["type"][1] == capi.PAIR_PAIRED and c["distance"][1] == INT64_MAX and tuple(c["score"][1]) == (120, 0) and c["aligned"][1] == 1
    # pair 2: rescued from the first mate (forward at 107); the rescued alignment runs from 502 over 48 bases: its outer end is 550
    assert c["type"][2] == capi.PAIR_RESCUED_FROM_FIRST and c["distance"][2] == 550 - 107 and tuple(c["score"][2]) == (130, 90) and c["aligned"][2] == 3
    assert tuple(a["counts"]["rescued_count"][2]) == (1, 0)
    # pair 3: rescued from the second mate (reverse, outer end 10 * 61 - 1 = 609); the rescued mate reads forward from 205
    assert c["type"][3] == capi.PAIR_RESCUED_FROM_SECOND and c["distance"][3] == 609 - 205 and tuple(c["score"][3]) == (95, 145) and c["aligned"][3] == 3
    assert tuple(a["counts"]["rescued_count"][3]) == (0, 1)
    # pair 4: rescue found nothing and the stage had nothing: the rescued mate is not aligned, the distance unreachable — which the rule requires
    assert c["type"][4] == capi.PAIR_RESCUED_FROM_FIRST and c["distance"][4] == INT64_MAX and tuple(c["score"][4]) == (110, 0) and c["aligned"][4] == 1
    rc, out, score, _ = shim_pairs(capi.PairMapqScheme(1.3862943611198906, 400.0, 40.0, 1, 15, 29, 0), a)
    assert rc == 0 and (out["status"] == 0).all() and score[4] == 110.0 and score[1] == 0.0       # (the mapped mate's score; the floor: the worse mate's score)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    return capi.Engine(lib=ENGINE, device=0)


def engine_pairs(eng, scheme, a):
    return capi.pair_mapq_call(eng.lib.vgk_pair_mapq, (eng.h,), scheme, **a)


def doubles_agree(g, w):
    """infinities and zeros (with their sign) exactly, otherwise to 1e-12 relative"""
    special = np.isinf(w) | (w == 0) | np.isinf(g) | (g == 0)
    same_special = (g[special] == w[special]) & (np.signbit(g[special]) == np.signbit(w[special]))
    return same_special.all() and (np.abs(g[~special] - w[~special]) <= 1e-12 * np.maximum(np.abs(w[~special]), 1.0)).all()


def hold_to_the_shim(got, want, aside, what):
    """got, want: (results, pair_score, order).  status, n_chosen, pair_score bit for bit; order equal; the caps to 1e-12; uncapped, score_group and mapq equal —
    on the pairs set aside within 1"""
    (g, g_score, g_order), (w, w_score, w_order) = got, want
    assert (g["status"] == w["status"]).all(), (what, np.nonzero(g["status"] != w["status"])[0][:5])
    assert (g["n_chosen"] == w["n_chosen"]).all() and g_score.tobytes() == w_score.tobytes(), what
    assert (g_order == w_order).all(), (what, np.nonzero(g_order != w_order)[0][:5])
    for name in ("fragment_cluster_cap", "explored_cap"):
        assert doubles_agree(g[name].ravel(), w[name].ravel()), (what, name)
    # applied_cap is a cap where a cap made it, an integer where the unpaired quality did: a cap's tolerance, or the integers' rule below
    integer_cap = (w["applied_cap"] == np.round(w["applied_cap"])) & np.isfinite(w["applied_cap"]) & (w["applied_cap"] != 0)
    assert doubles_agree(g["applied_cap"][~integer_cap], w["applied_cap"][~integer_cap]), what
    assert (np.abs(g["applied_cap"][integer_cap] - w["applied_cap"][integer_cap]) <= aside[:, None].repeat(2, axis=1)[integer_cap]).all(), what
    for name in ("uncapped", "score_group", "mapq"):
        a, b = g[name].astype(np.float64).reshape(len(g), -1), w[name].astype(np.float64).reshape(len(w), -1)
        off = (a != b).any(axis=1)
        print(what, name, "differ on", int(off.sum()), "pairs, all set aside:", bool((aside | ~off).all()))
        assert (aside | ~off).all(), (what, name, np.nonzero(off & ~aside)[0][:5])
        both_finite = (a != INT32_MAX) & (b != INT32_MAX)
        assert (np.abs(a - b)[both_finite] <= 1).all(), (what, name)
        assert ((a == INT32_MAX) == (b == INT32_MAX))[~aside].all(), (what, name)


@pytest.mark.gpu
def test_the_engine_equals_the_shim_on_the_corpus(corpus, host_aligner, gpu):
    """Every variant: given caps and caps computed in the call.  The computed-cap call must also equal a vgk_read_mapq call followed by a given-cap call byte
    for byte — on every pair but those with a mate the sweep stops on, which only the one call can refuse (vgk_read_mapq hands a stopped read's cap on as 0)."""
    wl, per_variant = corpus
    for v, want, score, order in per_variant:
        rc, got, got_score, got_order = engine_pairs(gpu, wl.scheme(v), wl.arrays(v))
        assert rc == 0, v["name"]
        aside, _ = set_aside(host_aligner[0], wl, v, want, score, order)
        assert aside.mean() <= 0.02
        hold_to_the_shim((got, got_score, got_order), (want, score, order), aside, v["name"])
        launches = gpu.pair_mapq_last_launches(); C = np.diff(wl.cand_off.astype(np.int64))
        large = sum(1 for p in range(wl.n) if C[p] > 64 and p not in wl.refusals)
        assert launches == (wl.n - large - len(wl.refusals), large, len(wl.refusals)), (v["name"], launches)
        ms = gpu.pair_mapq_last_ms()
        assert ms[1] > 0 and (ms[0] > 0) == (v["caps"] == "computed" and v.get("quality", True))
        if v["name"] == "caps in the call":
            a, _ = shim_mate_caps(wl)
            rc, reads = capi.read_mapq_call(gpu.lib.vgk_read_mapq, (gpu.h,), capi.ReadMapqScheme(wl.log_base, 1.0, 0, wl.k, 0, 0), **a)
            assert rc == 0
            two = dict(wl.arrays(dict(v, caps="given")), given_cap=reads["explored_cap"])
            rc, then, then_score, then_order = engine_pairs(gpu, wl.scheme(v), two)
            assert rc == 0 and then_score.tobytes() == got_score.tobytes()
            stopped = (reads["status"] != 0).reshape(-1, 2).any(axis=1)
            assert sorted(np.nonzero(stopped)[0]) == sorted(wl.mate_stops) and (got["status"][stopped] == capi.VGK_EINVAL).all() and stopped.sum() > 10
            assert got[~stopped].tobytes() == then[~stopped].tobytes()
            keep = np.repeat(~stopped, C)
            assert got_order[keep].tobytes() == then_order[keep].tobytes()


@pytest.mark.gpu
def test_every_limit_from_both_sides(corpus, host_aligner, gpu):
    """the launches' edges — a launch of one pair, the slab launch alone, refused pairs beside slab pairs — held to the shim exactly as the whole corpus is"""
    wl, per_variant = corpus
    limit = gpu.pair_mapq_limits()[0]
    assert limit == 64                                                # (the workload plants its pairs around this size)
    below, exact, beyond = (wl.special["%d candidates" % c] for c in (limit - 1, limit, limit + 1))
    hundreds = [wl.special["%d candidates" % c] for c in (300, 450, 600)]
    refused = sorted(wl.refusals)
    for v, want, score, order in (per_variant[1], per_variant[2]):
        coff = wl.cand_off.astype(np.int64)
        aside, _ = set_aside(host_aligner[0], wl, v, want, score, order)
        for pairs, launches in (([below], (1, 0, 0)), ([exact], (1, 0, 0)), ([beyond], (0, 1, 0)), ([below, exact, beyond], (2, 1, 0)), ([0], (1, 0, 0)), ([0, 1, 2] + hundreds, (3, 3, 0)),
                                (refused, (0, 0, len(refused))), (refused[:2] + [beyond, 7], (1, 1, 2))):
            rc, got, got_score, got_order = engine_pairs(gpu, wl.scheme(v), wl.arrays(v, pairs))
            assert rc == 0 and len(got) == len(pairs)
            assert gpu.pair_mapq_last_launches() == launches, (pairs, gpu.pair_mapq_last_launches())
            idx = np.concatenate([np.arange(coff[p], coff[p + 1]) for p in pairs]).astype(np.int64)
            hold_to_the_shim((got, got_score, got_order), (want[pairs], score[idx], order[idx]), aside[pairs], "%s, pairs %s" % (v["name"], pairs))
            n_first = launches[0] + launches[2]                       # (a refused pair rides in the first pair launch)
            swept = v["caps"] == "computed"
            sweep_launches, pair_launches = gpu.pair_mapq_last_kernel_launches()
            assert pair_launches == int(len(idx) > 0) + int(n_first > 0) + int(launches[1] > 0), (pairs, pair_launches)
            assert (sweep_launches >= 1) == swept and sweep_launches <= 2, (pairs, sweep_launches)
    v = wl.variants[0]
    # n = 0
    empty = dict(cand_off=np.zeros(1, dtype=np.uint64), candidates=np.zeros(0, dtype=capi.PAIR_CANDIDATE_DT), counts=np.zeros(0, dtype=capi.PAIR_COUNTS_DT))
    rc, got, _, _ = engine_pairs(gpu, wl.scheme(v), empty)
    assert rc == 0 and len(got) == 0 and gpu.pair_mapq_last_launches() == (0, 0, 0) and gpu.pair_mapq_last_kernel_launches() == (0, 0)
    # the call's own refusals
    for field, value in (("flags", 2), ("log_base", 0.0), ("log_base", math.inf), ("fragment_sd", 0.0), ("fragment_sd", math.nan), ("fragment_mean", math.inf)):
        bad = wl.scheme(v); setattr(bad, field, value)
        assert engine_pairs(gpu, bad, wl.arrays(v, [7]))[0] == capi.VGK_EINVAL, field
    a = wl.arrays(v, [7, 8]); a["cand_off"] = a["cand_off"].copy(); a["cand_off"][1] = a["cand_off"][2] + np.uint64(1)
    assert engine_pairs(gpu, wl.scheme(v), a)[0] == capi.VGK_EINVAL
    a = wl.arrays(v, [7, 8]); a["cand_off"] = a["cand_off"].copy(); a["cand_off"][0] = 1
    assert engine_pairs(gpu, wl.scheme(v), a)[0] == capi.VGK_EINVAL
    a = wl.arrays(v, [7, 8]); a["unpaired_off"] = a["unpaired_off"] + np.uint64(1)
    assert engine_pairs(gpu, wl.scheme(v), a)[0] == capi.VGK_EINVAL


@pytest.mark.gpu
def test_end_to_end_the_gaf_lines_of_both_mates_carry_the_shim_s_quality(host_aligner):
    """2 000 pairs of the configs[3]-shaped workload with qualities: paired_stage (seeding, extension, tails, mate rescue) -> pipeline.pair_mapq, one candidate
    per pair from the stage's read_score, the fragment distance from the workload's column coordinates, the mates' caps swept inside the call -> gaf_lines over
    the composed alignments of the same reads; column 12 of each mate's first line is the shim's value for that mate (the set-aside rule as above)"""
    h, al, log_base = host_aligner
    wl = workloads.PairedWorkload(2000, ref_len=300_000, seed=5, hard=0.25)
    rng = np.random.default_rng(3)
    level = np.repeat(rng.choice(np.array([6, 14, 24, 34]), wl.n), wl.read_len)      # a read's own quality level, so that the caps spread
    quality = (level + rng.integers(0, 8, len(wl.reads))).astype(np.uint8)
    eng = capi.Engine(capi.Scoring.simple(1, 4, 6, 1, 5), lib=ENGINE, device=0)
    graph = (wl.node_len, wl.seq)
    index = eng.haplo_index(graph, wl.threads); mindex = eng.minimizer_index(graph, wl.threads, k=29, w=11)
    aligner = pipeline.HostAlignerHandle(ENGINE)
    stage = pipeline.paired_stage(eng, index, mindex, wl, aligner, oriented_len=np.repeat(wl.node_len, 2), device=True)
    # ... and the resident route's answer (the rescue half on the resident graph) makes the same candidates
    resident = aligner.rescue_graph(wl)
    stage_resident = pipeline.paired_stage(eng, index, mindex, wl, aligner, device=True, resident=resident)
    resident.close(); aligner.close()
    one, two = pipeline.pair_mapq_inputs(stage, wl), pipeline.pair_mapq_inputs(stage_resident, wl)
    assert one["candidates"].tobytes() == two["candidates"].tobytes() and one["counts"].tobytes() == two["counts"].tobytes() and (one["candidates"]["type"] >= 2).sum() > 100
    seeded = pipeline.seed_long_reads(eng, mindex, wl.reads, wl.read_off, 29, choice="device")
    details = {}
    mapq = pipeline.pair_mapq(eng, stage, wl, log_base, seeded=seeded, quality=quality, details=details)
    assert mapq.shape == (wl.n_pairs, 2)
    # the shim over the same inputs
    a = {name: details[name] for name in ("cand_off", "candidates", "counts", "minimizer_off", "minimizers", "regions", "explored", "read_off", "quality")}
    rc, want, score, order = shim_pairs(details["scheme"], a)
    assert rc == 0 and (want["status"] == 0).all() and score.tobytes() == details["pair_score"].tobytes()

    class View:                                                       # what set_aside reads of a workload
        pass
    view = View()
    view.n = wl.n_pairs; view.cand_off = a["cand_off"]; view.candidates = a["candidates"]; view.counts = a["counts"]; view.refusals = {}; view.log_base = log_base
    view.scheme = lambda v: details["scheme"]
    aside, _ = set_aside(h, view, {}, want, score, order)
    assert aside.mean() <= 0.02
    hold_to_the_shim((details["per_pair"], details["pair_score"], np.zeros(wl.n_pairs, dtype=np.uint32)), (want, score, order), aside, "end to end")
    # the lines: one composed alignment set per read, the read's quality on its first alignment
    moff = seeded["minimizer_off"].astype(np.int64)
    gs = capi.GaplessSet(wl.reads, wl.read_off, seeded["seeds"], seeded["seed_off"][moff])
    composed = pipeline.align_stage_device(eng, index, gs, composed=True, composed_policy=dict(window_length=39))["composed"]
    aln_off = composed["aln_off"].astype(np.int64); has = aln_off[:-1] < aln_off[1:]
    per_alignment = np.zeros(len(composed["alignments"]), dtype=np.int32)
    per_alignment[aln_off[:-1][has]] = mapq.ravel()[has]
    seqs, seq_off, results, aln_score = pipeline.read_alignments_gaf_view(wl.reads, wl.read_off, composed)
    node_off = np.concatenate([[0], np.cumsum(wl.node_len)]).astype(np.uint64)
    lines = pipeline.gaf_lines(seqs, seq_off, results, composed["mappings"], composed["edits"], wl.seq, node_off, mapq=per_alignment, score=aln_score)
    assert has.mean() > 0.9
    reads = np.nonzero(has)[0]
    column12 = np.array([int(lines[int(aln_off[r])].split(b"\t")[11]) for r in reads])
    shim = want["mapq"].ravel()[reads]
    differ = column12 != shim
    assert (column12 == mapq.ravel()[reads]).all() and (aside[reads // 2] | ~differ).all() and (np.abs(column12 - shim) <= 1).all()
    types = a["candidates"]["type"]
    print("pairs: %d PAIRED, %d rescued; quality below 60: %d, at 60: %d, at 0: %d" % ((types == 0).sum(), (types >= 2).sum(), (column12 < 60).sum(), (column12 == 60).sum(), (column12 == 0).sum()))
    assert (types == 0).sum() > 500 and (types >= 2).sum() > 100 and (column12 > 0).sum() > 1000 and len(set(column12.tolist())) > 5
