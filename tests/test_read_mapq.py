"""vgk_minimizer_regions and vgk_read_mapq (include/vgk_engine.h): a read's mapping quality on the device — the quality of its alignments' scores under
faster_cap over its explored minimizers, and the agglomerations that cap needs.

The pins, from the outside in: the reference's two unit tests of faster_cap (src/unittest/minimizer_mapper.cpp:154-252), already held by
tests/test_mapq_cap.py on vgh_faster_cap, are driven through the new entry points; the host shim (vgh_read_mapq: MappingQualityCalculator and faster_cap in
the reference's loop shape) must give vgh_faster_cap's cap and vgh_compute_mapping_quality's quality bit for bit; the serial statement of the device rule
(mq_read_one / mq_region_one of vg_amd/csrc/read_mapq_device.hpp, behind tests/emu/read_mapq_driver.cpp) must equal the shim bit for bit in all four output
fields — same libm, same operation order, no contraction; the agglomerations of shim and serial statement must equal a brute-force statement over every
window; and the engine must equal the shim: status always, the cap to 1e-12 (the device library's log10), the two integers exactly except on reads the
shim's own doubles put within reach of a rounding boundary (set_aside), where they may differ by 1."""
import collections
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import util
from vg_amd import capi, pipeline, workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = os.path.join(ROOT, "vg_amd", "libvgamd.so")
DRIVER = os.path.join(ROOT, "tests", "emu", "libvgamd_readmapq.so")
KW = [(5, 3), (11, 4), (29, 11), (31, 50)]
M64 = (1 << 64) - 1


# ---- the brute-force statement of the agglomerations --------------------------------------------------------------------------------------------------
def wang_hash_array(key):
    u = np.uint64
    with np.errstate(over="ignore"):
        key = ~key + (key << u(21)); key = key ^ (key >> u(24))
        key = key + (key << u(3)) + (key << u(8)); key = key ^ (key >> u(14))
        key = key + (key << u(2)) + (key << u(4)); key = key ^ (key >> u(28))
        return key + (key << u(31))


def brute_force(read, k, w, cover=None):
    """read: str.  For every window the leftmost smallest wang_hash among its valid k-mers (a k-mer stands for itself and its reverse complement: the smaller
    hash, forward on a tie), per instance the span of windows won -> [(offset, key, start, length)] in offset order"""
    L = len(read)
    if L < k + w - 1:
        return []
    code = np.full(256, -1, dtype=np.int64)
    code[[ord(c) for c in "ACGT"]] = [0, 1, 2, 3]
    c = code[np.frombuffer(read.encode(), dtype=np.uint8)]
    n = L - k + 1
    fwd = np.zeros(n, dtype=np.uint64); rev = np.zeros(n, dtype=np.uint64); valid = np.ones(n, dtype=bool)
    for i in range(k):
        x = c[i:i + n]
        valid &= x >= 0
        x = np.where(x < 0, 0, x).astype(np.uint64)
        fwd = fwd << np.uint64(2) | x; rev |= (np.uint64(3) - x) << np.uint64(2 * i)
    hf, hr = wang_hash_array(fwd), wang_hash_array(rev)
    h = np.where(hr < hf, hr, hf); key = np.where(hr < hf, rev, fwd)
    view = np.lib.stride_tricks.sliding_window_view
    leftmost_smallest = view(np.where(valid, h, np.uint64(M64)), w).argmin(axis=1) + np.arange(n - w + 1)      # (argmin: the first among equals)
    some_valid = view(valid, w).any(axis=1)
    spans = collections.OrderedDict()
    previous = None
    for s in range(L - k - w + 2):
        best = int(leftmost_smallest[s]) if some_valid[s] else None
        if best is None:
            if cover is not None:
                cover["a window with no valid k-mer"] += 1
            previous = None
            continue
        if best not in spans:
            spans[best] = [s, s]
            if cover is not None and previous is not None:
                cover["takes over by a smaller hash" if previous >= s else "takes over because its predecessor slid out"] += 1
        spans[best][1] = s
        previous = best
    out = [(j, int(key[j]), a, b + w + k - 1 - a) for j, (a, b) in spans.items()]
    if cover is not None and out and out[-1][2] + out[-1][3] == L:
        cover["an agglomeration that ends at the read's last base"] += 1
    return out


def region_corpus_reads(seed=7):
    rng = np.random.default_rng(seed)
    rand = lambda n: "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))
    reads = [rand(int(n)) for n in rng.integers(12, 401, 1960)]
    reads += [rand(k + w - 1) for k, w in KW] + [rand(k + w - 2) for k, w in KW]                      # exactly one window | none
    reads += ["A" * 100, "C" * 57 + rand(40), "ACAC" * 40, "T" * 400]                                 # runs of one base: equal hashes, the leftmost keeps the window
    for n_run in (1, 2, 5, 14, 33, 40, 90, 200):                                                      # N runs shorter and longer than a window
        body = list(rand(300)); a = int(rng.integers(0, 300 - n_run)); body[a:a + n_run] = "N" * n_run; reads.append("".join(body))
    reads += ["N" * 120, rand(60) + "N" * 100 + rand(60), "N" + rand(120) + "N"]
    for _ in range(12):                                                                               # lower case: no k-mer there, as the list call masks it
        body = rand(int(rng.integers(60, 300))); a = int(rng.integers(0, len(body) - 10)); reads.append(body[:a] + body[a:a + 7].lower() + body[a + 7:])
    while len(reads) < 1999:
        reads.append(rand(int(rng.integers(12, 401))))
    reads.append(rand(6000))
    return reads


@pytest.fixture(scope="module")
def region_corpus():
    """-> reads (flat, offsets), and per (k, w): the brute-force lists with their agglomerations, and what the corpus reaches"""
    reads = region_corpus_reads()
    assert len(reads) == 2000
    flat = np.frombuffer("".join(reads).encode(), dtype=np.uint8); off = np.concatenate([[0], np.cumsum([len(s) for s in reads])]).astype(np.uint64)
    per_kw = {}
    for k, w in KW:
        cover = collections.Counter()
        lists = [brute_force(s, k, w, cover) for s in reads]
        moff = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
        recs = np.zeros(int(moff[-1]), dtype=capi.READ_MINIMIZER_DT); want = np.zeros(int(moff[-1]), dtype=capi.MINIMIZER_REGION_DT)
        rows = [row for x in lists for row in x]
        recs["offset"] = [row[0] for row in rows]; recs["key"] = np.array([row[1] for row in rows], dtype=np.uint64)
        want["start"] = [row[2] for row in rows]; want["length"] = [row[3] for row in rows]
        per_kw[(k, w)] = (moff, recs, want, cover)
    return flat, off, per_kw


def shim_regions(flat, off, k, w, moff, recs):
    return capi.minimizer_regions_call(pipeline._host_lib().vgh_minimizer_regions, (), k, w, off, moff, recs,
                                       between=(ctypes.c_void_p(np.ascontiguousarray(flat).ctypes.data),), tail=(ctypes.c_int(4),))


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------------
def test_agglomerations_of_shim_and_serial_statement_are_the_brute_force_ones(region_corpus):
    flat, off, per_kw = region_corpus
    drv = ctypes.CDLL(DRIVER)
    reached = collections.Counter()
    for (k, w), (moff, recs, want, cover) in per_kw.items():
        rc, serial = capi.minimizer_regions_call(drv.vgt_minimizer_regions_serial, (), k, w, off, moff, recs)
        assert rc == 0 and (serial == want).all(), (k, w, np.nonzero(serial != want)[0][:5])
        rc, shim = shim_regions(flat, off, k, w, moff, recs)
        assert rc == 0 and (shim == want).all(), (k, w, np.nonzero(shim != want)[0][:5])
        # ... and workloads.read_minimizers, which makes the lists of ReadMapqWorkload, is the same statement
        m2, r2, g2, _ = workloads.read_minimizers(flat, off, k, w)
        assert (m2 == moff).all() and (r2["offset"] == recs["offset"]).all() and (r2["key"] == recs["key"]).all() and (g2 == want).all(), (k, w)
        reached.update(cover)
        # a read with no complete window has no minimizers; one of exactly k + w - 1 bases has one window
        lengths = np.diff(off.astype(np.int64)); counts = np.diff(moff.astype(np.int64))
        assert (counts[lengths < k + w - 1] == 0).all() and (lengths == k + w - 1).any()
    print(dict(reached))
    for what in ("takes over by a smaller hash", "takes over because its predecessor slid out", "a window with no valid k-mer", "an agglomeration that ends at the read's last base"):
        assert reached[what] > 0, what


def test_a_list_that_is_not_its_read_s_is_refused(region_corpus):
    flat, off, per_kw = region_corpus
    drv = ctypes.CDLL(DRIVER)
    moff, recs, _, _ = per_kw[(29, 11)]
    r = int(np.nonzero(np.diff(moff.astype(np.int64)) >= 2)[0][0]); j = int(moff[r])
    beyond = recs.copy(); beyond["offset"][j + 1] = int(off[r + 1] - off[r]) - 28
    swapped = recs.copy(); swapped["offset"][j], swapped["offset"][j + 1] = recs["offset"][j + 1], recs["offset"][j]
    for bad in (beyond, swapped):
        assert capi.minimizer_regions_call(drv.vgt_minimizer_regions_serial, (), 29, 11, off, moff, bad)[0] == capi.VGK_EINVAL
    assert capi.minimizer_regions_call(drv.vgt_minimizer_regions_serial, (), 0, 11, off, moff, recs)[0] == capi.VGK_EINVAL
    assert capi.minimizer_regions_call(drv.vgt_minimizer_regions_serial, (), 29, 65, off, moff, recs)[0] == capi.VGK_EINVAL


@pytest.fixture(scope="module")
def host_aligner():
    h = util.host()
    h.vgh_log_base.restype = ctypes.c_double; h.vgh_log_base.argtypes = [ctypes.c_void_p]
    h.vgh_compute_mapping_quality.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_int, ctypes.c_int]
    h.vgh_read_mapq_direct.restype = ctypes.c_double
    h.vgh_read_mapq_direct.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    h.vgh_faster_cap.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    al = util.HostAligner(util.ORACLE_LIB)
    return h, al, h.vgh_log_base(al.ptr)


def shim_mapq(scheme, a):
    return capi.read_mapq_call(pipeline._host_lib().vgh_read_mapq, (), scheme, tail=(ctypes.c_int(4),), **a)


def serial_mapq(scheme, a):
    return capi.read_mapq_call(ctypes.CDLL(DRIVER).vgt_read_mapq_serial, (), scheme, **a)


@pytest.fixture(scope="module")
def corpus(host_aligner):
    """ReadMapqWorkload with the scorer's log base, and per variant the shim's answer"""
    wl = workloads.ReadMapqWorkload(log_base=host_aligner[2])
    per_variant = []
    for v in wl.variants:
        rc, want = shim_mapq(wl.scheme(v), wl.arrays(v))
        assert rc == 0, v
        per_variant.append((v, want))
    return wl, per_variant


def scaled_scores(wl, v, r):
    """log_base * (the scores of read r after :957-968), in float64 as the shim computes them"""
    s = wl.scores[int(wl.score_off[r]):int(wl.score_off[r + 1])].astype(np.float64)
    if v.get("score_window", 0):
        s = s * float(v["score_window"]) / float(int(wl.read_off[r + 1] - wl.read_off[r]))
    return wl.log_base * (s * float(v.get("score_scale", 1.0)))


def set_aside(h, wl, v, want):
    """The reads whose integers may differ by 1 between two correct libraries: the shim's own pre-truncation double within 1e-3 of an integer while
    below 61, its pre-rounding double within 1e-6 of a half-integer, or the sum of exp(other - best) at the edge of the infinite case"""
    aside = np.zeros(wl.n, dtype=bool)
    first = 1 if v.get("flags", 0) & capi.READ_MAPQ_FIRST else 0
    for r in range(wl.n):
        if want["status"][r] != 0:
            continue
        bonus = 2.0 if want["uncapped"][r] == capi.INT32_MAX else 1.0
        pre_round = min(bonus * want["explored_cap"][r], want["uncapped"][r])
        if math.isfinite(pre_round) and abs(pre_round - math.floor(pre_round) - 0.5) < 1e-6:
            aside[r] = True
        if wl.unmapped[r]:
            continue
        s = np.ascontiguousarray(scaled_scores(wl, v, r))
        m = np.ascontiguousarray(wl.mult[int(wl.score_off[r]):int(wl.score_off[r + 1])]) if v.get("multiplicity") else None
        others = ctypes.c_double()
        direct = h.vgh_read_mapq_direct(s.ctypes.data, len(s), None if m is None else m.ctypes.data, first, ctypes.byref(others))
        if (direct < 61 and abs(direct - round(direct)) < 1e-3) or 5e-15 <= others.value <= 5e-14:
            aside[r] = True
    return aside


def test_the_serial_statement_equals_the_shim_bit_for_bit(corpus):
    wl, per_variant = corpus
    for v, want in per_variant:
        rc, got = serial_mapq(wl.scheme(v), wl.arrays(v))
        assert rc == 0 and got.tobytes() == want.tobytes(), (v["name"], np.nonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])[0][:5])
        stops = wl.stops(v)
        assert sorted(np.nonzero(want["status"])[0]) == sorted(stops) and (want["status"][sorted(stops)] == capi.VGK_EINVAL).all(), v["name"]
        bad = want[sorted(stops)]
        assert (bad["mapq"] == 0).all() and (bad["uncapped"] == 0).all() and (bad["explored_cap"] == 0).all()
        assert ((want["mapq"] >= 0) & (want["mapq"] <= 60)).all()
    # a minimizer with k == 0 in the scheme: every read with qualities and an explored minimizer stops; nothing else does
    v = dict(name="k of 0", k=0)
    rc, got = serial_mapq(wl.scheme(v), wl.arrays(v)); rcs, want = shim_mapq(wl.scheme(v), wl.arrays(v))
    assert rc == 0 and rcs == 0 and got.tobytes() == want.tobytes()
    has_explored = np.add.reduceat(np.append(wl.explored, 0).astype(np.int64), wl.min_off[:-1].astype(np.int64)) * (np.diff(wl.min_off.astype(np.int64)) > 0) > 0
    no_scores = np.zeros(wl.n, dtype=bool); no_scores[wl.special["no scores"]] = True
    assert ((want["status"] != 0) == (has_explored | no_scores)).all()


def test_the_shim_s_cap_and_quality_are_faster_cap_s_and_the_calculator_s(corpus, host_aligner):
    wl, per_variant = corpus
    h, al, log_base = host_aligner
    v, want = per_variant[0]
    assert v["name"] == "short-read route"
    table = np.zeros((len(wl.mins), 6), dtype=np.uint64)
    table[:, 0] = workloads.wang_hash64(wl.mins["key"]); table[:, 1] = wl.mins["offset"]; table[:, 3] = wl.regions["start"]; table[:, 4] = wl.regions["length"]; table[:, 5] = wl.k
    checked = 0
    for r in range(wl.n):
        if want["status"][r] != 0:
            continue
        lo, hi = int(wl.min_off[r]), int(wl.min_off[r + 1]); a, b = int(wl.read_off[r]), int(wl.read_off[r + 1])
        ms = np.ascontiguousarray(table[lo:hi]); ex = np.ascontiguousarray(np.nonzero(wl.explored[lo:hi])[0], dtype=np.uint64)
        cap = ctypes.c_double()
        assert h.vgh_faster_cap(ms.ctypes.data, hi - lo, ex.ctypes.data, len(ex), b"N" * (b - a), wl.qual[a:b].tobytes(), b - a, ctypes.byref(cap)) == 0, r
        assert np.float64(cap.value).tobytes() == np.float64(want["explored_cap"][r]).tobytes(), (r, cap.value, want["explored_cap"][r])
        if not wl.unmapped[r]:
            s = wl.scores[int(wl.score_off[r]):int(wl.score_off[r + 1])].astype(np.float64)
            assert h.vgh_compute_mapping_quality(al.ptr, (ctypes.c_double * len(s))(*s), len(s), 0, 0) == want["uncapped"][r], r
        checked += 1
    assert checked > 4000
    # ... and the first-score form, without its multiplicities (vgh_compute_mapping_quality takes none)
    v = dict(name="first", flags=capi.READ_MAPQ_FIRST | capi.READ_MAPQ_NO_EXPLORED_CAP)
    rc, want = shim_mapq(wl.scheme(v), wl.arrays(v))
    for r in range(0, wl.n, 7):
        if want["status"][r] == 0 and not wl.unmapped[r]:
            s = wl.scores[int(wl.score_off[r]):int(wl.score_off[r + 1])].astype(np.float64)
            assert h.vgh_compute_mapping_quality(al.ptr, (ctypes.c_double * len(s))(*s), len(s), 0, 1) == want["uncapped"][r], r


def test_the_corpus_reaches_what_the_rule_must_reach(corpus):
    wl, per_variant = corpus
    by_name = {v["name"]: (v, want) for v, want in per_variant}
    reach = collections.Counter()
    lengths = np.diff(wl.read_off.astype(np.int64))
    assert len(lengths) >= 4016 and ((lengths[:4000] >= 20) & (lengths[:4000] <= 250)).all() and ((lengths[4000:4016] >= 4000) & (lengths[4000:4016] <= 8000)).all()
    v, want = by_name["no qualities"]
    reach["no qualities"] = int(np.isinf(want["explored_cap"][want["status"] == 0]).all() and (want["status"] == 0).sum() > 4000)
    v, want = by_name["short-read route"]
    ok = want["status"] == 0
    n_explored = np.array([int(wl.explored[int(wl.min_off[r]):int(wl.min_off[r + 1])].sum()) for r in range(wl.n)])
    n_scores = np.diff(wl.score_off.astype(np.int64))
    reach["no explored minimizer"] = int((ok & (n_explored == 0) & (want["explored_cap"] == 0) & np.signbit(want["explored_cap"])).sum())       # -0.0, as the reference
    reach["one alignment"] = int((ok & (n_scores == 1)).sum())
    reach["the unmapped byte"] = int((ok & (wl.unmapped != 0) & (want["mapq"] == 0) & (want["uncapped"] == 0)).sum())
    assert (want["mapq"][ok & (wl.unmapped != 0)] == 0).all()
    for r in range(wl.n):
        s = wl.scores[int(wl.score_off[r]):int(wl.score_off[r + 1])]
        if len(s) >= 2 and (s == s.max()).sum() >= 2:
            reach["equal top scores"] += 1
        if len(s) >= 2 and s[0] < s.max():
            reach["a first score that is not the largest"] += 1
        lo, hi = int(wl.min_off[r]), int(wl.min_off[r + 1])
        g = wl.regions[lo:hi][wl.explored[lo:hi] != 0]
        if len(g) >= 2 and ok[r]:
            order = np.lexsort((g["start"], g["start"].astype(np.int64) + g["length"]))
            ends = (g["start"].astype(np.int64) + g["length"])[order]
            if (g["start"][order][1:] > np.maximum.accumulate(ends)[:-1]).any():
                reach["a gap between agglomerations"] += 1
        q = wl.qual[int(wl.read_off[r]):int(wl.read_off[r + 1])]
        if ok[r] and n_explored[r] and (q == 0).any():
            reach["a quality byte of 0"] += 1
        if ok[r] and n_explored[r] and (q >= 93).any():
            reach["a quality byte of 93 or more"] += 1
    infinite = ok & (want["uncapped"] == capi.INT32_MAX) & (wl.unmapped == 0)
    reach["a gap wide enough for INT32_MAX"] = int(infinite.sum())
    # ... where the escape bonus is 2: the quality is the doubled cap wherever that lies below 60
    doubled = infinite & (2 * want["explored_cap"] < 59) & (want["explored_cap"] > 1)
    reach["the escape bonus of 2"] = int(doubled.sum())
    assert (want["mapq"][doubled] == np.round(2 * want["explored_cap"][doubled])).all()
    v, want = by_name["chain route"]
    firsts = [r for r in range(wl.n) if want["status"][r] == 0 and not wl.unmapped[r] and wl.score_off[r + 1] - wl.score_off[r] >= 2
              and wl.scores[int(wl.score_off[r])] < wl.scores[int(wl.score_off[r]):int(wl.score_off[r + 1])].max()]
    reach["the FIRST form with a first score that is not the largest"] = len(firsts)
    assert (want["uncapped"][firsts] < 4).all()                       # (a first alignment that is not the best is at most a coin flip)
    reach["score_window on"] = int(v.get("score_window", 0) > 0 and v.get("score_scale", 1.0) != 1.0)
    reach["multiplicities above 1"] = int((wl.mult > 1).sum())
    _, plain = by_name["short-read route"]
    assert (plain["uncapped"] != want["uncapped"]).any()
    v, want = by_name["chain route, no cap"]
    reach["NO_EXPLORED_CAP"] = int(np.isinf(want["explored_cap"][want["status"] == 0]).all())
    assert (want["mapq"][want["status"] == 0] == np.clip(want["uncapped"][want["status"] == 0], 0, 60)).all()
    v, want = by_name["lengths of their own"]
    stops = wl.stops(v)
    for what in ("no scores", "own length 0", "own length 33", "impossible to disrupt", "region behind the read"):
        reach["stops: " + what] = int(what in stops.values())
    print(dict(reach))
    assert [what for what, count in reach.items() if count == 0] == [] and len(reach) == 20


def test_few_reads_lie_at_a_rounding_boundary(corpus, host_aligner):
    """the share of reads the engine's comparison sets aside, computed by the shim alone: at most 2 % (by uniformity about 0.2 %)"""
    wl, per_variant = corpus
    for v, want in per_variant:
        share = set_aside(host_aligner[0], wl, v, want).mean()
        print(v["name"], share)
        assert share <= 0.02, (v["name"], share)


def g_key(k):              # 'G' * k, two bits per base, first base highest
    v = 0
    for _ in range(k):
        v = (v << 2) | 2
    return v


def reference_cap_cases(tries=2000):
    """The reference's two faster_cap cases (src/unittest/minimizer_mapper.cpp:154-252; generators as in tests/test_mapq_cap.py) as one call's arrays: read 0 is
    150 G's under 25-base cores with 10-base flanks at every offset, reads 1 .. tries random agglomerations over 100 G's at quality 60"""
    from test_mapq_cap import cover_in_minimizers
    rng = np.random.default_rng(2026)
    rows, counts, lengths, qual = [], [], [], []
    ms = cover_in_minimizers("G" * 150, 25, 10, 1)
    rows += [(g_key(25), m[1], m[3], m[4], 25) for m in ms]; counts.append(len(ms)); lengths.append(150); qual += [0x1E] * 150
    L = 100
    for _ in range(tries):
        n = int(rng.integers(0, 100)) + 5
        for _ in range(n):
            core_width = int(rng.integers(0, min(L // 2 - 1, 31))) + 1
            run_length = int(rng.integers(0, min(L - core_width, 32 - core_width)))
            flank_width = int(rng.integers(0, 10))
            core_start = int(rng.integers(0, L - core_width - run_length))
            start = core_start; length = core_width + run_length + 2 * flank_width
            if flank_width > start:
                length -= flank_width - start; start = 0
            else:
                start -= flank_width
            if start + length > L:
                length = L - start
            rows.append((g_key(core_width), core_start, start, length, core_width))
        counts.append(n); lengths.append(L); qual += [60] * L
    recs = np.zeros(len(rows), dtype=capi.READ_MINIMIZER_DT); regions = np.zeros(len(rows), dtype=capi.MINIMIZER_REGION_DT)
    recs["key"] = np.array([r[0] for r in rows], dtype=np.uint64); recs["offset"] = [r[1] for r in rows]; recs["reserved"] = [r[4] for r in rows]
    regions["start"] = [r[2] for r in rows]; regions["length"] = [r[3] for r in rows]
    n = len(counts)
    return dict(score_off=np.arange(n + 1, dtype=np.uint64), scores=np.full(n, 100, dtype=np.int32), minimizer_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64),
                minimizers=recs, regions=regions, explored=np.ones(len(rows), dtype=np.uint8), read_off=np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64),
                quality=np.array(qual, dtype=np.uint8))


def cap_scheme(log_base=1.0):
    return capi.ReadMapqScheme(log_base, 1.0, 0, 25, capi.READ_MAPQ_OWN_LENGTH, 0)


def caps_agree(got, want):
    """explored_cap: infinities and -0.0 exactly, otherwise to 1e-12 relative (absolute near 0)"""
    g, w = got["explored_cap"], want["explored_cap"]
    special = np.isinf(w) | (w == 0) | np.isinf(g) | (g == 0)
    same_special = (g[special] == w[special]) & (np.signbit(g[special]) == np.signbit(w[special]))
    return same_special.all() and (np.abs(g[~special] - w[~special]) <= 1e-12 * np.maximum(np.abs(w[~special]), 1.0)).all()


def test_the_reference_s_two_faster_cap_cases(tmp_path):
    a = reference_cap_cases(2000)
    rc, shim = shim_mapq(cap_scheme(), a); rcs, serial = serial_mapq(cap_scheme(), a)
    assert rc == 0 and rcs == 0
    for out in (shim, serial):
        assert (out["status"] == 0).all() and np.isfinite(out["explored_cap"]).all() and (out["explored_cap"] > 0).all()
    assert caps_agree(serial, shim)                                   # (agglomerations that tie may be multiplied in another order: ulps)
    assert (serial["uncapped"] == shim["uncapped"]).all()


def write_call(path, k, w, flags, score_window, scheme_k, log_base, score_scale, a):
    n = len(a["read_off"]) - 1
    mult, un, q = a.get("multiplicity"), a.get("unmapped"), a.get("quality")
    head = np.array([k, w, n, len(a["scores"]), len(a["minimizers"]), int(a["read_off"][-1]), flags, score_window, scheme_k, mult is not None, un is not None, q is not None], dtype=np.uint64)
    with open(path, "wb") as f:
        f.write(head.tobytes()); f.write(np.array([log_base, score_scale], dtype=np.float64).tobytes())
        for arr, dt in ((a["read_off"], np.uint64), (a["score_off"], np.uint64), (a["minimizer_off"], np.uint64), (a["scores"], np.int32), (mult, np.float64), (un, np.uint8),
                        (a["minimizers"], capi.READ_MINIMIZER_DT), (a["explored"], np.uint8), (a["regions"], capi.MINIMIZER_REGION_DT), (q, np.uint8)):
            if arr is not None:
                f.write(np.ascontiguousarray(arr, dtype=dt).tobytes())


def test_the_serial_statement_under_the_host_sanitizers(corpus, region_corpus, tmp_path):
    """the driver as a program of its own under -fsanitize=address,undefined, on both corpora and the reference's cases: the same answers, nothing reported"""
    wl, per_variant = corpus
    subprocess.check_call(["make", "-s", "readmapq_san"], cwd=ROOT)
    drv = ctypes.CDLL(DRIVER)
    calls = []
    for v, want in per_variant[:1] + per_variant[2:3] + per_variant[4:]:
        calls.append((wl.k, wl.w, wl.scheme(v), wl.arrays(v), want))
    calls.append((25, 11, cap_scheme(), reference_cap_cases(200), None))
    flat, off, per_kw = region_corpus
    for (k, w), (moff, recs, want_regions, _) in per_kw.items():
        n = len(off) - 1
        a = dict(score_off=np.zeros(n + 1, dtype=np.uint64), scores=np.zeros(0, dtype=np.int32), minimizer_off=moff, minimizers=recs, regions=want_regions,
                 explored=np.ones(len(recs), dtype=np.uint8), read_off=off, quality=np.full(len(flat), 30, dtype=np.uint8), unmapped=np.ones(n, dtype=np.uint8))
        calls.append((k, w, capi.ReadMapqScheme(1.0, 1.0, 0, k, 0, 0), a, None))
    for k, w, scheme, a, want in calls:
        write_call(tmp_path / "call.bin", k, w, scheme.flags, scheme.score_window, scheme.k, scheme.log_base, scheme.score_scale, a)
        done = subprocess.run([os.path.join(ROOT, "tests", "emu", "read_mapq_san"), str(tmp_path / "call.bin"), str(tmp_path / "answer.bin")], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "", done.stderr[-2000:]
        raw = open(tmp_path / "answer.bin", "rb").read()
        rcs = np.frombuffer(raw[:16], dtype=np.int64)
        rc_regions, regions = capi.minimizer_regions_call(drv.vgt_minimizer_regions_serial, (), k, w, a["read_off"], a["minimizer_off"], a["minimizers"])
        rc, out = serial_mapq(scheme, a)
        assert int(rcs[0]) == rc_regions and int(rcs[1]) == rc == 0
        assert raw[16:] == regions.tobytes() + out.tobytes()
        if want is not None:
            assert out.tobytes() == want.tobytes()


def test_the_entry_points_are_the_engine_library_s_own():
    engine_h = open(os.path.join(ROOT, "include", "vgk_engine.h")).read(); vgk_h = open(os.path.join(ROOT, "include", "vgk.h")).read()
    lib = ctypes.CDLL(ENGINE)
    for name in ("vgk_minimizer_regions", "vgk_read_mapq", "vgk_read_mapq_limits", "vgk_read_mapq_last_ms", "vgk_read_mapq_last_launches"):
        assert name + "(" in engine_h and name + "(" not in vgk_h and hasattr(lib, name), name
    assert hasattr(pipeline._host_lib(), "vgh_read_mapq") and hasattr(pipeline._host_lib(), "vgh_minimizer_regions")
    out = (ctypes.c_uint32 * 4)()
    assert lib.vgk_read_mapq_limits(out) == 0 and out[0] >= 1 and out[1] == 1 and out[2] == 1


def test_the_kernels_use_no_scratch():
    """what DESIGN.md section 35 says of the kernels, read off the built library (tools/kernel_registers.py): no scratch memory, no spills, and LDS that leaves
    three workgroups of the sweep per CU (160 KiB / 3)"""
    import sys
    rows = []
    for pattern in ("read_mapq", "minimizer_regions"):
        done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_registers.py"), ENGINE, pattern], capture_output=True, text=True)
        assert done.returncode == 0, done.stderr[-1000:]
        rows += [line.split() for line in done.stdout.splitlines() if pattern in line]
    assert len(rows) == 3, rows
    for row in rows:
        spills, scratch, lds = int(row[row.index("spills") + 1]), int(row[row.index("scratch") + 1]), int(row[row.index("lds") + 1])
        assert spills == 0 and scratch == 0 and lds <= 160 * 1024 // 3, row


def test_the_emulated_backend_says_unsupported():
    if not os.path.exists(util.EMU_LIB):
        subprocess.check_call(["make", "-s", "emu"], cwd=ROOT)
    eng = capi.Engine(lib=util.EMU_LIB)
    a = reference_cap_cases(2)
    rc, _ = capi.read_mapq_call(eng.lib.vgk_read_mapq, (eng.h,), cap_scheme(), **a)
    assert rc == capi.VGK_EUNSUPPORTED
    read = np.frombuffer(b"ACGTTGCATTGACCAGTAGGCATCGATCGGATTACAGGCTAAGCTTAGGCAT", dtype=np.uint8)
    moff, recs, _, _ = workloads.read_minimizers(read, [0, len(read)], 11, 4)
    rc, _ = capi.minimizer_regions_call(eng.lib.vgk_minimizer_regions, (eng.h,), 11, 4, [0, len(read)], moff, recs)
    assert len(recs) > 3 and rc == capi.VGK_EUNSUPPORTED


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    return capi.Engine(lib=ENGINE, device=0)


def engine_mapq(eng, scheme, a):
    return capi.read_mapq_call(eng.lib.vgk_read_mapq, (eng.h,), scheme, **a)


def hold_to_the_shim(got, want, aside, what):
    """status equal everywhere; the cap to 1e-12; uncapped and mapq equal — on the reads set aside within 1"""
    assert (got["status"] == want["status"]).all(), (what, np.nonzero(got["status"] != want["status"])[0][:5])
    assert caps_agree(got, want), what
    for name in ("uncapped", "mapq"):
        g, w = got[name].astype(np.float64), want[name].astype(np.float64)
        off = g != w
        print(what, name, "differ on", int(off.sum()), "reads, all set aside:", bool((aside | ~off).all()))
        assert (aside | ~off).all(), (what, name, np.nonzero(off & ~aside)[0][:5])
        both_finite = off & (g != capi.INT32_MAX) & (w != capi.INT32_MAX)
        assert (np.abs(g - w)[both_finite] <= 1).all(), (what, name)
        if name == "uncapped":                                        # INT32_MAX on one side only: the edge of the infinite case, which the band of the sum covers
            assert ((g == capi.INT32_MAX) == (w == capi.INT32_MAX))[~aside].all(), what


@pytest.mark.gpu
def test_the_engine_s_agglomerations_equal_the_shim_s(region_corpus, gpu):
    flat, off, per_kw = region_corpus
    for (k, w), (moff, recs, want, _) in per_kw.items():
        rc, shim = shim_regions(flat, off, k, w, moff, recs)
        got = gpu.minimizer_regions(k, w, off, moff, recs)
        assert rc == 0 and (got == shim).all() and (got == want).all(), (k, w)
    assert gpu.read_mapq_last_ms()[0] > 0
    moff, recs, _, _ = per_kw[(29, 11)]
    swapped = recs.copy(); j = int(moff[int(np.nonzero(np.diff(moff.astype(np.int64)) >= 2)[0][0])])
    swapped["offset"][j], swapped["offset"][j + 1] = recs["offset"][j + 1], recs["offset"][j]
    assert capi.minimizer_regions_call(gpu.lib.vgk_minimizer_regions, (gpu.h,), 29, 11, off, moff, swapped)[0] == capi.VGK_EINVAL
    assert capi.minimizer_regions_call(gpu.lib.vgk_minimizer_regions, (gpu.h,), 29, 11, off[:1], moff[:1], recs[:0])[0] == 0       # n = 0


@pytest.mark.gpu
def test_the_engine_equals_the_shim_on_the_corpus_and_the_reference_s_cases(corpus, host_aligner, gpu):
    wl, per_variant = corpus
    for v, want in per_variant:
        rc, got = engine_mapq(gpu, wl.scheme(v), wl.arrays(v))
        assert rc == 0, v["name"]
        aside = set_aside(host_aligner[0], wl, v, want)
        assert aside.mean() <= 0.02
        hold_to_the_shim(got, want, aside, v["name"])
        launches = gpu.read_mapq_last_launches()
        refused = [r for r, what in wl.stops(v).items() if what != "impossible to disrupt"]       # (that one is found by the sweep itself, over the slab)
        assert sum(launches) == wl.n and launches[2] == len(refused), (v["name"], launches)
    assert gpu.read_mapq_last_ms()[1] > 0
    a = reference_cap_cases(2000)
    rc, got = engine_mapq(gpu, cap_scheme(), a); rcs, want = shim_mapq(cap_scheme(), a)
    assert rc == 0 and rcs == 0 and np.isfinite(got["explored_cap"]).all() and (got["explored_cap"] > 0).all()
    hold_to_the_shim(got, want, np.zeros(len(want), dtype=bool), "the reference's cases")          # (one score of 100: the null-alignment term only, far from any boundary)


@pytest.mark.gpu
def test_every_limit_from_both_sides(corpus, gpu):
    wl, per_variant = corpus
    v, want = per_variant[0]
    limit = gpu.read_mapq_limits()[0]
    assert limit == 64                                                # (the workload plants its two staircase reads at this size)
    exact, beyond = wl.special["exactly the LDS limit"], wl.special["one beyond the LDS limit"]
    assert int(wl.explored[int(wl.min_off[exact]):int(wl.min_off[exact + 1])].sum()) == limit and int(wl.explored[int(wl.min_off[beyond]):int(wl.min_off[beyond + 1])].sum()) == limit + 1
    stops = sorted(wl.stops(v))
    swept = [r for r in stops if wl.stops(v)[r] == "impossible to disrupt"]                         # refused by the sweep itself, over the slab: 130 explored minimizers
    for reads, launches in (([exact], (1, 0, 0)), ([beyond], (0, 1, 0)), ([exact, beyond], (1, 1, 0)), ([7], (1, 0, 0)), (stops, (0, len(swept), len(stops) - len(swept))),
                            (list(range(4000, 4016)) + [beyond], None)):
        rc, got = engine_mapq(gpu, wl.scheme(v), wl.arrays(v, reads))
        assert rc == 0 and len(got) == len(reads)
        if launches is not None:
            assert gpu.read_mapq_last_launches() == launches, (reads, gpu.read_mapq_last_launches())
        else:                                                         # the long reads: all over the slab
            assert gpu.read_mapq_last_launches()[1] == len(reads)
        assert (got["status"] == want["status"][reads]).all() and caps_agree(got, want[reads]), reads
        assert (np.abs(got["mapq"] - want["mapq"][reads]) <= 1).all()
    # n = 0
    empty = dict(score_off=np.zeros(1, dtype=np.uint64), scores=np.zeros(0, dtype=np.int32), minimizer_off=np.zeros(1, dtype=np.uint64), minimizers=np.zeros(0, dtype=capi.READ_MINIMIZER_DT),
                 regions=np.zeros(0, dtype=capi.MINIMIZER_REGION_DT), explored=np.zeros(0, dtype=np.uint8), read_off=np.zeros(1, dtype=np.uint64))
    rc, got = engine_mapq(gpu, wl.scheme(v), empty)
    assert rc == 0 and len(got) == 0 and gpu.read_mapq_last_launches() == (0, 0, 0)
    # the call's own refusals
    bad = wl.scheme(v); bad.flags = 8
    assert engine_mapq(gpu, bad, wl.arrays(v, [7]))[0] == capi.VGK_EINVAL
    bad = wl.scheme(v); bad.log_base = 0.0
    assert engine_mapq(gpu, bad, wl.arrays(v, [7]))[0] == capi.VGK_EINVAL
    a = wl.arrays(v, [7, 8]); a["score_off"] = a["score_off"][::-1].copy()
    assert engine_mapq(gpu, wl.scheme(v), a)[0] == capi.VGK_EINVAL


@pytest.mark.gpu
def test_end_to_end_the_gaf_lines_carry_the_shim_s_quality(host_aligner):
    """2 000 reads of the configs[2]-shaped workload with qualities: find_seeds -> extension -> vgk_tail_stage_composed -> pipeline.read_mapq -> gaf_lines;
    column 12 of every read's first line is the shim's value for that read (the set-aside rule as above)"""
    h, al, log_base = host_aligner
    scoring = (1, 4, 6, 1, 5)
    wl = workloads.GaplessWorkload(2000, seed=21, graph_bp=150000, inserted_reads=0.3)
    rng = np.random.default_rng(3)
    level = np.repeat(rng.choice(np.array([6, 14, 24, 34]), wl.gs.n), np.diff(np.asarray(wl.gs.read_off, dtype=np.int64)))      # a read's own quality level, so that the caps spread
    quality = (level + rng.integers(0, 8, len(wl.gs.reads))).astype(np.uint8)
    eng = capi.Engine(capi.Scoring.simple(*scoring), lib=ENGINE, device=0)
    index = eng.haplo_index(wl.nodes, wl.threads); mindex = eng.minimizer_index(wl.nodes, wl.threads, k=29, w=11)
    seeded = pipeline.seed_long_reads(eng, mindex, wl.gs.reads, wl.gs.read_off, 29, choice="device")
    moff = seeded["minimizer_off"].astype(np.int64)
    seed_off = seeded["seed_off"][moff]
    assert int(np.diff(seed_off.astype(np.int64)).max()) <= 64
    gs = capi.GaplessSet(wl.gs.reads, wl.gs.read_off, seeded["seeds"], seed_off)
    stage = pipeline.align_stage_device(eng, index, gs, composed=True, composed_policy=dict(window_length=39))
    composed = stage["composed"]
    details = {}
    mapq = pipeline.read_mapq(eng, seeded, composed, wl.gs.read_off, quality, 29, 11, log_base, details=details)
    seqs, seq_off, results, score = pipeline.read_alignments_gaf_view(wl.gs.reads, wl.gs.read_off, composed)
    node_seq = np.frombuffer("".join(wl.nodes).encode(), dtype=np.uint8)
    node_off = np.concatenate([[0], np.cumsum([len(s) for s in wl.nodes])]).astype(np.uint64)
    lines = pipeline.gaf_lines(seqs, seq_off, results, composed["mappings"], composed["edits"], node_seq, node_off, mapq=mapq, score=score)
    # the shim over the same inputs, its agglomerations included
    rc, regions = shim_regions(wl.gs.reads, wl.gs.read_off, 29, 11, seeded["minimizer_off"], seeded["minimizers"])
    assert rc == 0 and (regions == details["regions"]).all()
    scheme = capi.ReadMapqScheme(log_base, 1.0, 0, 29, 0, 0)
    a = dict(score_off=details["score_off"], scores=details["scores"], minimizer_off=seeded["minimizer_off"], minimizers=seeded["minimizers"], regions=regions,
             explored=details["explored"], read_off=wl.gs.read_off, quality=quality, unmapped=details["unmapped"])
    rc, want = shim_mapq(scheme, a)
    assert rc == 0 and (want["status"] == 0).all()

    class View:                                                       # what set_aside reads of a workload
        pass
    view = View()
    view.n = wl.gs.n; view.unmapped = details["unmapped"]; view.scores = details["scores"]; view.score_off = details["score_off"]
    view.read_off = np.asarray(wl.gs.read_off, dtype=np.uint64); view.log_base = log_base; view.mult = None
    aside = set_aside(h, view, {}, want)
    assert aside.mean() <= 0.02
    hold_to_the_shim(details["per_read"], want, aside, "end to end")
    aln_off = composed["aln_off"].astype(np.int64)
    column12 = np.array([int(lines[int(aln_off[r])].split(b"\t")[11]) for r in range(wl.gs.n)])
    assert (column12 == details["per_read"]["mapq"]).all()
    differ = column12 != want["mapq"]
    assert (aside | ~differ).all() and (np.abs(column12 - want["mapq"]) <= 1).all()
    print("mapq below 60: %d, at 60: %d, at 0: %d" % ((column12 < 60).sum(), (column12 == 60).sum(), (column12 == 0).sum()))
    assert (column12 < 60).any() and (column12 == 60).any()
    assert int(details["explored"].sum()) > 2000
