"""find_seeds' choice on the device (include/vgk_engine.h: vgk_minimizer_choose, vgk_minimizer_find_seeds) against the host shim's select_minimizers
(vgh_select_minimizers_of_read), verdict byte for verdict byte; find_seeds_restated of test_seed_policy.py is the second reference on the short lists.
The lists are crafted: no index is needed for the choice alone, so the shapes are small and pointed."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import util
from test_seed_policy import DEFAULTS, find_seeds_restated, select

K = 11
LDS_MAX, LDS_BASES = 4096, 32767                  # MZ_CHOOSE_LDS_MAX, MZ_CHOOSE_LDS_BASES of vg_amd/csrc/minimizer_device.hpp
HITS = [0, 1, 1, 1, 2, 3, 8, 9, 10, 11, 40, 41, 499, 500, 501, 3000]
CLASSES = dict(TAKEN=0, DOWNSAMPLED=1, NO_HITS=2, HARD_HIT_CAP=3, OVERLAPPING=4, MAX_MIN=5, HIT_CAP=6)


def policies():
    from vg_amd import pipeline
    long_read = dict(pipeline.GIRAFFE_LONG_READ_POLICY)
    return dict(
        long_read=long_read,
        # giraffe's hifi preset (src/subcommand/giraffe_main.cpp:957-970): the score filter off, downsampling, its budget; the flank left at 250
        hifi=dict(long_read, hit_cap=0, score_fraction=1.0, hard_hit_cap=13614, window_count=15, max_window_length=227, max_unique_min=79, num_bp_per_min=152),
        # the three of test_long_reads_are_seeded_without_caps
        small1=dict(DEFAULTS, hit_cap=2, hard_hit_cap=40, score_fraction=0.8, max_unique_min=30, num_bp_per_min=50),
        small2=dict(DEFAULTS, hit_cap=10, hard_hit_cap=500, score_fraction=0.9, max_unique_min=500, num_bp_per_min=1000),
        small3=dict(DEFAULTS, hit_cap=1, hard_hit_cap=8, score_fraction=0.5, max_unique_min=10, num_bp_per_min=100, exclude_overlapping_min=True, window_count=8, max_window_length=64),
        budget=dict(long_read, max_unique_min=10, num_bp_per_min=100))


def a_read(rng, L, alphabet="ACGT"):
    return "".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), L))


def a_list(rng, L, n, n_keys, hits=HITS, offsets=None):
    """n minimizers of K bases at distinct offsets of a read of L bases, in read order; a key has one hit count"""
    offs = np.sort(rng.choice(np.arange(L - K + 1), size=n, replace=False)) if offsets is None else offsets
    hits_of = [int(rng.choice(hits)) for _ in range(n_keys)]
    keys = rng.integers(0, n_keys, n)
    return [(int(key) * 7919 + 13, int(o), K, hits_of[int(key)]) for key, o in zip(keys, offs)]


@functools.lru_cache(maxsize=None)
def corpus():
    """(name, read, minimizers) — made once, shared, never changed"""
    rng = np.random.default_rng(20261017)
    out = []
    for n in (0, 1, 63, 64, 65):                                             # around the old selection's 64
        out.append(("n%d" % n, a_read(rng, 600), a_list(rng, 600, n, max(1, n // 2))))
    for n in (LDS_MAX - 1, LDS_MAX, LDS_MAX + 1):                            # around the in-LDS sort capacity
        out.append(("n%d" % n, a_read(rng, 6000), a_list(rng, 6000, n, 1500)))
    out.append(("slab", a_read(rng, 12000), a_list(rng, 12000, 9000, 4000)))  # well above it
    for L in (LDS_BASES, LDS_BASES + 1):                                     # around the in-LDS bitmaps' length
        out.append(("L%d" % L, a_read(rng, L), a_list(rng, L, 300, 150)))
    out.append(("one_key", a_read(rng, 2000), [(77, int(o), K, 3) for o in np.sort(rng.choice(1990, 300, replace=False))]))
    out.append(("all_one_hit", a_read(rng, 8000), [(1000 + 3 * j, int(o), K, 1) for j, o in enumerate(np.sort(rng.choice(7990, 3000, replace=False)))]))
    for hard in (8, 40, 500, 13614):                                         # hits exactly the hard cap and one above, side by side: tab[hard] against 1.0
        offs = np.sort(rng.choice(1990, 120, replace=False))
        out.append(("hard%d" % hard, a_read(rng, 2000), [(5000 + j, int(o), K, hard + (j & 1)) for j, o in enumerate(offs)]))
    out.append(("raw_bytes", a_read(rng, 1500, "ACGTNacgtn"), a_list(rng, 1500, 200, 150, hits=[1, 1, 1, 11, 12])))      # N and lower case: the bytes as given seed the shuffle
    out.append(("empty", "", []))
    out.append(("ends", a_read(rng, 700), a_list(rng, 700, 50, 30, offsets=np.concatenate([[0], np.sort(rng.choice(np.arange(1, 689), 48, replace=False)), [689]]))))
    for j in range(6):                                                       # 1 500-base reads for the budgets that bite; repetitive ones for the caps
        out.append(("r1500_%d" % j, a_read(rng, 1500), a_list(rng, 1500, 380, 200 if j < 3 else 25)))
    for j in range(3):
        out.append(("none_hit_%d" % j, a_read(rng, 1500), a_list(rng, 1500, 200, 60, hits=[0, 0, 1, 11, 30, 600])))
    return tuple(out)


def packed():
    reads = "".join(r for _, r, _ in corpus())
    off = np.concatenate([[0], np.cumsum([len(r) for _, r, _ in corpus()])]).astype(np.uint64)
    moff = np.concatenate([[0], np.cumsum([len(ms) for _, _, ms in corpus()])]).astype(np.uint64)
    from vg_amd import capi
    recs = np.zeros(int(moff[-1]), dtype=capi.READ_MINIMIZER_DT)
    flat = [m for _, _, ms in corpus() for m in ms]
    recs["key"] = [m[0] for m in flat]; recs["offset"] = [m[1] for m in flat]; recs["hits"] = [m[3] for m in flat]
    return np.frombuffer(reads.encode(), dtype=np.uint8), off, moff, recs


@functools.lru_cache(maxsize=None)
def shim_verdicts(name):
    """the first reference: the host shim's select_minimizers with the read's sequence, over the whole corpus"""
    subprocess.check_call(["make", "-s", "host"], cwd=util.ROOT)
    P = policies()[name]
    return tuple(np.array(select(list(ms), len(r), P, r)[0] if ms else [], dtype=np.uint8) for _, r, ms in corpus())


POLICY_NAMES = ["long_read", "hifi", "small1", "small2", "small3", "budget"]


# ---- without a GPU ----------------------------------------------------------------------------------------------------------------------
def engine_header_symbols():
    text = open(os.path.join(util.ROOT, "include", "vgk_engine.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vgk_[a-z_0-9]+)\s*\(", text)))


def test_engine_header_declares_what_only_the_engine_exports():
    from test_capi_symbols import declared_symbols
    syms = engine_header_symbols()
    for s in ("vgk_minimizer_choose", "vgk_minimizer_find_seeds", "vgk_minimizer_choose_last_ms", "vgk_batch_refill_stats"):
        assert s in syms
    assert not set(syms) & set(declared_symbols())                           # nothing of it in vgk.h: the oracle need not export it
    if not os.path.exists(util.ENGINE_LIB):
        subprocess.check_call(["make", "-s", "lib"], cwd=util.ROOT)
    h = ctypes.CDLL(util.ENGINE_LIB)
    for s in syms:
        assert hasattr(h, s), s
    h.vgk_abi_version.restype = ctypes.c_int
    assert h.vgk_abi_version() == 6


def test_the_corpus_reaches_every_filter():
    """a condition on the inputs, asserted on the SHIM's output: every class of verdict at least ten times"""
    counts = np.zeros(7, dtype=np.int64)
    for name in POLICY_NAMES:
        for v in shim_verdicts(name):
            counts += np.bincount(v, minlength=7)
    for cls, code in CLASSES.items():
        assert counts[code] >= 10, (cls, counts.tolist())


def test_the_shim_equals_the_restatement_on_the_short_lists():
    for name in POLICY_NAMES:
        P = policies()[name]
        for (case, r, ms), v in zip(corpus(), shim_verdicts(name)):
            if 0 < len(ms) <= 120:
                assert find_seeds_restated(list(ms), len(r), P, r)[0] == v.tolist(), (name, case)


def serial_lane_code(P):
    subprocess.check_call(["make", "-s", "choose"], cwd=util.ROOT)
    from vg_amd import capi
    h = ctypes.CDLL(os.path.join(util.ROOT, "tests", "emu", "libvgamd_choose.so"))
    reads, off, moff, recs = packed()
    verdict = np.full(max(len(recs), 1), 255, dtype=np.uint8); pol = capi.find_seeds_policy(P); rank = ctypes.c_uint32()
    h.vgt_choose_serial.argtypes = [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 2 + [ctypes.c_uint32] + [ctypes.c_void_p] * 4
    assert h.vgt_choose_serial(ctypes.byref(pol), K, reads.ctypes.data, off.ctypes.data, len(off) - 1, moff.ctypes.data, recs.ctypes.data, verdict.ctypes.data, ctypes.byref(rank)) == 0
    return verdict, moff, rank.value


@pytest.mark.parametrize("name", POLICY_NAMES)
def test_serial_lane_code_equals_the_shim(name):
    """mz_choose_one (the statement of the device's rule, the kernel's checker) through tests/emu/choose_driver.cpp"""
    P = policies()[name]
    verdict, moff, rank = serial_lane_code(P)
    for i, ((case, _, _), want) in enumerate(zip(corpus(), shim_verdicts(name))):
        got = verdict[int(moff[i]):int(moff[i + 1])]
        assert got.tolist() == want.tolist(), (name, case, int(np.argmax(got != want)))
    # the rank the kernel sorts a minimizer beyond the hard cap by (score 1.0) stands where the doubles say: against the table made the same way
    import math
    hard = P["hard_hit_cap"]; tab = [0.0] + [1.0 + math.log(hard) - math.log(h) for h in range(1, hard + 1)]
    below = [2 * h for h in range(1, hard + 1) if tab[h] > 1.0]; equal = [2 * h for h in range(1, hard + 1) if tab[h] == 1.0]
    assert (rank in equal) if equal else (rank == (max(below) + 1 if below else 1))


# ---- on the MI355X ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def engine():
    from vg_amd import capi
    return capi.Engine(lib=util.ENGINE_LIB)


@pytest.mark.gpu
@pytest.mark.parametrize("name", POLICY_NAMES)
def test_choice_on_the_device_equals_the_shim(name):
    reads, off, moff, recs = packed()
    verdict = engine().minimizer_choose(policies()[name], K, reads, off, moff, recs)
    for i, ((case, _, _), want) in enumerate(zip(corpus(), shim_verdicts(name))):
        got = verdict[int(moff[i]):int(moff[i + 1])]
        assert got.tolist() == want.tolist(), (name, case, int(np.argmax(got != want)))
    assert engine().minimizer_choose_last_ms() > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("seed,k,w,n_reads,L,policy", [(41, 9, 5, 24, 1500, "small3"), (42, 9, 5, 12, 2500, "small1"), (43, 11, 7, 8, 6000, "small2"), (44, 11, 7, 40, 3000, "hifi")])
def test_fused_call_equals_the_three_calls_with_the_host_choice(seed, k, w, n_reads, L, policy):
    import test_minimizer as tm
    from vg_amd import capi, pipeline, workloads
    wl = workloads.GaplessWorkload(4, seed=seed, graph_bp=30000, n_haplotypes=4, snp_every=60, indel_every=400)
    rng = np.random.default_rng(seed)
    reads, _ = tm.sample_reads(rng, wl.nodes, wl.threads, n_reads, L)
    reads = [r for r in reads if r] + ["", "ACGT" * 3]
    reads[0] = reads[0][:40] + "Nn" + reads[0][42:]
    flat = np.frombuffer("".join(reads).encode(), dtype=np.uint8); off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    eng = engine(); P = policies()[policy]
    mi = eng.minimizer_index(wl.nodes, wl.threads, k, w)
    host = pipeline.seed_long_reads(eng, mi, flat, off, k, policy=P, threads=3, choice="host")
    dev = pipeline.seed_long_reads(eng, mi, flat, off, k, policy=P, choice="device")
    assert len(host["minimizers"]) > 64 * 4 and 0 < int(host["take"].sum()) < len(host["take"])
    for name in ("minimizer_off", "minimizers", "take", "seed_off", "seeds", "seeds_per_read"):
        assert len(dev[name]) == len(host[name]) and dev[name].tobytes() == host[name].tobytes(), name
    # too little room: VGK_EOPS with both needed sizes from one call, whichever output was short
    pol = capi.find_seeds_policy(P); n = len(off) - 1; n_m = len(host["minimizers"]); n_s = len(host["seeds"])
    for cap_m, cap_s in ((0, 0), (n_m - 1, n_s), (n_m, n_s - 1)):
        moff = np.zeros(n + 1, dtype=np.uint64); recs = np.zeros(n_m, dtype=capi.READ_MINIMIZER_DT); take = np.zeros(n_m, dtype=np.uint8)
        soff = np.zeros(n_m + 1, dtype=np.uint64); seeds = np.zeros(n_s, dtype=capi.SEED_DT); written = (ctypes.c_size_t * 2)()
        rc = eng.lib.vgk_minimizer_find_seeds(eng.h, mi.h, ctypes.byref(pol), flat.ctypes.data, off.ctypes.data, n, moff.ctypes.data, recs.ctypes.data if cap_m else None,
                                              take.ctypes.data if cap_m else None, cap_m, soff.ctypes.data if cap_m else None, seeds.ctypes.data if cap_s else None, cap_s, written)
        assert rc == capi.VGK_EOPS and (written[0], written[1]) == (n_m, n_s), (cap_m, cap_s, rc)
        assert (moff == host["minimizer_off"]).all()


@pytest.mark.gpu
def test_argument_errors():
    from vg_amd import capi
    eng = engine(); P = policies()["long_read"]
    read = np.frombuffer(b"ACGT" * 50, dtype=np.uint8); off = np.array([0, 200], dtype=np.uint64); moff = np.array([0, 3], dtype=np.uint64)
    recs = np.zeros(3, dtype=capi.READ_MINIMIZER_DT); recs["key"] = [5, 6, 7]; recs["offset"] = [0, 50, 189]; recs["hits"] = [1, 2, 3]
    assert eng.minimizer_choose(P, K, read, off, moff, recs).tolist() == [0, 0, 0]

    def refused(policy, records=recs):
        pol = capi.find_seeds_policy(policy); verdict = np.zeros(3, dtype=np.uint8)
        return eng.lib.vgk_minimizer_choose(eng.h, ctypes.byref(pol), K, read.ctypes.data, off.ctypes.data, 1, moff.ctypes.data, records.ctypes.data, verdict.ctypes.data) == capi.VGK_EINVAL
    assert refused(dict(P, hard_hit_cap=0)) and refused(dict(P, hard_hit_cap=65536))
    assert refused(dict(P, score_fraction=-0.1)) and refused(dict(P, score_fraction=1.5)) and refused(dict(P, score_fraction=float("nan")))
    late = recs.copy(); late["offset"][2] = 190                               # offset + k > read length
    assert refused(P, late)
    assert refused(dict(P, window_count=10, max_window_length=10))            # a window of 10 bases, minimizers of 11
    assert eng.minimizer_choose(dict(P, hard_hit_cap=65535), K, read, off, moff, recs).tolist() == [0, 0, 0]
