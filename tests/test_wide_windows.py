"""Long reads as windows of the resident graph: vgk_gssw_align_windows (include/vgk_engine.h; vg_amd/csrc/gssw_wide_window_api.cpp).

Windows the packed kernels refuse (more than 1024 DP rows, scores beyond 11 bits) are packed ON THE DEVICE for the wide kernels
(vg_amd/csrc/gssw_wide_pack_device.hpp).  Two things are held here:
  * without a GPU: the serial statement of the device rule gives, byte for byte, the arenas the host packer of explicit graphs (wide_pack_one,
    gssw_wide_pack.hpp) gives for the induced subgraphs of the same windows — tests/emu/wide_windows_driver.cpp runs both;
  * on the MI355X: the call's results equal the oracle's and the engine's own vgk_gssw_align on the induced subgraphs, op for op.
The corpus is one resident graph in the shape of test_gssw_wide.bubble_chain_problem (segment, two alleles, sometimes a deletion edge past
them: node 3k is a segment, 3k + 1 and 3k + 2 its alleles); reads are noisy walks from the window's first node (the wide tests' generator,
restricted to a window)."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import util
from gen import BASES
from test_windows import assert_same, graph_arrays, induced_problem_set
from vg_amd import capi

LOCAL, XDROP, PINNED, TB = capi.VGK_GSSW_LOCAL, capi.VGK_XDROP_PINNED, capi.VGK_GSSW_PINNED, capi.VGK_GSSW_TRACEBACK
VGK_EINVAL, VGK_ETOOLONG, VGK_EUNSUPPORTED = -1, capi.VGK_ETOOLONG, -8
WIDEWIN_LIB = os.path.join(util.ROOT, "tests", "emu", "libvgamd_widewin.so")
DEFAULT = (1, 4, 6, 1, 5)
WIDE_SCORES = (20, 9, 12, 3, 10)

# WideProb, NodeRec (vg_amd/csrc/gssw_wide_device.hpp, gssw_device.hpp) and the classify stage's verdict (gssw_wide_pack_device.hpp)
WIDEPROB_DT = np.dtype([(f, "<u4") for f in ("col_off", "R", "L", "prof_off", "node_off", "n_nodes", "flags", "ops_off", "ops_cap", "max_gap")] +
                       [("bonus_start", "<i4"), ("bonus_end", "<i4")] + [(f, "<u4") for f in ("K", "n_strips", "Lpad", "n_slots")] +
                       [(f, "<u8") for f in ("scratch_off", "tb_off", "carry_off", "strip_dwords")])
NODEREC_DT = np.dtype([("col_start", "<u4"), ("col_end", "<u4"), ("pred_begin", "<u4"), ("n_pred", "<u4"), ("slot", "<i4"), ("pinning", "<u4")])
META_DT = np.dtype([("status", "<i4"), ("route", "<u4"), ("need", "<u8")])
assert WIDEPROB_DT.itemsize == 96 and NODEREC_DT.itemsize == 24
CI_NODE_START, CI_STORE_END, CI_SEED_SLOW = 8, 16, 32


# ---- the corpus ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus_graph(seed=20261018, n_sites=240, seg_len=60):
    """-> (nodes, preds): about 720 nodes, about 11 k columns"""
    rng = np.random.default_rng(seed)
    nodes, preds, last = [], [], []
    for _ in range(n_sites):
        seg = "".join(BASES[i] for i in rng.integers(0, 4, int(rng.integers(seg_len // 2, seg_len + 1))))
        nodes.append(seg); preds.append(list(last))
        s = len(nodes) - 1
        nodes.append(BASES[int(rng.integers(0, 4))]); preds.append([s])
        nodes.append("".join(BASES[i] for i in rng.integers(0, 4, int(rng.integers(1, 4))))); preds.append([s])
        last = [s + 1, s + 2] if rng.random() < 0.8 else [s + 2, s + 1, s]
    return nodes, preds


def successors(preds):
    succ = [[] for _ in preds]
    for v, pr in enumerate(preds):
        for q in pr:
            succ[q].append(v)
    return succ


def walk_read(rng, nodes, succ, a, k, mode, length, sub=0.04, indel=0.02):
    """a noisy walk from the window's first node through random successors inside the window; X-drop from its first base, LOCAL after a skip of 0-30
    bases; where the walk runs out of window the rest is random bases"""
    v, ref = a, []
    total = 0
    while total < length + length // 8 + 64:
        ref.append(nodes[v]); total += len(nodes[v])
        nx = [w for w in succ[v] if w < a + k]
        if not nx:
            break
        v = nx[int(rng.integers(0, len(nx)))]
    out = []
    for c in "".join(ref):
        r = rng.random()
        if r < sub:
            out.append(BASES[int(rng.integers(0, 4))])
        elif r < sub + indel / 2:
            continue
        elif r < sub + indel:
            out.append(BASES[int(rng.integers(0, 4))]); out.append(c)
        else:
            out.append(c)
    skip = 0 if mode == XDROP else int(rng.integers(0, 31))
    read = "".join(out)[skip:skip + length]
    if len(read) < length:
        read += "".join(BASES[i] for i in rng.integers(0, 4, length - len(read)))
    return read


# the truncation cases: where a window begins and ends among (segment, first allele, second allele)
CASES = ("segment", "allele1", "allele2", "ends_on_allele1")


def place_window(nodes, case, length, near):
    """-> (first_node, n_nodes) of a window of the case that begins at or after node `near` and holds a walk of `length` bases (or runs to the graph's end)"""
    a = max(3, near - near % 3) + {"segment": 0, "allele1": 1, "allele2": 2, "ends_on_allele1": 0}[case]
    cols, b = 0, a
    while b < len(nodes) and cols < length + length // 32 + 48:
        cols += len(nodes[b]); b += 1
    if case == "ends_on_allele1":
        while (b - 1) % 3 != 1:
            b -= 1
    return a, b - a


class Windows:
    """window problems over the corpus graph: the WindowSet, the arrays behind it, which windows are walk-derived"""

    def __init__(self, nodes, preds, specs, seed):
        """specs: (first_node, n_nodes, flags, read length, read) with read None = a walk"""
        rng = np.random.default_rng(seed)
        succ = successors(preds)
        reads, self.walked = [], []
        for a, k, flags, length, read in specs:
            self.walked.append(read is None)
            reads.append(walk_read(rng, nodes, succ, a, k, flags & 15, length) if read is None else read)
        self.nodes, self.preds = nodes, preds
        self.reads = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy()
        self.read_off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
        self.first = np.array([s[0] for s in specs]); self.count = np.array([s[1] for s in specs])
        self.flags = np.array([s[2] for s in specs], dtype=np.uint32)
        self.max_gap = np.array([60 if (s[2] & 15) == XDROP else 0 for s in specs])
        col = np.concatenate([[0], np.cumsum([len(s) for s in nodes])])
        self.cols = col[np.minimum(self.first + self.count, len(nodes))] - col[self.first]
        self.n = len(specs)
        self.walked = np.array(self.walked)

    def window_set(self):
        return capi.WindowSet(self.reads, self.read_off, self.first, self.count, self.flags, self.max_gap, cols=self.cols)

    def problem_set(self, keep=None):
        keep = np.arange(self.n) if keep is None else np.asarray(keep)
        reads = [self.reads[self.read_off[i]:self.read_off[i + 1]] for i in keep]
        off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
        return induced_problem_set(self.nodes, self.preds, np.concatenate(reads), off, self.first[keep], self.count[keep], self.flags[keep], self.max_gap[keep])

    def rows(self):
        return np.diff(self.read_off) + ((self.flags & 15) == XDROP)

    def cells(self):
        return int((self.rows() * self.cols).sum())


def spec(nodes, case, mode, length, near, traceback=True):
    a, k = place_window(nodes, case, length, near)
    return (a, k, mode | (TB if traceback else 0), length, None)


LOCAL_LENGTHS = (1024, 1025, 2048, 2049, 4096, 4097)      # 1024 rows: the packed route's last; 2048 | 2049: 8 -> 16 rows per lane; 4096 | 4097: one strip -> two
XDROP_LENGTHS = (1023, 1024, 2047, 2048, 4095, 4096)      # (X-drop has one row more)


@functools.lru_cache(maxsize=None)
def limits_set():
    """one window per length at the routes' and kernels' edges; every truncation case at the two shortest lengths of a mode, in turn at the others"""
    nodes, preds = corpus_graph()
    specs, turn = [], 0
    for mode, lengths in ((LOCAL, LOCAL_LENGTHS), (XDROP, XDROP_LENGTHS)):
        for length in lengths:
            cases = CASES if length <= 1025 else (CASES[turn % 4],)
            for case in cases:
                specs.append(spec(nodes, case, mode, length, near=3 + 9 * len(specs)))
            turn += 1
    return Windows(nodes, preds, specs, seed=1)


def expected_wide(w, scores=DEFAULT):
    """which windows of the set the packed kernels do not take (the two tests of win_size_one)"""
    match, bonus = scores[0], scores[4]
    rows = w.rows(); read_len = np.diff(w.read_off)
    packed = (rows <= 1024) & (rows * match + 2 * bonus <= 2046) & ~(((w.flags & 15) == XDROP) & (read_len * match + bonus >= 1023))
    return ~packed


@functools.lru_cache(maxsize=None)
def strips_set():
    nodes, preds = corpus_graph()
    return Windows(nodes, preds, [spec(nodes, "allele2", LOCAL, 9000, 3), spec(nodes, "segment", XDROP, 9000, 9), spec(nodes, "allele1", LOCAL, 5600, 200)], seed=2)


@functools.lru_cache(maxsize=None)
def mixed_set():
    """about 60 short windows and 10 long ones in random order, two of them score-only, and five malformed ones among them
    -> (Windows, {index: expected status})"""
    nodes, preds = corpus_graph()
    rng = np.random.default_rng(3)
    specs = []
    for q in range(60):
        specs.append(spec(nodes, CASES[q % 4], (LOCAL, XDROP)[q % 2], int(rng.integers(60, 301)), int(rng.integers(3, 600)), traceback=q != 7))
    for q in range(10):
        specs.append(spec(nodes, CASES[q % 4], (LOCAL, XDROP)[q % 2], int(rng.integers(1100, 2501)), int(rng.integers(3, 400)), traceback=q != 4))
    a, k = place_window(nodes, "segment", 200, 30)
    filler = "ACGT" * 20000
    bad = {"empty": (a, 0, LOCAL | TB, 200, filler[:200]), "beyond": (len(nodes) - 4, 9, LOCAL | TB, 200, filler[:200]),
           "read_beyond": (a, k, LOCAL | TB, 200, filler[:200]), "pinned": (a, k, PINNED | TB, 200, filler[:200]),
           "too_long": (a, k, XDROP | TB, 65535, filler[:65535]), "one_node": (a, 1, LOCAL | TB, 1100, None)}
    names = [None] * len(specs) + list(bad)
    specs += list(bad.values())
    order = rng.permutation(len(specs))
    specs = [specs[j] for j in order]; names = [names[j] for j in order]
    w = Windows(nodes, preds, specs, seed=4)
    status = {names.index("empty"): VGK_EINVAL, names.index("beyond"): VGK_EINVAL, names.index("read_beyond"): VGK_EINVAL,
              names.index("pinned"): VGK_EINVAL, names.index("too_long"): VGK_ETOOLONG}
    return w, status, names.index("read_beyond")


def mixed_window_set():
    w, status, read_beyond = mixed_set()
    ws = w.window_set()
    ws.array["read_off"][read_beyond] = w.reads.size - 100             # 200 bases from 100 before the buffer's end
    return ws


@functools.lru_cache(maxsize=None)
def wide_scores_set():
    """short windows under a scoring whose scores leave 11 bits: all of them wide"""
    nodes, preds = corpus_graph()
    rng = np.random.default_rng(5)
    specs = [spec(nodes, CASES[q % 4], (LOCAL, XDROP)[q % 2], int(rng.integers(150, 401)), int(rng.integers(3, 600))) for q in range(40)]
    return Windows(nodes, preds, specs, seed=6)


@functools.lru_cache(maxsize=None)
def cases_set():
    """small windows of every truncation case and both modes, a one-node window, a window of the whole graph"""
    nodes, preds = corpus_graph()
    specs = [spec(nodes, case, mode, 90, near) for near in (3, 150, 420) for case in CASES for mode in (LOCAL, XDROP)]
    specs += [(5, 1, LOCAL | TB, 40, None), (7, 1, XDROP | TB, 40, None), (0, len(nodes), LOCAL, 300, None)]
    return Windows(nodes, preds, specs, seed=7)


# ---- without a GPU: the device rule against the host packer -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def driver():
    subprocess.check_call(["make", "-s", "widewin"], cwd=util.ROOT)
    lib = ctypes.CDLL(WIDEWIN_LIB)
    vp, u32, i32, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_size_t
    lib.vgt_wide_windows_pack.argtypes = [vp, u32, i32, i32, vp, vp, sz, vp, u32, ctypes.c_int, u32]
    lib.vgt_wide_windows_get.argtypes = [ctypes.c_int, ctypes.c_int, vp, sz]; lib.vgt_wide_windows_get.restype = sz
    lib.vgt_wide_windows_classify.argtypes = [i32, i32, u32, vp, sz, vp, u32, vp]
    return lib


def context_numbers(scores):
    """what vgk_create derives from a scoring: bias, largest score, largest bonus"""
    sc = capi.Scoring.simple(*scores)
    return sc, max(1, -min(sc.matrix)), max(max(sc.matrix), 0), scores[4]


def pack_both_ways(w, scores=DEFAULT, all_wide=False, lanes=256):
    """-> ({arena: bytes} by the device rule, the same by wide_pack_one on the induced subgraphs, the order, the windows packed)"""
    lib = driver()
    sc, bias, mx, mb = context_numbers(scores)
    node_len, seq, pred_off, pred_idx = graph_arrays(w.nodes, w.preds)
    g = np.zeros(1, dtype=capi.GRAPH_DT)
    g["n_nodes"] = len(node_len); g["node_len"] = node_len.ctypes.data; g["seq"] = seq.ctypes.data; g["pred_off"] = pred_off.ctypes.data; g["pred_idx"] = pred_idx.ctypes.data
    ws = w.window_set()
    m = lib.vgt_wide_windows_pack(ctypes.addressof(sc), bias, mx, mb, g.ctypes.data, ws.reads.ctypes.data, ws.reads.size, ws.array.ctypes.data, ws.n, int(all_wide), lanes)
    assert m >= 0, m

    def get(side, which):
        size = lib.vgt_wide_windows_get(side, which, None, 0)
        buf = np.zeros(max(size, 1), dtype=np.uint8)
        lib.vgt_wide_windows_get(side, which, buf.ctypes.data, size)
        return buf[:size]
    names = ("probs", "colinfo", "prof", "nodes", "preds")
    dev = {nm: get(0, k) for k, nm in enumerate(names)}; host = {nm: get(1, k) for k, nm in enumerate(names)}
    return dev, host, get(0, 5).view(np.uint32), m


def assert_arenas_equal(w, scores=DEFAULT, all_wide=False, lanes=256):
    dev, host, order, m = pack_both_ways(w, scores, all_wide, lanes)
    wide = np.ones(w.n, dtype=bool) if all_wide else expected_wide(w, scores)
    assert m == wide.sum() > 0
    pd, ph = dev["probs"].view(WIDEPROB_DT), host["probs"].view(WIDEPROB_DT)
    assert len(pd) == len(ph) == m
    for f in WIDEPROB_DT.names:
        assert (pd[f] == ph[f]).all(), ("WideProb." + f, np.nonzero(pd[f] != ph[f])[0][:8])
    for name in ("probs", "colinfo", "prof", "nodes", "preds"):
        assert len(dev[name]) == len(host[name]), name
        bad = np.nonzero(dev[name] != host[name])[0]
        assert len(bad) == 0, (name, "first differing byte", int(bad[0]), "of", len(dev[name]))
    assert (dev["colinfo"][-8:] == 128).all()                            # the CI_INVALID pad
    # the order: a permutation; 8 rows per lane first, then 16; each class by L * R descending, index ascending among equals
    assert sorted(order.tolist()) == list(range(m))
    keys = [(0 if pd["K"][k] == 8 else 1, -int(pd["L"][k]) * int(pd["R"][k]), int(k)) for k in order]
    assert keys == sorted(keys)
    return pd, dev


@pytest.mark.parametrize("which", ["limits", "strips", "mixed", "cases"])
def test_the_device_rule_gives_the_host_packers_arenas(which):
    if which == "mixed":
        w, status, _ = mixed_set()
        keep = [i for i in range(w.n) if i not in status]
        nodes, preds = corpus_graph()
        specs = [(int(w.first[i]), int(w.count[i]), int(w.flags[i]), int(w.read_off[i + 1] - w.read_off[i]),
                  bytes(w.reads[w.read_off[i]:w.read_off[i + 1]]).decode()) for i in keep]
        w = Windows(nodes, preds, specs, seed=0)
    else:
        w = {"limits": limits_set, "strips": strips_set, "cases": cases_set}[which]()
    if which == "cases":
        for lanes in (1, 3, 64, 256):
            assert_arenas_equal(w, all_wide=True, lanes=lanes)            # (windows the packed kernels would take: the rule itself does not care)
    else:
        pd, _ = assert_arenas_equal(w)
        if which == "limits":
            assert set(pd["K"].tolist()) == {8, 16} and set(pd["n_strips"].tolist()) == {1, 2}
        if which == "strips":
            assert sorted(pd["n_strips"].tolist()) == [2, 3, 3]


def test_the_device_rule_under_a_scoring_beyond_11_bits():
    w = wide_scores_set()
    assert expected_wide(w, WIDE_SCORES).all()
    assert_arenas_equal(w, scores=WIDE_SCORES)


def window_flags(preds, a, k, xdrop):
    """the rule, restated: per node of the window its in-window predecessors, chain, slow, store"""
    inw = [[q for q in preds[v] if q >= a] for v in range(a, a + k)]
    chain = [len(p) == 1 and p[0] == a + j - 1 for j, p in enumerate(inw)]
    slow = [(j > 0 or xdrop) and not chain[j] for j in range(k)]
    store = [False] * k
    for j in range(k):
        if slow[j]:
            for q in inw[j]:
                store[q - a] = True
    return inw, chain, slow, store


def test_the_corpus_reaches_every_truncation_case():
    nodes, preds = corpus_graph()
    _, r_chain, r_slow, r_store = window_flags(preds, 0, len(nodes), False)          # the resident graph's own flags
    seen = set()
    sets = [limits_set(), strips_set(), cases_set(), mixed_set()[0]]
    for w in sets:
        for i in range(w.n):
            a, k, xdrop = int(w.first[i]), int(w.count[i]), (int(w.flags[i]) & 15) == XDROP
            if k == 0 or a + k > len(nodes):
                continue
            inw, chain, slow, store = window_flags(preds, a, k, xdrop)
            if preds[a]:
                seen.add("a first node whose predecessors lie outside")
            if a % 3 in (1, 2):
                seen.add("a first node that is an allele")
            if a % 3 == 2 and k > 1 and chain[1] and not r_chain[a + 1]:
                seen.add("a chain link by truncation")
            if any(j > 0 and preds[a + j] and not inw[j] for j in range(k)):
                seen.add("a source inside the window")
            if (a + k - 1) % 3 == 1 and any(r_store[a + j] and not store[j] for j in range(k)):
                seen.add("a store flag dropped")
            if k == 1:
                seen.add("a one-node window")
    assert seen == {"a first node whose predecessors lie outside", "a first node that is an allele", "a chain link by truncation",
                    "a source inside the window", "a store flag dropped", "a one-node window"}
    # ... and the arenas show them: in the cases set the window that begins on a second allele has its second node without CI_SEED_SLOW
    w = cases_set()
    pd, dev = assert_arenas_equal(w, all_wide=True)
    i = next(i for i in range(w.n) if w.first[i] % 3 == 2 and (w.flags[i] & 15) == LOCAL)
    rec = dev["nodes"].view(NODEREC_DT)[pd["node_off"][i]:pd["node_off"][i] + pd["n_nodes"][i]]
    ci = dev["colinfo"][pd["col_off"][i]:pd["col_off"][i] + pd["R"][i]]
    assert rec["n_pred"][1] == 1 and ci[rec["col_start"][1]] & CI_NODE_START and not ci[rec["col_start"][1]] & CI_SEED_SLOW
    assert len(preds[int(w.first[i]) + 1]) >= 2                            # (in the resident graph it seeds from two alleles)


def test_classify_statuses_and_routes():
    w, status, _ = mixed_set()
    ws = mixed_window_set()
    nodes, _ = corpus_graph()
    col = np.concatenate([[0], np.cumsum([len(s) for s in nodes])]).astype(np.uint32)
    meta = np.zeros(ws.n, dtype=META_DT)
    _, _, mx, mb = context_numbers(DEFAULT)
    driver().vgt_wide_windows_classify(mx, mb, len(nodes), col.ctypes.data, ws.reads.size, ws.array.ctypes.data, ws.n, meta.ctypes.data)
    wide = expected_wide(w)
    for i in range(ws.n):
        assert meta["status"][i] == status.get(i, 0), i
        assert meta["route"][i] == (0 if i in status else 2 if wide[i] else 1), i
    assert (meta["need"][meta["route"] == 2] > 0).all() and (meta["need"][meta["route"] != 2] == 0).all()


def test_the_emulator_has_no_stage_for_it_yet():
    """the emulator library keeps building and answers VGK_EUNSUPPORTED: the day it gains the stage, this is revisited"""
    subprocess.check_call(["make", "-s", "emu"], cwd=util.ROOT)
    eng = capi.Engine(lib=util.EMU_LIB)
    w = cases_set()
    g = eng.graph(*graph_arrays(w.nodes, w.preds))
    with pytest.raises(capi.VgkError, match="outside the kernels' range"):
        eng.align_windows_call(g, w.window_set())
    assert eng.align_windows_last(3) == 0.0


C_TO_CTYPES = {"vgk_ctx*": ctypes.c_void_p, "const vgk_dgraph*": ctypes.c_void_p, "const char*": ctypes.c_char_p, "size_t": ctypes.c_size_t,
               "const vgk_window_problem*": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "vgk_result*": ctypes.c_void_p, "vgk_op*": ctypes.c_void_p,
               "size_t*": ctypes.POINTER(ctypes.c_size_t), "int": ctypes.c_int}


def test_header():
    """the declarations in vgk_engine.h: engine only, and argument for argument what the binding passes"""
    from test_capi_symbols import declared_symbols
    from test_seed_choice_device import engine_header_symbols
    for s in ("vgk_gssw_align_windows", "vgk_gssw_align_windows_last"):
        assert s in engine_header_symbols() and s not in declared_symbols()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(util.ROOT, "include", "vgk_engine.h")).read(), flags=re.S)
    for name, ret, argtypes in (("vgk_gssw_align_windows", "int", capi.ALIGN_WINDOWS_ARGTYPES), ("vgk_gssw_align_windows_last", "double", capi.ALIGN_WINDOWS_LAST_ARGTYPES)):
        m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m and m.group(1) == ret
        params = [" ".join(p.split()) for p in m.group(2).split(",")]
        types = [re.sub(r"\s*\w+$", "", p).replace(" *", "*") for p in params]              # drop the parameter's name
        assert [C_TO_CTYPES[t] for t in types] == argtypes, types


# ---- on the MI355X ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _engine(scores):
    return capi.Engine(capi.Scoring.simple(*scores), lib=util.ENGINE_LIB)


@functools.lru_cache(maxsize=None)
def _resident(scores):
    nodes, preds = corpus_graph()
    return _engine(scores).graph(*graph_arrays(nodes, preds))


def engine(scores=DEFAULT):
    return _engine(scores)


def resident(scores=DEFAULT):
    """the corpus graph, resident on engine(scores)'s context"""
    return _resident(scores)


def oracle_reference(which, scores=DEFAULT):
    return _oracle_reference(which, scores)


@functools.lru_cache(maxsize=None)
def _oracle_reference(which, scores):
    """the oracle on the induced subgraphs of a set's well-formed windows, computed once -> (results, ops, the windows' indices)"""
    w, keep = reference_windows(which)
    ps = w.problem_set(keep)
    res, ops = capi.Engine(capi.Scoring.simple(*scores), lib=util.ORACLE_LIB).align(ps)
    res.setflags(write=False); ops.setflags(write=False)
    # no silent skips: every walk-derived long window aligns, and well — a miss here blames the generator
    read_len = np.diff(w.read_off)[keep]
    long_walks = w.walked[keep] & (read_len > 1024) & (w.count[keep] > 1)
    assert (res["status"][long_walks] == 0).all() and (res["score"][long_walks] * 2 > read_len[long_walks] * scores[0]).all(), which
    return res, ops, keep


def reference_windows(which):
    if which == "mixed":
        w, status, _ = mixed_set()
        return w, np.array([i for i in range(w.n) if i not in status])
    w = {"limits": limits_set, "strips": strips_set, "wide_scores": wide_scores_set}[which]()
    return w, np.arange(w.n)


def engine_reference(which, scores=DEFAULT):
    return _engine_reference(which, scores)


@functools.lru_cache(maxsize=None)
def _engine_reference(which, scores):
    """the engine's own vgk_gssw_align on the same induced subgraphs"""
    w, keep = reference_windows(which)
    res, ops = engine(scores).align_call(w.problem_set(keep))
    res.setflags(write=False); ops.setflags(write=False)
    return res, ops


def ops_of(res, ops, i):
    return ops[res["ops_begin"][i]:res["ops_begin"][i] + res["n_ops"][i]].view(np.uint64)


def assert_equals_references(which, res, ops, scores=DEFAULT):
    """res / ops: the call's results for the set's well-formed windows (in their order)"""
    ro, oo, keep = oracle_reference(which, scores)
    for i in range(len(keep)):
        ctx = "%s window %d" % (which, keep[i])
        assert res["status"][i] == ro["status"][i] and res["score"][i] == ro["score"][i], ctx
        if res["status"][i] == 0 and res["score"][i] > 0:
            for f in ("end_node", "end_offset", "end_read", "first_offset", "n_ops"):
                assert res[f][i] == ro[f][i], (f, ctx)
            assert (ops_of(res, ops, i) == ops_of(ro, oo, i)).all(), ctx
    re_, oe = engine_reference(which, scores)
    assert_same(res, ops, re_, oe, which + ": the window call vs vgk_gssw_align on the induced subgraphs")


@functools.lru_cache(maxsize=None)
def limits_call():
    w = limits_set()
    eng = engine()
    res, ops = eng.align_windows_call(resident(), w.window_set())
    res.setflags(write=False); ops.setflags(write=False)
    return res, ops, [eng.align_windows_last(k) for k in range(6)]


@pytest.mark.gpu
def test_the_limits():
    w = limits_set()
    assert w.cells() < 2e8
    res, ops, last = limits_call()
    assert_equals_references("limits", res, ops)
    wide = expected_wide(w)
    assert (~wide).sum() == 4 and last[3] == wide.sum() == 20 and last[4] == 1      # (an X-drop read of 1023 bases fails win_size_one's third test under the default scoring: 1023 + 5 >= XOFF; the LOCAL 1024s are the packed route's)
    assert last[0] > 0 and last[1] > 0 and last[2] > 0 and last[5] == 8 * res["n_ops"][wide].sum()
    assert (res["status"] == 0).all() and (np.diff(res["ops_begin"]) == res["n_ops"][:-1]).all()        # the ops lie in problem order


@pytest.mark.gpu
def test_strips():
    w = strips_set()
    assert w.cells() < 2.1e8
    res, ops = engine().align_windows_call(resident(), w.window_set())
    assert_equals_references("strips", res, ops)
    assert engine().align_windows_last(3) == 3 and (res["score"] > np.diff(w.read_off) // 2).all()


@pytest.mark.gpu
def test_a_mixed_call():
    w, status, _ = mixed_set()
    ws = mixed_window_set()
    res, ops = engine().align_windows_call(resident(), ws)
    for i, st in status.items():
        assert res["status"][i] == st, i
        assert all(res[f][i] == 0 for f in ("score", "end_node", "end_offset", "end_read", "first_offset", "n_ops")), i
    _, keep = reference_windows("mixed")
    assert_equals_references("mixed", res[keep], ops)
    assert engine().align_windows_last(3) == expected_wide(w)[keep].sum() == 11
    # the ops lie in problem order, malformed windows between them taking none; two windows are score-only
    assert (res["ops_begin"] == np.concatenate([[0], np.cumsum(res["n_ops"])[:-1]])).all() and len(ops) == res["n_ops"].sum()
    score_only = [i for i in keep if not w.flags[i] & TB]
    assert len(score_only) == 2 and (res["n_ops"][score_only] == 0).all() and (res["score"][score_only] > 0).all()


@pytest.mark.gpu
def test_scores_beyond_11_bits():
    w = wide_scores_set()
    eng = engine(WIDE_SCORES)
    res, ops = eng.align_windows_call(resident(WIDE_SCORES), w.window_set())
    assert eng.align_windows_last(3) == w.n
    assert_equals_references("wide_scores", res, ops, WIDE_SCORES)
    assert (res["score"] > 2047).sum() >= 10


@pytest.mark.gpu
def test_sub_batches():
    w = limits_set()
    res, ops, _ = limits_call()
    old = os.environ.get("VGAMD_MAX_BATCH_BYTES")
    os.environ["VGAMD_MAX_BATCH_BYTES"] = str(40 << 20)
    try:
        r2, o2 = engine().align_windows_call(resident(), w.window_set())
    finally:
        if old is None:
            del os.environ["VGAMD_MAX_BATCH_BYTES"]
        else:
            os.environ["VGAMD_MAX_BATCH_BYTES"] = old
    assert engine().align_windows_last(4) >= 3
    assert r2.tobytes() == res.tobytes() and o2.tobytes() == ops.tobytes()


@pytest.mark.gpu
def test_an_op_array_that_runs_out():
    """the wide windows of the limits set, into an op array that holds the first half of their ops: as vgk_gssw_align answers the same problems"""
    w = limits_set()
    wide = np.nonzero(expected_wide(w))[0]
    nodes, preds = corpus_graph()
    sub = Windows(nodes, preds, [(int(w.first[i]), int(w.count[i]), int(w.flags[i]), 0, bytes(w.reads[w.read_off[i]:w.read_off[i + 1]]).decode()) for i in wide], seed=0)
    eng = engine()
    full, full_ops = eng.align_windows_call(resident(), sub.window_set())
    cap = int(full["n_ops"].sum()) // 2
    res, ops = eng.align_windows_call(resident(), sub.window_set(), ops_cap=cap)
    ps = sub.problem_set()
    ra = np.zeros(ps.n, dtype=capi.RESULT_DT); oa = np.zeros(cap, dtype=capi.OP_DT); written = ctypes.c_size_t()
    assert eng.lib.vgk_gssw_align(eng.h, ps.ptr, ps.n, ra.ctypes.data, oa.ctypes.data, cap, ctypes.byref(written)) == 0
    assert res.tobytes() == ra.tobytes() and ops.tobytes() == oa[:written.value].tobytes()
    out = res["status"] == capi.VGK_EOPS
    assert out.any() and (~out).any() and (res["status"][~out] == 0).all()
    assert (res["score"] == full["score"]).all() and (res["n_ops"][out] == 0).all()
    # the rule, window by window in problem order (gssw_wide_api.cpp: wide_align): a window whose ops fit what is left takes its place, one whose
    # ops do not gets VGK_EOPS and takes none — so a smaller window behind it may still fit
    at = 0
    for i in range(len(res)):
        fits = at + full["n_ops"][i] <= cap
        assert out[i] == (not fits) and res["ops_begin"][i] == at, i
        for f in ("score", "end_node", "end_offset", "end_read", "first_offset"):
            assert res[f][i] == full[f][i], (f, i)
        if fits:
            assert res["n_ops"][i] == full["n_ops"][i] and (ops_of(res, ops, i) == ops_of(full, full_ops, i)).all(), i
            at += int(full["n_ops"][i])
    assert len(ops) == at
    first_out = int(out.argmax())                                           # the windows before the first that did not fit: unchanged, every byte
    assert first_out > 0 and res[:first_out].tobytes() == full[:first_out].tobytes()


@pytest.mark.gpu
def test_a_context_reused():
    w = limits_set()
    eng = engine()
    first, first_ops = eng.align_windows_call(resident(), w.window_set())
    nodes, preds = corpus_graph()
    small = Windows(nodes, preds, [spec(nodes, "allele1", XDROP, 1300, 90), spec(nodes, "segment", LOCAL, 80, 300)], seed=8)
    rs, _ = eng.align_windows_call(resident(), small.window_set())
    assert (rs["status"] == 0).all() and rs["score"][0] > 650 and eng.align_windows_last(3) == 1
    empty = capi.WindowSet(np.zeros(1, np.uint8), [0], [], [], np.zeros(0, np.uint32), cols=[])
    re_, oe = eng.align_windows_call(resident(), empty)
    assert len(re_) == 0 and len(oe) == 0 and eng.align_windows_last(3) == 0
    last, last_ops = eng.align_windows_call(resident(), w.window_set())
    assert first.tobytes() == last.tobytes() and first_ops.tobytes() == last_ops.tobytes()


@pytest.mark.gpu
def test_a_second_graph_on_the_same_context():
    """no table of the first graph is cached: the same windows over another graph of the same shape give that graph's results"""
    nodes2, preds2 = corpus_graph(seed=77, n_sites=120)
    specs = [spec(nodes2, "allele2", LOCAL, 1500, 3), spec(nodes2, "ends_on_allele1", XDROP, 1200, 60), spec(nodes2, "segment", LOCAL, 200, 200)]
    w2 = Windows(nodes2, preds2, specs, seed=9)
    eng = engine()
    limits_call()                                                              # (the first graph has been used on this context)
    g2 = eng.graph(*graph_arrays(nodes2, preds2))
    res, ops = eng.align_windows_call(g2, w2.window_set())
    ro, oo = capi.Engine(lib=util.ORACLE_LIB).align(w2.problem_set())
    assert_same(res, ops, ro, oo, "windows of a second graph vs the oracle")
    assert (res["score"] > np.diff(w2.read_off) // 2).all() and eng.align_windows_last(3) == 2
    again, again_ops = eng.align_windows_call(resident(), limits_set().window_set())
    assert again.tobytes() == limits_call()[0].tobytes() and again_ops.tobytes() == limits_call()[1].tobytes()
