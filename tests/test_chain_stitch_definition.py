"""vgk_chain_stitch held to a definition (tests/refstitch.py) and to the limits of its launch, its output and its bounds.

Oracle (oracle/vgo_chain.c) and kernel (vg_amd/csrc/chain_device.hpp) were written from one reading of the reference's simplify and to_path: byte
parity between them (tests/test_chain_stitch.py) passes a rule both misread.  Here the expectation is refstitch's — per base, from what a path
means —, made once per corpus (lru_cache) and shared by three drivers: the oracle, the emulated kernel, and the HIP kernel under -m gpu.

    1  cut-invariance     a truth alignment along an arbitrary walk, cut anywhere into ALIGNMENT / PATH pieces: the answer is the uncut truth's
    2  the old generator  test_chain_stitch.random_pieces with LINK pieces: every status-0 read inside the definition's domain equals it
    3  reach              which special cases of the streaming kernel the corpus of 1 contains (generator and reference alone), each > 0
    4  edges              n_reads around the launch's blocks, reads without pieces, one read of ~20 000 pieces, caps at / under / inside / 0
    5  malformed pieces   ranges past their arrays by 1 and near 2^32, bad links, kinds, nodes: that read VGK_EINVAL, every other untouched
    6  bounds past 2^32   valid pieces whose bounds sum past what the 32-bit prefix sums hold: VGK_ETOOBIG or the right answer
    7  the same calls (LINK-free) as a program of its own under AddressSanitizer and UBSan (make chainstitch_san)

The malformed and wrapping calls of 5 and 6 went through the emulator and the sanitizer program before any of them went to a GPU."""
import ctypes
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import refstitch
import util
from refstitch import DEL, INS, MATCH, MISMATCH, NO_NODE
from test_chain_stitch import flat, path_pieces, random_pieces, hand_cases, golden_paths
from test_wfa import random_wfa_case
from vg_amd import capi

OK, EINVAL, ENOMEM, EOPS, ETOOBIG = capi.VGK_OK, capi.VGK_EINVAL, capi.VGK_ENOMEM, capi.VGK_EOPS, capi.VGK_ETOOBIG
PIECE, MAPPING, RESULT = capi.CHAIN_PIECE_DT, capi.CHAIN_MAPPING_DT, capi.CHAIN_RESULT_DT


def build_emu():
    subprocess.check_call(["make", "-s", "-j8", "emu", "oracle"], cwd=util.ROOT)


def lib_of(which, build=True):
    """the library behind a driver; the CPU libraries are made here unless the caller is a GPU test (which builds nothing: they are there)"""
    if which != "gpu" and build:
        build_emu()
    return {"oracle": util.ORACLE_LIB, "emu": util.EMU_LIB, "gpu": util.ENGINE_LIB}[which]


DRIVERS = ["oracle", "emu", pytest.param("gpu", marks=pytest.mark.gpu)]
ENGINES = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]


class Call:
    """one vgk_chain_stitch call's inputs"""

    def __init__(self, node_len, pieces, off, nodes=(), mappings=(), edits=()):
        self.node_len = list(node_len)
        self.pieces = np.ascontiguousarray(pieces, dtype=PIECE); self.off = np.ascontiguousarray(off, dtype=np.uint64)
        self.nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        self.mappings = np.ascontiguousarray(mappings if len(mappings) else [], dtype=MAPPING)
        self.edits = np.ascontiguousarray(edits, dtype=np.uint32)
        self.n = len(self.off) - 1

    def index(self, eng):
        return eng.haplo_index(["A" * n for n in self.node_len], [list(range(0, 2 * len(self.node_len), 2))])

    def read(self, r, links=None):
        return refstitch.pieces_of(self.pieces, self.off, r, self.nodes, self.mappings, self.edits, links)

    def oriented_len(self):
        return [self.node_len[o // 2] for o in range(2 * len(self.node_len))]


class Answer:
    def __init__(self, rc, written, res, om, oe, mcap, ecap):
        self.rc, self.written, self.res, self.om, self.oe, self.mcap, self.ecap = rc, written, res, om, oe, mcap, ecap

    def read(self, r):
        return flat(self.res, self.om, self.oe, r)

    def fits(self, r):
        return int(self.res["mapping_begin"][r]) + int(self.res["n_mappings"][r]) <= self.mcap and int(self.res["edit_begin"][r]) + int(self.res["n_edits"][r]) <= self.ecap

    def same_as(self, other):
        """status, sizes and places of every read; mappings and runs of every read that fits (what lies behind a read that does not fit is not stated)"""
        if (self.rc, self.written) != (other.rc, other.written) or self.res.tobytes() != other.res.tobytes():
            return False
        if self.rc == OK:
            return self.om.tobytes() == other.om.tobytes() and self.oe.tobytes() == other.oe.tobytes()
        return all(self.read(r) == other.read(r) for r in range(len(self.res)) if self.res["status"][r] == OK and self.fits(r))


def stitch(eng, idx, c, mapping_cap=None, edit_cap=None):
    """the C call itself (capi.Engine.chain_stitch raises on the statuses this file is about); without caps: room for the totals, asked for first"""
    res = np.zeros(c.n, dtype=RESULT)

    def once(mcap, ecap):
        om = np.zeros(max(mcap, 1), dtype=MAPPING); oe = np.zeros(max(ecap, 1), dtype=np.uint32)
        written = (ctypes.c_size_t * 2)()
        rc = eng.lib.vgk_chain_stitch(eng.h, idx.h, c.pieces.ctypes.data if len(c.pieces) else None, c.off.ctypes.data, c.n, c.nodes.ctypes.data if len(c.nodes) else None, len(c.nodes),
                                      c.mappings.ctypes.data if len(c.mappings) else None, len(c.mappings), c.edits.ctypes.data if len(c.edits) else None, len(c.edits),
                                      res.ctypes.data, om.ctypes.data if mcap else None, mcap, oe.ctypes.data if ecap else None, ecap, ctypes.byref(written))
        w = (int(written[0]), int(written[1]))
        return Answer(rc, w, res.copy(), om[:min(w[0], mcap)], oe[:min(w[1], ecap)], mcap, ecap)
    if mapping_cap is not None:
        return once(mapping_cap, edit_cap)
    a = once(0, 0)
    return once(*a.written) if a.rc == EOPS else a


def run_call(which, c, **caps):
    eng = capi.Engine(lib=lib_of(which))
    return stitch(eng, c.index(eng), c, **caps)


def equals_definition(a, r, want):
    maps, frm, to = want
    got = refstitch.merge_insertions(a.read(r))
    return a.res["status"][r] == OK and got == maps and int(a.res["from_length"][r]) == frm and int(a.res["to_length"][r]) == to


# ---- the hand cases and the reference's vectors, re-derived from the definition ------------------------------------------------------------------
def test_the_definition_gives_the_hand_cases_and_the_reference_vectors():
    """the eight hand cases' expectations (tests/test_chain_stitch.py) and ref_simplify.json's two path cases, from refstitch alone"""
    for case, want in hand_cases():
        read = [("path", [(n, o, e) for n, o, e in case])]
        assert refstitch.in_domain(read), case
        got = refstitch.refstitch(read, [20] * 16)[0]
        assert got == refstitch.merge_insertions([(NO_NODE if n is None else n, o, e) for n, o, e in want]), (case, got)
    cases = golden_paths()
    assert len(cases) == 3
    lens = [20] * 140
    c0, p0 = cases[0]
    assert refstitch.in_domain([("path", p0)])
    assert refstitch.refstitch([("path", p0)], lens)[0] == [(134, 0, [(MATCH, 1), (INS, 4)]), (132, 0, [(DEL, 3)]), (130, 0, [(MATCH, 17)])]
    for c, p in cases:
        if not refstitch.in_domain([("path", p)]):
            continue
        got = refstitch.refstitch([("path", p)], lens)[0]; e = c["expect"]
        assert len(got) == e["mapping_size"], c["source"]
        if e["node_ids"]:
            assert [g[0] // 2 + 1 for g in got] == e["node_ids"], c["source"]
        for k, n in e["edit_sizes"].items():
            assert len(got[int(k)][2]) == n, c["source"]
    assert sum(refstitch.in_domain([("path", p)]) for _, p in cases) >= 2
    # trimming BEFORE segmenting would be wrong: the bare insertion stays on the deleted node, behind the deleted bases
    assert refstitch.refstitch([("path", [(0, 0, [(DEL, 20)]), (None, 0, [(INS, 3)])])], lens) == ([(0, 20, [(INS, 3)])], 0, 3)


# ---- 1. cut-invariance ------------------------------------------------------------------------------------------------------------------------------
def rle(kinds):
    out = []
    for k in kinds:
        if out and out[-1][0] == k:
            out[-1][1] += 1
        else:
            out.append([k, 1])
    return [(k, n) for k, n in out]


class Builder:
    """the flat arrays of a call, piece by piece"""

    def __init__(self):
        self.pieces, self.off, self.nodes, self.mappings, self.edits = [], [0], [], [], []

    def runs(self, rs):
        b = len(self.edits); self.edits += [(n << 2) | k for k, n in rs]
        return b, len(rs)

    def alignment(self, path, node_offset, rs):
        eb, ne = self.runs(rs)
        self.pieces.append((capi.PIECE_ALIGNMENT, 0, node_offset, len(self.nodes), len(path), eb, ne, 0)); self.nodes += path

    def path(self, ms):
        self.pieces.append((capi.PIECE_PATH, 0, 0, len(self.mappings), len(ms), 0, 0, 0))
        for node, offset, rs in ms:
            eb, ne = self.runs(rs)
            self.mappings.append((NO_NODE if node is None else node, offset, eb, ne))

    def end_read(self):
        self.off.append(len(self.pieces))

    def call(self, node_len):
        return Call(node_len, np.array(self.pieces, dtype=PIECE) if self.pieces else np.zeros(0, dtype=PIECE), self.off, self.nodes,
                    np.array(self.mappings, dtype=MAPPING) if self.mappings else np.zeros(0, dtype=MAPPING), self.edits)


def random_truth(rng, olen):
    """an alignment of 1-14 runs along an arbitrary walk (stitch checks no edges: repeats and self-loops included) -> per-base events"""
    ev = []
    node = int(rng.integers(0, len(olen)))
    at = int(rng.integers(0, olen[node]))
    last = None
    for _ in range(int(rng.integers(1, 15))):
        kind = int(rng.choice([k for k in (MATCH, MISMATCH, INS, DEL) if k != last])); last = kind
        for _ in range(int(rng.integers(1, 7))):
            if kind == INS:
                ev.append((INS,)); continue
            if at == olen[node]:
                node, at = (node if rng.random() < 0.2 else int(rng.integers(0, len(olen)))), 0
            ev.append((kind, node, at)); at += 1
    return ev


def aln_of(ev, olen):
    """events that follow a walk -> the neutral "aln" piece: the nodes touched, the first graph base's offset, the runs"""
    graph = [e for e in ev if e[0] != INS]
    path = [e[1] for i, e in enumerate(graph) if i == 0 or graph[i - 1][2] == olen[graph[i - 1][1]] - 1]
    return ("aln", path, graph[0][2] if graph else 0, rle([e[0] for e in ev]))


def split_runs(rng, rs, zero=False):
    """runs left unmerged now and then; for stated mappings, zero-length runs sprinkled in"""
    out = []
    for k, n in rs:
        if zero and rng.random() < 0.15:
            out.append((int(rng.integers(0, 4)), 0))
        if n > 1 and rng.random() < 0.25:
            a = int(rng.integers(1, n)); out += [(k, a), (k, n - a)]
        else:
            out.append((k, n))
    if zero and rng.random() < 0.1:
        out.append((int(rng.integers(0, 4)), 0))
    return out


def cut_read(rng, b, ev, olen):
    """the truth cut at random points — node ends and the inside of runs included — into ALIGNMENT and PATH pieces"""
    n = len(ev)
    cuts = sorted(set(int(x) for x in rng.integers(1, n, size=int(rng.integers(0, 6)))) if n > 1 else [])
    ends = [i + 1 for i, e in enumerate(ev[:-1]) if e[0] != INS and e[2] == olen[e[1]] - 1]
    if ends and rng.random() < 0.5:
        cuts = sorted(set(cuts + [ends[int(rng.integers(0, len(ends)))]]))
    seen_graph = False
    for a, z in zip([0] + cuts, cuts + [n]):
        chunk = ev[a:z]
        graph = [e for e in chunk if e[0] != INS]
        if not graph:                                   # insertions only: unlocalized, or a mapping without a position
            if rng.random() < 0.5:
                b.alignment([], 0, [(INS, len(chunk))])
            else:
                k = int(rng.integers(1, len(chunk))) if len(chunk) > 1 and rng.random() < 0.4 else len(chunk)
                b.path([(None, 0, split_runs(rng, [(INS, k)], zero=True))] + ([(None, 0, [(INS, len(chunk) - k)])] if k < len(chunk) else []))
        elif rng.random() < 0.5:
            _, path, off, rs = aln_of(chunk, olen)
            b.alignment(path, off, split_runs(rng, rs))
        else:                                           # stated mappings: split at every node change, and at random
            groups, cur = [], []
            for i, e in enumerate(chunk):
                prev = next((x for x in reversed(chunk[:i]) if x[0] != INS), None)
                must = e[0] != INS and prev is not None and (e[1] != prev[1] or e[2] != prev[2] + 1)
                if cur and (must or rng.random() < 0.15):
                    groups.append(cur); cur = []
                cur.append(e)
            groups.append(cur)
            ms, had = [], seen_graph
            for g in groups:
                where = next((e for e in g if e[0] != INS), None)
                rs = split_runs(rng, rle([e[0] for e in g]), zero=True)
                if where:
                    ms.append((where[1], where[2], rs)); had = True
                elif had and rng.random() < 0.3:        # insertions standing on a mapping with some position of its own: behind a graph event, inside the domain
                    ms.append((int(rng.integers(0, len(olen))), int(rng.integers(0, 3)), rs))
                else:
                    ms.append((None, 0, rs))
                if rng.random() < 0.08:                 # a mapping without edits
                    ms.append((int(rng.integers(0, len(olen))) if rng.random() < 0.5 else None, 0, []))
            b.path(ms)
        seen_graph = seen_graph or bool(graph)
    b.end_read()


@functools.lru_cache(maxsize=None)
def cut_corpus(seed, n_reads=3000):
    """-> (call, per read the definition's answer for the UNCUT truth, per read the truth's events)"""
    rng = np.random.default_rng(seed)
    node_len = [int(x) for x in rng.integers(1, 9, size=int(rng.integers(8, 17)))]
    olen = [node_len[o // 2] for o in range(2 * len(node_len))]
    b = Builder(); want = []; truths = []
    for _ in range(n_reads):
        ev = random_truth(rng, olen)
        truths.append(ev)
        want.append(refstitch.refstitch([aln_of(ev, olen)], olen))
        cut_read(rng, b, ev, olen)
    return b.call(node_len), want, truths


CUT_SEEDS = (11, 12, 13)


@functools.lru_cache(maxsize=None)
def oracle_answer(seed):
    ora = capi.Engine(lib=util.ORACLE_LIB)
    c = cut_corpus(seed)[0]
    return stitch(ora, c.index(ora), c)


@pytest.mark.parametrize("which", DRIVERS)
@pytest.mark.parametrize("seed", CUT_SEEDS)
def test_cut_invariance(seed, which):
    """3 000 truths per seed, one call each: wherever and into whatever pieces a truth is cut, the answer is refstitch of the uncut truth"""
    c, want, _ = cut_corpus(seed)
    a = run_call(which, c)
    assert a.rc == OK
    wrong = [r for r in range(c.n) if not equals_definition(a, r, want[r])]
    assert not wrong, (seed, which, len(wrong), wrong[:3], [(c.read(r), a.read(r), want[r]) for r in wrong[:2]])
    # (which insertion runs stay side by side is the one thing the definition leaves open: there the oracle's bytes decide)
    assert which == "oracle" or a.same_as(oracle_answer(seed)), (seed, which)


def test_the_cut_reads_lie_in_the_domain_and_mean_their_truths():
    """the generator's own sanity: every cut read is inside the domain, and the definition is cut-invariant on it"""
    c, want, _ = cut_corpus(CUT_SEEDS[0])
    olen = c.oriented_len()
    for r in range(0, c.n, 7):
        read = c.read(r)
        assert refstitch.in_domain(read) and refstitch.refstitch(read, olen) == want[r], (r, read)


# ---- 2. the existing generator under the definition -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def old_generator_case(seed, n_reads=150):
    """-> (nodes, threads, wfa problems, the oracle's wfa results, the call, per read None | the definition's answer)"""
    rng = np.random.default_rng(seed)
    nodes, threads, wp = random_wfa_case(rng, 80)
    ora = capi.Engine(lib=util.ORACLE_LIB); oi = ora.haplo_index(nodes, threads)
    links = ora.wfa_extend(oi, wp)
    pieces, off, pn, pm, pe = random_pieces(np.random.default_rng(seed + 1000), ora, oi, nodes, links[0], n_reads)
    c = Call([len(s) for s in nodes], pieces, off, pn, pm, pe)
    olen = c.oriented_len()
    want = []
    for r in range(c.n):
        try:
            read = c.read(r, links)
            want.append(refstitch.refstitch(read, olen) if refstitch.in_domain(read) else None)
        except refstitch.Malformed:
            want.append(None)
    return nodes, threads, wp, links, c, want


def check_old_generator(which, seeds, forms):
    in_domain = status0 = n_links = 0
    lib_of(which)
    for seed in seeds:
        nodes, threads, wp, links, c, want = old_generator_case(seed)
        for form in forms:
            eng = capi.Engine(lib=lib_of(which)); idx = eng.haplo_index(nodes, threads)
            if which != "oracle":
                eng.lib.vgk_wfa_set_form(eng.h, form)
            mine = eng.wfa_extend(idx, wp)
            a = stitch(eng, idx, c)
            assert a.rc == OK
            for r in range(c.n):
                if a.res["status"][r] != OK:
                    continue
                status0 += 1
                if want[r] is None:
                    continue
                k = int((c.pieces["kind"][int(c.off[r]):int(c.off[r + 1])] == capi.PIECE_LINK).sum())
                if k:                                   # (what the definition was made from is what THIS engine's wfa_extend returned to the host, too)
                    n_links += k
                    assert c.read(r, mine) == c.read(r, links), (seed, form, r)
                in_domain += 1
                assert equals_definition(a, r, want[r]), (seed, form, r, c.read(r, links), a.read(r), want[r])
    print("status-0 reads %d, inside the domain %d (%.1f %%), with LINK pieces %d" % (status0, in_domain, 100.0 * in_domain / status0, n_links))
    assert in_domain >= 0.8 * status0 and n_links > 100


def test_old_generator_equals_the_definition_oracle():
    check_old_generator("oracle", range(12), (0,))


def test_old_generator_equals_the_definition_emulated():
    check_old_generator("emu", range(12), (0, 1, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("form", (0, 2))
def test_old_generator_equals_the_definition_on_the_gpu(form):
    check_old_generator("gpu", range(12), (form,))


# ---- 3. what the corpus reaches ------------------------------------------------------------------------------------------------------------------------
def stated_mappings(read, olen):
    """the mappings a read's pieces state, one after the other, runs of one kind merged: (node | None, offset, [(kind, n)...]).  An "aln" piece's
    are its walk's (a new one at every node the walk enters)."""
    out = []
    for p in read:
        if p[0] == "path":
            out += [(node, off, rle([k for k, n in rs for _ in range(n)])) for node, off, rs in p[1]]
            continue
        _, path, at, rs = p
        if not path:
            out.append((None, 0, rle([k for k, n in rs for _ in range(n)]))); continue
        step, kinds, start = 0, [], at
        for k, n in rs:
            for _ in range(n):
                kinds.append(k)
                if k != INS:
                    at += 1
                    if at == olen[path[step]]:
                        step += 1
                        if step < len(path):
                            out.append((path[step - 1], start, rle(kinds))); kinds, start, at = [], 0, 0
        if step < len(path) or kinds:
            out.append((path[min(step, len(path) - 1)], start, rle(kinds)))
    return [m for m in out if m[2]]


def census(read, olen, seen):
    """which of the streaming kernel's special cases a read goes through, from its stated mappings and the definition's segments alone"""
    ms = stated_mappings(read, olen)
    ev = refstitch.events(read, olen)
    segs = refstitch.segments(ev)
    base = lambda s: any(e[0] != DEL for e in s)
    kept = [s for s in segs]
    if not any(base(s) for s in segs):
        seen["an empty result"] += 1
        return
    front = 0
    while not base(kept[0]):
        kept.pop(0); front += 1
    back = 0
    while not base(kept[-1]):
        kept.pop(); back += 1
    seen["dropped deletion-only mappings at the front"] += front > 0
    seen["dropped deletion-only mappings at the back"] += back > 0
    seen["a trimmed leading deletion, offset moved"] += kept[0][0][0] == DEL
    seen["one mapping keeping a trailing deletion"] += len(kept) == 1 and kept[0][-1][0] == DEL
    # the last mapping kept, as the kernel's registers hold it: node, offset, graph bases, last run's kind, insertion runs side by side
    l = None
    for node, off, rs in ms:
        if l is None:
            l = dict(node=node, off=off, frm=sum(n for k, n in rs if k != INS), last=rs[-1][0], mixed=False); continue
        moved = rs[0][0] == INS
        if moved:
            seen["an insertion moved onto the previous mapping"] += 1
            if l["last"] == INS:
                l["mixed"] = True
            l["last"] = INS; rs = rs[1:]
        if l["node"] is None and node is not None:
            seen["a leading position-less mapping taking the next one's position"] += 1
            l["node"], l["off"] = node, off
        elif node is None and l["node"] is not None:
            node, off = l["node"], l["frm"]
        joins = (l["node"] is None and node is None) or (l["node"] is not None and node is not None and l["node"] == node and l["off"] + l["frm"] == off)
        if joins:
            if rs:
                if l["mixed"]:
                    seen["a join after side-by-side insertions"] += 1
                else:
                    seen["a join whose meeting runs merge" if rs[0][0] == l["last"] else "a join whose meeting runs do not merge"] += 1
                seen["a join of a single run" if len(rs) == 1 else "a join of several runs"] += 1
                l["last"] = rs[-1][0]
            l["mixed"] = False if rs or l["mixed"] else l["mixed"]
            l["frm"] += sum(n for k, n in rs if k != INS)
        elif rs:
            if l["node"] is not None and l["node"] == node and off == 0 and l["off"] + l["frm"] == olen[node]:
                seen["a self-loop that must not join"] += 1
            seen["insertion runs left side by side"] += l["mixed"]
            l = dict(node=node, off=off, frm=sum(n for k, n in rs if k != INS), last=rs[-1][0], mixed=False)
    seen["insertion runs left side by side"] += l is not None and l["mixed"]


REACH = ["an empty result", "one mapping keeping a trailing deletion", "a trimmed leading deletion, offset moved", "dropped deletion-only mappings at the front",
         "dropped deletion-only mappings at the back", "an insertion moved onto the previous mapping", "insertion runs left side by side",
         "a join whose meeting runs merge", "a join whose meeting runs do not merge", "a join after side-by-side insertions", "a join of a single run",
         "a join of several runs", "a leading position-less mapping taking the next one's position", "a self-loop that must not join"]


def test_what_the_corpus_reaches():
    """from generator and reference alone, on the seeds of test_cut_invariance: every special case of the streaming kernel is there, counted"""
    seen = {k: 0 for k in REACH}
    for seed in CUT_SEEDS:
        c, _, _ = cut_corpus(seed)
        olen = c.oriented_len()
        for r in range(c.n):
            census(c.read(r), olen, seen)
    for k in REACH:
        print("%6d  %s" % (seen[k], k))
    assert all(seen[k] > 0 for k in REACH), seen


# ---- 4. edges of the launch and of the output ---------------------------------------------------------------------------------------------------
def sub_call(c, reads):
    """the call made of the given reads of c (None: a read without pieces), over c's arrays"""
    pieces, off = [], [0]
    for r in reads:
        if r is not None:
            pieces += [c.pieces[k] for k in range(int(c.off[r]), int(c.off[r + 1]))]
        off.append(len(pieces))
    return Call(c.node_len, np.array(pieces, dtype=PIECE) if pieces else np.zeros(0, dtype=PIECE), off, c.nodes, c.mappings, c.edits)


@pytest.mark.parametrize("which", ENGINES)
def test_launch_sizes_and_reads_without_pieces(which):
    """n_reads on either side of the stitch kernel's 64 lanes and the gather's 4 reads per block; reads without pieces between the others, and alone"""
    c, want, _ = cut_corpus(CUT_SEEDS[0])
    ora = capi.Engine(lib=lib_of("oracle", which != "gpu")); eng = capi.Engine(lib=lib_of(which))
    oi, ei = c.index(ora), c.index(eng)
    for n in (1, 3, 4, 5, 63, 64, 65, 257):
        reads = list(range(100, 100 + n))
        for k in range(0, n, 5):
            if n > 1 and k % 2:
                reads[k] = None
        s = sub_call(c, reads)
        a, o = stitch(eng, ei, s), stitch(ora, oi, s)
        assert a.rc == OK and a.same_as(o), n
        for j, r in enumerate(reads):
            assert equals_definition(a, j, want[r] if r is not None else ([], 0, 0)), (n, j)
    for n in (1, 5, 65):
        s = sub_call(c, [None] * n)
        a, o = stitch(eng, ei, s), stitch(ora, oi, s)
        assert a.rc == OK and a.written == (0, 0) and a.same_as(o) and not a.res["n_mappings"].any() and not a.res["status"].any(), n


@functools.lru_cache(maxsize=None)
def long_read_case():
    """one read of ~20 000 pieces — the cut pieces of the corpus's reads behind each other — between ordinary reads: its answer is the definition's for
    the truths behind each other"""
    c, want, truths = cut_corpus(21, 9000)
    olen = c.oriented_len()
    take = 0
    while int(c.off[take]) < 20000:
        take += 1
    assert take + 80 <= c.n
    pieces = [c.pieces[k] for k in range(int(c.off[take]))]
    long_want = refstitch.refstitch([aln_of(ev, olen) for ev in truths[:take]], olen)
    lead, trail = list(range(take, take + 40)), list(range(take + 40, take + 80))
    s = sub_call(c, lead + [None] + trail)
    at = int(s.off[len(lead)])
    s = Call(c.node_len, np.concatenate([s.pieces[:at], np.array(pieces, dtype=PIECE), s.pieces[at:]]),
             np.concatenate([s.off[:len(lead) + 1], s.off[len(lead) + 1:] + np.uint64(len(pieces))]), c.nodes, c.mappings, c.edits)
    return s, [want[r] for r in lead] + [long_want] + [want[r] for r in trail]


@pytest.mark.parametrize("which", DRIVERS)
def test_one_read_of_twenty_thousand_pieces(which):
    """the gather's stride beyond 64 mappings, stretch offsets far into the work arrays"""
    s, want = long_read_case()
    assert int(s.off[41] - s.off[40]) >= 20000 and len(want[40][0]) > 20000
    a = run_call(which, s)
    assert a.rc == OK
    for r in range(s.n):
        assert equals_definition(a, r, want[r]), r


@pytest.mark.parametrize("which", ENGINES)
def test_caps_at_under_inside_and_zero(which):
    """mapping_cap / edit_cap at exactly the totals, one short of each, cut inside read k, and 0: `written` reports the totals, reads before the first
    that does not fit equal the full call, reads from it on carry VGK_EOPS with their sizes, the call answers VGK_EOPS — and all of it is the oracle's"""
    c, want, _ = cut_corpus(CUT_SEEDS[2])
    s = sub_call(c, range(200, 265))
    ora = capi.Engine(lib=lib_of("oracle", which != "gpu")); eng = capi.Engine(lib=lib_of(which))
    oi, ei = s.index(ora), s.index(eng)
    full = stitch(eng, ei, s)
    M, E = full.written
    assert full.rc == OK and M > 65 and E > M
    k = next(r for r in range(20, s.n) if full.res["n_mappings"][r] >= 2 and full.res["n_edits"][r] >= 2)
    inside_m = int(full.res["mapping_begin"][k]) + 1; inside_e = int(full.res["edit_begin"][k]) + 1
    for mcap, ecap in ((M, E), (M - 1, E), (M, E - 1), (inside_m, E), (M, inside_e), (0, E), (M, 0), (0, 0)):
        a, o = stitch(eng, ei, s, mapping_cap=mcap, edit_cap=ecap), stitch(ora, oi, s, mapping_cap=mcap, edit_cap=ecap)
        assert a.written == (M, E) and a.same_as(o), (mcap, ecap)
        end_m = full.res["mapping_begin"].astype(np.int64) + full.res["n_mappings"]; end_e = full.res["edit_begin"].astype(np.int64) + full.res["n_edits"]
        misfit = np.nonzero((end_m > mcap) | (end_e > ecap))[0]
        first = int(misfit[0]) if len(misfit) else s.n
        assert a.rc == (EOPS if first < s.n else OK), (mcap, ecap)
        for r in range(s.n):
            for f in ("mapping_begin", "n_mappings", "edit_begin", "n_edits", "from_length", "to_length"):
                assert a.res[f][r] == full.res[f][r], (mcap, ecap, r, f)
            if r < first:
                assert a.res["status"][r] == OK and a.read(r) == full.read(r) and equals_definition(a, r, want[200 + r]), (mcap, ecap, r)
            else:
                assert a.res["status"][r] == EOPS, (mcap, ecap, r)


# ---- 5. malformed piece lists -------------------------------------------------------------------------------------------------------------------
BIG = 0xffffffff


def malformed_cases():
    """name -> (call with the bad read(s), the indexes of the bad reads, needs a wfa_extend call before)"""
    c, _, _ = cut_corpus(CUT_SEEDS[0])
    base = sub_call(c, range(300, 310))
    n_or = 2 * len(c.node_len)
    nn, nm, ne = len(c.nodes), len(c.mappings), len(c.edits)
    # stated mappings of the bad PATH pieces, behind the corpus's own (which stay where they are)
    extra = [(0, 0, ne, 1), (0, 0, 1, BIG), (n_or, 0, 0, 1), (0, 0, 0, 1), (0, 0, BIG - 1, 2)]
    A, P, L = capi.PIECE_ALIGNMENT, capi.PIECE_PATH, capi.PIECE_LINK
    good_a = tuple(int(x) for x in next(p for p in base.pieces if p["kind"] == A and p["path_len"] > 0))
    bad = {
        "alignment_path_past_by_1": (A, 0, 0, nn, 1, 0, 1, 0),
        "alignment_path_len_past_by_1": (A, 0, 0, 1, nn, 0, 1, 0),
        "alignment_edits_past_by_1": (A, 0, 0, 0, 1, ne, 1, 0),
        "alignment_path_near_2_32": (A, 0, 0, 1, BIG, 0, 1, 0),
        "alignment_path_begin_near_2_32": (A, 0, 0, BIG - 15, 0x20, 0, 1, 0),
        "alignment_edits_near_2_32": (A, 0, 0, 0, 1, 1, BIG, 0),
        "alignment_both_near_2_32": (A, 0, 0, BIG, BIG, BIG, BIG, 0),
        "path_past_by_1": (P, 0, 0, nm + len(extra), 1, 0, 0, 0),
        "path_near_2_32": (P, 0, 0, 1, BIG, 0, 0, 0),
        "path_begin_near_2_32": (P, 0, 0, BIG, 2, 0, 0, 0),
        "mapping_edits_past_by_1": (P, 0, 0, nm + 0, 1, 0, 0, 0),
        "mapping_n_edits_ffffffff": (P, 0, 0, nm + 1, 1, 0, 0, 0),
        "mapping_edit_begin_near_2_32": (P, 0, 0, nm + 4, 1, 0, 0, 0),
        "mapping_behind_a_good_one": (P, 0, 0, nm + 3, 2, 0, 0, 0),
        "mapping_node_past_the_index": (P, 0, 0, nm + 2, 1, 0, 0, 0),
        "link_without_a_call": (L, 0, 0, 0, 0, 0, 0, 0),
        "link_beyond_the_call": (L, 1, 0, 0, 0, 0, 0, 0),
        "link_ffffffff": (L, BIG, 0, 0, 0, 0, 0, 0),
        "kind_3": (3,) + good_a[1:],
        "kind_ffffffff": (BIG,) + good_a[1:],
    }
    out = {}
    for name, pc in bad.items():
        pieces = np.concatenate([base.pieces[:int(base.off[5])], np.array([pc], dtype=PIECE), base.pieces[int(base.off[5]):]])
        off = np.concatenate([base.off[:6], base.off[5:] + np.uint64(1)])
        out[name] = (Call(c.node_len, pieces, off, c.nodes, np.concatenate([c.mappings, np.array(extra, dtype=MAPPING)]), c.edits), [5], name == "link_beyond_the_call")
    # a good piece first, then the bad one: what the good one made is dropped with the read
    pieces = np.concatenate([base.pieces[:int(base.off[5])], np.array([good_a, bad["alignment_path_near_2_32"]], dtype=PIECE), base.pieces[int(base.off[5]):]])
    out["bad_behind_a_good_piece"] = (Call(c.node_len, pieces, np.concatenate([base.off[:6], base.off[5:] + np.uint64(2)]), c.nodes, c.mappings, c.edits), [5], False)
    # a node beyond the index: first on an alignment's path, and where its walk arrives later
    b = Builder()
    for r in range(3):
        b.alignment([0], 0, [(MATCH, 1)]); b.end_read()
    b.alignment([n_or], 0, [(MATCH, 1)]); b.end_read()
    b.alignment([0, BIG - 1], 0, [(MATCH, c.node_len[0] + 1)]); b.end_read()
    for r in range(3):
        b.alignment([1], 0, [(MISMATCH, 1)]); b.end_read()
    out["alignment_node_past_the_index"] = (b.call(c.node_len), [3, 4], False)
    # the wrap of the 32-bit prefix sums by refused pieces: four reads of path_len 0x3fffffff over a `nodes` array of one entry, six valid reads behind
    b = Builder()
    b.nodes.append(0)
    for r in range(4):
        b.pieces.append((A, 0, 0, 0, 0x3fffffff, 0, 1, 0)); b.end_read()
    b.edits.append((1 << 2) | MATCH)
    for r in range(6):
        b.pieces.append((A, 0, 0, 0, 1, 0, 1, 0)); b.end_read()
    out["four_reads_of_3fffffff"] = (b.call(c.node_len), [0, 1, 2, 3], False)
    return out


MALFORMED = ["alignment_path_past_by_1", "alignment_path_len_past_by_1", "alignment_edits_past_by_1", "alignment_path_near_2_32", "alignment_path_begin_near_2_32",
             "alignment_edits_near_2_32", "alignment_both_near_2_32", "path_past_by_1", "path_near_2_32", "path_begin_near_2_32", "mapping_edits_past_by_1",
             "mapping_n_edits_ffffffff", "mapping_edit_begin_near_2_32", "mapping_behind_a_good_one", "mapping_node_past_the_index", "link_without_a_call",
             "link_beyond_the_call", "link_ffffffff", "kind_3", "kind_ffffffff", "bad_behind_a_good_piece", "alignment_node_past_the_index", "four_reads_of_3fffffff"]


def without(s, bad):
    keep = [r for r in range(s.n) if r not in bad]
    pieces, off = [], [0]
    for r in keep:
        pieces += [s.pieces[k] for k in range(int(s.off[r]), int(s.off[r + 1]))]; off.append(len(pieces))
    return Call(s.node_len, np.array(pieces, dtype=PIECE), off, s.nodes, s.mappings, s.edits), keep


def check_malformed(which, name):
    s, bad, wfa = malformed_cases()[name]
    answers = []
    for lib in (lib_of(which), lib_of("oracle", which != "gpu")):
        eng = capi.Engine(lib=lib)
        idx = s.index(eng)
        if wfa:                                         # one problem: LINK 0 exists, LINK 1 does not
            eng.wfa_extend(idx, [dict(seq="A" * s.node_len[0], mode="connect", **{"from": (0, 0), "to": (2, 0)})])
        a = stitch(eng, idx, s)
        good, keep = without(s, bad)
        g = stitch(eng, idx, good)
        assert a.rc == OK and g.rc == OK, (name, a.rc, g.rc)
        for r in bad:
            assert a.res["status"][r] == EINVAL and a.res["n_mappings"][r] == 0 and a.res["n_edits"][r] == 0 and a.res["from_length"][r] == 0 and a.res["to_length"][r] == 0, (name, r)
        assert a.written == g.written and a.res[keep].tobytes() == g.res.tobytes() and a.om.tobytes() == g.om.tobytes() and a.oe.tobytes() == g.oe.tobytes(), name
        assert not g.res["status"].any(), name
        answers.append(a)
    assert answers[0].same_as(answers[1]), name


@pytest.mark.parametrize("name", MALFORMED)
def test_malformed_pieces_emulated(name):
    """the bad read: VGK_EINVAL, sizes 0; every other read byte for byte what the call without it gives; the call VGK_OK; all as the oracle has it"""
    assert sorted(malformed_cases()) == sorted(MALFORMED)
    check_malformed("emu", name)


@pytest.mark.gpu
def test_malformed_pieces_on_the_gpu():
    for name in MALFORMED:
        check_malformed("gpu", name)


# ---- 6. bounds that sum past 2^32 with valid pieces --------------------------------------------------------------------------------------------
def big_bounds_call(total_path_len, per_read=64):
    """ALIGNMENT pieces that all name (a prefix of) one `nodes` array of 2^20 entries with a single 5-base match run on its first node: every piece is
    valid and makes one mapping, and the bounds — a mapping per node named — sum to total_path_len"""
    n_nodes = 1 << 20
    b = Builder()
    b.nodes = [0] * n_nodes
    b.edits.append((5 << 2) | MATCH)
    left = total_path_len
    while left:
        take = min(left, n_nodes); left -= take
        b.pieces.append((capi.PIECE_ALIGNMENT, 0, 0, 0, take, 0, 1, 0))
        if len(b.pieces) % per_read == 0:
            b.end_read()
    if b.off[-1] != len(b.pieces):
        b.end_read()
    return b.call([8, 3])


# the edit bound of a piece is its path_len + 1: with 4096 pieces, 0xffffeff0 nodes named make edit bounds of exactly 0xfffffff0, the most that is taken
BIG_BOUNDS = {"just_below": 0xffffeff0, "past_2_32": (1 << 32) + 4096}


def check_big_bounds(which, name):
    s = big_bounds_call(BIG_BOUNDS[name])
    eng = capi.Engine(lib=lib_of(which))
    a = stitch(eng, s.index(eng), s, mapping_cap=len(s.pieces), edit_cap=len(s.pieces))
    print(name, which, "->", a.rc)
    assert a.rc in ((ETOOBIG, ENOMEM, OK) if name == "just_below" else (ETOOBIG, OK)), (name, a.rc)
    if a.rc == OK:
        ora = capi.Engine(lib=lib_of("oracle", which != "gpu"))
        o = stitch(ora, s.index(ora), s, mapping_cap=len(s.pieces), edit_cap=len(s.pieces))
        assert o.rc == OK and a.same_as(o), name
        for r in range(s.n):
            assert a.read(r) == [(0, 0, [(MATCH, 5)])] * int(s.off[r + 1] - s.off[r]), (name, r)
    del eng
    return a.rc


@pytest.mark.parametrize("name", sorted(BIG_BOUNDS))
def test_bounds_past_2_32_emulated(name):
    """VGK_ETOOBIG, or the right answer (one mapping per piece; VGK_ENOMEM too where the work arrays of the sum just below the limit cannot be had) —
    never an answer made in work arrays sized by a wrapped sum"""
    check_big_bounds("emu", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BIG_BOUNDS))
def test_bounds_past_2_32_on_the_gpu(name):
    check_big_bounds("gpu", name)


# ---- 7. the same calls as a program of its own under the host sanitizers ----------------------------------------------------------------------------
SAN = os.path.join(util.ROOT, "tests", "emu", "chain_stitch_san")


def write_call(path, s, mcap, ecap):
    with open(path, "wb") as f:
        f.write(b"VGKC")
        f.write(struct.pack("<I", len(s.node_len))); f.write(np.array(s.node_len, dtype="<u4").tobytes()); f.write(b"A" * sum(s.node_len))
        thread = np.arange(0, 2 * len(s.node_len), 2, dtype="<u4")
        f.write(struct.pack("<III", 1, 0, len(thread))); f.write(thread.tobytes())
        f.write(struct.pack("<I", s.n)); f.write(s.off.tobytes())
        f.write(s.pieces.tobytes())
        for a in (s.nodes, s.mappings, s.edits):
            f.write(struct.pack("<Q", len(a))); f.write(a.tobytes())
        f.write(struct.pack("<QQ", mcap, ecap))


def sanitized(tmp_path, name, s, mcap, ecap):
    call, out = str(tmp_path / (name + ".call")), str(tmp_path / (name + ".out"))
    write_call(call, s, mcap, ecap)
    p = subprocess.run([SAN, call, out], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (name, p.returncode, p.stderr[-2000:])
    with open(out, "rb") as f:
        raw = f.read()
    create_rc, rc, wm, we = struct.unpack_from("<iiQQ", raw, 0)
    assert create_rc == OK, name
    at = 24
    res = np.frombuffer(raw, dtype=RESULT, count=s.n, offset=at).copy(); at += res.nbytes
    om = np.frombuffer(raw, dtype=MAPPING, count=min(wm, mcap), offset=at).copy(); at += om.nbytes
    oe = np.frombuffer(raw, dtype=np.uint32, count=min(we, ecap), offset=at).copy(); at += oe.nbytes
    assert at == len(raw), name
    return Answer(rc, (wm, we), res, om, oe, mcap, ecap)


def sanitizer_calls():
    """name -> (call, mapping_cap | None, edit_cap | None): the LINK-free calls of 1 (one seed), 4, 5 and 6"""
    out = {"cut_corpus": (cut_corpus(CUT_SEEDS[0])[0], None, None), "twenty_thousand_pieces": (long_read_case()[0], None, None)}
    c = cut_corpus(CUT_SEEDS[0])[0]
    for n in (1, 5, 64, 65):
        out["n_reads_%d" % n] = (sub_call(c, [None if k % 7 == 3 else 100 + k for k in range(n)]), None, None)
    out["no_pieces_at_all"] = (sub_call(c, [None] * 5), None, None)
    s = sub_call(cut_corpus(CUT_SEEDS[2])[0], range(200, 265))
    out.update({"caps_%s" % k: (s, k, None) for k in ("exact", "mappings_short", "edits_short", "inside", "zero")})
    for name, (m, bad, wfa) in malformed_cases().items():
        if not name.startswith("link"):
            out[name] = (m, None, None)
    out["bounds_past_2_32"] = (big_bounds_call(BIG_BOUNDS["past_2_32"]), 4200, 4200)
    return out


SANITIZER_CALLS = (["cut_corpus", "twenty_thousand_pieces", "n_reads_1", "n_reads_5", "n_reads_64", "n_reads_65", "no_pieces_at_all", "caps_exact", "caps_mappings_short",
                    "caps_edits_short", "caps_inside", "caps_zero"] + [n for n in MALFORMED if not n.startswith("link")] + ["bounds_past_2_32"])


@pytest.mark.parametrize("name", SANITIZER_CALLS)
def test_calls_are_clean_under_the_host_sanitizers(name, tmp_path):
    """AddressSanitizer and UBSan over vgk_haplo_create + vgk_chain_stitch on the emulated backend (make chainstitch_san), one child process per call:
    exit status 0, nothing on stderr, and the emulator library's answer"""
    build_emu()
    subprocess.check_call(["make", "-s", "-j8", "chainstitch_san"], cwd=util.ROOT)
    calls = sanitizer_calls()
    assert sorted(calls) == sorted(SANITIZER_CALLS)
    s, mcap, ecap = calls[name]
    eng = capi.Engine(lib=util.EMU_LIB); idx = s.index(eng)
    full = stitch(eng, idx, s)
    if mcap is None:
        mcap, ecap = full.written
    elif isinstance(mcap, str):
        M, E = full.written
        mcap, ecap = {"exact": (M, E), "mappings_short": (M - 1, E), "edits_short": (M, E - 1), "inside": (M // 2, E), "zero": (0, 0)}[mcap]
    want = stitch(eng, idx, s, mapping_cap=mcap, edit_cap=ecap)
    got = sanitized(tmp_path, name, s, mcap, ecap)
    assert got.same_as(want), (name, got.rc, want.rc, got.written, want.written)
