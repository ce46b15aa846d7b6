"""vgk_read_alignments (include/vgk_engine.h): giraffe's alignments of a short read, composed from its extension set and its tails' alignments.

The reference holds no unit test of find_optimal_tail_alignments, extension_to_alignment or add_to_path (a search of src/unittest finds none), so the
pin is `restate` below: an independent restatement of the rule in Python, index-based, written from the rule's description (Paths as lists, the left
tail flipped as a list reversal, add_to_path over lists) and sharing no code with the engine, whose serial statement (ra_read_one of
vg_amd/csrc/read_alignments_device.hpp, behind tests/emu/read_alignments_driver.cpp) streams edits instead.  The serial statement must equal the
restatement header for header, mapping for mapping and run for run on workloads.ReadAlignmentsWorkload's corpus — which is asserted to reach every
branch of the rule —, the host shim (vgh_read_alignments, the reference's loop shape over Paths) must equal the serial statement byte for byte, and the
engine must equal the host shim byte for byte."""
import collections
import ctypes
import os
import subprocess

import numpy as np
import pytest

from vg_amd import capi, pipeline, workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = os.path.join(ROOT, "vg_amd", "libvgamd.so")
DRIVER = os.path.join(ROOT, "tests", "emu", "libvgamd_readaln.so")
MATCH, MISMATCH, INSERTION, DELETION = 0, 1, 2, 3
WINDOW = 39
POLICIES = [dict(extension_score_threshold=1, max_local_extensions=0xffffffff), dict(extension_score_threshold=0, max_local_extensions=0xffffffff),
            dict(extension_score_threshold=1, max_local_extensions=1), dict(extension_score_threshold=1, max_local_extensions=2),
            dict(extension_score_threshold=3, max_local_extensions=0xffffffff)]


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------------
def pareto(points):
    """points: [(value, cost)] -> the frontier, sorted by (value, cost)"""
    if not points:
        return []
    v = sorted(points, key=lambda p: (p[1], -p[0]))
    kept = [v[0]]
    for p in v[1:]:
        if p[0] > kept[-1][0]:
            kept.append(p)
    return sorted(kept)


def restate(wl, threshold, max_local, window_length, cover):
    """-> per read a list of dict(kind, extension, score, mappings = [[node, offset, [(kind, length)]]], identity = (num, den), status)"""
    match, mismatch, gap_open, gap_extend, bonus = wl.scoring
    olen = [int(x) for x in wl.oriented_len]
    obase = np.concatenate([[0], np.cumsum(wl.oriented_len.astype(np.int64))])
    oseq = wl.oriented_seq.tobytes().decode()
    node_seq = lambda o: oseq[obase[o]:obase[o + 1]]
    ext, res, nodes, mism, tails, ops = wl.ext, wl.res, wl.path_nodes, wl.mism, wl.tails, wl.ops
    tail_at = {(int(t["ext"]), int(t["left"])): k for k, t in enumerate(tails)}
    gap = lambda n: 0 if n == 0 else gap_open + (n - 1) * gap_extend
    gap_to = lambda start, limit: gap_open if start >= limit else gap_open + (limit - start - 1) * gap_extend

    def flank(length, frontier):
        best = gap(length)
        for value, cost in frontier:
            best = min(best, cost + gap_to(value, length))
            if value >= length:
                break
        return best

    def extension_path(e, read):
        path = [int(x) for x in nodes[e["path_begin"]:e["path_begin"] + e["path_len"]]]
        mm = [int(x) for x in mism[e["mism_begin"]:e["mism_begin"] + e["n_mismatches"]]]
        out, at, off = [], int(e["read_begin"]), int(e["offset"])
        if len(path) == 1:
            cover["extension on one node"] += 1
        for node in path:
            limit = min(at + olen[node] - off, int(e["read_end"]))
            if olen[node] == 1:
                cover["one-base node"] += 1
            edits = []
            for m in [m for m in mm if at <= m < limit]:
                if m == e["read_begin"]:
                    cover["mismatch at read_begin"] += 1
                if m == e["read_end"] - 1:
                    cover["mismatch at read_end - 1"] += 1
                if off + (m - at) == 0:
                    cover["mismatch at a node's first base"] += 1
                if off + (m - at) == olen[node] - 1:
                    cover["mismatch at a node's last base"] += 1
                if m + 1 in mm:
                    cover["two adjacent mismatches"] += 1
            cursor = at
            for m in mm:
                if cursor <= m < limit:
                    if m > cursor:
                        edits.append((MATCH, m - cursor))
                    edits.append((MISMATCH, 1)); cursor = m + 1
            if cursor < limit:
                edits.append((MATCH, limit - cursor))
            out.append([node, off, edits]); at, off = limit, 0
        return out

    def tail_path(e, x, left, read):
        """the tail's Path in read order, or [] for a closed end"""
        L = len(read)
        begin, end = (0, int(e["read_begin"])) if left else (int(e["read_end"]), L)
        if begin >= end:
            return [], 0
        path = [int(v) for v in nodes[e["path_begin"]:e["path_begin"] + e["path_len"]]]
        k = tail_at.get((x, left))
        if k is None or tails[k]["n_ops"] == 0:
            if left:
                where = (path[0], int(e["offset"]))
            else:
                where = (path[-1], int(e["offset"]) + int(e["read_end"]) - int(e["read_begin"]) - sum(olen[v] for v in path[:-1]))
            return [[where[0], where[1], [(INSERTION, end - begin)]]], 0
        t = tails[k]
        seq = read[begin:end]
        if left:
            seq = "".join({"A": "T", "C": "G", "G": "C", "T": "A"}.get(c, "N") for c in reversed(seq))
        o = ops[int(t["ops_begin"]):int(t["ops_begin"]) + int(t["n_ops"])]
        if o["op"][0] == capi.OP_I:
            cover["a tail whose first op is an insertion"] += 1
        if o["op"][0] == capi.OP_D:
            cover["a tail whose first op is a deletion"] += 1
        if o["op"][-1] == capi.OP_S:
            cover["a tail ending in S"] += 1
        out, q, pos = [], 0, int(t["first_offset"])
        for i in range(len(o)):
            node, length, op = int(o["node"][i]), int(o["len"][i]), int(o["op"][i])
            graph = op in (capi.OP_M, capi.OP_D)
            if i == 0 or node != int(o["node"][i - 1]) or (graph and pos >= olen[node]):
                if i:
                    pos = 0
                out.append([node, pos, []])
            edits = out[-1][2]
            if op == capi.OP_M:
                run = 0
                for j in range(length):
                    if seq[q + j] in "ACGT" and seq[q + j] == node_seq(node)[pos + j]:
                        run += 1
                    else:
                        if run:
                            edits.append((MATCH, run))
                        edits.append((MISMATCH, 1)); run = 0
                if run:
                    edits.append((MATCH, run))
                q += length; pos += length
            elif op == capi.OP_D:
                edits.append((DELETION, length)); pos += length
            else:
                edits.append((INSERTION, length)); q += length
        if left:                                              # reverse_complement_path
            out = [[m[0] ^ 1, olen[m[0]] - (m[1] + sum(n for kind, n in m[2] if kind != INSERTION)), m[2][::-1]] for m in reversed(out)]
        return out, int(t["score"])

    def total_insertion(m):
        return len(m[2]) == 1 and m[2][0][0] == INSERTION

    def add_to_path(target, more, what):
        for m in more:
            if target and (m[0] >> 1) == (target[-1][0] >> 1):
                prev = target[-1]
                combine = False
                if m[1] != 0:
                    combine = True
                    if what == "middle":
                        cover["a left tail merged into the extension's first mapping"] += 1
                elif total_insertion(prev) or total_insertion(m):
                    combine = True
                    if total_insertion(prev):
                        prev[0], prev[1] = m[0], m[1]
                else:
                    cover["a second visit of one node id at offset 0"] += 1
                if combine:
                    prev[2].extend(m[2])
                    continue
            target.append([m[0], m[1], list(m[2])])

    def compose(e, x, read):
        left, _ = tail_path(e, x, 1, read)
        middle = extension_path(e, read)
        right, _ = tail_path(e, x, 0, read)
        if left and not total_insertion(left[-1]) and not (left[-1][0] >> 1 == middle[0][0] >> 1 and middle[0][1] != 0) and middle[0][1] == 0:
            cover["a left tail ending at a node boundary"] += 1
        clipped = [bool(p) and len(p) == 1 and total_insertion(p[0]) for p in (left, right)]
        cover["soft clip: " + ("both" if all(clipped) else "left" if clipped[0] else "right" if clipped[1] else "none")] += 1
        path = [[m[0], m[1], list(m[2])] for m in left]
        add_to_path(path, middle, "middle"); add_to_path(path, right, "right")
        edits = [ed for m in path for ed in m[2]]
        total = sum(n for kind, n in edits if kind != DELETION)
        matched = sum(n for kind, n in edits if kind == MATCH)
        for k, (kind, n) in enumerate(edits):
            if kind == INSERTION and (k == 0 or k == len(edits) - 1):
                total -= n
        return path, (matched if total else 0, total)

    answer = []
    for r in range(wl.n):
        read = wl.read_strings[r]; L = len(read)
        g = res[r]; first, n = int(g["ext_begin"]), int(g["n_ext"])
        E = [ext[first + k] for k in range(n)]
        full = [bool(e["left_full"]) and bool(e["right_full"]) for e in E]
        if "N" in read:
            cover["a read with an N"] += 1
        if g["full_length"]:
            lead = 0
            while lead < n and full[lead]:
                lead += 1
            cover["a full-length set with %s" % ("one full extension" if lead == 1 else "three full extensions" if lead == 3 else "%d" % lead)
                  + (" followed by a partial one" if lead < n else "")] += 1
            answer.append([dict(kind=capi.READ_ALN_DIRECT, extension=first + k, score=int(E[k]["score"]), mappings=extension_path(E[k], read),
                                identity=(L - int(E[k]["n_mismatches"]), L), status=0) for k in range(lead)])
            continue
        min_tails = max(2, 1 + sum(full))
        lf, rf = [], []
        for k, e in enumerate(E):
            if full[k]:
                continue
            lp, mp, rp = gap(int(e["read_begin"])), int(e["n_mismatches"]) * (match + mismatch), gap(L - int(e["read_end"]))
            lf.append((int(e["read_end"]), mp + lp)); rf.append((L - int(e["read_begin"]), mp + rp))
            if e["n_mismatches"]:
                lf.append((int(mism[e["mism_begin"]]), lp)); rf.append((L - int(mism[e["mism_begin"] + e["n_mismatches"] - 1]) - 1, rp))
        lf.append((window_length - 1, 0)); rf.append((window_length - 1, 0))
        lf, rf = pareto(lf), pareto(rf)
        order = sorted(range(n), key=lambda k: -int(E[k]["score"]))
        if n > 1 and E[order[0]]["score"] == E[order[1]]["score"]:
            cover["a score tie at the top"] += 1
        if threshold == 0 and n > 1:
            cover["threshold 0"] += 1
        cutoff = int(E[order[0]]["score"]) - threshold if n else 0
        unskipped, partial, limit = 0, False, -1
        win = dict(score=0, ext=None, start=0, end=0); second = dict(score=0, ext=None)
        for k in order:
            e = E[k]; score = int(e["score"])
            if threshold != 0 and score <= cutoff:
                if unskipped >= min_tails:
                    continue
                cover["min_tails forcing an extension below the cutoff"] += 1
            elif max_local != 0xffffffff and unskipped >= max_local:
                cover["max_local_extensions of %d cutting" % max_local] += 1
                continue
            unskipped += 1
            if limit < 0:
                limit = score - threshold
            if not full[k]:
                if partial and score <= limit:
                    estimate = L * match + 2 * bonus - int(e["n_mismatches"]) * (match + mismatch)
                    if not e["left_full"]:
                        estimate -= flank(int(e["read_begin"]), lf)
                    if not e["right_full"]:
                        estimate -= flank(L - int(e["read_end"]), rf)
                    if estimate <= win["score"]:
                        cover["the estimate skip taken"] += 1
                        continue
                partial = True
            left, ls = tail_path(e, first + k, 1, read); right, rs = tail_path(e, first + k, 0, read)
            path = [int(v) for v in nodes[e["path_begin"]:e["path_begin"] + e["path_len"]]]
            total = score + ls + rs
            start = ((left[0][0] if left else path[0]) >> 1) + 1; end = ((right[-1][0] if right else path[-1]) >> 1) + 1
            ws, we = (0, 0) if win["score"] == 0 else (win["start"], win["end"])
            dl, dr = ws != start, we != end
            if total > win["score"] or win["score"] == 0:
                if win["score"] != 0 and dl and dr:
                    second = dict(score=win["score"], ext=win["ext"])
                    cover["a runner-up that is the previous winner pushed down"] += 1
                win = dict(score=total, ext=k, start=start, end=end)
            elif total > second["score"] or second["score"] == 0:
                if dl and dr:
                    second = dict(score=total, ext=k)
                elif dl or dr:
                    cover["a candidate better than the runner-up rejected for sharing one end node"] += 1
        if second["ext"] is None:
            cover["an empty second best"] += 1
        out = []
        for kind, which in ((capi.READ_ALN_BEST, win), (capi.READ_ALN_SECOND, second)):
            if which["ext"] is None:
                out.append(dict(kind=kind, extension=capi.READ_ALN_NO_EXTENSION, score=0, mappings=[], identity=(0, 0), status=0))
            else:
                path, identity = compose(E[which["ext"]], first + which["ext"], read)
                out.append(dict(kind=kind, extension=first + which["ext"], score=which["score"], mappings=path, identity=identity, status=0))
        answer.append(out)
    return answer


# ---- the serial statement and the engine behind one shape ---------------------------------------------------------------------------------------------
def serial_call(wl, arrays=None, caps=None, shim=False, **policy):
    """the serial statement's driver, or (shim) the host shim's vgh_read_alignments: the same arguments, the shim's with a thread count behind them"""
    lib = pipeline._host_lib() if shim else ctypes.CDLL(DRIVER)
    scores = np.array(wl.scoring, dtype=np.int32)
    head = (ctypes.c_void_p(scores.ctypes.data), ctypes.c_void_p(wl.oriented_len.ctypes.data), ctypes.c_void_p(wl.oriented_seq.ctypes.data), ctypes.c_uint64(len(wl.oriented_len)))
    a = dict(wl.call_arrays(), **(arrays or {}))
    return capi.read_alignments_call(lib.vgh_read_alignments if shim else lib.vgt_read_alignments_serial, head, a["reads"], a["read_off"], a["results"], a["extensions"], a["nodes"],
                                     a["mismatches"], a["tails"], a["ops"], window_length=WINDOW, caps=caps, tail=(ctypes.c_int(4),) if shim else (), **policy)


def shim_call(wl, arrays=None, caps=None, **policy):
    return serial_call(wl, arrays, caps, shim=True, **policy)


def as_lists(out, n):
    """a call's output in restate's shape"""
    aln, maps, edits = out["alignments"], out["mappings"], out["edits"]
    answer = []
    for r in range(n):
        rows = []
        for a in range(int(out["aln_off"][r]), int(out["aln_off"][r + 1])):
            h = aln[a]
            assert h["read"] == r
            ms = []
            for m in maps[int(h["mapping_begin"]):int(h["mapping_begin"]) + int(h["n_mappings"])]:
                ms.append([int(m["node"]), int(m["offset"]), [(int(w) & 3, int(w) >> 2) for w in edits[int(m["edit_begin"]):int(m["edit_begin"]) + int(m["n_edits"])]]])
            assert sum(len(m[2]) for m in ms) == h["n_edits"]
            rows.append(dict(kind=int(h["kind"]), extension=int(h["extension"]), score=int(h["score"]), mappings=ms, identity=(int(h["identity_num"]), int(h["identity_den"])),
                             status=int(h["status"])))
        answer.append(rows)
    return answer


def same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("aln_off", "alignments", "mappings", "edits"))


@pytest.fixture(scope="module")
def corpus():
    wl = workloads.ReadAlignmentsWorkload(1500, seed=5)
    cover = collections.Counter()
    per_policy = []
    for p in POLICIES:
        rc, out = serial_call(wl, **p)
        assert rc == 0
        per_policy.append((p, out, restate(wl, p["extension_score_threshold"], p["max_local_extensions"], WINDOW, cover)))
    return wl, per_policy, cover


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------------
def test_shim_serial_statement_and_restatement_agree(corpus):
    wl, per_policy, _ = corpus
    for p, out, want in per_policy:
        rc, shim = shim_call(wl, **p)
        assert rc == 0 and shim["written"] == out["written"] and same_bytes(shim, out), p
        got = as_lists(out, wl.n)
        for r in range(wl.n):
            assert got[r] == want[r], (p, r)


BRANCHES = ["the estimate skip taken", "min_tails forcing an extension below the cutoff", "max_local_extensions of 1 cutting", "max_local_extensions of 2 cutting", "threshold 0",
            "a runner-up that is the previous winner pushed down", "a candidate better than the runner-up rejected for sharing one end node", "an empty second best",
            "a score tie at the top", "soft clip: left", "soft clip: right", "soft clip: both", "a left tail merged into the extension's first mapping",
            "a left tail ending at a node boundary", "a tail whose first op is an insertion", "a tail whose first op is a deletion", "a tail ending in S",
            "a second visit of one node id at offset 0", "mismatch at read_begin", "mismatch at read_end - 1", "mismatch at a node's first base", "mismatch at a node's last base",
            "two adjacent mismatches", "one-base node", "extension on one node", "a read with an N", "a full-length set with one full extension",
            "a full-length set with three full extensions followed by a partial one"]


def test_the_corpus_reaches_every_branch(corpus):
    _, _, cover = corpus
    print({b: cover[b] for b in BRANCHES})
    assert [b for b in BRANCHES if cover[b] == 0] == []


def rescore(wl, read, a):
    match, mismatch, gap_open, gap_extend, bonus = wl.scoring
    edits = []
    for m in a["mappings"]:
        for kind, n in m[2]:                                  # (a deletion that runs on over a node boundary is one gap)
            if edits and kind == DELETION and edits[-1][0] == DELETION:
                edits[-1] = (DELETION, edits[-1][1] + n)
            else:
                edits.append((kind, n))
    score = 0
    for k, (kind, n) in enumerate(edits):
        outer = k == 0 or k == len(edits) - 1
        if kind == MATCH:
            score += n * match
        elif kind == MISMATCH:
            score -= n * mismatch
        elif not (kind == INSERTION and outer):
            score -= gap_open + (n - 1) * gap_extend
    if edits:
        score += bonus * ((edits[0][0] != INSERTION) + (edits[-1][0] != INSERTION))
    return score


def test_properties_of_every_alignment(corpus):
    wl, per_policy, _ = corpus
    olen = wl.oriented_len
    checked = 0
    for p, out, _ in per_policy[:2]:
        got = as_lists(out, wl.n)
        for r in range(wl.n):
            read = wl.read_strings[r]
            for k, a in enumerate(got[r]):
                h = out["alignments"][int(out["aln_off"][r]) + k]
                if not a["mappings"]:
                    assert a["extension"] == capi.READ_ALN_NO_EXTENSION and a["score"] == 0
                    continue
                assert h["to_length"] == len(read)
                assert h["from_length"] == sum(n for m in a["mappings"] for kind, n in m[2] if kind != INSERTION)
                for m in a["mappings"]:
                    spent = sum(n for kind, n in m[2] if kind != INSERTION)
                    assert m[1] + spent <= olen[m[0]] and (m[1] < olen[m[0]] or spent == 0), (r, k, m)
                for x, y in zip(a["mappings"][:-1], a["mappings"][1:]):
                    if x[0] != y[0]:
                        assert (x[0], y[0]) in wl.steps, (r, k, x, y)
                if "N" not in read:
                    assert rescore(wl, read, a) == a["score"], (r, k)
                checked += 1
    assert checked > 2000


def test_gaf_lines_give_back_the_reads(corpus):
    wl, per_policy, _ = corpus
    _, out, _ = per_policy[0]
    seqs, seq_off, results, score = pipeline.read_alignments_gaf_view(wl.reads, wl.read_off, out)
    node_seq = np.frombuffer("".join(wl.nodes).encode(), dtype=np.uint8)
    node_off = np.concatenate([[0], np.cumsum([len(s) for s in wl.nodes])]).astype(np.uint64)
    lines = pipeline.gaf_lines(seqs, seq_off, results, out["mappings"], out["edits"], node_seq, node_off, score=score)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    aligned = 0
    for a, line in enumerate(lines):
        f = line.decode().split("\t")
        read = wl.read_strings[int(out["alignments"]["read"][a])]
        cs = [x for x in f if x.startswith("cs:Z:")][0][5:]
        path = ""
        if f[5] != "*":
            steps = f[5].replace("<", " <").replace(">", " >").split()
            path = "".join(wl.nodes[int(s[1:]) - 1] if s[0] == ">" else "".join(comp[c] for c in reversed(wl.nodes[int(s[1:]) - 1])) for s in steps)
            aligned += 1
        at, back, i = int(f[7]), [], 0
        while i < len(cs):
            j = i + 1
            while j < len(cs) and cs[j] not in ":*+-":
                j += 1
            body = cs[i + 1:j]
            if cs[i] == ":":
                back.append(path[at:at + int(body)]); at += int(body)
            elif cs[i] == "*":
                back.append(body[1]); at += 1
            elif cs[i] == "+":
                back.append(body)
            else:
                at += len(body)
            i = j
        assert "".join(back) == read.upper(), a
    assert aligned > 1000


def corrupt(wl, what):
    """the call's arrays with read 3 ... made malformed in one way"""
    a = {k: v.copy() for k, v in wl.call_arrays().items()}
    r = next(r for r in range(wl.n) if wl.res["n_ext"][r] >= 2 and len(wl.read_strings[r]) > 60 and wl.ext["n_mismatches"][wl.res["ext_begin"][r]] >= 2
             and any(t["ext"] == wl.res["ext_begin"][r] and t["n_ops"] > 1 for t in wl.tails))
    x = int(wl.res["ext_begin"][r]); t = next(k for k, t in enumerate(wl.tails) if t["ext"] == x and t["n_ops"] > 1)
    e, tl = a["extensions"], a["tails"]
    if what == "extensions beyond the array":
        a["results"]["n_ext"][r] = len(e)
    elif what == "path beyond the array":
        e["path_begin"][x] = len(a["nodes"])
    elif what == "mismatch outside the interval":
        a["mismatches"][e["mism_begin"][x]] = e["read_end"][x]
    elif what == "mismatches not ascending":
        m = e["mism_begin"][x]; a["mismatches"][m], a["mismatches"][m + 1] = a["mismatches"][m + 1], a["mismatches"][m]
    elif what == "tail's read_begin":
        tl["read_begin"][t] += 1; tl["read_end"][t] += 1
    elif what == "tail's ops beyond the array":
        tl["ops_begin"][t] = len(a["ops"])
    elif what == "tail's ops spend too many read bases":
        a["ops"]["len"][tl["ops_begin"][t]] += 300
    elif what == "tail's ops spend too many node bases":
        k = next(k for k in range(int(tl["ops_begin"][t]), int(tl["ops_begin"][t] + tl["n_ops"][t])) if a["ops"]["op"][k] in (capi.OP_M, capi.OP_D))
        a["ops"]["op"][k] = capi.OP_D; a["ops"]["len"][k] = 60
    elif what == "node outside the index":
        a["nodes"][e["path_begin"][x]] = len(wl.oriented_len)
    elif what == "an empty path":
        e["path_len"][x] = 0
    elif what == "offset outside the first node":
        e["offset"][x] = wl.oriented_len[a["nodes"][e["path_begin"][x]]]
    elif what == "an empty read interval":
        e["read_end"][x] = e["read_begin"][x]
    elif what == "a read interval beyond the read":
        e["read_end"][x] = len(wl.read_strings[r]) + 1
    elif what == "a path that does not hold the interval":
        e["path_len"][x] += 1
    elif what == "left_full against the interval":
        e["left_full"][x] ^= 1
    elif what == "an op of length 0":
        a["ops"]["len"][tl["ops_begin"][t]] = 0
    elif what == "an op of an unknown kind":
        a["ops"]["op"][tl["ops_begin"][t]] = 4
    elif what == "an op on a node outside the index":
        a["ops"]["node"][tl["ops_begin"][t]] = len(wl.oriented_len)
    elif what == "two tails for one end":
        a["tails"] = np.concatenate([tl, tl[t:t + 1]])
    elif what == "a tail on a closed end":
        # an extension of another read that is full on the right gets this tail
        y = next(int(k) for k in range(len(e)) if e["right_full"][k] and not (wl.res["ext_begin"][r] <= k < wl.res["ext_begin"][r] + wl.res["n_ext"][r]))
        extra = tl[t:t + 1].copy(); extra["ext"] = y; extra["left"] = 0
        a["tails"] = np.concatenate([tl, extra])
        r = int(np.searchsorted(wl.res["ext_begin"], y, side="right")) - 1
    elif what == "full_length on a set whose first extension is not full":
        r = next(k for k in range(wl.n) if not wl.res["full_length"][k] and wl.res["n_ext"][k] and not wl.ext["left_full"][wl.res["ext_begin"][k]])
        a["results"]["full_length"][r] = 1
    else:
        raise KeyError(what)
    return r, a


MALFORMED = ["extensions beyond the array", "path beyond the array", "mismatch outside the interval", "mismatches not ascending", "tail's read_begin", "tail's ops beyond the array",
             "tail's ops spend too many read bases", "tail's ops spend too many node bases", "node outside the index", "an empty path", "offset outside the first node",
             "an empty read interval", "a read interval beyond the read", "a path that does not hold the interval", "left_full against the interval", "an op of length 0",
             "an op of an unknown kind", "an op on a node outside the index", "two tails for one end", "a tail on a closed end",
             "full_length on a set whose first extension is not full"]


def check_malformed(call, wl, good):
    for what in MALFORMED:
        r, arrays = corrupt(wl, what)
        rc, out = call(arrays)
        assert rc == 0, what
        got = as_lists(out, wl.n)
        assert [a["status"] for a in got[r]] == [capi.VGK_EINVAL] and got[r][0]["mappings"] == [], what
        assert all(got[k] == good[k] for k in range(wl.n) if k != r), what


def test_a_malformed_read_is_refused_alone(corpus):
    wl, per_policy, _ = corpus
    p, out, _ = per_policy[0]
    check_malformed(lambda arrays: serial_call(wl, arrays, **p), wl, as_lists(out, wl.n))
    check_malformed(lambda arrays: shim_call(wl, arrays, **p), wl, as_lists(out, wl.n))
    a = wl.call_arrays(); off = a["read_off"].copy(); off[2] = off[3] + 1
    assert serial_call(wl, dict(read_off=off), **p)[0] == capi.VGK_EINVAL                     # offsets that do not ascend: the call
    t = a["tails"].copy(); t["ext"][0] = len(a["extensions"])
    assert serial_call(wl, dict(tails=t), **p)[0] == capi.VGK_EINVAL and shim_call(wl, dict(tails=t), **p)[0] == capi.VGK_EINVAL and shim_call(wl, dict(read_off=off), **p)[0] == capi.VGK_EINVAL


def test_capacities_one_short(corpus):
    wl, per_policy, _ = corpus
    p, out, _ = per_policy[0]
    w = out["written"]
    for k in range(3):
        caps = tuple(w[j] - (j == k) for j in range(3))
        for call in (serial_call, shim_call):
            rc, short = call(wl, caps=caps, **p)
            assert rc == capi.VGK_EOPS and short["written"] == w, k
    rc, exact = serial_call(wl, caps=w, **p)
    assert rc == 0 and same_bytes(exact, out)


def test_the_entry_points_are_the_engine_library_s_own():
    engine_h = open(os.path.join(ROOT, "include", "vgk_engine.h")).read(); vgk_h = open(os.path.join(ROOT, "include", "vgk.h")).read()
    lib = ctypes.CDLL(ENGINE)
    for name in ("vgk_read_alignments", "vgk_read_alignments_limits", "vgk_read_alignments_last_ms"):
        assert name + "(" in engine_h and name + "(" not in vgk_h and hasattr(lib, name), name
    assert hasattr(pipeline._host_lib(), "vgh_read_alignments")
    out = (ctypes.c_uint32 * 4)()
    assert lib.vgk_read_alignments_limits(out) == 0 and out[0] >= 1


def test_the_kernels_use_no_scratch_and_little_lds():
    """what DESIGN.md section 34 says of the kernels, read off the built library (tools/kernel_registers.py): no scratch memory, no spills, and LDS that
    leaves at least 8 wavefronts of the selection per CU (160 KiB / 8 = 20 KiB)"""
    import sys
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_registers.py"), ENGINE, "read_alignments"], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-1000:]
    rows = [line.split() for line in done.stdout.splitlines() if "read_alignments" in line]
    assert len(rows) == 3, done.stdout
    for row in rows:
        spills, scratch, lds = int(row[row.index("spills") + 1]), int(row[row.index("scratch") + 1]), int(row[row.index("lds") + 1])
        assert spills == 0 and scratch == 0 and lds <= 20 * 1024, row


def test_the_serial_statement_under_the_host_sanitizers(corpus, tmp_path):
    """the driver as a program of its own under -fsanitize=address,undefined, on the corpus: same answer, nothing reported"""
    wl, per_policy, _ = corpus
    subprocess.check_call(["make", "-s", "readaln_san"], cwd=ROOT)
    a = wl.call_arrays()
    for p, out, _ in per_policy[:3]:
        head = np.array(list(wl.scoring) + [len(wl.oriented_len), len(wl.oriented_seq), p["extension_score_threshold"], p["max_local_extensions"], WINDOW, wl.n,
                                            len(a["extensions"]), len(a["nodes"]), len(a["mismatches"]), len(a["tails"]), len(a["ops"])], dtype=np.uint64)
        with open(tmp_path / "call.bin", "wb") as f:
            for arr in (head, wl.oriented_len, wl.oriented_seq, a["read_off"], a["reads"], a["results"], a["extensions"], a["nodes"], a["mismatches"], a["tails"], a["ops"]):
                f.write(np.ascontiguousarray(arr).tobytes())
        done = subprocess.run([os.path.join(ROOT, "tests", "emu", "read_alignments_san"), str(tmp_path / "call.bin"), str(tmp_path / "answer.bin")], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "", done.stderr[-2000:]
        raw = open(tmp_path / "answer.bin", "rb").read()
        h = np.frombuffer(raw[:32], dtype=np.uint64)
        assert int(h[0]) == 0 and tuple(int(x) for x in h[1:]) == out["written"]
        want = b"".join(out[k].tobytes() for k in ("aln_off", "alignments", "mappings", "edits"))
        assert raw[32:] == want


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu(corpus):
    wl = corpus[0]
    eng = capi.Engine(capi.Scoring.simple(*wl.scoring), lib=ENGINE, device=0)
    return eng, eng.haplo_index(wl.nodes, wl.threads)


def engine_call(eng, index, wl, arrays=None, caps=None, **policy):
    a = dict(wl.call_arrays(), **(arrays or {}))
    return capi.read_alignments_call(eng.lib.vgk_read_alignments, (eng.h, index.h), a["reads"], a["read_off"], a["results"], a["extensions"],
                                     a["nodes"], a["mismatches"], a["tails"], a["ops"], window_length=WINDOW, caps=caps, **policy)


@pytest.mark.gpu
def test_the_engine_equals_the_host_shim_on_the_branch_corpus(corpus, gpu):
    wl, per_policy, _ = corpus
    eng, index = gpu
    for p, out, _ in per_policy:
        rc, got = engine_call(eng, index, wl, **p)
        rcs, shim = shim_call(wl, **p)
        assert rc == 0 and rcs == 0 and got["written"] == shim["written"] and same_bytes(got, shim) and same_bytes(got, out), p
    ms = eng.read_alignments_last_ms()
    assert all(x > 0 for x in ms), ms
    p, out, _ = per_policy[0]
    check_malformed(lambda arrays: engine_call(eng, index, wl, arrays, **p), wl, as_lists(out, wl.n))
    w = out["written"]
    for k in range(3):
        rc, short = engine_call(eng, index, wl, caps=tuple(w[j] - (j == k) for j in range(3)), **p)
        assert rc == capi.VGK_EOPS and short["written"] == w, k


@pytest.mark.gpu
@pytest.mark.parametrize("n_reads", [0, 1, 63, 64, 65, 20000])
def test_the_engine_equals_the_host_shim_at_every_batch_size(n_reads):
    """read lengths 1 .. 200 cycle within every batch; sets of 1, 2, 3, 63, 64, 65 extensions and one beyond the LDS limit in the large one"""
    lib = ctypes.CDLL(ENGINE); out4 = (ctypes.c_uint32 * 4)(); assert lib.vgk_read_alignments_limits(out4) == 0
    sizes = (1, 2, 3, int(out4[0]), int(out4[0]) + 1) if n_reads < 20000 else (1, 2, 3, 2, 1, 3, 63, 1, 2, 64, 3, 1, 65, 2, int(out4[0]), int(out4[0]) + 1, 2 * int(out4[0]) + 3, 1, 2, 3)
    wl = workloads.ReadAlignmentsWorkload(min(n_reads, 2000), seed=100 + n_reads, set_sizes=sizes)
    arrays = wl.tiled(n_reads // 2000) if n_reads > 2000 else None          # (20 000 reads: 2 000 made, ten copies of them)
    eng = capi.Engine(capi.Scoring.simple(*wl.scoring), lib=ENGINE, device=0)
    index = eng.haplo_index(wl.nodes, wl.threads)
    rc, want = shim_call(wl, arrays)
    assert rc == 0
    rc, got = engine_call(eng, index, wl, arrays)
    assert rc == 0 and got["written"] == want["written"] and same_bytes(got, want)
    assert len(got["aln_off"]) == n_reads + 1
    if n_reads >= 5:
        assert int(wl.res["n_ext"].max()) > int(out4[0])


@pytest.mark.gpu
def test_a_context_used_again(corpus, gpu):
    """two calls in a row, the second smaller, then the tail stage's own buffers: no scratch slot of this call is another call's"""
    wl, per_policy, _ = corpus
    eng, index = gpu
    p, out, _ = per_policy[0]
    rc, first = engine_call(eng, index, wl, **p)
    small = workloads.ReadAlignmentsWorkload(70, seed=9)
    index2 = eng.haplo_index(small.nodes, small.threads)
    rc2, got = engine_call(eng, index2, small)
    rc3, want = shim_call(small)
    assert rc == 0 and rc2 == 0 and rc3 == 0 and same_bytes(first, out) and same_bytes(got, want)
    gw = workloads.GaplessWorkload(300, seed=11, graph_bp=40000, inserted_reads=0.3)
    hi = eng.haplo_index(gw.nodes, gw.threads)
    stage = pipeline.align_stage_device(eng, hi, gw.gs, aligned=True)
    composed = pipeline.read_alignments(eng, hi, gw.gs, stage)
    again = pipeline.align_stage_device(eng, hi, gw.gs)
    assert (again["read_score"] == stage["read_score"]).all()
    best = composed["alignments"][composed["alignments"]["kind"] != capi.READ_ALN_SECOND]
    assert len(best) >= gw.gs.n and (best["status"] == 0).all()
    rc, once_more = engine_call(eng, index, wl, **p)
    assert rc == 0 and same_bytes(once_more, out)


def oriented_arrays(nodes):
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    seqs = []
    for s in nodes:
        b = s.encode(); seqs += [b, b.translate(comp)[::-1]]
    return np.array([len(b) for b in seqs], dtype=np.uint32), np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()


def processed_extensions(L, E, totals, scoring, threshold, max_local, window_length, mism):
    """Which extensions of a set that is not full-length find_optimal_tail_alignments aligns, worked out from the policy alone (no Path is made): the walk
    of process_until_threshold_e with min_tails, the cutoff, max_local_extensions and the estimate's skip.  totals: per extension its score + tails.
    -> (the extensions aligned, in order; how many the estimate dropped)"""
    match, mismatch, gap_open, gap_extend, bonus = scoring
    gap = lambda k: 0 if k == 0 else gap_open + (k - 1) * gap_extend
    full = [bool(e["left_full"]) and bool(e["right_full"]) for e in E]
    lf, rf = [(window_length - 1, 0)], [(window_length - 1, 0)]
    for e, f in zip(E, full):
        if f:
            continue
        lp, mp, rp = gap(int(e["read_begin"])), int(e["n_mismatches"]) * (match + mismatch), gap(L - int(e["read_end"]))
        lf.append((int(e["read_end"]), mp + lp)); rf.append((L - int(e["read_begin"]), mp + rp))
        if e["n_mismatches"]:
            lf.append((int(mism[e["mism_begin"]]), lp)); rf.append((L - int(mism[e["mism_begin"] + e["n_mismatches"] - 1]) - 1, rp))
    lf, rf = pareto(lf), pareto(rf)

    def flank(length, frontier):
        best = gap(length)
        for value, cost in frontier:
            best = min(best, cost + (gap_open if value >= length else gap_open + (length - value - 1) * gap_extend))
            if value >= length:
                break
        return best
    order = sorted(range(len(E)), key=lambda k: -int(E[k]["score"]))
    min_tails = max(2, 1 + sum(full))
    cutoff = int(E[order[0]]["score"]) - threshold
    unskipped, partial, limit, winning, done, dropped = 0, False, -1, 0, [], 0
    for k in order:
        score = int(E[k]["score"])
        if threshold != 0 and score <= cutoff:
            if unskipped >= min_tails:
                continue
        elif max_local != 0xffffffff and unskipped >= max_local:
            continue
        unskipped += 1
        if limit < 0:
            limit = score - threshold
        if not full[k]:
            if partial and score <= limit:
                estimate = L * match + 2 * bonus - int(E[k]["n_mismatches"]) * (match + mismatch)
                estimate -= 0 if E[k]["left_full"] else flank(int(E[k]["read_begin"]), lf)
                estimate -= 0 if E[k]["right_full"] else flank(L - int(E[k]["read_end"]), rf)
                if estimate <= winning:
                    dropped += 1
                    continue
            partial = True
        done.append(k)
        if totals[k] > winning or winning == 0:
            winning = totals[k]
    return done, dropped


@pytest.mark.gpu
def test_the_resident_form_on_the_alignment_stage():
    """vgk_tail_stage_composed on the shape of test_alignment_stage_on_the_gpu_equals_the_oracles: its totals are vgk_tail_stage_aligned's, its alignments are
    vgk_read_alignments' over that call's downloaded tails and the host shim's over the ORACLE pipeline's tails, byte for byte; and every BEST score is the
    largest total among the extensions the policy aligns — read_score exactly where the maximising extension is among them."""
    scoring = (1, 4, 6, 1, 5)
    wl = workloads.GaplessWorkload(30000, seed=10, graph_bp=400000, inserted_reads=0.3)
    eng = capi.Engine(capi.Scoring.simple(*scoring), lib=ENGINE, device=0)
    index = eng.haplo_index(wl.nodes, wl.threads)
    stage = pipeline.align_stage_device(eng, index, wl.gs, aligned=True)
    explicit = pipeline.read_alignments(eng, index, wl.gs, stage, window_length=WINDOW)
    resident = pipeline.align_stage_device(eng, index, wl.gs, composed=True, composed_policy=dict(window_length=WINDOW))
    assert (resident["ext_total"] == stage["ext_total"]).all() and (resident["read_score"] == stage["read_score"]).all() and resident["stats"] == stage["stats"]
    assert resident["ext"].tobytes() == stage["ext"].tobytes() and resident["mism"].tobytes() == stage["mism"].tobytes()      # (the deferred copies were finished)
    got = resident["composed"]
    assert got["written"] == explicit["written"] and same_bytes(got, explicit)
    assert all(x > 0 for x in eng.read_alignments_last_ms())
    # capacities one short: VGK_EOPS with what is needed, the totals complete
    for k in range(3):
        with pytest.raises(capi.VgkError):
            pipeline.align_stage_device(eng, index, wl.gs, composed=True, composed_policy=dict(window_length=WINDOW), composed_caps=tuple(got["written"][j] - (j == k) for j in range(3)))
        assert eng.read_alignments_written == got["written"], k
    # ... the host shim over the oracle pipeline's tails
    ora = capi.Engine(capi.Scoring.simple(*scoring), lib=os.path.join(ROOT, "oracle", "libvgoracle.so"))
    olen, oseq = oriented_arrays(wl.nodes)
    want_stage = pipeline.align_stage(ora, ora.haplo_index(wl.nodes, wl.threads), olen, wl.gs)
    arrays = pipeline.winning_alignment_arrays(want_stage)
    nt = len(arrays["ext"])
    otails = np.zeros(nt, dtype=capi.TAIL_ALIGNMENT_DT)
    for name in ("ext", "left", "read_begin", "read_end", "score", "n_ops", "first_offset"):
        otails[name] = arrays[name]
    otails["ops_begin"] = np.cumsum(arrays["n_ops"]) - arrays["n_ops"]
    oops = np.zeros(len(arrays["ops_node"]), dtype=capi.OP_DT)
    oops["node"] = arrays["ops_node"]; oops["op"] = arrays["ops_op"]; oops["len"] = arrays["ops_len"]
    sc = np.array(scoring, dtype=np.int32)
    head = (ctypes.c_void_p(sc.ctypes.data), ctypes.c_void_p(olen.ctypes.data), ctypes.c_void_p(oseq.ctypes.data), ctypes.c_uint64(len(olen)))
    n_ext = len(stage["ext"])
    rc, want = capi.read_alignments_call(pipeline._host_lib().vgh_read_alignments, head, wl.gs.reads, wl.gs.read_off, want_stage["res"], want_stage["ext"][:n_ext], want_stage["nodes"],
                                         want_stage["mism"], otails, oops, window_length=WINDOW, caps=got["written"], tail=(ctypes.c_int(8),))
    assert rc == 0 and nt == stage["stats"][0] and same_bytes(got, want)
    # ... and the scores against the policy (threshold 1, no limit on the extensions)
    aln = got["alignments"]
    assert (aln["status"] == 0).all()
    lead = aln[got["aln_off"][:-1].astype(np.int64)]                  # every read's first alignment: BEST, or the first DIRECT one
    assert (lead["read"] == np.arange(wl.gs.n)).all() and (lead["kind"] != capi.READ_ALN_SECOND).all()
    res, ext, total, score = stage["res"], stage["ext"], stage["ext_total"], stage["read_score"][:wl.gs.n]
    lengths = (wl.gs.read_off[1:] - wl.gs.read_off[:-1]).astype(np.int64)
    reachable = unreachable = explained = 0
    for r in range(wl.gs.n):
        b, k = int(res["ext_begin"][r]), int(res["n_ext"][r])
        if res["full_length"][r]:
            best = int(ext["score"][b])                                # the first full extension, as it is
            assert int(total[b]) == best
            explained += best < score[r]                               # (a full-length set is converted as it is: a partial extension's total is never looked at)
        else:
            done, dropped = processed_extensions(int(lengths[r]), [ext[b + j] for j in range(k)], [int(total[b + j]) for j in range(k)], scoring, 1, 0xffffffff, WINDOW, stage["mism"])
            best = max(int(total[b + j]) for j in done)
            if best < score[r]:
                explained += dropped > 0 or len(done) < k
        assert int(lead["score"][r]) == best, r
        if best == score[r]:
            reachable += 1
        else:
            unreachable += 1
    print("reads %d: BEST == read_score on %d, below it on %d (every one with an extension the cutoff or the estimate left out: %d)" % (wl.gs.n, reachable, unreachable, explained))
    assert int((lead["score"] == score).sum()) == reachable and int((lead["score"] < score).sum()) == unreachable == explained and reachable + unreachable == wl.gs.n
    assert reachable > wl.gs.n * 9 // 10
    aligned = aln[aln["n_mappings"] > 0]
    assert (aligned["to_length"] == lengths[aligned["read"]]).all()


@pytest.mark.gpu
def test_one_large_set_alone_runs_over_the_slab():
    """a single read whose set is beyond the LDS limit: the first launch has nothing, the slab launch everything"""
    lib = ctypes.CDLL(ENGINE); out4 = (ctypes.c_uint32 * 4)(); assert lib.vgk_read_alignments_limits(out4) == 0
    wl = workloads.ReadAlignmentsWorkload(1, seed=77, read_lengths=(150,), set_sizes=(3 * int(out4[0]) + 1,), full_sets=0.0)
    assert int(wl.res["n_ext"][0]) > int(out4[0])
    eng = capi.Engine(capi.Scoring.simple(*wl.scoring), lib=ENGINE, device=0)
    rc, got = engine_call(eng, eng.haplo_index(wl.nodes, wl.threads), wl)
    rcs, want = shim_call(wl)
    assert rc == 0 and rcs == 0 and same_bytes(got, want) and len(got["alignments"]) == 2
