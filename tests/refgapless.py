"""Haplotype-consistent gapless extension stated from the thread lists: no GBWT, no records, no ranges as data.

The haplotypes are the 2 x n_threads oriented sequences: every thread, and its reverse with every node flipped (oriented node = 2 x index +
is_reverse).  A COPY of an oriented node is a pair (sequence, position); a path's copies are the positions where the whole path occurs
contiguously.  Everything below is counted over copies:

  search state of a path   the copies of path[-1], sorted by their reversed prefix (the nodes before them in their sequence, nearest first; a
                           prefix that ends sorts lowest, remaining ties by sequence number), hold the copies preceded by path[:-1] as one
                           contiguous block of ranks [lo, hi]; the backward range is the same rule on the flipped, reversed path.
  one seed's winner        the finished entry of the highest score of an exhaustive search over paths (GaplessExtender::extend, the reference's
                           src/gbwt_extender.cpp:533-700, with match_initial / match_forward / match_backward :213-296 and set_score :201-209);
                           which of several top entries wins is the queue's order, which this file does not restate.
  a returned extension     lies on its path, lists exactly its mismatches, scores what a recount gives, carries the state of its path.
  a returned set           full-length: every member full, mismatch counts ascending, overlaps bounded (:301-329); otherwise no duplicates
                           (:332-365) and, trimmed, no sub-interval that scores higher (:421-529).

Written for clarity, not speed: every count is a scan over the copies."""
import functools

MASK = "#"                                   # what a non-ACGT read base becomes: a base that never matches (ReadMasker, :160-176)
_COMPLEMENT = str.maketrans("ACGTN", "TGCAN")


def mask(read):
    return "".join(c if c in "ACGT" else MASK for c in read)


class Haplotypes:
    def __init__(self, nodes, threads):
        self.nodes = list(nodes)
        self.seqs = []
        for t in threads:
            t = [int(o) for o in t]
            self.seqs.append(tuple(t))
            self.seqs.append(tuple(o ^ 1 for o in reversed(t)))
        self.at = {}                         # oriented node -> its copies
        for s, seq in enumerate(self.seqs):
            for p, o in enumerate(seq):
                self.at.setdefault(o, []).append((s, p))
        self.copies = functools.lru_cache(maxsize=None)(self._copies)
        self.ranked = functools.lru_cache(maxsize=None)(self._ranked)
        self.state = functools.lru_cache(maxsize=None)(self._state)

    def bases(self, o):
        s = self.nodes[o >> 1]
        return s[::-1].translate(_COMPLEMENT) if o & 1 else s

    def length(self, o):
        return len(self.nodes[o >> 1])

    def _copies(self, path):
        """(sequence, position of path[0]) wherever the whole path occurs"""
        n = len(path)
        return tuple((s, p) for s, p in self.at.get(path[0], ()) if self.seqs[s][p:p + n] == path)

    def successors(self, path):
        """distinct nodes that follow the path in some copy, ascending, with the number of copies that go there"""
        out = {}
        for s, p in self.copies(path):
            q = p + len(path)
            if q < len(self.seqs[s]):
                x = self.seqs[s][q]
                out[x] = out.get(x, 0) + 1
        return sorted(out.items())

    def predecessors(self, path):
        out = {}
        for s, p in self.copies(path):
            if p > 0:
                x = self.seqs[s][p - 1]
                out[x] = out.get(x, 0) + 1
        return sorted(out.items())

    def edges(self, o):
        """what leaves an oriented node: its distinct successors, a thread's end included"""
        out = set()
        for s, p in self.at.get(o, ()):
            out.add(self.seqs[s][p + 1] if p + 1 < len(self.seqs[s]) else -1)
        return out

    def _ranked(self, o):
        """the copies of a node in the order of their reversed prefixes (a tuple that is a prefix of another sorts before it)"""
        return tuple(sorted(self.at.get(o, ()), key=lambda c: (self.seqs[c[0]][:c[1]][::-1], c[0])))

    def _range(self, path):
        before = tuple(reversed(path[:-1])); k = len(before)
        ranks = [i for i, (s, p) in enumerate(self.ranked(path[-1])) if self.seqs[s][:p][::-1][:k] == before]
        if not ranks:
            return (0, -1)
        assert ranks == list(range(ranks[0], ranks[-1] + 1)), "the copies of a path are one block of ranks"
        return (ranks[0], ranks[-1])

    def _state(self, path):
        back = tuple(o ^ 1 for o in reversed(path))
        f, b = self._range(path), self._range(back)
        assert f[1] - f[0] == b[1] - b[0] == len(self.copies(path)) - 1
        return (path[-1], f[0], f[1], path[0] ^ 1, b[0], b[1])

    def revisiting(self):
        """nodes some thread visits twice"""
        out = set()
        for seq in self.seqs[::2]:
            seen = set()
            for o in seq:
                if o >> 1 in seen:
                    out.add(o >> 1)
                seen.add(o >> 1)
        return out


class Entry:
    __slots__ = ("path", "offset", "r0", "r1", "internal", "old", "left_full", "right_full", "left_max", "right_max", "score", "notes")

    def clone(self, **kw):
        e = Entry()
        for f in Entry.__slots__:
            setattr(e, f, getattr(self, f))
        for k, v in kw.items():
            setattr(e, k, v)
        return e

    def key(self):
        return (self.path, self.offset, self.r0, self.r1, self.internal, bool(self.left_full), bool(self.right_full), self.score)


def score_of(length, mismatches, left_full, right_full, match, mismatch, bonus):
    return length * match - mismatches * (match + mismatch) + bonus * int(bool(left_full)) + bonus * int(bool(right_full))


def limit_of(max_mm, old):
    return max(max_mm + 1, max_mm // 2 + old + 1)


def finished_entries(hap, read, seed, max_mm, scoring=(1, 4, 5)):
    """Every finished entry of one seed's search (`read` masked), or None when no thread visits the seed's node (outside this reference).
    An entry's `notes` name the rules its lineage met: init_mm, half (a step took a mismatch only the mm / 2 + old + 1 branch allows),
    stuck_right (closed because some copies could not go on), dropped_left (a left step that left the stuck copies behind)."""
    node, diff = seed
    if not hap.at.get(node):
        return None
    L = len(read)
    e = Entry()
    e.path = (node,); e.r0 = e.r1 = max(diff, 0); e.offset = max(-diff, 0); e.internal = 0; e.score = None; e.notes = frozenset()
    seq = hap.bases(node)
    assert e.r0 <= L and e.offset <= len(seq)
    k = e.offset
    while k < len(seq) and e.r1 < L:                             # the initial node: every mismatch is taken
        e.internal += read[e.r1] != seq[k]
        e.r1 += 1; k += 1
    e.old = e.internal
    if e.old:
        e.notes |= {"init_mm"}
    e.left_full = e.left_max = e.r0 == 0
    e.right_full = e.right_max = e.r1 >= L
    stack, done = [e], []
    while stack:
        e = stack.pop()
        if not e.right_max:
            limit = limit_of(max_mm, e.old); entered = 0
            for x, n in hap.successors(e.path):
                seq = hap.bases(x); r1, internal, k = e.r1, e.internal, 0
                while k < len(seq) and r1 < L:
                    if read[r1] != seq[k]:
                        if internal + 1 >= limit:
                            break
                        internal += 1
                    r1 += 1; k += 1
                if k == 0:
                    continue
                nx = e.clone(path=e.path + (x,), r1=r1, internal=internal)
                if internal > max(max_mm, e.internal):
                    nx.notes = nx.notes | {"half"}
                if r1 >= L:
                    nx.right_full = nx.right_max = True; nx.old = internal
                elif k < len(seq):
                    nx.right_max = True; nx.old = internal
                entered += n
                stack.append(nx)
            if entered < len(hap.copies(e.path)):
                stack.append(e.clone(right_max=True, old=e.internal, notes=e.notes | {"stuck_right"}))
            continue
        if not e.left_max:
            limit = limit_of(max_mm, e.old); entered = 0; found = []
            for x, n in hap.predecessors(e.path):
                seq = hap.bases(x); r0, internal, off = e.r0, e.internal, len(seq)
                while off > 0 and r0 > 0:
                    if read[r0 - 1] != seq[off - 1]:
                        if internal + 1 >= limit:
                            break
                        internal += 1
                    r0 -= 1; off -= 1
                if off >= len(seq):
                    continue
                nx = e.clone(path=(x,) + e.path, r0=r0, offset=off, internal=internal)
                if internal > max(max_mm, e.internal):
                    nx.notes = nx.notes | {"half"}
                if r0 == 0:
                    nx.left_full = nx.left_max = True
                elif off > 0:
                    nx.left_max = True
                entered += n
                found.append(nx)
            if found:
                if entered < len(hap.copies(e.path)):
                    for nx in found:
                        nx.notes = nx.notes | {"dropped_left"}
                stack.extend(found)
                continue
        e.score = score_of(e.r1 - e.r0, e.internal, e.left_full, e.right_full, *scoring)
        done.append(e)
    return done


def top_entries(done):
    best = max(e.score for e in done)
    top = {}
    for e in done:
        if e.score == best:
            top.setdefault(e.key(), e)
    return list(top.values())


# ---- what the engines hand back ---------------------------------------------------------------------------------------------------------
class Ext:
    """one vgk_extension with its nodes and mismatches"""

    def __init__(self, x, nodes, mism):
        self.path = tuple(int(o) for o in nodes[x["path_begin"]:x["path_begin"] + x["path_len"]])
        self.offset = int(x["offset"]); self.r0 = int(x["read_begin"]); self.r1 = int(x["read_end"])
        self.mism = [int(m) for m in mism[x["mism_begin"]:x["mism_begin"] + x["n_mismatches"]]]
        self.score = int(x["score"]); self.left_full = bool(x["left_full"]); self.right_full = bool(x["right_full"])
        self.state = tuple(int(v) if v < 0x80000000 else int(v) - (1 << 32) for v in x["state"])

    def key(self):
        return (self.path, self.offset, self.r0, self.r1, len(self.mism), self.left_full, self.right_full, self.score)

    def where(self, hap):
        """read position -> (oriented node, node offset); raises when the path does not cover the interval exactly"""
        out = {}
        pos, off = self.r0, self.offset
        assert self.path and self.offset < hap.length(self.path[0]), "offset inside the first node"
        for i, o in enumerate(self.path):
            assert pos < self.r1, "the last node is entered"
            n = min(hap.length(o) - off, self.r1 - pos)
            for k in range(n):
                out[pos + k] = (o, off + k)
            pos += n; off = 0
        assert pos == self.r1, "the path covers the read interval"
        return out


def sets_of(outputs):
    """(results, extensions, nodes, mismatches) -> per problem (status, full_length, [Ext])"""
    res, ext, nodes, mism = outputs
    return [(int(r["status"]), int(r["full_length"]), [Ext(ext[int(r["ext_begin"]) + k], nodes, mism) for k in range(int(r["n_ext"]))] if r["status"] == 0 else [])
            for r in res]


def visited(hap, e):
    return all(hap.at.get(o) for o in e.path)


def check_extension(hap, read, e, scoring=(1, 4, 5)):
    """validity of one returned extension (`read` masked); False when its path leaves the visited nodes (outside this reference)"""
    L = len(read)
    where = e.where(hap)
    assert 0 <= e.r0 < e.r1 <= L
    want = [p for p in range(e.r0, e.r1) if read[p] != hap.bases(where[p][0])[where[p][1]]]
    assert e.mism == want, ("mismatch positions", e.mism, want)
    assert e.score == score_of(e.r1 - e.r0, len(e.mism), e.left_full, e.right_full, *scoring), "score"
    assert not e.left_full or e.r0 == 0
    assert not e.right_full or e.r1 == L
    if not visited(hap, e):
        return False
    assert len(hap.copies(e.path)) >= 1, "some haplotype takes the path"
    assert e.state == hap.state(e.path), ("search state", e.state, hap.state(e.path))
    return True


def shared_positions(hap, a, b):
    wa, wb = a.where(hap), b.where(hap)
    return sum(1 for p, at in wa.items() if wb.get(p) == at)


def best_subinterval(read, hap, e, scoring=(1, 4, 5)):
    """the highest score of a sub-interval of the extension (the empty one scores 0); a bonus counts only where the sub-interval keeps an end
    that carries the flag"""
    match, mismatch, bonus = scoring
    bad = set(e.mism); best = 0
    for a in range(e.r0, e.r1):
        m = 0
        for b in range(a + 1, e.r1 + 1):
            m += (b - 1) in bad
            s = score_of(b - a, m, e.left_full and a == e.r0, e.right_full and b == e.r1, match, mismatch, bonus)
            best = max(best, s)
    return best


def check_set(hap, read, problem, status, full_length, exts, scoring=(1, 4, 5)):
    """the set rules over one problem's output (`read` masked).  -> number of extensions checked in full (on visited paths)"""
    assert status == 0
    n = sum(check_extension(hap, read, e, scoring) for e in exts)
    L = len(read)
    if full_length:
        assert exts
        for e in exts:
            assert e.left_full and e.right_full and e.r0 == 0 and e.r1 == L
        counts = [len(e.mism) for e in exts]
        assert counts == sorted(counts) and counts[0] <= problem["max_mismatches"]
        for j, b in enumerate(exts):
            for a in exts[:j]:
                assert shared_positions(hap, a, b) <= problem.get("overlap_threshold", 0.8) * (a.r1 - a.r0), "overlap"
    else:
        keys = [(e.r0, e.r1, e.offset, e.path) for e in exts]
        assert len(set(keys)) == len(keys), "duplicates"
        if problem.get("trim", True):
            for e in exts:
                assert best_subinterval(read, hap, e, scoring) <= e.score, ("a sub-interval scores higher", e.key())
    return n


def check_winner(hap, read, problem, status, exts, scoring=(1, 4, 5)):
    """a single-seed problem without trimming: the one extension is a top finished entry of the search.
    -> None (the seed's node is unvisited), or (ties at the top, notes of the entry that won)"""
    assert status == 0 and len(problem["seeds"]) == 1 and not problem.get("trim", True)
    done = finished_entries(hap, read, problem["seeds"][0], problem["max_mismatches"], scoring)
    if done is None:
        return None
    top = top_entries(done)
    if not exts:
        assert any(t.r1 == t.r0 for t in top), "no extension although the best finished entry is not empty"
        return (len(top), frozenset())
    assert len(exts) == 1
    for t in top:
        if t.key() == exts[0].key():
            return (len(top), t.notes)
    raise AssertionError(("not a top finished entry", exts[0].key(), [t.key() for t in top]))
