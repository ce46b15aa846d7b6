"""The alignment problems of this engine restated from their definitions, in plain Python / numpy int64.

Nothing here is shared with the implementations under test: no data layout, no tie rule, no traceback.  Every
function returns exact integers.  Inputs are the problem dicts of gen.py ({read, nodes, preds, pinning?, max_gap?,
qual?}), a capi.Scoring, and optionally the (matrix[256*25], bonuses[256]) tables of qualadj.py.

THE RULES (the specification; DESIGN.md repeats them)

Common.  A graph is a DAG, nodes in topological order, preds[v] = predecessor nodes.  A walk is a path of the DAG.
The substitution score of graph base g against read base r is matrix[5 * nt(g) + nt(r)], nt = A C G T -> 0..3,
anything else (N) -> 4; the matrix row / column 4 is what the scoring says (0 for Scoring.simple).  With quality
tables: matrix[25 * qual[i] + 5 * nt(g) + nt(r)] for read base i.  A gap of n bases costs gap_open + (n - 1) *
gap_extend.  gap_open >= gap_extend is assumed (asserted).

(a) Graph Smith-Waterman, LOCAL and PINNED: the best score over all walks, all read intervals and all alignments.
  * a deletion run continues across a node boundary at the extension price, over any predecessor;
  * an insertion may follow a deletion and a deletion an insertion, each paying its own gap_open;
  * the full-length bonus is added to the substitution score of read base 0 and of read base L-1: it is earned only
    when that base is aligned to a graph base by a diagonal move, never by an insertion, never by an empty
    alignment; a one-base read earns it twice.  With quality tables the bonus of an end is bonuses[qual of that
    end's base];
  * LOCAL: the maximum over all cells, never below 0;
  * PINNED (right-pinned): the bonus is earned at base 0 only; the score is the best alignment that consumes read
    base L-1 (by a diagonal move or an insertion) in the LAST column of a pinning node, 0 if that is negative.  The
    start is free (a local start: soft clip);
  * N against anything scores what the matrix says.

(b) X-drop extension in its un-pruned form (VGK_XDROP_PINNED through the gssw entry points): the exact semi-global
optimum.
  * left-pinned: the alignment starts before the first base of a source node (a node without predecessors) and at
    read base 0; no restart;
  * it may end anywhere; the empty extension scores 0, so the score is never negative;
  * a LEADING insertion (read bases before any graph base is consumed) is at most ceil8(max(1, max_gap_length))
    bases long, ceil8 = rounded up to a multiple of 8 (dozeu's 8-cell vectors, include/vgk.h "rows are grouped in
    dozeu's 8-cell vectors") [PARITY-UNPINNED: the reference's vectors all use max_gap_length far above their
    reads' lengths];
  * a leading deletion is allowed at the ordinary gap price [PARITY-UNPINNED: no reference vector starts with one];
  * the bonus (with quality tables: bonuses[qual[L-1]]) is added to the substitution score of read base L-1 only:
    earned by a diagonal move, not by an insertion of the last base [PARITY-UNPINNED: the header says "on consuming
    the last read base"; the reference's vectors hold no alignment that ends in an insertion];
  * everything else as in (a).
The pruned form (vgk_xdrop_band_align) is a heuristic: its score is at most this optimum.

(c) Banded global alignment with a band that excludes nothing: the global optimum of the whole read against any
walk from a source's first base to a sink's last base.  Nodes may be empty; an empty node passes the state of its
predecessors (or of the start) through unchanged.  No bonus.  A gap run continues across node boundaries and across
empty nodes.  Narrow bands: at most this optimum.

(d) check_alignment: see its docstring.

(e) WFA connect: wfa_connect_optimum, see its docstring.

(f) The k best banded global alignments (align_global_banded_multi) with a band that excludes nothing:
banded_kbest_scores, the k highest scores over DISTINCT alignments of (c), in descending order, fewer only when fewer
alignments exist.
  * an alignment is a source-to-sink walk (empty nodes are part of the walk: two walks that differ only in their empty
    nodes are two walks) and a sequence of single-base ops M / I / D that consumes the whole read and every base of
    the walk.  Two alignments are the same only if walk and ops are the same.  Scores are those of (c): an I may
    follow a D and a D an I, each paying its own gap_open, so an alignment has exactly one path through the states
    "last op was M / I / D" and the k-best dynamic program over those three states counts nothing twice;
  * EXCLUSION 1 (whole-read lead insertion): an alignment that begins with the insertion of the WHOLE read while its
    walk holds graph bases (which are then all deleted: 2I2D, 3I1D, 1I6D) is not an alignment of this family.  The
    reference's matrix has no row above read base 0: in the first column of a node that can begin a walk the
    insertion-then-deletion entry of row r stands for r + 1 inserted bases, and the entry of the bottom row is set to
    "none" (src/banded_global_aligner.cpp:577-579, :597-598, :604-605; restated in oracle/vgo_banded.c fill_node,
    "implied lead gaps of a source column").  The whole read inserted on a walk of empty nodes alone IS an alignment,
    one per such walk (next_empty_alignment, :2616-2668; the walks are listed at :2426-2563);
  * EXCLUSION 2 (empty nodes in front of a walk count once): alignments whose walks differ only in the chain of empty
    nodes in front of their first non-empty node are one alignment.  The traceback ends in the first column of that
    node and writes ONE chain of empty nodes in front of it, the last its search met, whichever empty source the
    chain begins at (empty_source_path: :1288-1295, :1393-1398, written out at :1739-1743);
  * EXCLUSION 3 (no deletion under a first column's bottom row): let n be a node that can begin a walk (a source, or a
    node reached from an empty source over empty nodes alone).  An alignment that deletes n's first base with the
    whole read already consumed is not an alignment of this family, EVEN when its walk enters n from a predecessor
    with bases: the "none" of exclusion 1 is written into the cell after every predecessor has been merged into it
    (:604-605, behind the loop over the seeds :373-544), so it removes what they had put there.  On a one-base read
    this is every deletion of such a first base behind read base 0;
  * what stays outside the definition, counted by the tests and held to the superset bound only: where a node n can
    begin a walk AND has predecessors with bases, the traceback takes "the walk begins here" only when no predecessor
    explains the cell, and never proposes it as an alternate (:1661-1736: the proposals at :1696-1701 and :1717-1722
    run over traceback_source_nodes, which the search over the seeds at :1386-1399 never adds an empty source to), so
    alignments that begin at n's empty source are missing from the alternates whenever a predecessor explains the
    cell.  That depends on the scores in the cell, not on (walk, ops) alone: no exclusion is stated for it;
  * DUPLICATES: a deflection across an edge names the predecessor with bases it lands on, not the empty nodes on the
    way (:1313-1314, :2724), and when taken follows the first chain of empty nodes that reaches that predecessor
    (:1176-1210, "don't have a better way of looking this up right now").  Where a node reaches one predecessor over
    two chains of empty nodes (the edge itself being the chain of none) the alternate over the second chain comes
    out as a copy of the one over the first: the same score, so the score list is that of the definition, but (walk,
    ops) twice.  ambiguous_empty_chains says whether a problem has such an edge.
  exclude_whole_read_lead_insertion = False drops all three exclusions: a superset of the family;
  * narrow bands and what the enumeration of the reference leaves out among walks through empty nodes (DESIGN.md,
    "k-best against the definition"): at every rank at most the score of that superset.

(g) The k best right-pinned alignments (align_pinned_multi): gssw's multi-traceback returns maximal tracebacks from
the best end cell, a procedure and not a problem statement, so there is no exact definition here, only a bound:
pinned_kbest_bound, the k highest POSITIVE scores over every distinct pinned alignment of (a):
  * the start is free: before any graph base c, with any number i < L of read bases soft-clipped, and the first op may
    be M, I or D; alignments are distinct when (c, i, ops) differ;
  * the bonus sits on read base 0 as in (a), earned by a diagonal move only;
  * the end: read base L-1 consumed, in the last column of a pinning node, in any of the states M, I, D.
Every alignment a pinned multi-traceback can return is one of these, so its j-th score is at most the j-th of the
bound; the first of the bound is the PINNED optimum of (a).
"""
import numpy as np

NEG = -(1 << 40)

MODE_LOCAL, MODE_PINNED, MODE_XDROP, MODE_BANDED = 0, 1, 2, 3
OP_M, OP_I, OP_D, OP_S = 0, 1, 2, 3

_NT = np.full(256, 4, dtype=np.int64)
for _k, _c in enumerate("ACGT"):
    _NT[ord(_c)] = _k
    _NT[ord(_c.lower())] = _k


def _codes(s):
    return _NT[np.frombuffer(s.encode(), dtype=np.uint8)]


class Scores:
    """Substitution scores of every graph letter against every read base, bonuses folded in per mode."""

    def __init__(self, problem, scoring, mode, qual_adj=None):
        read = problem["read"]
        self.L = L = len(read)
        self.go, self.ge = int(scoring.gap_open), int(scoring.gap_extend)
        assert self.go >= self.ge
        rd = _codes(read)
        if qual_adj is None:
            m = np.array([int(scoring.matrix[i]) for i in range(25)], dtype=np.int64).reshape(5, 5)
            self.sub = m[:, rd].copy()                                        # [graph letter][read base]
            b0 = b1 = int(scoring.full_length_bonus)
        else:
            q = np.asarray(problem["qual"], dtype=np.int64)
            m = np.asarray(qual_adj[0], dtype=np.int64).reshape(256, 5, 5)
            self.sub = m[q, :, rd].T.copy()
            bon = np.asarray(qual_adj[1], dtype=np.int64)
            b0, b1 = int(bon[q[0]]), int(bon[q[-1]])
        self.bonus_first = b0 if mode in (MODE_LOCAL, MODE_PINNED) else 0
        self.bonus_last = b1 if mode in (MODE_LOCAL, MODE_XDROP) else 0
        self.sub[:, 0] += self.bonus_first
        self.sub[:, L - 1] += self.bonus_last


def _insertions(H0, go, ge, ramp):
    """F[i] = max over k < i of H0[k] - (go + (i - k - 1) ge), as a prefix maximum."""
    A = np.maximum.accumulate(H0 + ramp)
    F = np.full(len(H0), NEG, dtype=np.int64)
    F[1:] = A[:-1] - go - (ramp[1:] - ge)
    return F


def gssw_optimum(problem, scoring, mode, qual_adj=None):
    """(a): the LOCAL or PINNED optimum."""
    assert mode in (MODE_LOCAL, MODE_PINNED)
    sc = Scores(problem, scoring, mode, qual_adj)
    L, go, ge = sc.L, sc.go, sc.ge
    nodes, preds = problem["nodes"], problem["preds"]
    ramp = np.arange(L, dtype=np.int64) * ge
    zero = np.zeros(L, dtype=np.int64)
    none = np.full(L, NEG, dtype=np.int64)
    outH, outE = [], []
    best = 0
    for v, s in enumerate(nodes):
        assert len(s) > 0
        if preds[v]:
            Hp = outH[preds[v][0]]; Ep = outE[preds[v][0]]
            for p in preds[v][1:]:
                Hp = np.maximum(Hp, outH[p]); Ep = np.maximum(Ep, outE[p])
        else:
            Hp, Ep = zero, none
        diag = np.empty(L, dtype=np.int64)
        for g in _codes(s):
            diag[0] = 0
            diag[1:] = Hp[:-1]
            diag += sc.sub[g]
            E = np.maximum(Hp - go, Ep - ge)
            H0 = np.maximum(np.maximum(diag, E), 0)
            H = np.maximum(H0, _insertions(H0, go, ge, ramp))
            if mode == MODE_LOCAL:
                best = max(best, int(H.max()))
            Hp, Ep = H, E
        outH.append(Hp); outE.append(Ep)
        if mode == MODE_PINNED and problem["pinning"][v]:
            best = max(best, int(Hp[L - 1]))
    return best


def xdrop_leading_insertion_limit(max_gap, round8=True):
    return (max(1, int(max_gap)) + 7) // 8 * 8 if round8 else max(1, int(max_gap))


def _gap_column(n, go, ge, limit=None):
    """Column before any graph base: row i = i read bases inserted."""
    col = np.full(n, NEG, dtype=np.int64)
    col[0] = 0
    k = n - 1 if limit is None else min(n - 1, limit)
    col[1:k + 1] = -(go + np.arange(k, dtype=np.int64) * ge)
    return col


def _semiglobal_columns(problem, sc, start, on_column=None):
    """Rows 0..L = read bases consumed; the state (H, E) behind every node, from `start` before every source.
    Empty nodes pass their incoming state through."""
    L, go, ge = sc.L, sc.go, sc.ge
    nodes, preds = problem["nodes"], problem["preds"]
    ramp = np.arange(L + 1, dtype=np.int64) * ge
    none = np.full(L + 1, NEG, dtype=np.int64)
    outH, outE = [], []
    for v, s in enumerate(nodes):
        if preds[v]:
            Hp = outH[preds[v][0]]; Ep = outE[preds[v][0]]
            for p in preds[v][1:]:
                Hp = np.maximum(Hp, outH[p]); Ep = np.maximum(Ep, outE[p])
        else:
            Hp, Ep = start, none
        for g in _codes(s):
            diag = np.full(L + 1, NEG, dtype=np.int64)
            diag[1:] = Hp[:-1] + sc.sub[g]
            E = np.maximum(Hp - go, Ep - ge)
            H0 = np.maximum(diag, E)
            H = np.maximum(H0, _insertions(H0, go, ge, ramp))
            H[H < NEG // 2] = NEG; E[E < NEG // 2] = NEG
            if on_column is not None:
                on_column(H)
            Hp, Ep = H, E
        outH.append(Hp); outE.append(Ep)
    return outH


def xdrop_optimum(problem, scoring, qual_adj=None, round8=True):
    """(b): the un-pruned left-pinned semi-global optimum.  round8 = False: the leading insertion bounded by max(1, max_gap_length) itself —
    not the rule in force, only for counting the problems whose optimum rests on the rounding [PARITY-UNPINNED]."""
    sc = Scores(problem, scoring, MODE_XDROP, qual_adj)
    start = _gap_column(sc.L + 1, sc.go, sc.ge, xdrop_leading_insertion_limit(problem.get("max_gap", 40), round8))
    best = [0]

    def see(H):
        best[0] = max(best[0], int(H.max()))
    _semiglobal_columns(problem, sc, start, see)
    return best[0]


def banded_global_optimum(problem, scoring, qual_adj=None):
    """(c): the global optimum over every source-to-sink walk."""
    sc = Scores(problem, scoring, MODE_BANDED, qual_adj)
    start = _gap_column(sc.L + 1, sc.go, sc.ge)
    outH = _semiglobal_columns(problem, sc, start)
    has_succ = [False] * len(problem["nodes"])
    for pr in problem["preds"]:
        for p in pr:
            has_succ[p] = True
    return max(int(outH[v][sc.L]) for v in range(len(outH)) if not has_succ[v])


def _top(lists, k):
    """rows of score lists side by side -> per row the k highest in descending order (a multiset union: nothing is merged away)"""
    a = np.concatenate(lists, axis=1)
    a = -np.sort(-a, axis=1)[:, :k]
    if a.shape[1] < k:
        a = np.concatenate([a, np.full((a.shape[0], k - a.shape[1]), NEG, dtype=np.int64)], axis=1)
    a[a < NEG // 2] = NEG
    return a


def _kbest_column(sub_g, Mp, Ip, Dp, go, ge, k):
    """One graph base.  Row i = i read bases consumed; (Mp, Ip, Dp) the k best scores of distinct partial alignments in front of the base whose
    last op was M / I / D -> the same behind it.  sub_g[i] = the base against read base i."""
    L = len(sub_g)
    M = np.full((L + 1, k), NEG, dtype=np.int64)
    M[1:] = _top([Mp, Ip, Dp], k)[:-1] + sub_g[:, None]
    M[M < NEG // 2] = NEG
    D = _top([Mp - go, Ip - go, Dp - ge], k)
    I = np.full((L + 1, k), NEG, dtype=np.int64)
    for i in range(1, L + 1):
        I[i] = _top([M[i - 1:i] - go, D[i - 1:i] - go, I[i - 1:i] - ge], k)[0]
    return M, I, D


def _descending(lists, k):
    a = np.concatenate([np.ravel(x) for x in lists]) if lists else np.zeros(0, dtype=np.int64)
    return [int(x) for x in -np.sort(-a[a > NEG // 2])[:k]]


def banded_kbest_scores(problem, scoring, k, qual_adj=None, exclude_whole_read_lead_insertion=True):
    """(f): the k highest scores of distinct global alignments, descending; shorter than k only when fewer exist.
    exclude_whole_read_lead_insertion = False: without any of (f)'s exclusions, the superset."""
    exclude = exclude_whole_read_lead_insertion
    sc = Scores(problem, scoring, MODE_BANDED, qual_adj)
    L, go, ge = sc.L, sc.go, sc.ge
    nodes, preds = problem["nodes"], problem["preds"]
    none = np.full((L + 1, k), NEG, dtype=np.int64)
    M0 = none.copy(); M0[0, 0] = 0
    I0 = none.copy(); I0[1:, 0] = -(go + np.arange(L, dtype=np.int64) * ge)             # the insertion ramp in front of a walk's first base
    whole = int(I0[L, 0])
    if exclude:
        I0[L, 0] = NEG                           # EXCLUSION 1: the whole read inserted survives only on walks of empty nodes alone, counted by `chains`
    # per node: the lists behind it of what has consumed a graph base, and the number of chains of empty nodes alone that end here
    out = []
    for v, s in enumerate(nodes):
        if preds[v]:
            M, I, D = (_top([out[p][x] for p in preds[v]], k) for x in range(3))
            chains = sum(out[p][3] for p in preds[v])
        else:
            M, I, D, chains = none, none, none, 1
        for g in _codes(s):
            if chains:                           # a walk may begin here.  EXCLUSION 2: over whichever chain of empty nodes, once
                n = 1 if exclude else min(chains, k)
                M, I = _top([M] + [M0] * n, k), _top([I] + [I0] * n, k)
            M, I, D = _kbest_column(sc.sub[g], M, I, D, go, ge, k)
            if chains and exclude:
                D[L] = NEG                       # EXCLUSIONS 1 and 3
            chains = 0
        out.append((M, I, D, chains))
    has_succ = [False] * len(nodes)
    for pr in preds:
        for p in pr:
            has_succ[p] = True
    ends = []
    for v in range(len(nodes)):
        if not has_succ[v]:
            M, I, D, chains = out[v]
            ends += [M[L], I[L], D[L], np.full(min(chains, k), whole, dtype=np.int64)]     # a walk of empty nodes alone: the whole read inserted, once per walk
    return _descending(ends, k)


def ambiguous_empty_chains(problem):
    """(f) DUPLICATES: does some node reach one predecessor with bases over two chains of empty nodes?"""
    nodes, preds = problem["nodes"], problem["preds"]
    for v in range(len(nodes)):
        seen, stack = set(), list(preds[v])
        while stack:
            p = stack.pop()
            if nodes[p]:
                if p in seen:
                    return True
                seen.add(p)
            else:
                stack += preds[p]
    return False


def empty_chain_walks(problem, walk):
    """(f) DUPLICATES: the number of walks that differ from `walk` (a list of nodes) only in the empty nodes BETWEEN two of its nodes with bases:
    the product, over consecutive nodes with bases, of the number of chains of empty nodes that join them.  The copies of one (walk, ops) among a
    problem's alternates stand for such walks, so there are at most this many."""
    nodes, preds = problem["nodes"], problem["preds"]
    based = [v for v in walk if nodes[v]]
    total = 1
    for u, v in zip(based, based[1:]):
        n, stack = 0, list(preds[v])
        while stack:
            p = stack.pop()
            if p == u:
                n += 1
            elif not nodes[p]:
                stack += preds[p]
        total *= max(n, 1)
    return total


def pinned_kbest_bound(problem, scoring, k, qual_adj=None):
    """(g): the k highest positive scores over every pinned alignment, descending: an upper bound, rank by rank, on what a pinned multi-traceback returns."""
    sc = Scores(problem, scoring, MODE_PINNED, qual_adj)
    L, go, ge = sc.L, sc.go, sc.ge
    nodes, preds = problem["nodes"], problem["preds"]
    none = np.full((L + 1, k), NEG, dtype=np.int64)
    fresh = np.zeros((L + 1, 1), dtype=np.int64); fresh[L] = NEG               # a start in front of a base with i < L read bases soft-clipped
    lead = np.full((L + 1, L), NEG, dtype=np.int64)                            # ... and the insertions that begin at such a start: j - i bases, for every i < j
    for j in range(1, L + 1):
        lead[j, :j] = -(go + np.arange(j, dtype=np.int64) * ge)
    lead = _top([lead], k)
    out, ends = [], []
    for v, s in enumerate(nodes):
        assert len(s) > 0
        if preds[v]:
            M, I, D = (_top([out[p][x] for p in preds[v]], k) for x in range(3))
        else:
            M, I, D = none, none, none
        for g in _codes(s):
            M, I, D = _kbest_column(sc.sub[g], _top([M, fresh], k), _top([I, lead], k), D, go, ge, k)
        out.append((M, I, D))
        if problem["pinning"][v]:
            ends += [M[L], I[L], D[L]]
    return [x for x in _descending(ends, k) if x > 0]


def optimum(problem, scoring, mode, qual_adj=None):
    if mode == MODE_XDROP:
        return xdrop_optimum(problem, scoring, qual_adj)
    if mode == MODE_BANDED:
        return banded_global_optimum(problem, scoring, qual_adj)
    return gssw_optimum(problem, scoring, mode, qual_adj)


def check_alignment(problem, scoring, mode, result_row, ops, qual_adj=None, expect_optimum=None):
    """(d): walk the op list of one result (status 0, score > 0, traceback asked for) and assert that it is an
    alignment of the read to a walk of the graph whose score, re-computed from the ops alone, is result.score.

    ops: the (node, len, op) records of this result only.  Checks: soft clips first / last only (none in X-drop's
    head, none in banded); M + I + S = read length; per node M + D stays inside [first_offset or 0, node length);
    a node is left only behind its last base and entered at base 0 over an edge of preds; X-drop starts at base 0 of
    a source with read base 0; PINNED ends on the last base of a pinning node with read base L-1; banded runs from a
    source's first base to a sink's last; (end_node, end_offset, end_read) is the last graph base and the last read
    base the alignment consumed; the re-score: matrix entry per M column, gap price per maximal I / D run (a run goes
    on across nodes and across zero-length ops), bonuses by the module's rules.  expect_optimum: asserted equal too.
    Returns the re-computed score."""
    sc = Scores(problem, scoring, mode, qual_adj)
    L, go, ge = sc.L, sc.go, sc.ge
    nodes, preds = problem["nodes"], problem["preds"]
    ops = [(int(o["node"]), int(o["len"]), int(o["op"])) for o in ops]
    assert ops, "no ops"
    first_offset = 0 if mode == MODE_BANDED else int(result_row["first_offset"])
    cur = ops[0][0]
    assert 0 <= cur < len(nodes)
    off = first_offset
    assert 0 <= off <= len(nodes[cur])
    if mode in (MODE_XDROP, MODE_BANDED):
        assert not preds[cur] and off == 0, "does not start at a source's first base"
    r = 0
    score = 0
    run = None                       # op of the gap run in progress
    last_graph = None                # (node, offset) of the last graph base consumed
    last_read = -1                   # last read base consumed by M or I
    codes = {}
    for k, (node, ln, op) in enumerate(ops):
        assert op in (OP_M, OP_I, OP_D, OP_S), op
        if node != cur:
            assert 0 <= node < len(nodes)
            assert off == len(nodes[cur]), "node %d left at offset %d of %d" % (cur, off, len(nodes[cur]))
            assert cur in preds[node], "no edge %d -> %d" % (cur, node)
            cur, off = node, 0
        if op == OP_S:
            assert mode in (MODE_LOCAL, MODE_PINNED, MODE_XDROP), "soft clip in a global alignment"
            assert k == 0 or k == len(ops) - 1, "soft clip inside the alignment"
            assert ln > 0
            if k == 0:
                assert mode != MODE_XDROP and len(ops) > 1, "soft clip at the pinned end"
            else:
                assert mode != MODE_PINNED, "soft clip at the pinned end"
            r += ln
            run = None
            continue
        if ln == 0:
            assert mode == MODE_BANDED and len(nodes[cur]) == 0, "zero-length op"
            continue
        if op == OP_M:
            assert off + ln <= len(nodes[cur]) and r + ln <= L
            if cur not in codes:
                codes[cur] = _codes(nodes[cur])
            score += int(sc.sub[codes[cur][off:off + ln], np.arange(r, r + ln)].sum())
            off += ln; r += ln
            last_graph, last_read = (cur, off - 1), r - 1
            run = None
        else:
            score -= (ln * ge) if run == op else (go + (ln - 1) * ge)
            run = op
            if op == OP_I:
                assert r + ln <= L
                r += ln; last_read = r - 1
            else:
                assert off + ln <= len(nodes[cur])
                off += ln; last_graph = (cur, off - 1)
    assert r == L, "ops consume %d of %d read bases" % (r, L)
    if mode == MODE_BANDED:
        assert off == len(nodes[cur]) and not any(cur in pr for pr in preds), "does not end at a sink's last base"
    else:
        if mode == MODE_PINNED:
            assert problem["pinning"][cur] and off == len(nodes[cur]), "does not end on a pinning node's last base"
        assert last_graph is not None
        assert (int(result_row["end_node"]), int(result_row["end_offset"])) == last_graph, (result_row, last_graph)
        assert int(result_row["end_read"]) == last_read, (result_row, last_read)
    assert score == int(result_row["score"]), "re-scored %d, reported %d" % (score, int(result_row["score"]))
    if expect_optimum is not None:
        assert score == expect_optimum, "alignment scores %d, the optimum is %d" % (score, expect_optimum)
    return score


def _global_affine(a, b, mismatch, go, ge):
    """Gap-affine global distance (a cost, >= 0) of sequences a and b: match 0, mismatch, gap of n = go + n * ge."""
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        k = n + m
        return 0 if k == 0 else go + k * ge
    A = np.frombuffer(a.encode(), dtype=np.uint8); B = np.frombuffer(b.encode(), dtype=np.uint8)
    INF = 1 << 40
    ramp = np.arange(m + 1, dtype=np.int64) * ge
    H = np.full(m + 1, INF, dtype=np.int64); H[0] = 0; H[1:] = go + ramp[1:]
    E = np.full(m + 1, INF, dtype=np.int64)                     # gap in b (a base consumed alone)
    for i in range(n):
        E = np.minimum(H + go + ge, E + ge)
        diag = np.full(m + 1, INF, dtype=np.int64)
        diag[1:] = H[:-1] + np.where(B == A[i], 0, mismatch)
        H0 = np.minimum(diag, E)
        P = np.minimum.accumulate(H0 - ramp)
        F = np.full(m + 1, INF, dtype=np.int64)
        F[1:] = P[:-1] + go + ramp[1:]
        H = np.minimum(H0, F)
    return int(H[m])


_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def oriented_sequence(nodes, o):
    s = nodes[o >> 1]
    return s if not (o & 1) else "".join(_COMP[c] for c in reversed(s))


WFA_DEFAULT_MODEL = ((0.03, 1, 6), (0.05, 1, 10), (0.1, 1, 20), (0.1, 10, 200))     # mismatches, gaps, gap_length, distance: (per_base, min, max)


def wfa_penalty_cap(seq_len, match, mismatch, go, ge, model=None):
    """The error model's cap on a connect's penalty (include/vgk.h vgk_wfa_error_model; an Event allows min(max, int(per_base * length) + min)
    of its kind): allowed mismatches * mismatch penalty + allowed gaps * gap-open penalty + allowed gap length * gap-extend penalty, in the
    penalties of wfa_connect_optimum.  An alignment whose penalty is AT the cap is still accepted."""
    allow = [min(int(mx), int(per_base * seq_len) + int(mn)) for per_base, mn, mx in (model or WFA_DEFAULT_MODEL)[:3]]
    return allow[0] * 2 * (match + mismatch) + allow[1] * 2 * (go - ge) + allow[2] * (2 * ge + match)


def wfa_connect_optimum(nodes, threads, seq, from_pos, to_pos, match, mismatch, go, ge):
    """(e): the smallest WFA penalty of `seq` aligned globally (both ends pinned: no bonus) against the bases strictly between
    from_pos = (oriented node, offset) and a LATER occurrence of to_pos on one haplotype thread — over every thread, in both
    orientations, and every pair of occurrences (threads may go round cycles).  None when no thread holds such a pair.
    Penalties as the header's equivalence gives them: match 0, mismatch 2 (match + mismatch), a gap of n bases
    2 (go - ge) + n (2 ge + match); an alignment of score s over g graph bases has penalty match * (g + len(seq)) - 2 s.
    The optimum is stated in PENALTY, not in score: the wavefront search ends at the first penalty that reaches `to`, so of two
    pairs with different numbers of bases between them the one with the lower penalty wins even where the longer one would
    score more (the two orders agree for pairs of equal length)."""
    best = None
    fn, fo = from_pos; tn, to = to_pos
    for t in threads:
        t = [int(x) for x in t]
        for th in (t, [x ^ 1 for x in reversed(t)]):
            starts = [i for i, x in enumerate(th) if x == fn]
            ends = [i for i, x in enumerate(th) if x == tn]
            if not starts or not ends:
                continue
            seqs = [oriented_sequence(nodes, x) for x in th]
            for i in starts:
                for j in ends:
                    if j < i or (j == i and to <= fo):
                        continue
                    between = seqs[i][fo + 1:to] if j == i else seqs[i][fo + 1:] + "".join(seqs[i + 1:j]) + seqs[j][:to]
                    pen = _global_affine(between, seq, 2 * (match + mismatch), 2 * (go - ge), 2 * ge + match)
                    if best is None or pen < best:
                        best = pen
    return best
