"""refstitch — what vgk_chain_stitch has to return, stated from what a path MEANS: the bases of the read in read order, each either on a base of
the graph or inserted, cut wherever the graph positions stop following each other.  Plain Python, per base; no mapping objects, no "last mapping
kept", nothing of the order in which simplify (reference src/path.cpp:1314-1497) does its work.  DESIGN §30 (h).

A read is a list of pieces in a neutral form (pieces_of makes it from the call's flat arrays):
    ("aln", [oriented node...], node_offset, [(kind, length)...])        an ALIGNMENT piece, or a LINK piece as wfa_extend returned it to the host
    ("path", [(oriented node | None, offset, [(kind, length)...])...])   a PATH piece: its mappings as stated
kinds: 0 match, 1 mismatch, 2 insertion, 3 deletion (include/vgk.h VGK_WFA_*).

1. events      every piece becomes per-base events in read order: a graph-consuming base (match, mismatch, deletion) is (kind, node, offset), an
               inserted base is (INS,).  An "aln" piece takes its positions from walking its node path from node_offset with the node lengths; a
               stated mapping from its own (node, offset).  Zero-length runs make no event.
2. segments    a graph event continues the current segment when it lies on the same oriented node at the previous graph event's offset + 1,
               otherwise it opens a new one; an insertion belongs to the segment of the graph event before it, insertions before the first graph
               event to the first segment; a read of insertions only is one segment without a position.
3. trim        AFTER segmenting: segments without a read base at either end go; the first kept segment loses its leading deletions (its offset
               moves on by as many bases); the last kept one loses its trailing deletions unless it is also the first (one mapping that holds every
               read base keeps its trailing deletion: path.cpp:1453-1470); no read base at all: an empty result.
4. output      per kept segment (node, offset, run-length kinds); without a position: (NO_NODE, 0, ...).

Domain (in_domain): the statement above is what the reference's rules come to when
    (a) a mapping without a position holds insertions only, and
    (b) no mapping that has a position but holds only insertions comes before the read's first graph event.
Outside of it the reference's position-adoption rules (:1361-1380) decide what a position-less or insertion-only mapping is given, by the order
of its work; there parity with the oracle stays the only check (tests/test_chain_stitch.py)."""

MATCH, MISMATCH, INS, DEL = 0, 1, 2, 3
NO_NODE = 0xffffffff


class Malformed(ValueError):
    """a piece the engine refuses (VGK_EINVAL): the definition says nothing about it"""


def pieces_of(pieces, piece_off, r, nodes, mappings, edits, links=None):
    """read r of a call -> its pieces in the neutral form.  links: (results, paths, edits) of the wfa_extend call LINK pieces name, or None."""
    out = []
    runs = lambda b, n: [(int(x) & 3, int(x) >> 2) for x in edits[b:b + n]]
    for k in range(int(piece_off[r]), int(piece_off[r + 1])):
        pc = pieces[k]
        kind = int(pc["kind"])
        if kind == 0:
            if links is None or int(pc["link"]) >= len(links[0]):
                raise Malformed("link")
            w = links[0][int(pc["link"])]
            if w["status"] != 0 or not w["ok"]:
                raise Malformed("link not ok")
            out.append(("aln", [int(x) for x in links[1][int(w["path_begin"]):int(w["path_begin"]) + int(w["path_len"])]], int(w["node_offset"]),
                        [(int(x) & 3, int(x) >> 2) for x in links[2][int(w["edit_begin"]):int(w["edit_begin"]) + int(w["n_edits"])]]))
        elif kind == 1:
            pb, pl, eb, ne = int(pc["path_begin"]), int(pc["path_len"]), int(pc["edit_begin"]), int(pc["n_edits"])
            if pb + pl > len(nodes) or eb + ne > len(edits):
                raise Malformed("range")
            out.append(("aln", [int(x) for x in nodes[pb:pb + pl]], int(pc["node_offset"]), runs(eb, ne)))
        elif kind == 2:
            pb, pl = int(pc["path_begin"]), int(pc["path_len"])
            if pb + pl > len(mappings):
                raise Malformed("range")
            ms = []
            for m in mappings[pb:pb + pl]:
                if int(m["edit_begin"]) + int(m["n_edits"]) > len(edits):
                    raise Malformed("range")
                ms.append((None if int(m["node"]) == NO_NODE else int(m["node"]), int(m["offset"]), runs(int(m["edit_begin"]), int(m["n_edits"]))))
            out.append(("path", ms))
        else:
            raise Malformed("kind")
    return out


def _stated(read):
    """the read's mappings as far as the domain looks at them: (has a position, has a graph-consuming base, has an inserted base).  An "aln" piece
    counts as one: the first mapping its walk makes holds a graph base whenever the piece holds one."""
    for p in read:
        for node, runs in ([(p[1] or None, p[3])] if p[0] == "aln" else [(m[0], m[2]) for m in p[1]]):
            yield (node is not None, any(n and k != INS for k, n in runs), any(n and k == INS for k, n in runs))


def in_domain(read):
    """(a) a mapping without a position holds insertions only; (b) no mapping that has a position but holds only insertions comes before the read's
    first graph event"""
    seen_graph = False
    for positioned, graph, ins in _stated(read):
        if not positioned and graph:
            return False                                    # (a)
        if positioned and ins and not graph and not seen_graph:
            return False                                    # (b)
        seen_graph = seen_graph or graph
    return True


def events(read, node_len):
    """-> [(INS,) | (kind, node, offset)] in read order; Malformed where a walk leaves its path"""
    ev = []
    for p in read:
        if p[0] == "aln":
            _, path, at, runs = p
            step = 0
            if path and (path[0] >= len(node_len) or at >= node_len[path[0]]):
                raise Malformed("offset")
            for kind, n in runs:
                for _ in range(n):
                    if kind == INS:
                        ev.append((INS,)); continue
                    if step >= len(path) or path[step] >= len(node_len):
                        raise Malformed("past the path")
                    ev.append((kind, path[step], at)); at += 1
                    if at == node_len[path[step]]:
                        step += 1; at = 0
        else:
            for node, offset, runs in p[1]:
                at = offset
                for kind, n in runs:
                    for _ in range(n):
                        if kind == INS:
                            ev.append((INS,)); continue
                        if node is None:
                            raise Malformed("outside the domain: (a)")
                        ev.append((kind, node, at)); at += 1
    return ev


def segments(ev):
    """-> [[event...]...]: cut where a graph event does not follow the one before it"""
    segs, last = [], None
    for e in ev:
        if e[0] != INS:
            if last is None and segs:
                pass                                        # insertions came first: they are in the first segment already
            elif last is None or e[1] != last[1] or e[2] != last[2] + 1:
                segs.append([])
            last = e
        elif not segs:
            segs.append([])
        segs[-1].append(e)
    return segs


def refstitch(read, node_len):
    """-> ([(node, offset, [(kind, length)...])...], from_length, to_length)"""
    segs = segments(events(read, node_len))
    has_base = lambda s: any(e[0] != DEL for e in s)
    while segs and not has_base(segs[0]):
        segs.pop(0)
    while segs and not has_base(segs[-1]):
        segs.pop()
    if not segs:
        return [], 0, 0
    at = [next(((e[1], e[2]) for e in s if e[0] != INS), None) for s in segs]       # a segment's position: its first graph event's
    first = segs[0]
    while first[0][0] == DEL:                               # (a trimmed segment that keeps only insertions stays where its deleted bases ended)
        first.pop(0); at[0] = (at[0][0], at[0][1] + 1)
    if len(segs) > 1:
        while segs[-1][-1][0] == DEL:
            segs[-1].pop()
    out = []
    for s, w in zip(segs, at):
        where = (None,) + w if w else None
        runs = []
        for e in s:
            if runs and runs[-1][0] == e[0]:
                runs[-1][1] += 1
            else:
                runs.append([e[0], 1])
        out.append((where[1] if where else NO_NODE, where[2] if where else 0, [(k, n) for k, n in runs]))
    return out, sum(1 for s in segs for e in s if e[0] != INS), sum(1 for s in segs for e in s if e[0] != DEL)


def merge_insertions(mappings):
    """an engine's answer with insertion runs side by side made one (path.cpp:1349 appends without merging); any OTHER kind side by side is an error"""
    out = []
    for node, offset, runs in mappings:
        merged = []
        for k, n in runs:
            assert n > 0, ("an empty run", mappings)
            if merged and merged[-1][0] == k:
                assert k == INS, ("runs of one kind side by side that are not insertions", mappings)
                merged[-1] = (k, merged[-1][1] + n)
            else:
                merged.append((k, n))
        out.append((node, offset, merged))
    return out
