"""vgk_pick_mappings (include/vgk_engine.h): a long read's mappings chosen from its chains' alignments — the multiplicity fix-up at the end of
do_alignment_on_chains (src/minimizer_mapper_from_chains.cpp:2241-2262, chain_ranges_are_equivalent :100-191) and pick_mappings_from_alignments
(:2265-2493).  No reference unit test names these loops, so the rule is pinned from the outside in: `own` below restates the cited lines in another
shape (all sort keys first, a Python set of tuples, counts as ints masked to 64 bits, equivalence from an interval table); the host shim
(vg_amd/host/pick_mappings.cpp, the reference's loop shape) must equal it in every field, doubles bit for bit; the serial device rule
(vg_amd/csrc/pick_mappings_device.hpp behind tests/emu/pick_mappings_driver.cpp) must equal the shim, also as a program of its own under the host
sanitizers; the engine must equal the shim (-m gpu)."""
import collections
import ctypes
import os
import subprocess

import numpy as np
import pytest

from util import ENGINE_LIB
from vg_amd import capi, pipeline, workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = os.path.join(ROOT, "vg_amd", "libvgamd.so")
DRIVER = os.path.join(ROOT, "tests", "emu", "libvgamd_pickmappings.so")
OK, EINVAL, EOPS = capi.VGK_OK, capi.VGK_EINVAL, capi.VGK_EOPS
NO_NODE = capi.WFA_NO_NODE
MATCH, MISMATCH, INS, DEL = 0, 1, 2, 3
M64 = (1 << 64) - 1
ARGS = ("reads", "read_off", "chain_off", "chains", "aln_off", "alns", "mappings", "edits")
LDS_NODES, LDS_SLOTS, LDS_ITEMS = 1024, 2048, 32       # vgk_pick_mappings_limits, held to the library's answer below


def schemes():
    return collections.OrderedDict([
        ("the defaults", capi.PickScheme.defaults()),
        ("three multimaps, half unique", capi.PickScheme.defaults(max_multimaps=3, min_unique_node_fraction=0.5)),
        ("sorted by chain score", capi.PickScheme.defaults(max_multimaps=2, min_unique_node_fraction=0.25, flags=capi.PICK_SORT_BY_CHAIN_SCORE)),
        ("all unique", capi.PickScheme.defaults(max_multimaps=2, min_unique_node_fraction=1.0)),
    ])


# ---- the statement in another shape ---------------------------------------------------------------------------------------------------------------------
class Minstd:
    """std::minstd_rand resumed from a state word; 0: made at the first draw, seeded from the read's bytes as LazyRNG seeds it"""
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


def interval_table(chains, cover):
    """equivalent[c][d] for every ordered pair of a read's chains: each chain's offsets as an interval first, then the pairs"""
    spans = []
    for c in chains:
        lo, hi = int(c["range"]["offset_start"]), int(c["range"]["offset_end"])
        if lo > hi:
            cover["a chain's offsets swapped into order"] += 1
        spans.append((min(lo, hi), max(lo, hi)))
    table = [[False] * len(chains) for _ in chains]
    for i, c in enumerate(chains):
        for j, d in enumerate(chains):
            a, b = c["range"], d["range"]                           # (i == j too: two alignments may come from one chain)
            if int(a["component"]) != int(b["component"]):
                cover["different components"] += 1
                continue
            if int(a["flags"]) & capi.CHAIN_RANGE_ROOT_SNARL:
                if int(a["child_start"]) != int(b["child_start"]):
                    cover["root snarl: the first seeds' ranks differ"] += 1
                    continue
                if int(a["child_start"]) != int(a["child_end"]):
                    cover["root snarl: chain 1 spans two children"] += 1
                    continue
                if int(b["child_start"]) != int(b["child_end"]):
                    cover["root snarl: chain 2 spans two children"] += 1
                    continue
                cover["root snarl: one child"] += 1
            elif int(b["flags"]) & capi.CHAIN_RANGE_ROOT_SNARL:
                cover["only chain 2 in a root snarl: not looked at"] += 1
            (s1, e1), (s2, e2) = spans[i], spans[j]
            if e1 < s2 or e2 < s1:
                cover["disjoint ranges"] += 1
                continue
            if s1 <= s2 and e2 <= e1:
                cover["range 1 contains range 2"] += 1
                table[i][j] = True
            elif s2 <= s1 and e1 <= e2:
                cover["range 2 contains range 1"] += 1
                table[i][j] = True
            else:
                if s2 < s1:
                    cover["overlap with range 2 first"] += 1
                common = min(e1, e2) - max(s1, s2)
                shorter = min(e1 - s1, e2 - s2)
                if 2 * common == shorter and shorter % 2 == 0:
                    cover["overlap exactly half: not equivalent"] += 1
                cover["overlap more than half" if common > shorter // 2 else "overlap at most half"] += 1
                table[i][j] = common > shorter // 2
    return table


def path_of(a, i):
    """alignment i's mappings as (node, [(kind, length)])"""
    g = a["alns"]["result"][i]
    out = []
    for m in a["mappings"][int(g["mapping_begin"]):int(g["mapping_begin"]) + int(g["n_mappings"])]:
        runs = a["edits"][int(m["edit_begin"]):int(m["edit_begin"]) + int(m["n_edits"])]
        out.append((int(m["node"]), [(int(e) & 3, int(e) >> 2) for e in runs]))
    return out


def malformed_read(a, r):
    C = int(a["chain_off"][r + 1]) - int(a["chain_off"][r])
    for c in a["chains"][int(a["chain_off"][r]):int(a["chain_off"][r + 1])]:
        if not np.isfinite(c["multiplicity"]):
            return True
    for i in range(int(a["aln_off"][r]), int(a["aln_off"][r + 1])):
        al = a["alns"][i]; g = al["result"]
        if int(al["source"]) >= C or int(g["mapping_begin"]) + int(g["n_mappings"]) > len(a["mappings"]):
            return True
        for m in a["mappings"][int(g["mapping_begin"]):int(g["mapping_begin"]) + int(g["n_mappings"])]:
            if int(m["edit_begin"]) + int(m["n_edits"]) > len(a["edits"]):
                return True
    return False


def own(s, a, rng_state=None, cover=None, cap=None):
    """-> (rc, capi.pick_mappings_call's dict); rng_state is updated in place"""
    cover = collections.Counter() if cover is None else cover
    n = len(a["chain_off"]) - 1
    if s.flags & ~capi.PICK_SORT_BY_CHAIN_SCORE or s.max_multimaps == 0 or s.min_unique_node_fraction != s.min_unique_node_fraction:
        return EINVAL, dict(written=0)
    if n == 0:
        return OK, dict(results=np.zeros(0, dtype=capi.PICK_RESULT_DT), verdicts=np.zeros(0, dtype=capi.PICK_VERDICT_DT), picked=np.zeros(0, dtype=np.uint32),
                        scores=np.zeros(0, dtype=np.int32), multiplicity=np.zeros(0, dtype=np.float64), written=0)
    for off in (a["chain_off"], a["aln_off"]) + ((a["read_off"],) if rng_state is not None else ()):
        if int(off[0]) != 0 or (np.diff(off.astype(np.int64)) < 0).any():
            return EINVAL, dict(written=0)
    room = int(a["aln_off"][n]) + n
    if room > (room if cap is None else cap):
        return EOPS, dict(written=room)
    results = np.zeros(n, dtype=capi.PICK_RESULT_DT); verdicts = np.zeros(len(a["alns"]), dtype=capi.PICK_VERDICT_DT)
    picked = np.zeros(room, dtype=np.uint32); scores = np.zeros(room, dtype=np.int32); mult_out = np.zeros(room, dtype=np.float64)
    seen_results = {}
    for r in range(n):
        if malformed_read(a, r):
            results["status"][r] = EINVAL
            continue
        lo, hi = int(a["aln_off"][r]), int(a["aln_off"][r + 1]); A = hi - lo
        chains = a["chains"][int(a["chain_off"][r]):int(a["chain_off"][r + 1])]
        alns = a["alns"][lo:hi]
        if A == 0:
            cover["a read without alignments"] += 1
        table = interval_table(chains, cover)
        source = [int(x) for x in alns["source"]]; est = [int(chains["score_estimate"][c]) for c in source]
        paths = [path_of(a, i) for i in range(lo, hi)]
        # multiplicities
        mult = []
        for i in range(A):
            lower = sum(1 for j in range(A) if j != i and est[i] >= est[j] and table[source[i]][source[j]])
            count = (int(alns["item_count"][i]) - lower) & M64
            if int(alns["item_count"][i]) < lower:
                cover["the count wraps below 0"] += 1
            cover["count > A" if count > A else "count == A" if count == A else "count < A"] += 1
            mult.append(float(chains["multiplicity"][source[i]]) + ((float(count) - float(A)) if count >= A else 0.0))
        # identities and sort keys, all of them first
        identity, keys = [], []
        for i, path in enumerate(paths):
            runs = [(mi, ei, k, l) for mi, (_, es) in enumerate(path) for ei, (k, l) in enumerate(es)]
            to_length = sum(l for _, _, k, l in runs if k != DEL); matched = sum(l for _, _, k, l in runs if k == MATCH)
            ends = set()
            if path and path[0][1] and path[0][1][0][0] == INS:
                ends.add((0, 0)); cover["a leading insertion"] += 1
            if path and path[-1][1] and path[-1][1][-1][0] == INS:
                ends.add((len(path) - 1, len(path[-1][1]) - 1)); cover["a trailing insertion"] += 1
            length = to_length - sum(path[mi][1][ei][1] for mi, ei in ends)
            if length == 0 and to_length > 0:
                cover["to_length 0 once its only insertion is taken off"] += 1
            identity.append(matched / length if length else 0.0)
            keys.append(float(est[i]) if s.flags & capi.PICK_SORT_BY_CHAIN_SCORE else float(int(alns["score"][i])) + identity[-1])
            if any(node == NO_NODE for node, _ in path):
                cover["a mapping without a node"] += 1
            named = [node for node, _ in path if node != NO_NODE]
            if len(set(named)) < len(named):
                cover["a node visited twice by one alignment"] += 1
            where = (int(alns["result"]["mapping_begin"][i]), int(alns["result"]["n_mappings"][i]))
            if where[1] and seen_results.get(where, i + lo) != i + lo:
                cover["two results naming the same mappings"] += 1
            seen_results.setdefault(where, i + lo)
            if int(alns["score"][i]) == 0:
                cover["an alignment of score 0"] += 1
            if int(alns["score"][i]) < 0:
                cover["an alignment of negative score"] += 1
        verdicts["identity"][lo:hi] = identity
        # the walk
        order = sorted(range(A), key=lambda i: -keys[i])
        width = sum(1 for i in order if keys[i] == keys[order[0]]) if A else 0
        rng = Minstd(rng_state[r], a["reads"][int(a["read_off"][r]):int(a["read_off"][r + 1])]) if rng_state is not None else None
        if width >= 2 and rng is not None:
            cover["a tie at the top that is shuffled"] += 1
            for i in range(1, width):
                j = rng() % (i + 1)
                order[j], order[i] = order[i], order[j]
        if not s.flags & capi.PICK_SORT_BY_CHAIN_SCORE and any(int(alns["score"][x]) == int(alns["score"][y]) and keys[x] != keys[y] for x, y in zip(order, order[1:])):
            cover["a tie of score broken by identity"] += 1
        used, taken, out = set(), 0, []
        for i in order:
            beyond = taken >= s.max_multimaps
            nodes = [(node, sum(l for k, l in es if k != INS)) for node, es in paths[i] if node != NO_NODE]
            if int(alns["score"][i]) <= 0:
                verdicts["fate"][i + lo] = capi.PICK_FAIL_SCORE
                verdicts["fraction_unique"][i + lo:i + lo + 1].view(np.uint64)[0] = capi.PICK_NOT_EVALUATED
                if beyond:
                    cover["failing a filter beyond the cut"] += 1
                continue
            total = sum(l for _, l in nodes); shared = sum(l for node, l in nodes if (node >> 1, node & 1) in used)
            fraction = (total - shared) / total if total > 0 else 1.0
            verdicts["fraction_unique"][i + lo] = fraction
            if fraction < s.min_unique_node_fraction:
                verdicts["fate"][i + lo] = capi.PICK_FAIL_UNIQUE
                cover["an alignment failing uniqueness"] += 1
                if beyond:
                    cover["failing a filter beyond the cut"] += 1
                continue
            if fraction == s.min_unique_node_fraction and 0 < fraction < 1:
                cover["a fraction exactly at the minimum: kept"] += 1
            if beyond:
                verdicts["fate"][i + lo] = capi.PICK_BEYOND_CUT
                cover["counted beyond the cut"] += 1
            else:
                verdicts["fate"][i + lo] = capi.PICK_MAPPING
                used |= set((node >> 1, node & 1) for node, _ in nodes)
                taken += 1
            out.append((i, int(alns["score"][i]), mult[i]))
        if rng is not None:
            rng_state[r] = rng.x
        if not taken:
            cover["a read that ends unmapped"] += 1
            out = [(capi.PICK_NONE, 0, 0.0)]
        first = lo + r
        results[r] = (OK, first, len(out), taken, 0 if taken else 1, 0)
        for k, (i, sc, m) in enumerate(out):
            picked[first + k] = i; scores[first + k] = sc; mult_out[first + k] = m
    return OK, dict(results=results, verdicts=verdicts, picked=picked, scores=scores, multiplicity=mult_out, written=room)


# ---- calls -------------------------------------------------------------------------------------------------------------------------------------------------
def shim_call(s, a, rng_state=None, cap=None, threads=2):
    return capi.pick_mappings_call(pipeline._host_lib().vgh_pick_mappings, (), s, *(a[k] for k in ARGS), rng_state=rng_state, tail=(ctypes.c_int(threads),), cap=cap)


def driver_call(s, a, rng_state=None, cap=None):
    return capi.pick_mappings_call(ctypes.CDLL(DRIVER).vgt_pick_mappings_serial, (), s, *(a[k] for k in ARGS), rng_state=rng_state, cap=cap)


def engine_call(gpu):
    def call(s, a, rng_state=None, cap=None):
        return capi.pick_mappings_call(gpu.lib.vgk_pick_mappings, (gpu.h,), s, *(a[k] for k in ARGS), rng_state=rng_state, cap=cap)
    return call


def same(got, want, what):
    (rc, g), (wrc, w) = got, want
    assert rc == wrc, (what, rc, wrc)
    if wrc not in (OK, EOPS):
        return
    assert g["written"] == w["written"], (what, g["written"], w["written"])
    if wrc == EOPS:
        return
    for name in capi.PICK_RESULT_DT.names:
        bad = np.nonzero(g["results"][name] != w["results"][name])[0]
        assert not len(bad), (what, "read", int(bad[0]), name, g["results"][bad[0]], w["results"][bad[0]])
    for name in capi.PICK_VERDICT_DT.names:                        # doubles by their bits
        x, y = np.ascontiguousarray(g["verdicts"][name]), np.ascontiguousarray(w["verdicts"][name])
        bad = np.nonzero(x.view(np.uint64 if x.dtype == np.float64 else x.dtype) != y.view(np.uint64 if y.dtype == np.float64 else y.dtype))[0]
        assert not len(bad), (what, "alignment", int(bad[0]), name, g["verdicts"][bad[0]], w["verdicts"][bad[0]])
    assert (g["picked"] == w["picked"]).all() and (g["scores"] == w["scores"]).all(), what
    assert g["multiplicity"].tobytes() == w["multiplicity"].tobytes(), what


def both(call, s, a, state, cap=None):
    """a call over a copy of the generator states -> ((rc, dict), the states it leaves)"""
    st = None if state is None else state.copy()
    return call(s, a, rng_state=st, cap=cap), st


def same_with_states(call, s, a, state, want, want_state, what):
    got, st = both(call, s, a, state)
    same(got, want, what)
    assert state is None or (st == want_state).all(), (what, "generator states")


# ---- reads by construction -----------------------------------------------------------------------------------------------------------------------------------
def chain(estimate, multiplicity=1.0, component=0, offsets=(0, 10), root=False, ranks=(0, 0)):
    return dict(estimate=estimate, multiplicity=multiplicity, component=component, offsets=offsets, root=root, ranks=ranks)


def aln(source, score, path=None, item_count=1, share=None):
    """path: [(node, [(kind, length)])]; share: the number of an earlier alignment of the read whose mappings this one names as well"""
    return dict(source=source, score=score, path=path, item_count=item_count, share=share)


def matches(nodes, length=10):
    return [(int(node), [(MATCH, length)]) for node in nodes]


def build(specs, seed=1):
    """specs: per read (bases, [chain()], [aln()]) -> the call's arrays"""
    rng = np.random.default_rng(seed)
    reads, read_off, chain_off, aln_off = [], [0], [0], [0]
    chains, alns, mappings, edits = [], [], [], []
    for L, cs, als in specs:
        reads.append(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, L)]); read_off.append(read_off[-1] + L)
        for c in cs:
            chains.append((c["estimate"], 0, c["multiplicity"], (c["component"], capi.CHAIN_RANGE_ROOT_SNARL if c["root"] else 0, c["ranks"][0], c["ranks"][1], 0, c["offsets"][0], c["offsets"][1])))
        where = []
        for x in als:
            if x["share"] is not None:
                begin, count = where[x["share"]]
            else:
                begin, count = len(mappings), len(x["path"])
                for node, es in x["path"]:
                    mappings.append((node, 0, len(edits), len(es)))
                    edits.extend((l << 2) | k for k, l in es)
            where.append((begin, count))
            alns.append((x["source"], x["score"], x["item_count"], (0, begin, count, 0, 0, 0, 0, 0)))
        chain_off.append(len(chains)); aln_off.append(len(alns))
    return dict(reads=np.concatenate(reads) if reads else np.zeros(0, dtype=np.uint8), read_off=np.array(read_off, dtype=np.uint64), chain_off=np.array(chain_off, dtype=np.uint64),
                chains=np.array(chains, dtype=capi.PICK_CHAIN_DT), aln_off=np.array(aln_off, dtype=np.uint64), alns=np.array(alns, dtype=capi.PICK_ALIGNMENT_DT),
                mappings=np.array(mappings, dtype=capi.CHAIN_MAPPING_DT), edits=np.array(edits, dtype=np.uint32))


def random_path(rng, pool):
    """a few mappings over a small pool of oriented nodes, most of them plain matches of ten bases"""
    n = int(rng.integers(1, 7)); path = []
    for k in range(n):
        node = NO_NODE if rng.random() < 0.04 else int(rng.choice(pool))
        shape = rng.random()
        if node == NO_NODE:
            es = [(INS, int(rng.integers(1, 5)))]
        elif shape < 0.7:
            es = [(MATCH, 10)]
        elif shape < 0.8:
            es = [(MATCH, 4), (MISMATCH, 1), (MATCH, 5)]
        elif shape < 0.9:
            es = [(MATCH, 6), (DEL, 2), (MATCH, 2)]
        else:
            es = [(MATCH, 5), (INS, int(rng.integers(1, 4))), (MATCH, 5)]
        if k == 0 and rng.random() < 0.08:
            es = [(INS, 3)] + es
        if k == n - 1 and rng.random() < 0.08:
            es = es + [(INS, 2)]
        path.append((node, es))
    return path


def random_read(rng):
    C = int(rng.integers(1, 5)); A = int(rng.integers(0, 6))
    cs = []
    for _ in range(C):
        lo = int(rng.integers(0, 30)); hi = lo + int(rng.integers(0, 24))
        offsets = (hi, lo) if rng.random() < 0.2 else (lo, hi)
        root = rng.random() < 0.35
        ranks = (int(rng.integers(0, 2)), 0); ranks = (ranks[0], ranks[0] if rng.random() < 0.7 else 1 - ranks[0])
        cs.append(chain(int(rng.choice([10, 20, 20, 30])), float(rng.choice([0.0, 1.0, 1.0, 2.5])), int(rng.random() < 0.15), offsets, root, ranks))
    pool = rng.integers(2, 2000, int(rng.integers(3, 12))).astype(np.int64)
    als = []
    for i in range(A):
        score = int(rng.choice([-3, 0, 7, 12, 12, 12, 20]))
        if i and rng.random() < 0.1:
            als.append(aln(int(rng.integers(0, C)), score, item_count=int(rng.integers(0, A + 3)), share=int(rng.integers(0, i))))
        else:
            als.append(aln(int(rng.integers(0, C)), score, random_path(rng, pool), item_count=int(rng.integers(0, A + 3))))
    return (int(rng.integers(1, 40)), cs, als)


def planted_reads():
    """the cases a random read seldom is, a dozen of each"""
    out = []
    for k in range(12):
        a, b, c, d = 100 + 8 * k, 102 + 8 * k, 104 + 8 * k, 106 + 8 * k
        two = [chain(30, offsets=(0, 20)), chain(20, component=1, offsets=(0, 20))]
        # half of the second alignment lies on the first one's nodes: exactly the minimum of the second scheme
        out.append((20, two, [aln(0, 20, matches([a, b])), aln(1, 12, matches([a, c]))]))
        # its own node twice: both visits count as unique; the neighbour on the same node twice fails
        out.append((20, two, [aln(0, 20, matches([a, b, a])), aln(1, 12, matches([a, a, d]))]))
        # an alignment that is one insertion: identity 0.0, nothing to be unique about
        out.append((20, two, [aln(0, 9, [(NO_NODE, [(INS, 7 + k)])]), aln(1, 9, [(c, [(INS, 2)])])]))
        # a best chain counted once with two equivalent lower chains aligned: the count wraps
        three = [chain(30, offsets=(0, 20)), chain(20, offsets=(2, 18)), chain(10, offsets=(4, 16))]
        out.append((20, three, [aln(0, 20, matches([a]), item_count=1), aln(1, 12, matches([b]), item_count=3), aln(2, 7, matches([c]), item_count=5)]))
        # two ranges that overlap by exactly half of the shorter one, and by one more
        out.append((20, [chain(20, offsets=(0, 10)), chain(20, offsets=(6, 14 + k)), chain(20, offsets=(5, 13))],
                    [aln(0, 12, matches([a])), aln(1, 12, matches([b])), aln(2, 12, matches([c]))]))
        # a tie of score that identity breaks; an alignment beyond the cut that fails, and one that is counted
        out.append((20, two, [aln(0, 12, [(a, [(MATCH, 8), (MISMATCH, 2)])]), aln(1, 12, matches([b])), aln(1, 12, matches([b, c])), aln(0, 5, matches([d])), aln(0, 0, matches([d]))]))
    return out


def edge_reads():
    """the sizes at which a kernel can go wrong: the wavefront's stride, the LDS table's limit, its collisions, the order's limit, a statistics wavefront's edge"""
    two = [chain(30, offsets=(0, 20)), chain(20, component=1, offsets=(0, 20))]
    out = []
    for n in (1, 63, 64, 65, 129):
        nodes = np.arange(5000, 5000 + 2 * n, 2)
        out.append((30, two, [aln(0, 20, matches(nodes)), aln(1, 12, matches(np.concatenate([nodes[:n // 2], nodes[:n - n // 2] + 1])))]))
    for n in (LDS_NODES - 1, LDS_NODES, LDS_NODES + 1):
        nodes = np.arange(20000, 20000 + 2 * n, 2)
        out.append((30, two, [aln(0, 20, matches(nodes)), aln(1, 12, matches(np.concatenate([nodes[-40:], [9, 11]])))]))
    # every key in one slot of the LDS table: nodes chosen from the header's hash
    all_nodes = np.arange(1, 1 << 20, dtype=np.uint64)
    slot = ((all_nodes * 2654435761) & 0xffffffff) >> (32 - 11)
    colliding = all_nodes[slot == 77][:300].astype(np.int64)
    assert len(colliding) == 300 and LDS_SLOTS == 1 << 11
    out.append((30, two, [aln(0, 20, matches(colliding[:200])), aln(1, 12, matches(np.concatenate([colliding[150:300], colliding[:30]])))]))
    for n in (LDS_ITEMS, LDS_ITEMS + 1):
        out.append((30, two, [aln(k % 2, 5 + (k * 7) % 11, matches([30000 + 2 * (k % 9), 30001 + 2 * k])) for k in range(n)]))
    # an alignment across the edge of a statistics wavefront, a neighbour of one mapping before it
    out.append((30, two, [aln(0, 20, matches(np.arange(40000, 40120, 2))), aln(1, 12, matches([40000])), aln(0, 11, matches(np.arange(40001, 40021, 2))), aln(1, 10, matches(np.arange(40200, 40800, 2)))]))
    return out


def states_for(a, seed):
    """generator states as a funnel leaves them: some not made yet, some under way"""
    rng = np.random.default_rng(seed); n = len(a["chain_off"]) - 1
    return np.where(rng.random(n) < 0.5, 0, rng.integers(1, 2147483646, n)).astype(np.uint32)


@pytest.fixture(scope="module")
def corpus():
    subprocess.check_call(["make", "-s", "pickmappings"], cwd=ROOT)
    rng = np.random.default_rng(20261021)
    cover = collections.Counter(); runs = []
    for k, (name, s) in enumerate(schemes().items()):
        specs = [random_read(rng) for _ in range(680)] + planted_reads()
        a = build(specs, seed=k + 1)
        state = states_for(a, k) if k != 2 else None              # one scheme without generators: nothing is shuffled
        want, want_state = both(lambda s, a, rng_state, cap: own(s, a, rng_state, cover, cap), s, a, state)
        runs.append(dict(name=name, scheme=s, a=a, state=state, want=want, want_state=want_state))
    edge = build(edge_reads(), seed=9)
    return dict(runs=runs, cover=cover, edge=edge)


CASES = """a tie at the top that is shuffled|a tie of score broken by identity|an alignment of score 0|an alignment of negative score|an alignment failing uniqueness
a fraction exactly at the minimum: kept|counted beyond the cut|failing a filter beyond the cut|a read that ends unmapped|a read without alignments
to_length 0 once its only insertion is taken off|a leading insertion|a trailing insertion|a mapping without a node|a node visited twice by one alignment
two results naming the same mappings|different components|root snarl: the first seeds' ranks differ|root snarl: chain 1 spans two children
root snarl: chain 2 spans two children|root snarl: one child|only chain 2 in a root snarl: not looked at|a chain's offsets swapped into order|disjoint ranges
range 1 contains range 2|range 2 contains range 1|overlap with range 2 first|overlap exactly half: not equivalent|overlap more than half|overlap at most half
the count wraps below 0|count > A|count == A|count < A"""


def test_the_corpus_holds_every_case(corpus):
    """the census is the statement's own, on the CPU: every case the rule distinguishes occurs at least ten times among about 3 000 reads"""
    assert sum(len(r["a"]["chain_off"]) - 1 for r in corpus["runs"]) >= 2900
    for case in CASES.replace("\n", "|").split("|"):
        assert corpus["cover"][case] >= 10, (case, corpus["cover"][case])
    for r in corpus["runs"]:
        assert (r["want"][1]["results"]["status"] == OK).all()


def test_the_wrap_is_the_reference_s():
    """a best chain with item_count 1 and two equivalent lower chains aligned: the count is 2^64 - 1, the multiplicity the chain's + 2^64 - 3"""
    a = build([planted_reads()[3]])
    rc, out = shim_call(capi.PickScheme.defaults(), a)
    assert rc == OK and out["multiplicity"][0] == 1.0 + (float(M64) - 3.0) and out["multiplicity"][0] > 1.8e19
    same((rc, out), own(capi.PickScheme.defaults(), a), "the wrap")


def test_the_shim_equals_the_statement_in_another_shape(corpus):
    for r in corpus["runs"]:
        same_with_states(shim_call, r["scheme"], r["a"], r["state"], r["want"], r["want_state"], "shim, " + r["name"])
    for name, s in schemes().items():
        same(shim_call(s, corpus["edge"]), own(s, corpus["edge"]), "shim, edge reads, " + name)


def test_the_serial_device_rule_equals_the_shim(corpus):
    for r in corpus["runs"]:
        want, want_state = both(shim_call, r["scheme"], r["a"], r["state"])
        same_with_states(driver_call, r["scheme"], r["a"], r["state"], want, want_state, "serial rule, " + r["name"])
    for name, s in schemes().items():
        same(driver_call(s, corpus["edge"]), shim_call(s, corpus["edge"]), "serial rule, edge reads, " + name)


def test_the_edge_reads_say_what_they_were_built_for(corpus):
    s = schemes()["three multimaps, half unique"]
    rc, out = own(s, corpus["edge"])
    v, res, off = out["verdicts"], out["results"], corpus["edge"]["aln_off"].astype(np.int64)
    assert rc == OK and (res["status"] == OK).all()
    assert [int(x) for x in corpus["edge"]["alns"]["result"]["n_mappings"][off[:5]]] == [1, 63, 64, 65, 129]
    assert [int(x) for x in corpus["edge"]["alns"]["result"]["n_mappings"][off[5:8]]] == [LDS_NODES - 1, LDS_NODES, LDS_NODES + 1]
    # the second alignment of a stride read shares half its nodes, to the mapping; of a limit read 40 of 42; of the colliding read everything
    assert all(v["fraction_unique"][off[k] + 1] == (n - n // 2) * 10 / (n * 10) for k, n in enumerate((1, 63, 64, 65, 129)))
    assert all(v["fraction_unique"][off[k] + 1] == 2 / 42 and v["fate"][off[k] + 1] == capi.PICK_FAIL_UNIQUE for k in (5, 6, 7))
    assert v["fraction_unique"][off[8] + 1] == 100 / 180 and v["fate"][off[8] + 1] == capi.PICK_MAPPING
    assert [int(off[k + 1] - off[k]) for k in (9, 10)] == [LDS_ITEMS, LDS_ITEMS + 1]
    assert [int(x) for x in corpus["edge"]["alns"]["result"]["n_mappings"][off[11]:off[12]]] == [60, 1, 10, 300]


# ---- malformed calls and sizing --------------------------------------------------------------------------------------------------------------------------------
def malformed():
    """(what, scheme, the call, the reads that must answer VGK_EINVAL alone — or None: the call is refused)"""
    s = schemes()["three multimaps, half unique"]
    base = lambda: build([random_read(np.random.default_rng(k)) for k in (3, 4, 5)] + planted_reads()[:2])
    out = []
    a = base(); a["alns"]["source"][int(a["aln_off"][3])] = 2
    out.append(("a source outside the read's chains", s, a, [3]))
    a = base(); a["aln_off"][2] = a["aln_off"][3] + 1
    out.append(("descending offsets", s, a, None))
    a = base(); a["alns"]["result"]["n_mappings"][int(a["aln_off"][4])] = len(a["mappings"])
    out.append(("a result past the mappings", s, a, [4]))
    a = base(); a["mappings"]["n_edits"][-1] = 2
    out.append(("a mapping past the edit runs", s, a, [4]))
    a = base(); a["chains"]["multiplicity"][int(a["chain_off"][3])] = float("nan")
    out.append(("a NaN multiplicity", s, a, [3]))
    out.append(("unknown flags", capi.PickScheme.defaults(flags=2), base(), None))
    out.append(("max_multimaps 0", capi.PickScheme.defaults(max_multimaps=0), base(), None))
    return out


def hold_malformed(call, what):
    for name, s, a, refused in malformed():
        rc, want = own(s, a)
        got = call(s, a)
        assert (rc == EINVAL) == (refused is None), name
        same(got, (rc, want), what + ": " + name)
        if refused is not None:
            res = got[1]["results"]
            assert [int(r) for r in np.nonzero(res["status"] == EINVAL)[0]] == refused, (what, name)
            for r in refused:
                assert all(int(res[f][r]) == 0 for f in capi.PICK_RESULT_DT.names if f != "status")
                assert not got[1]["verdicts"][int(a["aln_off"][r]):int(a["aln_off"][r + 1])].tobytes().strip(b"\0")
    empty = build([])
    rc, got = call(capi.PickScheme.defaults(), empty)
    assert rc == OK and got["written"] == 0, what


def hold_sizing(call, r, what):
    room = int(r["a"]["aln_off"][-1]) + len(r["a"]["chain_off"]) - 1
    got, _ = both(call, r["scheme"], r["a"], r["state"], cap=room - 1)
    assert got[0] == EOPS and got[1]["written"] == room and not got[1]["results"].tobytes().strip(b"\0"), what
    same_with_states(call, r["scheme"], r["a"], r["state"], r["want"], r["want_state"], what + ": exactly the room")


def test_malformed_calls_are_refused_where_the_header_says(corpus):
    hold_malformed(shim_call, "shim")
    hold_malformed(driver_call, "serial rule")


def test_sizing(corpus):
    hold_sizing(shim_call, corpus["runs"][1], "shim")
    hold_sizing(driver_call, corpus["runs"][1], "serial rule")


# ---- the serial rule as a program of its own under the host sanitizers -------------------------------------------------------------------------------------------
def write_call(path, s, a, state, cap):
    with open(path, "wb") as f:
        f.write(np.array([len(a["chain_off"]) - 1, len(a["chains"]), len(a["alns"]), len(a["mappings"]), len(a["edits"]), len(a["reads"]), 0 if state is None else 1, cap], dtype=np.uint64).tobytes())
        f.write(bytes(s))
        for x in (a["read_off"], a["reads"]) + (() if state is None else (state,)) + (a["chain_off"], a["chains"], a["aln_off"], a["alns"], a["mappings"], a["edits"]):
            f.write(np.ascontiguousarray(x).tobytes())


def read_answer(path, a, state):
    raw = open(path, "rb").read()
    head = np.frombuffer(raw[:16], dtype=np.uint64)
    rc = int(head[0].astype(np.int64)); w = int(head[1])
    if rc != OK:
        return (rc, dict(written=w)), None
    at = 16; out = {}
    for name, dt, count in (("results", capi.PICK_RESULT_DT, len(a["chain_off"]) - 1), ("verdicts", capi.PICK_VERDICT_DT, len(a["alns"])), ("picked", np.uint32, w), ("scores", np.int32, w),
                            ("multiplicity", np.float64, w), ("state", np.uint32, 0 if state is None else len(state))):
        size = np.dtype(dt).itemsize * count
        out[name] = np.frombuffer(raw[at:at + size], dtype=dt); at += size
    assert at == len(raw)
    return (rc, dict(out, written=w)), out.pop("state")


def test_the_serial_rule_under_the_host_sanitizers(corpus, tmp_path):
    """the driver as a program of its own under -fsanitize=address,undefined over the whole corpus, the edge reads and the malformed calls, at exactly the room
    the answer needs: the statement's answers, nothing reported.  No Python process is involved in the run."""
    subprocess.check_call(["make", "-s", "pickmappings_san"], cwd=ROOT)
    program = os.path.join(ROOT, "tests", "emu", "pick_mappings_san")

    def run(s, a, state, cap):
        write_call(tmp_path / "call.bin", s, a, state, cap)
        done = subprocess.run([program, str(tmp_path / "call.bin"), str(tmp_path / "answer.bin")], capture_output=True, text=True)
        assert done.returncode in (0, 1) and done.stderr == "", done.stderr[-2000:]
        return read_answer(tmp_path / "answer.bin", a, state)
    for r in corpus["runs"]:
        got, st = run(r["scheme"], r["a"], r["state"], r["want"][1]["written"])
        same(got, r["want"], "under the sanitizers, " + r["name"])
        assert r["state"] is None or (st == r["want_state"]).all()
    s = schemes()["three multimaps, half unique"]
    same(run(s, corpus["edge"], None, len(corpus["edge"]["alns"]) + len(corpus["edge"]["chain_off"]) - 1)[0], own(s, corpus["edge"]), "under the sanitizers, edge reads")
    for name, sm, a, refused in malformed():
        rc, want = own(sm, a)
        same(run(sm, a, None, len(a["alns"]) + len(a["chain_off"]) - 1)[0], (rc, want), "under the sanitizers, " + name)
    r = corpus["runs"][0]; room = r["want"][1]["written"]
    assert run(r["scheme"], r["a"], r["state"], room - 1)[0] == (EOPS, dict(written=room))


def test_the_entry_point_is_the_engine_library_s_own():
    engine_h = open(os.path.join(ROOT, "include", "vgk_engine.h")).read(); vgk_h = open(os.path.join(ROOT, "include", "vgk.h")).read()
    lib = ctypes.CDLL(ENGINE)
    for name in ("vgk_pick_mappings", "vgk_pick_mappings_limits", "vgk_pick_mappings_last_ms", "vgk_pick_mappings_last_launches"):
        assert name + "(" in engine_h and name + "(" not in vgk_h and hasattr(lib, name), name
    assert hasattr(pipeline._host_lib(), "vgh_pick_mappings") and hasattr(ctypes.CDLL(DRIVER), "vgt_pick_mappings_serial")
    assert "PARITY-UNPINNED" in engine_h[engine_h.index("a long read's mappings chosen on the device"):engine_h.index("vgk_pick_mappings_limits")]
    assert "2241-2262" in engine_h and "THE WRAP" in engine_h[engine_h.index("a long read's mappings chosen on the device"):]
    out = (ctypes.c_uint32 * 4)()
    assert lib.vgk_pick_mappings_limits(out) == OK and tuple(out) == (LDS_NODES, LDS_SLOTS, LDS_ITEMS, 64)


def test_long_read_mapq_over_the_shim(corpus):
    """pipeline.long_read_mapq with the host shim for both steps: the read's quality on the primary alone, secondaries flagged, the demapping rule applied"""
    r = corpus["runs"][1]; a = r["a"]; n = len(a["chain_off"]) - 1
    args = (r["scheme"], a["reads"], a["read_off"], a["chain_off"], a["chains"], a["aln_off"], a["alns"], (None, a["mappings"], a["edits"]))
    out = pipeline.long_read_mapq(None, *args, log_base=0.4, score_scale=1.0, score_window=0, min_mapq0_score=0)
    want = r["want"][1] if r["state"] is None else own(r["scheme"], a)[1]
    assert (out["pick"]["results"] == want["results"]).all() and not out["demapped"].any()
    res = want["results"]; lo = a["aln_off"].astype(np.int64)
    for q in range(n):
        mine = [int(x) for x in want["picked"][int(res["first"][q]):int(res["first"][q]) + int(res["n_mappings"][q])]]
        assert [int(x) for x in np.nonzero(out["reported"][lo[q]:lo[q + 1]])[0]] == sorted(mine)
        assert [int(x) for x in np.nonzero(out["secondary"][lo[q]:lo[q + 1]])[0]] == sorted(mine[1:])
        if mine:
            assert out["mapq"][lo[q] + mine[0]] == out["read_mapq"][q] and out["mapq"][lo[q]:lo[q + 1]].sum() == out["read_mapq"][q]
    assert (out["read_mapq"][res["unmapped"] == 1] == 0).all() and (out["read_mapq"] > 0).any() and (out["read_mapq"] <= 60).all()
    # a multiplicity of 2^64 weighs the primary down to nothing; a window and a scale change qualities, never the pick
    other = pipeline.long_read_mapq(None, *args, log_base=0.4, score_scale=0.5, score_window=10, min_mapq0_score=0)
    assert (other["pick"]["results"] == out["pick"]["results"]).all() and (other["read_mapq"] != out["read_mapq"]).any()
    # the demapping rule: quality 0 and a top score below the setting -> one unmapped entry of score 0
    hard = pipeline.long_read_mapq(None, *args, log_base=0.4, min_mapq0_score=13)
    top = want["scores"][res["first"]]
    assert (hard["demapped"] == ((out["read_mapq"] == 0) & (top < 13))).all() and hard["demapped"].any() and (hard["demapped"] & (res["unmapped"] == 0)).any()
    at = hard["score_off"].astype(np.int64)
    assert all(at[q + 1] - at[q] == 1 and hard["scores"][at[q]] == 0 and hard["n_mappings"][q] == 1 and not hard["reported"][lo[q]:lo[q + 1]].any() for q in np.nonzero(hard["demapped"])[0])


def launches_of(s, a):
    """(reads picked in LDS, over the slab, refused) as the header says it: a read goes over the slab when it has more alignments than the order's limit or
    when the mapping counts of its max_multimaps largest alignments together pass the table's"""
    slab = 0
    for r in range(len(a["aln_off"]) - 1):
        counts = sorted((int(x) for x in a["alns"]["result"]["n_mappings"][int(a["aln_off"][r]):int(a["aln_off"][r + 1])]), reverse=True)
        slab += len(counts) > LDS_ITEMS or sum(counts[:s.max_multimaps]) > LDS_NODES
    return (len(a["aln_off"]) - 1 - slab, slab, 0)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    return capi.Engine(capi.Scoring.simple(1, 4, 6, 1, 5), lib=ENGINE, device=0)


@pytest.mark.gpu
def test_the_engine_equals_the_shim_in_every_field(corpus, gpu):
    for r in corpus["runs"]:
        want, want_state = both(shim_call, r["scheme"], r["a"], r["state"])
        same_with_states(engine_call(gpu), r["scheme"], r["a"], r["state"], want, want_state, "engine against the shim, " + r["name"])
        same(want, r["want"], "shim, " + r["name"])
        assert gpu.pick_mappings_last_launches() == (len(r["a"]["chain_off"]) - 1, 0, 0)
    assert all(x > 0 for x in gpu.pick_mappings_last_ms())


@pytest.mark.gpu
def test_the_engine_s_launch_edges(corpus, gpu):
    assert gpu.pick_mappings_limits() == (LDS_NODES, LDS_SLOTS, LDS_ITEMS, 64)
    for name, s in schemes().items():
        same(engine_call(gpu)(s, corpus["edge"]), shim_call(s, corpus["edge"]), "edge reads, " + name)
        # beyond the table's limit with one multimap: the read of limit + 1 mappings; with more, whoever's largest alignments together pass it; the 33 alignments always
        assert gpu.pick_mappings_last_launches() == launches_of(s, corpus["edge"]), name
    assert launches_of(schemes()["the defaults"], corpus["edge"]) == (10, 2, 0) and launches_of(s, corpus["edge"])[1] > 2
    s = schemes()["three multimaps, half unique"]
    for n in (1, 64, 65):
        a = build([random_read(np.random.default_rng(100 + k)) for k in range(n)])
        state = states_for(a, n)
        want, want_state = both(shim_call, s, a, state)
        same_with_states(engine_call(gpu), s, a, state, want, want_state, "%d reads" % n)


@pytest.mark.gpu
def test_the_engine_s_sizing(corpus, gpu):
    hold_sizing(engine_call(gpu), corpus["runs"][1], "engine")


@pytest.mark.gpu
def test_the_engine_refuses_malformed_calls_and_takes_an_empty_one(gpu):
    hold_malformed(engine_call(gpu), "engine")
    assert gpu.pick_mappings_last_launches() == (0, 0, 0)


@pytest.mark.gpu
def test_end_to_end_on_the_gpu(gpu):
    """the chain stage's composed alignments of 40 long reads, declared as reads of three alignments each — the alignment, a second result naming the same
    mappings, the alignment of another read —, through pipeline.long_read_mapq on the engine and over the shim; the qualities into GAF"""
    wl = workloads.LongReadWorkload(40, read_len=15000)
    cs = pipeline.ChainStage(wl, lib=ENGINE_LIB)
    o = cs.run(threads=3, compose=True)
    res, maps, runs = (np.array(x) for x in o["alignments"]); chain_score = np.array(o["chain_score"], dtype=np.int64)
    cs.close()
    n = 40
    assert len(res) == n and (res["status"] == OK).all() and (chain_score > 1000).all()
    node_sets = [set(int(x) for x in maps["node"][int(g["mapping_begin"]):int(g["mapping_begin"]) + int(g["n_mappings"])]) for g in res]
    stranger = [next(q % n for q in range(r + 1, r + n) if not node_sets[r] & node_sets[q % n]) for r in range(n)]
    chains = np.zeros(3 * n, dtype=capi.PICK_CHAIN_DT); alns = np.zeros(3 * n, dtype=capi.PICK_ALIGNMENT_DT)
    chains["multiplicity"] = 1.0; chains["range"]["component"] = np.arange(3 * n) % 3; chains["range"]["offset_end"] = 100
    for r in range(n):
        for k, (which, score) in enumerate(((r, chain_score[r]), (r, chain_score[r] - 1), (stranger[r], chain_score[stranger[r]] // 2))):
            alns[3 * r + k] = (k, score, 1, tuple(res[which]))
            chains["score_estimate"][3 * r + k] = score
    whole = wl.whole_reads()
    off = np.arange(0, 3 * n + 1, 3, dtype=np.uint64)
    s = capi.PickScheme.defaults(max_multimaps=3, min_unique_node_fraction=0.5)
    args = (s, whole["reads"], whole["read_off"], off, chains, off, alns, (res, maps, runs))
    state = np.zeros(n, dtype=np.uint32); shim_state = state.copy()
    got = pipeline.long_read_mapq(gpu, *args, log_base=0.4, rng_state=state)
    want = pipeline.long_read_mapq(None, *args, log_base=0.4, rng_state=shim_state)
    same((OK, got["pick"]), (OK, want["pick"]), "end to end: the pick")
    assert got["per_read"].tobytes() == want["per_read"].tobytes() and (got["mapq"] == want["mapq"]).all() and (got["secondary"] == want["secondary"]).all()
    assert (state == shim_state).all() and gpu.pick_mappings_last_launches() == launches_of(s, dict(aln_off=off, alns=alns))
    assert launches_of(s, dict(aln_off=off, alns=alns))[1] > 0                                # (some 500 mappings per alignment: the slab's territory)
    v = got["pick"]["verdicts"]
    assert (v["fate"][0::3] == capi.PICK_MAPPING).all() and (v["fate"][1::3] == capi.PICK_FAIL_UNIQUE).all() and (v["fraction_unique"][1::3] == 0.0).all()
    assert (v["fate"][2::3] == capi.PICK_MAPPING).all() and (got["pick"]["results"]["n_mappings"] == 2).all() and (got["pick"]["results"]["n_scores"] == 2).all()
    assert got["reported"][0::3].all() and got["secondary"][2::3].all() and not got["secondary"][0::3].any() and (got["read_mapq"] > 0).all()
    reads = [bytes(whole["reads"][int(whole["read_off"][r]):int(whole["read_off"][r + 1])]) for r in range(n)]
    node_seq = np.frombuffer("".join(wl.nodes).encode(), dtype=np.uint8); node_off = np.cumsum([0] + [len(x) for x in wl.nodes]).astype(np.uint64)
    lines = pipeline.gaf_lines(whole["reads"], whole["read_off"], res, maps, runs, node_seq, node_off, names=[b"read%d" % r for r in range(n)], mapq=got["mapq"][0::3],
                               score=chain_score.astype(np.int32))
    assert len(reads) == n and all(line.decode().split("\t")[11] == str(int(got["read_mapq"][r])) for r, line in enumerate(lines))
