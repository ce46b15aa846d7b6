"""ctypes binding of the C ABI in include/vgk.h.

Plumbing only: problems are described with numpy arrays (so a million of them
can be assembled without a Python loop) and handed to the shared library as the
plain-pointer structs the header declares.  The default library is the HIP
product (vg_amd/libvgamd.so); loading fails loudly if it has not been built.
"""
import ctypes
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "libvgamd.so")

VGK_OK = 0
VGK_EINVAL, VGK_ENODEV, VGK_ENOMEM, VGK_ETOOLONG, VGK_EOVERFLOW, VGK_EOPS = -1, -2, -3, -4, -5, -6      # include/vgk.h
VGK_ETOOBIG, VGK_ENOBAND, VGK_EUNSUPPORTED = -7, -8, -9
VGK_GSSW_LOCAL = 0
VGK_GSSW_PINNED = 1
VGK_XDROP_PINNED = 2
VGK_GSSW_TRACEBACK = 16
OP_M, OP_I, OP_D, OP_S = 0, 1, 2, 3
OP_CHARS = "MIDS"

# struct layouts (must match include/vgk.h)
GRAPH_DT = np.dtype([("n_nodes", "<u4"), ("_pad", "<u4"), ("node_len", "<u8"), ("seq", "<u8"),
                     ("pred_off", "<u8"), ("pred_idx", "<u8")])
PROBLEM_DT = np.dtype([("read", "<u8"), ("read_len", "<u4"), ("flags", "<u4"), ("graph", GRAPH_DT), ("pinning", "<u8"),
                       ("max_gap_length", "<u4"), ("reserved", "<u4"), ("qual", "<u8")])
RESULT_DT = np.dtype([("score", "<i4"), ("status", "<i4"), ("end_node", "<i4"), ("end_offset", "<i4"),
                      ("end_read", "<i4"), ("first_offset", "<i4"), ("n_ops", "<u4"), ("ops_begin", "<u4")])
OP_DT = np.dtype([("node", "<u4"), ("len", "<u2"), ("op", "u1"), ("pad", "u1")])
WINDOW_DT = np.dtype([("read_off", "<u8"), ("read_len", "<u4"), ("flags", "<u4"), ("first_node", "<u4"), ("n_nodes", "<u4"),
                      ("max_gap_length", "<u4"), ("reserved", "<u4")])
assert WINDOW_DT.itemsize == 32
EXTENSION_DT = np.dtype([("read_off", "<u8"), ("read_len", "<u4"), ("flags", "<u4"), ("first_node", "<u4"), ("n_nodes", "<u4"), ("max_gap_length", "<u4"),
                         ("start_node", "<u4"), ("start_offset", "<u4"), ("query_offset", "<u4"), ("leftward", "<u4"), ("reserved", "<u4")])
assert EXTENSION_DT.itemsize == 48
RESCUE_REQUEST_DT = np.dtype([("mapped", "<u4"), ("lost", "<u4"), ("node_lo", "<u4"), ("node_hi", "<u4"), ("seed_begin", "<i4"), ("seed_end", "<i4"),
                              ("seed_node", "<i4"), ("seed_offset", "<i4"), ("reverse", "<u4"), ("reserved", "<u4")])
assert RESCUE_REQUEST_DT.itemsize == 40
BANDED_DT = np.dtype([("read", "<u8"), ("qual", "<u8"), ("read_len", "<u4"), ("flags", "<u4"), ("graph", GRAPH_DT),
                      ("band_padding", "<i4"), ("reserved", "<u4"), ("max_cells", "<u8")])
VGK_BANDED_PERMISSIVE = 1
SEED_DT = np.dtype([("node", "<u4"), ("diff", "<i4")])
MINIMIZER_HIT_DT = np.dtype([("key", "<u8"), ("node", "<u4"), ("offset", "<u4")])
TAIL_ALIGNMENT_DT = np.dtype([("ext", "<u4"), ("left", "<u4"), ("read_begin", "<u4"), ("read_end", "<u4"), ("score", "<i4"), ("status", "<i4"),
                              ("ops_begin", "<u4"), ("n_ops", "<u4"), ("first_offset", "<u4"), ("n_trees", "<u4")])
GAPLESS_DT = np.dtype([("read", "<u8"), ("read_len", "<u4"), ("n_seeds", "<u4"), ("seeds", "<u8"), ("max_mismatches", "<u4"),
                       ("flags", "<u4"), ("overlap_threshold", "<f8")])
EXT_DT = np.dtype([("path_begin", "<u4"), ("path_len", "<u4"), ("offset", "<u4"), ("read_begin", "<u4"), ("read_end", "<u4"),
                   ("mism_begin", "<u4"), ("n_mismatches", "<u4"), ("score", "<i4"), ("left_full", "u1"), ("right_full", "u1"),
                   ("pad", "u1", 2), ("state", "<u4", 6)])
GAPLESS_RESULT_DT = np.dtype([("status", "<i4"), ("ext_begin", "<u4"), ("n_ext", "<u4"), ("full_length", "<u4")])
VGK_GAPLESS_TRIM = 1
VGK_GAPLESS_DEFER = 2
WFA_DT = np.dtype([("seq", "<u8"), ("seq_len", "<u4"), ("mode", "<u4"), ("from_node", "<u4"), ("from_offset", "<u4"),
                   ("to_node", "<u4"), ("to_offset", "<u4")])
WFA_RESULT_DT = np.dtype([("status", "<i4"), ("ok", "<i4"), ("score", "<i4"), ("node_offset", "<u4"), ("seq_offset", "<u4"),
                          ("length", "<u4"), ("path_begin", "<u4"), ("path_len", "<u4"), ("edit_begin", "<u4"), ("n_edits", "<u4")])
WFA_EVENT_DT = np.dtype([("per_base", "<f8"), ("min", "<i4"), ("max", "<i4")])
WFA_CONNECT, WFA_SUFFIX, WFA_PREFIX = 0, 1, 2
WFA_MATCH, WFA_MISMATCH, WFA_INSERTION, WFA_DELETION = 0, 1, 2, 3
WFA_NO_NODE = 0xffffffff
WFA_DEFAULT_MODEL = ((0.03, 1, 6), (0.05, 1, 10), (0.1, 1, 20), (0.1, 10, 200))      # gbwt_extender.hpp:386-395
READ_MINIMIZER_DT = np.dtype([("key", "<u8"), ("offset", "<u4"), ("hits", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])      # vgk_read_minimizer


class FindSeedsPolicy(ctypes.Structure):       # vgk_find_seeds_policy (include/vgk_engine.h)
    _fields_ = [("hit_cap", ctypes.c_uint32), ("hard_hit_cap", ctypes.c_uint32), ("minimizer_score_fraction", ctypes.c_double),
                ("max_unique_min", ctypes.c_uint32), ("num_bp_per_min", ctypes.c_uint32), ("minimizer_coverage_flank", ctypes.c_uint32), ("exclude_overlapping_min", ctypes.c_uint32),
                ("minimizer_downsampling_window_count", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("minimizer_downsampling_max_window_length", ctypes.c_uint64)]


def find_seeds_policy(P):
    """a policy in the keys of pipeline.GIRAFFE_LONG_READ_POLICY -> FindSeedsPolicy"""
    return FindSeedsPolicy(int(P["hit_cap"]), int(P["hard_hit_cap"]), float(P["score_fraction"]), int(P["max_unique_min"]), int(P["num_bp_per_min"]), int(P["coverage_flank"]),
                           int(bool(P["exclude_overlapping_min"])), int(P["window_count"]), 0, min(int(P["max_window_length"]), (1 << 64) - 1))

# vgk_chain_items (include/vgk_engine.h): anchors, candidate transitions and the chains found
CHAIN_ANCHOR_DT = np.dtype([("read_start", "<u4"), ("length", "<u4"), ("margin_before", "<u4"), ("margin_after", "<u4"), ("score", "<i4"), ("start_hint_offset", "<u4"),
                            ("end_hint_offset", "<u4"), ("base_seed_length", "<u4"), ("start_paths", "<u8"), ("end_paths", "<u8")])
CHAIN_CANDIDATE_DT = np.dtype([("from", "<u4"), ("to", "<u4"), ("graph_distance", "<u4")])
CHAIN_FOUND_DT = np.dtype([("score", "<i4"), ("item_begin", "<u4"), ("n_items", "<u4"), ("rec_begin", "<u4"), ("n_rec", "<u4"), ("n_rec_left", "<u4")])
CHAIN_NOWHERE = 0xffffffff
# ChainScoringScheme's defaults (src/algorithms/chain_items.hpp:407-418), one chain, no read lookback, find_best_chain's indel limit of 100
CHAIN_SCHEME_DEFAULTS = dict(item_bonus=0, recombination_penalty=0, consistency_bonus=0, max_chains=1, gap_scale=1.0, max_read_lookback_bases=0xffffffff, max_indel_bases=100)


class ChainScheme(ctypes.Structure):           # vgk_chain_scheme
    _fields_ = [("item_bonus", ctypes.c_int32), ("recombination_penalty", ctypes.c_int32), ("consistency_bonus", ctypes.c_int32), ("max_chains", ctypes.c_uint32),
                ("gap_scale", ctypes.c_double), ("max_read_lookback_bases", ctypes.c_uint32), ("max_indel_bases", ctypes.c_uint32)]


def chain_scheme(S=None):
    """a scheme in the keys of CHAIN_SCHEME_DEFAULTS (missing ones: the defaults) -> ChainScheme"""
    S = dict(CHAIN_SCHEME_DEFAULTS, **(S or {}))
    return ChainScheme(int(S["item_bonus"]), int(S["recombination_penalty"]), int(S["consistency_bonus"]), int(S["max_chains"]), float(S["gap_scale"]),
                       int(S["max_read_lookback_bases"]), int(S["max_indel_bases"]))


def chain_items_call(fn, head, scheme, anchor_off, anchors, cand_off, candidates, read_lookback=None, indel_limit=None, tail=()):
    """one call with vgk_chain_items' arguments (the engine's, the host shim's vgh_find_best_chains, the serial lane code's): head / tail = what the
    function takes before the scheme / behind table_source -> (rc, dict(chain_off, chains, items, rec_right, rec_left, table_score, table_source))"""
    aoff = np.ascontiguousarray(anchor_off, dtype=np.uint64); coff = np.ascontiguousarray(cand_off, dtype=np.uint64); n = len(aoff) - 1
    anchors = np.ascontiguousarray(anchors, dtype=CHAIN_ANCHOR_DT); candidates = np.ascontiguousarray(candidates, dtype=CHAIN_CANDIDATE_DT)
    sch = scheme if isinstance(scheme, ChainScheme) else chain_scheme(scheme)
    look = None if read_lookback is None else np.ascontiguousarray(read_lookback, dtype=np.uint32); lim = None if indel_limit is None else np.ascontiguousarray(indel_limit, dtype=np.uint32)
    sizes = np.diff(aoff.astype(np.int64)) if n else np.zeros(0, dtype=np.int64)
    room = int(np.maximum(1, np.minimum(sizes, sch.max_chains)).sum()) if n else 0
    out = dict(chain_off=np.zeros(n + 1, dtype=np.uint64), chains=np.zeros(max(room, 1), dtype=CHAIN_FOUND_DT))
    for name in ("items", "rec_right", "rec_left", "table_source"):
        out[name] = np.zeros(max(len(anchors), 1), dtype=np.uint32)
    out["table_score"] = np.zeros(max(len(anchors), 1), dtype=np.int32)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * len(head) + [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 13 + [type(t) for t in tail]
    rc = fn(*head, ctypes.byref(sch), n, aoff.ctypes.data, anchors.ctypes.data if len(anchors) else None, coff.ctypes.data, candidates.ctypes.data if len(candidates) else None,
            None if look is None else look.ctypes.data, None if lim is None else lim.ctypes.data, out["chain_off"].ctypes.data, out["chains"].ctypes.data,
            out["items"].ctypes.data, out["rec_right"].ctypes.data, out["rec_left"].ctypes.data, out["table_score"].ctypes.data, out["table_source"].ctypes.data, *tail)
    if rc == VGK_OK:
        out["chains"] = out["chains"][:int(out["chain_off"][-1])]
        for name in ("items", "rec_right", "rec_left", "table_source", "table_score"):
            out[name] = out[name][:len(anchors)]
    return rc, out


# vgk_extension_anchors (include/vgk_engine.h): seeds in, chaining anchors and where they come from out
ANCHOR_SEED_DT = np.dtype([("node", "<u4"), ("diff", "<i4"), ("stapled", "<u4"), ("length", "<u2"), ("is_reverse", "<u2"), ("paths", "<u8")])
ANCHOR_ORIGIN_DT = np.dtype([("seed_first", "<u4"), ("seed_last", "<u4"), ("n_seq", "<u4"), ("rep_begin", "<u4"), ("n_rep", "<u4"), ("extension", "<u4"),
                             ("read_begin", "<u4"), ("read_end", "<u4")])
assert ANCHOR_SEED_DT.itemsize == 24 and ANCHOR_ORIGIN_DT.itemsize == 32
VGK_ANCHORS_FROM_SEEDS = 1
VGK_ANCHORS_FULL_LENGTH = 1
ANCHORS_NO_EXTENSION = 0xffffffff


def extension_anchors_call(fn, head, match, mismatch, flags, max_mismatches, seed_off, seeds, ext_off=None, extensions=None, full_length=None, nodes=None, mismatches=None,
                           tail=(), caps=None):
    """one call with vgk_extension_anchors' arguments (the engine's, the host shim's vgh_extension_anchors, the serial lane code's): head / tail = ctypes
    values the function takes before `match` / behind `written`.  caps = (anchors, represented): the room offered (default: the call's bounds, so one call
    does) -> (rc, dict(anchor_off, anchors, origins, rep_off, represented, status, written))"""
    soff = np.ascontiguousarray(seed_off, dtype=np.uint64); n = len(soff) - 1
    seeds = np.ascontiguousarray(seeds, dtype=ANCHOR_SEED_DT)
    eoff = None if ext_off is None else np.ascontiguousarray(ext_off, dtype=np.uint64)
    ext = None if extensions is None else np.ascontiguousarray(extensions, dtype=EXT_DT)
    full = None if full_length is None else np.ascontiguousarray(full_length, dtype=np.uint32)
    nod = np.zeros(0, dtype=np.uint32) if nodes is None else np.ascontiguousarray(nodes, dtype=np.uint32)
    mis = np.zeros(0, dtype=np.uint32) if mismatches is None else np.ascontiguousarray(mismatches, dtype=np.uint32)
    cap_a, cap_r = caps if caps is not None else (len(seeds), len(seeds) + (0 if ext is None else len(ext)))
    out = dict(anchor_off=np.zeros(n + 1, dtype=np.uint64), rep_off=np.zeros(n + 1, dtype=np.uint64), status=np.zeros(max(n, 1), dtype=np.uint32),
               anchors=np.zeros(max(cap_a, 1), dtype=CHAIN_ANCHOR_DT), origins=np.zeros(max(cap_a, 1), dtype=ANCHOR_ORIGIN_DT), represented=np.zeros(max(cap_r, 1), dtype=np.uint32))
    written = (ctypes.c_size_t * 2)()
    ptr = lambda a: None if a is None or not len(a) else a.ctypes.data
    fn.restype = ctypes.c_int
    fn.argtypes = [type(t) for t in head] + [ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t] \
        + [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p] + [type(t) for t in tail]
    rc = fn(*head, int(match), int(mismatch), int(flags), int(max_mismatches), n, soff.ctypes.data, ptr(seeds), None if eoff is None else eoff.ctypes.data, ptr(ext), ptr(full),
            ptr(nod), len(nod), ptr(mis), len(mis), out["anchor_off"].ctypes.data, out["anchors"].ctypes.data, out["origins"].ctypes.data, cap_a,
            out["rep_off"].ctypes.data, out["represented"].ctypes.data, cap_r, out["status"].ctypes.data, written, *tail)
    out["written"] = (int(written[0]), int(written[1]))
    out["status"] = out["status"][:n]
    if rc == VGK_OK:
        out["anchors"] = out["anchors"][:out["written"][0]]; out["origins"] = out["origins"][:out["written"][0]]; out["represented"] = out["represented"][:out["written"][1]]
    return rc, out


# vgk_read_alignments (include/vgk_engine.h): extension sets and their tails' alignments in, giraffe's alignments per read out
READ_ALIGNMENT_DT = np.dtype([("status", "<i4"), ("mapping_begin", "<u4"), ("n_mappings", "<u4"), ("edit_begin", "<u4"), ("n_edits", "<u4"), ("from_length", "<u4"),
                              ("to_length", "<u4"), ("read", "<u4"), ("kind", "<u4"), ("extension", "<u4"), ("score", "<i4"), ("identity_num", "<u4"),
                              ("identity_den", "<u4"), ("reserved", "<u4")])
assert READ_ALIGNMENT_DT.itemsize == 56
READ_ALN_DIRECT, READ_ALN_BEST, READ_ALN_SECOND = 0, 1, 2
READ_ALN_NO_EXTENSION = 0xffffffff


class ReadAlignmentsPolicy(ctypes.Structure):   # vgk_read_alignments_policy
    _fields_ = [("extension_score_threshold", ctypes.c_uint32), ("max_local_extensions", ctypes.c_uint32), ("window_length", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


def read_alignments_call(fn, head, reads, read_off, results, extensions, nodes, mismatches, tails=None, ops=None, extension_score_threshold=1,
                         max_local_extensions=0xffffffff, window_length=39, caps=None, policy_flags=0, tail=()):
    """one call with vgk_read_alignments' arguments (the engine's, the host shim's vgh_read_alignments, the serial lane code's): head / tail = the ctypes
    values the function takes before `policy` / behind `written`.  caps = (alignments, mappings, edit runs): the room offered; None: sized by a first call with no room, as a C caller would
    -> (rc, dict(aln_off, alignments READ_ALIGNMENT_DT, mappings CHAIN_MAPPING_DT, edits, written))"""
    reads = np.ascontiguousarray(reads, dtype=np.uint8); off = np.ascontiguousarray(read_off, dtype=np.uint64); n = len(off) - 1
    res = np.ascontiguousarray(results, dtype=GAPLESS_RESULT_DT); ext = np.ascontiguousarray(extensions, dtype=EXT_DT)
    nod = np.ascontiguousarray(nodes, dtype=np.uint32); mis = np.ascontiguousarray(mismatches, dtype=np.uint32)
    tl = np.zeros(0, dtype=TAIL_ALIGNMENT_DT) if tails is None else np.ascontiguousarray(tails, dtype=TAIL_ALIGNMENT_DT)
    op = np.zeros(0, dtype=OP_DT) if ops is None else np.ascontiguousarray(ops, dtype=OP_DT)
    policy = ReadAlignmentsPolicy(int(extension_score_threshold), int(max_local_extensions), int(window_length), int(policy_flags))
    ptr = lambda a: a.ctypes.data if len(a) else None
    fn.restype = ctypes.c_int
    fn.argtypes = [type(t) for t in head] + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p] + [ctypes.c_void_p, ctypes.c_size_t] * 5 \
        + [ctypes.c_void_p] + [ctypes.c_void_p, ctypes.c_size_t] * 3 + [ctypes.c_void_p] + [type(t) for t in tail]
    written = (ctypes.c_size_t * 3)()
    aln_off = np.zeros(n + 1, dtype=np.uint64)
    rooms = [caps] if caps is not None else [(0, 0, 0), None]
    for room in rooms:
        cap = room if room is not None else tuple(int(x) for x in written)
        aln = np.zeros(max(cap[0], 1), dtype=READ_ALIGNMENT_DT); maps = np.zeros(max(cap[1], 1), dtype=CHAIN_MAPPING_DT); edits = np.zeros(max(cap[2], 1), dtype=np.uint32)
        rc = fn(*head, ctypes.byref(policy), ptr(reads), off.ctypes.data, n, ptr(res), ptr(ext), len(ext), ptr(nod), len(nod), ptr(mis), len(mis), ptr(tl), len(tl),
                ptr(op), len(op), aln_off.ctypes.data, aln.ctypes.data, cap[0], maps.ctypes.data, cap[1], edits.ctypes.data, cap[2], written, *tail)
        if rc != VGK_EOPS:
            break
    w = tuple(int(x) for x in written)
    out = dict(aln_off=aln_off, alignments=aln, mappings=maps, edits=edits, written=w)
    if rc == VGK_OK:
        out.update(alignments=aln[:w[0]], mappings=maps[:w[1]], edits=edits[:w[2]])
    return rc, out


# vgk_minimizer_regions / vgk_read_mapq (include/vgk_engine.h): a read's mapping quality from its alignments' scores and its explored minimizers
MINIMIZER_REGION_DT = np.dtype([("start", "<u4"), ("length", "<u4")])
READ_MAPQ_RESULT_DT = np.dtype([("mapq", "<i4"), ("status", "<i4"), ("uncapped", "<f8"), ("explored_cap", "<f8")])
assert MINIMIZER_REGION_DT.itemsize == 8 and READ_MAPQ_RESULT_DT.itemsize == 24
READ_MAPQ_FIRST, READ_MAPQ_NO_EXPLORED_CAP, READ_MAPQ_OWN_LENGTH = 1, 2, 4
INT32_MAX = 0x7fffffff


class ReadMapqScheme(ctypes.Structure):         # vgk_read_mapq_scheme
    _fields_ = [("log_base", ctypes.c_double), ("score_scale", ctypes.c_double), ("score_window", ctypes.c_uint32), ("k", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


def minimizer_regions_call(fn, head, k, w, read_off, minimizer_off, minimizers, between=(), tail=()):
    """one call with vgk_minimizer_regions' arguments (the engine's, the serial lane code's, the host shim's vgh_minimizer_regions): head / between / tail =
    the ctypes values the function takes before `k` / behind `w` (the shim: the reads) / behind `regions` -> (rc, regions MINIMIZER_REGION_DT)"""
    off = np.ascontiguousarray(read_off, dtype=np.uint64); moff = np.ascontiguousarray(minimizer_off, dtype=np.uint64); n = len(off) - 1
    recs = np.ascontiguousarray(minimizers, dtype=READ_MINIMIZER_DT)
    regions = np.zeros(max(len(recs), 1), dtype=MINIMIZER_REGION_DT)
    fn.restype = ctypes.c_int
    fn.argtypes = [type(t) for t in head] + [ctypes.c_uint32, ctypes.c_uint32] + [type(t) for t in between] + [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p] \
        + [type(t) for t in tail]
    rc = fn(*head, int(k), int(w), *between, off.ctypes.data, n, moff.ctypes.data, recs.ctypes.data if len(recs) else None, regions.ctypes.data, *tail)
    return rc, regions[:len(recs)]


def read_mapq_call(fn, head, scheme, score_off, scores, minimizer_off, minimizers, regions, explored, read_off, quality=None, multiplicity=None, unmapped=None, tail=()):
    """one call with vgk_read_mapq's arguments (the engine's, the host shim's vgh_read_mapq, the serial lane code's): head / tail = the ctypes values the
    function takes before `scheme` / behind `out`.  scheme: a ReadMapqScheme -> (rc, results READ_MAPQ_RESULT_DT)"""
    soff = np.ascontiguousarray(score_off, dtype=np.uint64); moff = np.ascontiguousarray(minimizer_off, dtype=np.uint64); off = np.ascontiguousarray(read_off, dtype=np.uint64)
    n = len(off) - 1
    sc = np.ascontiguousarray(scores, dtype=np.int32); recs = np.ascontiguousarray(minimizers, dtype=READ_MINIMIZER_DT); reg = np.ascontiguousarray(regions, dtype=MINIMIZER_REGION_DT)
    ex = np.ascontiguousarray(explored, dtype=np.uint8)
    assert len(reg) == len(recs) == len(ex) and len(soff) == len(moff) == n + 1
    q = None if quality is None else np.ascontiguousarray(quality, dtype=np.uint8)
    mult = None if multiplicity is None else np.ascontiguousarray(multiplicity, dtype=np.float64)
    un = None if unmapped is None else np.ascontiguousarray(unmapped, dtype=np.uint8)
    out = np.zeros(max(n, 1), dtype=READ_MAPQ_RESULT_DT)
    if q is not None and not len(q):
        q = np.zeros(1, dtype=np.uint8)                               # (given, though no read has a base: still "with qualities")
    ptr = lambda a: a.ctypes.data if a is not None and len(a) else None
    fn.restype = ctypes.c_int
    fn.argtypes = [type(t) for t in head] + [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 11 + [type(t) for t in tail]
    rc = fn(*head, ctypes.byref(scheme), n, soff.ctypes.data, ptr(sc), ptr(mult), ptr(un), moff.ctypes.data, ptr(recs), ptr(reg), ptr(ex), off.ctypes.data,
            ptr(q), out.ctypes.data, *tail)
    return rc, out[:n]


# vgk_funnel_clusters / vgk_funnel_extension_sets / vgk_funnel_winners (include/vgk_engine.h): a short read's funnel between the stages
FUNNEL_CLUSTER_DT = np.dtype([("score", "<f8"), ("coverage", "<f8"), ("covered", "<u4"), ("rank", "<u4"), ("better_or_equal", "<u4"), ("verdict", "<u4")])
FUNNEL_SET_DT = np.dtype([("estimate", "<i4"), ("rank", "<u4"), ("better_or_equal", "<u4"), ("verdict", "<u4")])
FUNNEL_PICK_DT = np.dtype([("set", "<u4"), ("alignment", "<u4")])
assert FUNNEL_CLUSTER_DT.itemsize == 32 and FUNNEL_SET_DT.itemsize == 16 and FUNNEL_PICK_DT.itemsize == 8
FUNNEL_OWN_LENGTH = 1
FUNNEL_UNDECIDED, FUNNEL_EXTEND, FUNNEL_FAIL_COVERAGE, FUNNEL_FAIL_SCORE, FUNNEL_FAIL_MAX_EXTENSIONS = 0, 1, 2, 3, 4
FUNNEL_SET_ALIGN, FUNNEL_SET_FAIL_SCORE, FUNNEL_SET_FAIL_MIN_SCORE, FUNNEL_SET_FAIL_MAX_ALIGNMENTS, FUNNEL_SET_FAILED = 1, 2, 3, 4, 5
FUNNEL_NONE = 0xffffffff


class FunnelPolicy(ctypes.Structure):           # vgk_funnel_policy; the defaults are giraffe's
    _fields_ = [("cluster_score_threshold", ctypes.c_double), ("pad_cluster_score_threshold", ctypes.c_double), ("cluster_coverage_threshold", ctypes.c_double),
                ("extension_set_score_threshold", ctypes.c_double), ("extension_set_min_score", ctypes.c_int32), ("min_extensions", ctypes.c_uint32),
                ("max_extensions", ctypes.c_uint32), ("min_extension_sets", ctypes.c_uint32), ("max_alignments", ctypes.c_uint32), ("max_multimaps", ctypes.c_uint32),
                ("k", ctypes.c_uint32), ("flags", ctypes.c_uint32)]

    @classmethod
    def giraffe(cls, k, flags=0, **changed):
        p = cls(50.0, 20.0, 0.3, 20.0, 20, 2, 800, 2, 8, 1, int(k), int(flags))
        for name, value in changed.items():
            assert hasattr(p, name), name
            setattr(p, name, value)
        return p


assert ctypes.sizeof(FunnelPolicy) == 64


def _funnel_ptr(a):
    return a.ctypes.data if a is not None and len(a) else None


def _funnel_sized(call, state, cap):
    """a funnel call at capacity `cap`, or (None) sized first with capacity 0 over a copy of the generator states -> (rc, written, rc of the sizing call)"""
    if cap is not None:
        rc, written = call(int(cap), state)
        return rc, written, None
    rc0, written = call(0, None if state is None else state.copy())
    if rc0 not in (VGK_OK, VGK_EOPS):
        return rc0, written, rc0
    rc, again = call(written, state)
    assert rc != VGK_OK or again == written
    return rc, again, rc0


# vgk_chain_links (include/vgk_engine.h): a chain's links — what find_chain_alignment's walk decides to align, and how
CHAIN_SITE_DT = np.dtype([("start_node", "<u4"), ("start_offset", "<u4"), ("end_node", "<u4"), ("end_offset", "<u4"), ("flags", "<u4")])
CHAIN_PROBLEM_DT = np.dtype([("read", "<u4"), ("anchor_set", "<u4"), ("item_begin", "<u4"), ("n_items", "<u4")])
CHAIN_LINKS_RESULT_DT = np.dtype([("status", "<i4"), ("flags", "<u4"), ("link_begin", "<u4"), ("n_links", "<u4"), ("kept_begin", "<u4"), ("n_kept", "<u4"),
                                  ("left_tail_length", "<u4"), ("longest_attempted_connection", "<u4"), ("anchor_score", "<i8"), ("seq_begin", "<u8")])
CHAIN_LINK_DT = np.dtype([("mode", "<u4"), ("route", "<u4"), ("from_node", "<u4"), ("from_offset", "<u4"), ("to_node", "<u4"), ("to_offset", "<u4"), ("read_begin", "<u4"),
                          ("length", "<u4"), ("graph_distance", "<u4"), ("chain", "<u4")])
assert CHAIN_SITE_DT.itemsize == 20 and CHAIN_PROBLEM_DT.itemsize == 16 and CHAIN_LINKS_RESULT_DT.itemsize == 48 and CHAIN_LINK_DT.itemsize == 40
CHAIN_ROUTE_WFA, CHAIN_ROUTE_DP, CHAIN_ROUTE_EMPTY, CHAIN_ROUTE_SOFTCLIP = 0, 1, 2, 3
CHAIN_SITE_SKIPPABLE = 1
CHAIN_LINKS_CUT = 1


class ChainLinksScheme(ctypes.Structure):       # vgk_chain_links_scheme; the defaults are MinimizerMapper's
    _fields_ = [("max_chain_connection", ctypes.c_uint64), ("max_tail_length", ctypes.c_uint64), ("max_middle_dp_length", ctypes.c_uint64), ("max_tail_dp_length", ctypes.c_uint64),
                ("max_dp_cells", ctypes.c_uint64), ("max_skipped_bases", ctypes.c_uint64), ("min_indel_avoid_bases", ctypes.c_uint64), ("match", ctypes.c_int32),
                ("full_length_bonus", ctypes.c_int32)]

    @classmethod
    def defaults(cls, **changed):
        p = cls(100, 100, 2 ** 31 - 1, 30000, 2 ** 64 - 1, 0, 0, 1, 5)
        for name, value in changed.items():
            assert hasattr(p, name), name
            setattr(p, name, value)
        return p

    @classmethod
    def hifi(cls, **changed):
        """giraffe's hifi preset where it differs from the defaults"""
        return cls.defaults(**dict(dict(max_chain_connection=233, max_tail_length=68, max_dp_cells=8000000000, min_indel_avoid_bases=50, max_skipped_bases=1000), **changed))


assert ctypes.sizeof(ChainLinksScheme) == 64


def chain_links_call(fn, head, scheme, reads, read_off, anchor_off, anchors, sites, items, dist_off, dist, chains, tail=(), caps=None, want_seqs=True):
    """one call with vgk_chain_links' arguments (the engine's, the host shim's vgh_chain_links, the serial driver's): head / tail = the ctypes values the
    function takes before `scheme` / behind `written`.  caps None: the bounds the header names (links: sum of n_items + 1, kept: sum of n_items, seqs:
    sum of the chains' reads' lengths); otherwise (link_cap, kept_cap, seq_cap)
    -> (rc, dict(results CHAIN_LINKS_RESULT_DT, links CHAIN_LINK_DT, kept, seq_off, seqs, written))"""
    off = np.ascontiguousarray(read_off, dtype=np.uint64); aoff = np.ascontiguousarray(anchor_off, dtype=np.uint64); doff = np.ascontiguousarray(dist_off, dtype=np.uint64)
    rd = np.ascontiguousarray(reads, dtype=np.uint8); anc = np.ascontiguousarray(anchors, dtype=CHAIN_ANCHOR_DT); st = np.ascontiguousarray(sites, dtype=CHAIN_SITE_DT)
    it = np.ascontiguousarray(items, dtype=np.uint32); ds = np.ascontiguousarray(dist, dtype=CHAIN_CANDIDATE_DT); ch = np.ascontiguousarray(chains, dtype=CHAIN_PROBLEM_DT)
    n_reads, n_sets, n = len(off) - 1, len(aoff) - 1, len(ch)
    assert len(doff) == len(aoff) and len(st) == len(anc)
    if caps is None:
        lens = np.diff(off.astype(np.int64))
        ok = ch["read"] < n_reads
        caps = (int(ch["n_items"].astype(np.int64).sum()) + n, int(ch["n_items"].astype(np.int64).sum()), int(lens[ch["read"][ok]].sum()) if n_reads else 0)
    link_cap, kept_cap, seq_cap = (int(c) for c in caps)
    results = np.zeros(max(n, 1), dtype=CHAIN_LINKS_RESULT_DT); links = np.zeros(max(link_cap, 1), dtype=CHAIN_LINK_DT); kept = np.zeros(max(kept_cap, 1), dtype=np.uint32)
    seq_off = np.zeros(link_cap + 1, dtype=np.uint64); seqs = np.zeros(max(seq_cap, 1), dtype=np.uint8); written = (ctypes.c_size_t * 3)()
    fn.restype = ctypes.c_int
    fn.argtypes = [type(t) for t in head] + [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 4 + [ctypes.c_size_t] + \
                  [ctypes.c_void_p] * 2 + [ctypes.c_uint32] + [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                                                      ctypes.c_void_p] + [type(t) for t in tail]
    rc = fn(*head, ctypes.byref(scheme), n_reads, _funnel_ptr(rd), off.ctypes.data, n_sets, aoff.ctypes.data, _funnel_ptr(anc), _funnel_ptr(st), _funnel_ptr(it), len(it),
            doff.ctypes.data, _funnel_ptr(ds), n, _funnel_ptr(ch), results.ctypes.data, links.ctypes.data if link_cap else None, link_cap, kept.ctypes.data if kept_cap else None, kept_cap,
            seqs.ctypes.data if want_seqs else None, seq_off.ctypes.data if want_seqs else None, seq_cap, written, *tail)
    w = tuple(int(x) for x in written)
    if rc != VGK_OK:
        return rc, dict(results=results[:n], written=w)
    return rc, dict(results=results[:n], links=links[:w[0]], kept=kept[:w[1]], seq_off=seq_off[:w[0] + 1] if want_seqs else None, seqs=seqs[:w[2]] if want_seqs else None, written=w)


def funnel_clusters_call(fn, head, policy, reads, read_off, minimizer_off, minimizers, minimizer_score, cluster_off, cluster_seed_off, sources, rng_state=None, tail=(), cap=None):
    """one call with vgk_funnel_clusters' arguments (the engine's, the host shim's vgh_funnel_clusters, the serial lane code's): head / tail = the ctypes values
    the function takes before `policy` / behind `written`.  rng_state: uint32 per read, updated in place.  cap None: sized with a first call
    -> (rc, dict(clusters FUNNEL_CLUSTER_DT, status, kept_off, kept, written, sizing_rc))"""
    off = np.ascontiguousarray(read_off, dtype=np.uint64); moff = np.ascontiguousarray(minimizer_off, dtype=np.uint64); coff = np.ascontiguousarray(cluster_off, dtype=np.uint64)
    soff = np.ascontiguousarray(cluster_seed_off, dtype=np.uint64); n = len(off) - 1
    rd = None if reads is None else np.ascontiguousarray(reads, dtype=np.uint8); recs = np.ascontiguousarray(minimizers, dtype=READ_MINIMIZER_DT)
    ms = np.ascontiguousarray(minimizer_score, dtype=np.float64); src = np.ascontiguousarray(sources, dtype=np.uint32)
    assert rng_state is None or (rng_state.dtype == np.uint32 and len(rng_state) >= n and rng_state.flags.c_contiguous)
    clusters = np.zeros(max(len(soff) - 1, 1), dtype=FUNNEL_CLUSTER_DT); status = np.zeros(max(n, 1), dtype=np.int32); kept_off = np.zeros(n + 1, dtype=np.uint64)
    box = {}
    fn.restype = ctypes.c_int
    fn.argtypes = [type(t) for t in head] + [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 13 + [ctypes.c_size_t, ctypes.c_void_p] + [type(t) for t in tail]

    def call(c, state):
        kept = np.zeros(max(c, 1), dtype=np.uint32); written = (ctypes.c_size_t * 1)()
        rc = fn(*head, ctypes.byref(policy), n, _funnel_ptr(rd), off.ctypes.data, moff.ctypes.data, _funnel_ptr(recs), _funnel_ptr(ms), coff.ctypes.data, soff.ctypes.data,
                _funnel_ptr(src), None if state is None else state.ctypes.data, clusters.ctypes.data, status.ctypes.data, kept_off.ctypes.data, kept.ctypes.data if c else None, c, written, *tail)
        box["kept"] = kept[:c]
        return rc, int(written[0])
    rc, written, rc0 = _funnel_sized(call, rng_state, cap)
    return rc, dict(clusters=clusters[:len(soff) - 1], status=status[:n], kept_off=kept_off, kept=box["kept"][:written] if rc == VGK_OK else box["kept"], written=written, sizing_rc=rc0)


def funnel_extension_sets_call(fn, head, policy, reads, read_off, set_off, results, extensions, kept_off, kept, cluster_seed_off, sources, minimizer_off, rng_state=None,
                               between=(), tail=(), cap=None):
    """one call with vgk_funnel_extension_sets' arguments; between = what the function takes behind `policy` (the shim and the serial code: gap open, gap extend)
    -> (rc, dict(sets FUNNEL_SET_DT, status, aligned_off, aligned, explored, written, sizing_rc))"""
    off = np.ascontiguousarray(read_off, dtype=np.uint64); toff = np.ascontiguousarray(set_off, dtype=np.uint64); koff = np.ascontiguousarray(kept_off, dtype=np.uint64)
    soff = np.ascontiguousarray(cluster_seed_off, dtype=np.uint64); moff = np.ascontiguousarray(minimizer_off, dtype=np.uint64); n = len(off) - 1
    rd = None if reads is None else np.ascontiguousarray(reads, dtype=np.uint8); res = np.ascontiguousarray(results, dtype=GAPLESS_RESULT_DT)
    ext = np.ascontiguousarray(extensions, dtype=EXT_DT); kp = np.ascontiguousarray(kept, dtype=np.uint32); src = np.ascontiguousarray(sources, dtype=np.uint32)
    assert rng_state is None or (rng_state.dtype == np.uint32 and len(rng_state) >= n and rng_state.flags.c_contiguous)
    sets = np.zeros(max(len(res), 1), dtype=FUNNEL_SET_DT); status = np.zeros(max(n, 1), dtype=np.int32); aligned_off = np.zeros(n + 1, dtype=np.uint64)
    explored = np.zeros(max(int(moff[-1]), 1), dtype=np.uint8)
    box = {}
    fn.restype = ctypes.c_int
    fn.argtypes = [type(t) for t in head] + [ctypes.c_void_p] + [type(t) for t in between] + [ctypes.c_uint32] + [ctypes.c_void_p] * 5 + [ctypes.c_size_t] + [ctypes.c_void_p] * 3 \
        + [ctypes.c_size_t] + [ctypes.c_void_p] * 7 + [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p] + [type(t) for t in tail]

    def call(c, state):
        aligned = np.zeros(max(c, 1), dtype=np.uint32); written = (ctypes.c_size_t * 1)()
        rc = fn(*head, ctypes.byref(policy), *between, n, _funnel_ptr(rd), off.ctypes.data, toff.ctypes.data, _funnel_ptr(res), _funnel_ptr(ext), len(ext), koff.ctypes.data, _funnel_ptr(kp),
                soff.ctypes.data, len(soff) - 1, _funnel_ptr(src), moff.ctypes.data, None if state is None else state.ctypes.data, sets.ctypes.data, status.ctypes.data,
                aligned_off.ctypes.data, aligned.ctypes.data if c else None, c, explored.ctypes.data, written, *tail)
        box["aligned"] = aligned[:c]
        return rc, int(written[0])
    rc, written, rc0 = _funnel_sized(call, rng_state, cap)
    return rc, dict(sets=sets[:len(res)], status=status[:n], aligned_off=aligned_off, aligned=box["aligned"][:written] if rc == VGK_OK else box["aligned"],
                    explored=explored[:int(moff[-1])], written=written, sizing_rc=rc0)


def funnel_winners_call(fn, head, policy, reads, read_off, aligned_off, aln_off, aln_score, aln_mappings, rng_state=None, tail=(), cap=None):
    """one call with vgk_funnel_winners' arguments -> (rc, dict(score_off, scores, reported FUNNEL_PICK_DT, n_reported, unmapped, written, sizing_rc))"""
    off = np.ascontiguousarray(read_off, dtype=np.uint64); aoff = np.ascontiguousarray(aligned_off, dtype=np.uint64); loff = np.ascontiguousarray(aln_off, dtype=np.uint64)
    n = len(off) - 1
    rd = None if reads is None else np.ascontiguousarray(reads, dtype=np.uint8); sc = np.ascontiguousarray(aln_score, dtype=np.int32); mp = np.ascontiguousarray(aln_mappings, dtype=np.uint32)
    assert rng_state is None or (rng_state.dtype == np.uint32 and len(rng_state) >= n and rng_state.flags.c_contiguous)
    score_off = np.zeros(n + 1, dtype=np.uint64); n_reported = np.zeros(max(n, 1), dtype=np.uint32); unmapped = np.zeros(max(n, 1), dtype=np.uint8)
    box = {}
    fn.restype = ctypes.c_int
    fn.argtypes = [type(t) for t in head] + [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 10 + [ctypes.c_size_t] + [ctypes.c_void_p] * 3 + [type(t) for t in tail]

    def call(c, state):
        scores = np.zeros(max(c, 1), dtype=np.int32); reported = np.zeros(max(c, 1), dtype=FUNNEL_PICK_DT); written = (ctypes.c_size_t * 1)()
        rc = fn(*head, ctypes.byref(policy), n, _funnel_ptr(rd), off.ctypes.data, aoff.ctypes.data, loff.ctypes.data, _funnel_ptr(sc), _funnel_ptr(mp),
                None if state is None else state.ctypes.data, score_off.ctypes.data, scores.ctypes.data if c else None, reported.ctypes.data if c else None, c,
                n_reported.ctypes.data, unmapped.ctypes.data, written, *tail)
        box["scores"] = scores[:c]; box["reported"] = reported[:c]
        return rc, int(written[0])
    rc, written, rc0 = _funnel_sized(call, rng_state, cap)
    keep = written if rc == VGK_OK else len(box["scores"])
    return rc, dict(score_off=score_off, scores=box["scores"][:keep], reported=box["reported"][:keep], n_reported=n_reported[:n], unmapped=unmapped[:n], written=written, sizing_rc=rc0)


# vgk_pair_mapq (include/vgk_engine.h): a pair's mapping qualities from its candidate pairings and its mates' explored caps
PAIR_CANDIDATE_DT = np.dtype([("score", "<i4", (2,)), ("distance", "<i8"), ("aln", "<u4", (2,)), ("better_cluster_count", "<u4"), ("type", "u1"), ("aligned", "u1"), ("reserved", "<u2")])
PAIR_COUNTS_DT = np.dtype([("unpaired_count", "<u4", (2,)), ("rescued_count", "<u4", (2,))])
PAIR_MAPQ_RESULT_DT = np.dtype([("mapq", "<i4", (2,)), ("status", "<i4"), ("n_chosen", "<u4"), ("uncapped", "<f8"), ("fragment_cluster_cap", "<f8"), ("explored_cap", "<f8", (2,)),
                                ("score_group", "<f8", (2,)), ("applied_cap", "<f8", (2,))])
assert PAIR_CANDIDATE_DT.itemsize == 32 and PAIR_COUNTS_DT.itemsize == 16 and PAIR_MAPQ_RESULT_DT.itemsize == 80
PAIR_PAIRED, PAIR_UNPAIRED, PAIR_RESCUED_FROM_FIRST, PAIR_RESCUED_FROM_SECOND = 0, 1, 2, 3
PAIR_MAPQ_NO_EXPLORED_CAP = 1
INT64_MAX = 0x7fffffffffffffff


class PairMapqScheme(ctypes.Structure):         # vgk_pair_mapq_scheme
    _fields_ = [("log_base", ctypes.c_double), ("fragment_mean", ctypes.c_double), ("fragment_sd", ctypes.c_double), ("max_multimaps", ctypes.c_uint32),
                ("max_rescue_attempts", ctypes.c_uint32), ("k", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


def pair_mapq_call(fn, head, scheme, cand_off, candidates, counts, unpaired_off=None, unpaired_scores=None, given_cap=None, minimizer_off=None, minimizers=None, regions=None,
                   explored=None, read_off=None, quality=None, tail=()):
    """one call with vgk_pair_mapq's arguments (the engine's, the host shim's vgh_pair_mapq, the serial lane code's): head / tail = the ctypes values the
    function takes before `scheme` / behind `order`.  scheme: a PairMapqScheme -> (rc, results PAIR_MAPQ_RESULT_DT, pair_score float64 per candidate, order
    uint32 per candidate)"""
    coff = np.ascontiguousarray(cand_off, dtype=np.uint64); n = len(coff) - 1
    cands = np.ascontiguousarray(candidates, dtype=PAIR_CANDIDATE_DT); cnt = np.ascontiguousarray(counts, dtype=PAIR_COUNTS_DT)
    assert len(cnt) == n and int(coff[-1]) == len(cands)
    opt = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)
    uoff, usc, caps = opt(unpaired_off, np.uint64), opt(unpaired_scores, np.int32), opt(given_cap, np.float64)
    moff, recs, reg, ex = opt(minimizer_off, np.uint64), opt(minimizers, READ_MINIMIZER_DT), opt(regions, MINIMIZER_REGION_DT), opt(explored, np.uint8)
    off, q = opt(read_off, np.uint64), opt(quality, np.uint8)
    assert (uoff is None or len(uoff) == 2 * n + 1) and (caps is None or len(caps) == 2 * n) and (moff is None or len(moff) == 2 * n + 1) and (off is None or len(off) == 2 * n + 1)
    if usc is not None and not len(usc):
        usc = np.zeros(1, dtype=np.int32)                             # (given, though no mate has one)
    if q is not None and not len(q):
        q = np.zeros(1, dtype=np.uint8)
    out = np.zeros(max(n, 1), dtype=PAIR_MAPQ_RESULT_DT); pair_score = np.zeros(max(len(cands), 1), dtype=np.float64); order = np.zeros(max(len(cands), 1), dtype=np.uint32)
    ptr = lambda a: a.ctypes.data if a is not None and len(a) else None
    fn.restype = ctypes.c_int
    fn.argtypes = [type(t) for t in head] + [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 15 + [type(t) for t in tail]
    rc = fn(*head, ctypes.byref(scheme), n, coff.ctypes.data, ptr(cands), ptr(cnt), ptr(uoff), ptr(usc), ptr(caps), ptr(moff), ptr(recs), ptr(reg), ptr(ex), ptr(off), ptr(q),
            out.ctypes.data, pair_score.ctypes.data, order.ctypes.data, *tail)
    return rc, out[:n], pair_score[:len(cands)], order[:len(cands)]


MINIMIZER_REVERSE = 1
# vgk_chain_stitch (include/vgk.h): pieces of a read's chain in, one composed alignment per read out
CHAIN_PIECE_DT = np.dtype([("kind", "<u4"), ("link", "<u4"), ("node_offset", "<u4"), ("path_begin", "<u4"), ("path_len", "<u4"), ("edit_begin", "<u4"), ("n_edits", "<u4"), ("reserved", "<u4")])
CHAIN_MAPPING_DT = np.dtype([("node", "<u4"), ("offset", "<u4"), ("edit_begin", "<u4"), ("n_edits", "<u4")])
CHAIN_RESULT_DT = np.dtype([("status", "<i4"), ("mapping_begin", "<u4"), ("n_mappings", "<u4"), ("edit_begin", "<u4"), ("n_edits", "<u4"), ("from_length", "<u4"), ("to_length", "<u4"), ("reserved", "<u4")])
PIECE_LINK, PIECE_ALIGNMENT, PIECE_PATH = 0, 1, 2
assert WFA_DT.itemsize == 32 and WFA_RESULT_DT.itemsize == 40 and WFA_EVENT_DT.itemsize == 16
assert CHAIN_PIECE_DT.itemsize == 32 and CHAIN_MAPPING_DT.itemsize == 16 and CHAIN_RESULT_DT.itemsize == 32
assert GAPLESS_DT.itemsize == 40 and EXT_DT.itemsize == 60 and GAPLESS_RESULT_DT.itemsize == 16
assert BANDED_DT.itemsize == 80
assert GRAPH_DT.itemsize == 40 and PROBLEM_DT.itemsize == 80 and RESULT_DT.itemsize == 32 and OP_DT.itemsize == 8


# vgk_pick_mappings (include/vgk_engine.h): a long read's mappings chosen from its chains' alignments — multiplicities, order, uniqueness
CHAIN_RANGE_DT = np.dtype([("component", "<u8"), ("flags", "<u4"), ("child_start", "<u4"), ("child_end", "<u4"), ("reserved", "<u4"), ("offset_start", "<u8"), ("offset_end", "<u8")])
PICK_CHAIN_DT = np.dtype([("score_estimate", "<i4"), ("reserved", "<u4"), ("multiplicity", "<f8"), ("range", CHAIN_RANGE_DT)])
PICK_ALIGNMENT_DT = np.dtype([("source", "<u4"), ("score", "<i4"), ("item_count", "<u8"), ("result", CHAIN_RESULT_DT)])
PICK_RESULT_DT = np.dtype([("status", "<i4"), ("first", "<u4"), ("n_scores", "<u4"), ("n_mappings", "<u4"), ("unmapped", "<u4"), ("reserved", "<u4")])
PICK_VERDICT_DT = np.dtype([("identity", "<f8"), ("fraction_unique", "<f8"), ("fate", "<u4"), ("reserved", "<u4")])
assert CHAIN_RANGE_DT.itemsize == 40 and PICK_CHAIN_DT.itemsize == 56 and PICK_ALIGNMENT_DT.itemsize == 48 and PICK_RESULT_DT.itemsize == 24 and PICK_VERDICT_DT.itemsize == 24
PICK_SORT_BY_CHAIN_SCORE = 1
CHAIN_RANGE_ROOT_SNARL = 1
PICK_MAPPING, PICK_BEYOND_CUT, PICK_FAIL_SCORE, PICK_FAIL_UNIQUE = 1, 2, 3, 4
PICK_NOT_EVALUATED = 0x7ff8000000000000         # the bits of fraction_unique where it was never evaluated
PICK_NONE = 0xffffffff                          # picked[]: the unmapped entry


class PickScheme(ctypes.Structure):             # vgk_pick_scheme; the defaults are MinimizerMapper's
    _fields_ = [("min_unique_node_fraction", ctypes.c_double), ("max_multimaps", ctypes.c_uint32), ("flags", ctypes.c_uint32)]

    @classmethod
    def defaults(cls, **changed):
        p = cls(0.0, 1, 0)
        for name, value in changed.items():
            assert hasattr(p, name), name
            setattr(p, name, value)
        return p


assert ctypes.sizeof(PickScheme) == 16


def pick_mappings_call(fn, head, scheme, reads, read_off, chain_off, chains, aln_off, alns, mappings, edits, rng_state=None, tail=(), cap=None):
    """one call with vgk_pick_mappings' arguments (the engine's, the host shim's vgh_pick_mappings, the serial driver's): head / tail = the ctypes values the
    function takes before `scheme` / behind `written`.  rng_state: uint32 per read, updated in place (None: nothing is shuffled, the reads are not passed).
    cap None: the room the header names (alignments + reads)
    -> (rc, dict(results PICK_RESULT_DT, verdicts PICK_VERDICT_DT, picked, scores, multiplicity, written))"""
    def ptr(a):
        return a.ctypes.data if a is not None and len(a) else None
    off = np.ascontiguousarray(read_off, dtype=np.uint64); coff = np.ascontiguousarray(chain_off, dtype=np.uint64); aoff = np.ascontiguousarray(aln_off, dtype=np.uint64)
    rd = None if reads is None else np.ascontiguousarray(reads, dtype=np.uint8)
    ch = np.ascontiguousarray(chains, dtype=PICK_CHAIN_DT); al = np.ascontiguousarray(alns, dtype=PICK_ALIGNMENT_DT)
    mp = np.ascontiguousarray(mappings, dtype=CHAIN_MAPPING_DT); ed = np.ascontiguousarray(edits, dtype=np.uint32)
    n = len(coff) - 1
    assert len(aoff) == len(coff) == len(off) and (rng_state is None or (rng_state.dtype == np.uint32 and len(rng_state) == n and rng_state.flags.c_contiguous))
    if cap is None:
        cap = len(al) + n
    cap = int(cap)
    results = np.zeros(max(n, 1), dtype=PICK_RESULT_DT); verdicts = np.zeros(max(len(al), 1), dtype=PICK_VERDICT_DT)
    picked = np.zeros(max(cap, 1), dtype=np.uint32); scores = np.zeros(max(cap, 1), dtype=np.int32); mult = np.zeros(max(cap, 1), dtype=np.float64)
    written = ctypes.c_size_t(0)
    fn.restype = ctypes.c_int
    fn.argtypes = [type(t) for t in head] + [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 8 + [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 5 + \
                  [ctypes.c_size_t, ctypes.c_void_p] + [type(t) for t in tail]
    rc = fn(*head, ctypes.byref(scheme), n, ptr(rd) if rng_state is not None else None, off.ctypes.data, rng_state.ctypes.data if rng_state is not None and n else None,
            coff.ctypes.data, ptr(ch), aoff.ctypes.data, ptr(al), ptr(mp), len(mp), ptr(ed), len(ed), results.ctypes.data, verdicts.ctypes.data, picked.ctypes.data, scores.ctypes.data,
            mult.ctypes.data, cap, ctypes.byref(written), *tail)
    w = int(written.value)
    if rc != VGK_OK:
        return rc, dict(results=results[:n], written=w)
    return rc, dict(results=results[:n], verdicts=verdicts[:len(al)], picked=picked[:w], scores=scores[:w], multiplicity=mult[:w], written=w)


class Scoring(ctypes.Structure):
    _fields_ = [("matrix", ctypes.c_int8 * 25), ("gap_open", ctypes.c_uint8), ("gap_extend", ctypes.c_uint8),
                ("full_length_bonus", ctypes.c_int8), ("reserved", ctypes.c_uint8)]

    @classmethod
    def simple(cls, match=1, mismatch=4, gap_open=6, gap_extend=1, bonus=5):
        """match/mismatch matrix with the all-zero N row/column (src/alignment_scorer.cpp:297-304)."""
        s = cls()
        for i in range(25):
            r, c = divmod(i, 5)
            s.matrix[i] = 0 if (r == 4 or c == 4) else (match if r == c else -mismatch)
        s.gap_open, s.gap_extend, s.full_length_bonus = gap_open, gap_extend, bonus
        return s


class Haplotypes(ctypes.Structure):
    _fields_ = [("n_nodes", ctypes.c_uint32), ("node_len", ctypes.c_void_p), ("seq", ctypes.c_void_p),
                ("n_threads", ctypes.c_uint32), ("thread_off", ctypes.c_void_p), ("thread_nodes", ctypes.c_void_p)]


class QualAdj(ctypes.Structure):
    _fields_ = [("matrix", ctypes.c_void_p), ("bonuses", ctypes.c_void_p)]


class VgkError(RuntimeError):
    pass


# vgk_gssw_align_windows / vgk_gssw_align_windows_last (include/vgk_engine.h)
ALIGN_WINDOWS_ARGTYPES = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32,
                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
ALIGN_WINDOWS_LAST_ARGTYPES = [ctypes.c_void_p, ctypes.c_int]


def load_library(path=None):
    path = path or os.environ.get("VGAMD_ENGINE_LIB") or DEFAULT_LIB
    if not os.path.exists(path):
        raise VgkError("engine library %s is missing: run `make lib` (python -c 'import __graft_entry__ as g; g.build()'); "
                       "there is no CPU fallback" % path)
    lib = ctypes.CDLL(path)
    vp, u32, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t
    lib.vgk_abi_version.restype = ctypes.c_int
    lib.vgk_strerror.restype = ctypes.c_char_p
    lib.vgk_strerror.argtypes = [ctypes.c_int]
    lib.vgk_create.argtypes = [ctypes.c_int, ctypes.POINTER(Scoring), ctypes.POINTER(vp)]
    lib.vgk_create_qual_adj.argtypes = [ctypes.c_int, ctypes.POINTER(Scoring), ctypes.POINTER(QualAdj), ctypes.POINTER(vp)]
    lib.vgk_destroy.argtypes = [vp]
    lib.vgk_device_info.argtypes = [vp, ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(sz)]
    lib.vgk_gssw_pack.argtypes = [vp, vp, u32, u32, ctypes.POINTER(vp)]
    lib.vgk_gssw_run.argtypes = [vp]
    lib.vgk_gssw_fetch.argtypes = [vp, vp, vp, sz, ctypes.POINTER(sz)]
    lib.vgk_gssw_align.argtypes = [vp, vp, u32, vp, vp, sz, ctypes.POINTER(sz)]
    lib.vgk_batch_free.argtypes = [vp]
    if hasattr(lib, "vgk_gssw_wide_last"):                     # (the oracle has no wide route)
        lib.vgk_gssw_wide_last.restype = ctypes.c_double
        lib.vgk_gssw_wide_last.argtypes = [vp, ctypes.c_int]
    if hasattr(lib, "vgk_gssw_align_windows"):                 # (engine only: include/vgk_engine.h)
        lib.vgk_gssw_align_windows.argtypes = ALIGN_WINDOWS_ARGTYPES
        lib.vgk_gssw_align_windows_last.restype = ctypes.c_double
        lib.vgk_gssw_align_windows_last.argtypes = ALIGN_WINDOWS_LAST_ARGTYPES
    lib.vgk_xdrop_band_align.argtypes = [vp, vp, u32, vp, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint64 * 2)]
    lib.vgk_graph_create.argtypes = [vp, vp, ctypes.POINTER(vp)]
    lib.vgk_graph_destroy.argtypes = [vp]
    lib.vgk_gssw_pack_windows.argtypes = [vp, vp, vp, sz, vp, u32, u32, ctypes.POINTER(vp)]
    lib.vgk_batch_sync.argtypes = [vp]
    lib.vgk_batch_kernel_ms.restype = ctypes.c_double
    lib.vgk_batch_kernel_ms.argtypes = [vp, ctypes.c_int]
    lib.vgk_banded_align.argtypes = [vp, vp, u32, vp, vp, sz, ctypes.POINTER(sz)]
    lib.vgk_haplo_create.argtypes = [vp, ctypes.POINTER(Haplotypes), ctypes.POINTER(vp)]
    lib.vgk_haplo_destroy.argtypes = [vp]
    lib.vgk_gapless_extend.argtypes = [vp, vp, vp, u32, vp, vp, sz, vp, sz, vp, sz, ctypes.POINTER(sz * 3)]
    lib.vgk_gapless_last_ms.restype = ctypes.c_double
    lib.vgk_gapless_last_ms.argtypes = [vp]
    lib.vgk_banded_align_multi.argtypes = [vp, vp, u32, u32, vp, vp, vp, sz, ctypes.POINTER(sz)]
    lib.vgk_gssw_align_multi.argtypes = [vp, vp, u32, u32, vp, vp, vp, sz, ctypes.POINTER(sz)]
    lib.vgk_gssw_multi_host_walks.argtypes = [vp]; lib.vgk_gssw_multi_host_walks.restype = ctypes.c_uint64
    lib.vgk_banded_rerun.argtypes = [vp]
    lib.vgk_gapless_rerun.argtypes = [vp]
    lib.vgk_wfa_extend.argtypes = [vp, vp, vp, vp, u32, vp, vp, sz, vp, sz, ctypes.POINTER(sz * 2)]
    lib.vgk_chain_stitch.argtypes = [vp, vp, vp, vp, u32, vp, sz, vp, sz, vp, sz, vp, vp, sz, vp, sz, ctypes.POINTER(sz * 2)]
    lib.vgk_chain_stitch_last_ms.restype = ctypes.c_double; lib.vgk_chain_stitch_last_ms.argtypes = [vp]
    lib.vgk_wfa_rerun.argtypes = [vp]
    lib.vgk_wfa_last_ms.restype = ctypes.c_double
    lib.vgk_wfa_last_ms.argtypes = [vp]
    lib.vgk_banded_last.restype = ctypes.c_double
    lib.vgk_banded_last.argtypes = [vp, ctypes.c_int]
    for f in ("vgk_batch_cells", "vgk_batch_alg_bytes", "vgk_batch_device_bytes", "vgk_batch_wave_steps"):
        getattr(lib, f).restype = ctypes.c_uint64
        getattr(lib, f).argtypes = [vp]
    return lib


class ProblemSet:
    """A batch of gssw problems laid out in shared numpy arenas.

    reads     : uint8 array of all read bases (ASCII), read i = reads[read_off[i]:read_off[i+1]]
    node_len  : uint32, all graphs' node lengths concatenated; graph i owns node_off[i]:node_off[i+1]
    seq       : uint8 ASCII graph bases, graph i's nodes concatenated starting at seq_off[i]
    pred_off  : uint32 per graph CSR offsets (n_nodes+1 entries each, LOCAL to the graph), laid out at node_off[i]+i
    pred_idx  : uint32 predecessor indices, graph i's edges start at edge_off[i]
    """

    def __init__(self, reads, read_off, node_len, node_off, seq, seq_off, pred_off, pred_idx, edge_off, flags, pinning=None,
                 max_gap=None, quals=None):
        self.reads = np.ascontiguousarray(reads, dtype=np.uint8)
        self.read_off = np.asarray(read_off, dtype=np.int64)
        self.node_len = np.ascontiguousarray(node_len, dtype=np.uint32)
        self.node_off = np.asarray(node_off, dtype=np.int64)
        self.seq = np.ascontiguousarray(seq, dtype=np.uint8)
        self.seq_off = np.asarray(seq_off, dtype=np.int64)
        self.pred_off = np.ascontiguousarray(pred_off, dtype=np.uint32)
        self.pred_idx = np.ascontiguousarray(pred_idx if len(pred_idx) else np.zeros(1, np.uint32), dtype=np.uint32)
        self.edge_off = np.asarray(edge_off, dtype=np.int64)
        self.flags = np.asarray(flags, dtype=np.uint32)
        self.pinning = None if pinning is None else np.ascontiguousarray(pinning, dtype=np.uint8)
        self.n = len(self.read_off) - 1
        n = self.n
        arr = np.zeros(n, dtype=PROBLEM_DT)
        arr["read"] = self.reads.ctypes.data + self.read_off[:-1]
        arr["read_len"] = np.diff(self.read_off)
        arr["flags"] = self.flags
        g = arr["graph"]
        g["n_nodes"] = np.diff(self.node_off)
        g["node_len"] = self.node_len.ctypes.data + 4 * self.node_off[:-1]
        g["seq"] = self.seq.ctypes.data + self.seq_off[:-1]
        g["pred_off"] = self.pred_off.ctypes.data + 4 * (self.node_off[:-1] + np.arange(n))
        g["pred_idx"] = self.pred_idx.ctypes.data + 4 * self.edge_off[:-1]
        arr["graph"] = g
        if self.pinning is not None:
            arr["pinning"] = self.pinning.ctypes.data + self.node_off[:-1]
        if max_gap is not None:
            arr["max_gap_length"] = np.asarray(max_gap, dtype=np.uint32)
        self.quals = None if quals is None else np.ascontiguousarray(quals, dtype=np.uint8)   # raw phred, same layout as reads
        if self.quals is not None:
            arr["qual"] = self.quals.ctypes.data + self.read_off[:-1]
        self.array = arr

    @property
    def ptr(self):
        return self.array.ctypes.data

    def subset(self, k):
        """First k problems (same arenas, no copies)."""
        s = object.__new__(ProblemSet)
        s.__dict__.update(self.__dict__)
        s.n = k; s.array = self.array[:k]; s.read_off = self.read_off[:k + 1]; s.seq_off = self.seq_off[:k + 1]
        return s

    @classmethod
    def from_lists(cls, problems):
        """problems: list of dicts {read: str, nodes: [str], preds: [[int]], flags: int, pinning: [0/1]|None}."""
        reads, read_off, node_len, node_off, seq, seq_off, pred_off, pred_idx, edge_off, flags, pinning = \
            [], [0], [], [0], [], [0], [], [], [0], [], []
        any_pin = any(p.get("pinning") is not None for p in problems)
        for p in problems:
            reads.append(np.frombuffer(p["read"].encode(), dtype=np.uint8)); read_off.append(read_off[-1] + len(p["read"]))
            nl = [len(s) for s in p["nodes"]]
            node_len.extend(nl); node_off.append(node_off[-1] + len(nl))
            s = "".join(p["nodes"]); seq.append(np.frombuffer(s.encode(), dtype=np.uint8)); seq_off.append(seq_off[-1] + len(s))
            off = [0]
            for pr in p["preds"]:
                pred_idx.extend(pr); off.append(off[-1] + len(pr))
            pred_off.extend(off); edge_off.append(edge_off[-1] + off[-1])
            flags.append(p["flags"])
            pinning.extend(p["pinning"] if p.get("pinning") is not None else [0] * len(nl))
        cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.uint8)
        quals = None
        if any(p.get("qual") is not None for p in problems):
            quals = np.concatenate([np.asarray(p["qual"], dtype=np.uint8) for p in problems])
        return cls(cat(reads), read_off, node_len, node_off, cat(seq), seq_off, pred_off, pred_idx, edge_off, flags,
                   pinning if any_pin else None, [p.get("max_gap", 40) for p in problems], quals)


class BandedSet(ProblemSet):
    """A batch of banded-global problems (vgk_banded_problem) over the same arenas as ProblemSet.
    problems: list of dicts {read, nodes: [str] (may be empty strings), preds, band_padding, permissive, max_cells?, qual?}."""

    @classmethod
    def from_lists(cls, problems):
        base = ProblemSet.from_lists([dict(p, flags=0, pinning=None) for p in problems])
        s = object.__new__(cls)
        s.__dict__.update(base.__dict__)
        arr = np.zeros(s.n, dtype=BANDED_DT)
        for k in ("read", "read_len", "graph"):
            arr[k] = base.array[k]
        arr["qual"] = base.array["qual"]
        arr["flags"] = [VGK_BANDED_PERMISSIVE if p.get("permissive", True) else 0 for p in problems]
        arr["band_padding"] = [p.get("band_padding", 1) for p in problems]
        arr["max_cells"] = [p.get("max_cells", 0) for p in problems]
        s.array = arr
        return s

    def subset(self, k):
        raise NotImplementedError

    def select(self, idx):
        """the problems idx of this set as a set of their own over the SAME arenas (only the problem structs are copied): a caller that
        keeps its extracted subgraphs flat picks a batch out of them without touching a base"""
        idx = np.asarray(idx, dtype=np.int64)
        s = object.__new__(type(self))
        s.__dict__.update(self.__dict__)
        s._arenas_of = self                                         # (keeps the arenas alive)
        s.array = np.ascontiguousarray(self.array[idx]); s.n = len(idx)
        rl = np.diff(self.read_off)[idx]; sl = np.diff(self.seq_off)[idx]; nn = self.array["graph"]["n_nodes"][idx].astype(np.int64)
        s.ops_cap = int(rl.sum() + sl.sum() + 2 * nn.sum() + 8 * s.n)
        return s


class Engine:
    """One engine context = one (device, scoring) pair, like one vg Aligner."""

    def __init__(self, scoring=None, device=0, lib=None, qual_adj=None):
        """qual_adj = (matrix int8[256*25], bonuses int8[256]) makes a quality-adjusted context (QualAdjAligner)."""
        self.lib = load_library(lib) if (lib is None or isinstance(lib, str)) else lib
        self.scoring = scoring or Scoring.simple()
        self.device = device
        h = ctypes.c_void_p()
        if qual_adj is not None:
            self._qm = np.ascontiguousarray(qual_adj[0], dtype=np.int8); self._qb = np.ascontiguousarray(qual_adj[1], dtype=np.int8)
            assert self._qm.size == 256 * 25 and self._qb.size == 256
            qa = QualAdj(self._qm.ctypes.data, self._qb.ctypes.data)
            rc = self.lib.vgk_create_qual_adj(device, ctypes.byref(self.scoring), ctypes.byref(qa), ctypes.byref(h))
        else:
            rc = self.lib.vgk_create(device, ctypes.byref(self.scoring), ctypes.byref(h))
        if rc != VGK_OK:
            raise VgkError("vgk_create: %s" % self.lib.vgk_strerror(rc).decode())
        self.h = h
        self._indexes = weakref.WeakSet()      # haplotype indexes live in this context: they go first

    def set_speculation(self, mode):
        """0 = by feedback (default), 1 = whenever a batch allows it, 2 = never (vgk_set_speculation)"""
        self.lib.vgk_set_speculation.argtypes = [ctypes.c_void_p, ctypes.c_int]
        self._check(self.lib.vgk_set_speculation(self.h, mode), "vgk_set_speculation")

    def speculation_state(self):
        """-> dict(on, observed, turned_off, turned_on, probe_interval, last_miss): the context's feedback on the speculative fill"""
        self.lib.vgk_speculation_state.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        c = (ctypes.c_uint64 * 4)(); m = ctypes.c_double()
        on = self.lib.vgk_speculation_state(self.h, c, ctypes.byref(m))
        return dict(on=bool(on), observed=int(c[0]), turned_off=int(c[1]), turned_on=int(c[2]), probe_interval=int(c[3]), last_miss=float(m.value))

    def close(self):
        if getattr(self, "h", None):
            for index in list(getattr(self, "_indexes", ())):
                index.close()
            self.lib.vgk_destroy(self.h); self.h = None

    __del__ = close

    def host_register(self, array):
        """vgk_host_register: page-lock a numpy array this caller keeps (copies out of it then run at the link's rate); False when refused"""
        a = np.ascontiguousarray(array)
        self.lib.vgk_host_register.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        return self.lib.vgk_host_register(self.h, a.ctypes.data, a.nbytes) == VGK_OK

    def host_unregister(self, array):
        self.lib.vgk_host_unregister.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        return self.lib.vgk_host_unregister(self.h, np.ascontiguousarray(array).ctypes.data) == VGK_OK

    def device_info(self):
        name = ctypes.create_string_buffer(256); cus = ctypes.c_int(); mem = ctypes.c_size_t()
        self.lib.vgk_device_info(self.h, name, 256, ctypes.byref(cus), ctypes.byref(mem))
        return name.value.decode(), cus.value, mem.value

    def _check(self, rc, what):
        if rc != VGK_OK:
            raise VgkError("%s: %s" % (what, self.lib.vgk_strerror(rc).decode()))

    def pack(self, ps, ops_per_problem=0):
        b = ctypes.c_void_p()
        self._check(self.lib.vgk_gssw_pack(self.h, ps.ptr, ps.n, ops_per_problem, ctypes.byref(b)), "vgk_gssw_pack")
        return Batch(self, b, ps, ops_per_problem)

    def graph(self, node_len, seq, pred_off, pred_idx):
        """One DAG (nodes in topological order, predecessor CSR) resident in HBM -> ResidentGraph."""
        return ResidentGraph(self, node_len, seq, pred_off, pred_idx)

    def pack_windows(self, graph, ws, ops_per_problem=0):
        """vgk_gssw_pack_windows: ws = WindowSet (reads + windows of `graph`); packed on the device."""
        b = ctypes.c_void_p()
        self._check(self.lib.vgk_gssw_pack_windows(self.h, graph.h, ws.reads.ctypes.data, ws.reads.size, ws.array.ctypes.data, ws.n,
                                                   ops_per_problem, ctypes.byref(b)), "vgk_gssw_pack_windows")
        return Batch(self, b, ws, ops_per_problem)

    def pack_extensions(self, graph, es, ops_per_problem=0):
        """vgk_gssw_pack_extensions: es = ExtensionSet; the sub-DAGs are derived on the device"""
        b = ctypes.c_void_p()
        self.lib.vgk_gssw_pack_extensions.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
        self._check(self.lib.vgk_gssw_pack_extensions(self.h, graph.h, es.reads.ctypes.data, es.reads.size, es.array.ctypes.data, es.n,
                                                      ops_per_problem, ctypes.byref(b)), "vgk_gssw_pack_extensions")
        return Batch(self, b, es, ops_per_problem)

    def rescue_requests(self, graph, mean, sd, stdevs=4.0, out=None):
        """vgk_rescue_requests over the sets the last gapless_extend(_seeded) call on this context left in HBM; graph: a DeviceGraph or a vgk_dgraph
        pointer (int) of the same device; out: a RESCUE_REQUEST_DT array to fill (grown when too small) -> the filled part"""
        gh = graph if isinstance(graph, int) else graph.h
        self.lib.vgk_rescue_requests.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        if out is None:
            out = np.zeros(4096, dtype=RESCUE_REQUEST_DT)
        w = ctypes.c_size_t()
        rc = self.lib.vgk_rescue_requests(self.h, gh, float(mean), float(sd), float(stdevs), out.ctypes.data, len(out), ctypes.byref(w))
        if rc == VGK_EOPS:
            out = np.zeros(int(w.value) + int(w.value) // 8 + 64, dtype=RESCUE_REQUEST_DT)
            rc = self.lib.vgk_rescue_requests(self.h, gh, float(mean), float(sd), float(stdevs), out.ctypes.data, len(out), ctypes.byref(w))
        self._check(rc, "vgk_rescue_requests")
        self._rescue_requests_buf = out
        return out[:int(w.value)]

    def align_extensions(self, graph, es, ops_per_problem=0):
        with self.pack_extensions(graph, es, ops_per_problem) as b:
            b.run()
            return b.fetch()

    def align_windows(self, graph, ws, ops_per_problem=0):
        with self.pack_windows(graph, ws, ops_per_problem) as b:
            b.run()
            return b.fetch()

    def align(self, ps, ops_per_problem=0):
        with self.pack(ps, ops_per_problem) as b:
            b.run()
            return b.fetch()

    def align_call(self, ps):
        """vgk_gssw_align (the one-call form: sub-batches, and the wide route for problems outside the packed kernels' range) -> (results, ops)."""
        res = np.zeros(ps.n, dtype=RESULT_DT)
        cap = int(np.diff(ps.read_off).sum() + np.diff(ps.seq_off).sum() + 4 * ps.n)
        ops = np.zeros(max(cap, 1), dtype=OP_DT)
        written = ctypes.c_size_t()
        self._check(self.lib.vgk_gssw_align(self.h, ps.ptr, ps.n, res.ctypes.data, ops.ctypes.data, cap, ctypes.byref(written)), "vgk_gssw_align")
        return res, ops[:written.value]

    def align_windows_call(self, graph, ws, ops_cap=None):
        """vgk_gssw_align_windows (the one-call form over a ResidentGraph: windows of any read length, each answered in its own status; the wide
        kernels take what the packed ones do not) -> (results, ops); ops_cap: entries of the op array (default: room for every window's ops)"""
        res = np.zeros(ws.n, dtype=RESULT_DT)
        if ops_cap is None:
            ops_cap = int(np.diff(ws.read_off).sum() + np.diff(ws.seq_off).sum() + 4 * ws.n)
        ops = np.zeros(max(int(ops_cap), 1), dtype=OP_DT)
        written = ctypes.c_size_t()
        reads = ws.reads.ctypes.data_as(ctypes.c_char_p)
        self._check(self.lib.vgk_gssw_align_windows(self.h, graph.h, reads, ws.reads.size, ws.array.ctypes.data, ws.n, res.ctypes.data,
                                                    ops.ctypes.data, int(ops_cap), ctypes.byref(written)), "vgk_gssw_align_windows")
        return res, ops[:written.value]

    def align_windows_last(self, which):
        """vgk_gssw_align_windows_last: 0 wide packing kernels ms, 1 wide fill ms, 2 wide walk ms, 3 windows that went wide, 4 wide sub-batches,
        5 op bytes copied back for the wide windows"""
        return float(self.lib.vgk_gssw_align_windows_last(self.h, which))

    def wide_last(self, which):
        """vgk_gssw_wide_last: the wide route's share of the last align_call (0 fill ms, 1 traceback ms, 2 cells, 3 traced cells, 4 launches)"""
        return float(self.lib.vgk_gssw_wide_last(self.h, which))

    def xdrop_band_align(self, ps, out=None):
        """vgk_xdrop_band_align over a ProblemSet of VGK_XDROP_PINNED problems -> (results, ops, (cells in band, cells of the rectangles)).
        out: (results, ops) arrays of an earlier call on the same set, written again (a caller that keeps its output buffers)."""
        if out is not None:
            res, ops = out; cap = len(ops)
        else:
            res = np.zeros(ps.n, dtype=RESULT_DT)
            cap = int(np.diff(ps.read_off).sum() + np.diff(ps.seq_off).sum() + len(ps.node_len) + 4 * ps.n)
            ops = np.zeros(max(cap, 1), dtype=OP_DT)
        written = ctypes.c_size_t(); stats = (ctypes.c_uint64 * 2)()
        self._check(self.lib.vgk_xdrop_band_align(self.h, ps.ptr, ps.n, res.ctypes.data, ops.ctypes.data, cap, ctypes.byref(written), ctypes.byref(stats)),
                    "vgk_xdrop_band_align")
        return res, ops[:written.value], (int(stats[0]), int(stats[1]))

    def xdrop_band_last_classes(self):
        """problems of the last xdrop_band_align call by the lanes they ran on: (8, 16, 64)"""
        self.lib.vgk_xdrop_band_last_class.restype = ctypes.c_uint64; self.lib.vgk_xdrop_band_last_class.argtypes = [ctypes.c_void_p, ctypes.c_int]
        return tuple(int(self.lib.vgk_xdrop_band_last_class(self.h, k)) for k in range(3))

    def align_multi(self, ps, max_alt_alns):
        """vgk_gssw_align_multi over a ProblemSet of pinned problems -> (results [n, max_alt_alns], n_alignments [n], ops)."""
        res = np.zeros((ps.n, max_alt_alns), dtype=RESULT_DT); cnt = np.zeros(ps.n, dtype=np.uint32)
        cap = int((np.diff(ps.read_off).sum() + np.diff(ps.seq_off).sum() + 4 * ps.n) * max_alt_alns)
        ops = np.zeros(max(cap, 1), dtype=OP_DT)
        written = ctypes.c_size_t()
        self._check(self.lib.vgk_gssw_align_multi(self.h, ps.ptr, ps.n, max_alt_alns, res.ctypes.data, cnt.ctypes.data, ops.ctypes.data, cap,
                                                  ctypes.byref(written)), "vgk_gssw_align_multi")
        self.multi_host_walks = int(self.lib.vgk_gssw_multi_host_walks(self.h))      # problems whose alternates a host thread walked
        return res, cnt, ops[:written.value]

    def banded_align(self, bs):
        """vgk_banded_align over a BandedSet -> (results, ops); per-problem failures are reported in results['status']."""
        res = np.zeros(bs.n, dtype=RESULT_DT)
        cap = getattr(bs, "ops_cap", None)
        if cap is None:
            cap = int(np.diff(bs.read_off).sum() + np.diff(bs.seq_off).sum() + 2 * len(bs.node_len) + 8 * bs.n)
        ops = np.zeros(max(cap, 1), dtype=OP_DT)
        written = ctypes.c_size_t()
        self._check(self.lib.vgk_banded_align(self.h, bs.ptr, bs.n, res.ctypes.data, ops.ctypes.data, cap, ctypes.byref(written)),
                    "vgk_banded_align")
        return res, ops[:written.value]

    def banded_align_multi(self, bs, max_alt_alns):
        """vgk_banded_align_multi -> (results [n, max_alt_alns], n_alignments [n], ops)"""
        res = np.zeros((bs.n, max_alt_alns), dtype=RESULT_DT)
        cnt = np.zeros(bs.n, dtype=np.uint32)
        cap = int((np.diff(bs.read_off).sum() + np.diff(bs.seq_off).sum() + 2 * len(bs.node_len) + 8 * bs.n) * max_alt_alns)
        ops = np.zeros(max(cap, 1), dtype=OP_DT)
        written = ctypes.c_size_t()
        self._check(self.lib.vgk_banded_align_multi(self.h, bs.ptr, bs.n, max_alt_alns, res.ctypes.data, cnt.ctypes.data, ops.ctypes.data, cap,
                                                    ctypes.byref(written)), "vgk_banded_align_multi")
        self.multi_host_walks = int(self.lib.vgk_gssw_multi_host_walks(self.h))      # problems whose alternates a host thread walked
        return res, cnt, ops[:written.value]

    def banded_rerun(self):
        self._check(self.lib.vgk_banded_rerun(self.h), "vgk_banded_rerun")

    def gapless_rerun(self):
        self._check(self.lib.vgk_gapless_rerun(self.h), "vgk_gapless_rerun")

    def banded_last(self, which):
        return self.lib.vgk_banded_last(self.h, which)

    def _out(self, name, n, dtype):
        """an output array of n elements.  reuse_outputs = True (a caller that consumes one call's outputs before the next call, like
        bench.py's steady-state loops — or any C caller with its own buffers): one array per output is kept and grown, so a call neither
        allocates nor page-faults hundreds of MB; the arrays a call returns are then views that the next call overwrites."""
        if not getattr(self, "reuse_outputs", False):
            return np.zeros(n, dtype=dtype)
        cache = self.__dict__.setdefault("_out_cache", {})
        a = cache.get(name)
        if a is None or len(a) < n or a.dtype != dtype:
            a = cache[name] = np.zeros(max(n, 1), dtype=dtype)
        return a[:n]

    def haplo_index(self, nodes, threads):
        """nodes: [str] in node-id order; threads: [[oriented node = 2 * index + is_reverse]].  -> HaploIndex"""
        return HaploIndex(self, nodes, threads)

    def gbz_load(self, gbz_bytes):
        """vgk_gbz_load: a GBZ image -> (node sequences [str], threads [[oriented node]])"""
        lib = self.lib
        out = ctypes.POINTER(Haplotypes)()
        lib.vgk_gbz_load.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
        self._check(lib.vgk_gbz_load(bytes(gbz_bytes), len(gbz_bytes), ctypes.byref(out)), "vgk_gbz_load")
        try:
            h = out.contents
            lens = np.ctypeslib.as_array(ctypes.cast(h.node_len, ctypes.POINTER(ctypes.c_uint32)), (h.n_nodes,)).copy()
            seq = ctypes.string_at(h.seq, int(lens.sum())).decode()
            at = [0] + [int(x) for x in np.cumsum(lens.astype(np.int64))]
            nodes = [seq[at[i]:at[i + 1]] for i in range(h.n_nodes)]
            toff = np.ctypeslib.as_array(ctypes.cast(h.thread_off, ctypes.POINTER(ctypes.c_uint32)), (h.n_threads + 1,)).copy()
            tn = np.ctypeslib.as_array(ctypes.cast(h.thread_nodes, ctypes.POINTER(ctypes.c_uint32)), (max(int(toff[-1]), 1),)).copy()
            threads = [[int(x) for x in tn[toff[t]:toff[t + 1]]] for t in range(h.n_threads)]
        finally:
            lib.vgk_haplotypes_free.argtypes = [ctypes.c_void_p]; lib.vgk_haplotypes_free.restype = None
            lib.vgk_haplotypes_free(out)
        return nodes, threads

    def haplo_index_from_gbwt(self, nodes, gbwt_bytes):
        """vgk_haplo_create_gbwt: the index from the image of a (simple-sds, bidirectional) GBWT file"""
        return HaploIndex(self, nodes, gbwt=gbwt_bytes)

    def gapless_extend(self, index, problems, defer=False):
        """problems: a GaplessSet, or a list of dicts {read, seeds: [(oriented node, read_offset - node_offset)], max_mismatches?,
        overlap_threshold?, trim?}.  -> (results, extensions, nodes, mismatches) as numpy arrays laid out like include/vgk.h."""
        gs = problems if isinstance(problems, GaplessSet) else GaplessSet.from_lists(problems)
        res = self._out("g_res", gs.n, GAPLESS_RESULT_DT)
        ext = self._out("g_ext", gs.ext_cap, EXT_DT); nodes = self._out("g_nodes", gs.node_cap, np.uint32); mism = self._out("g_mism", gs.mism_cap, np.uint32)
        written = (ctypes.c_size_t * 3)()
        if defer and gs.n:                                   # VGK_GAPLESS_DEFER rides on the first problem's flags (filled when the next tail_stage* call returns)
            gs.array["flags"][0] |= VGK_GAPLESS_DEFER
        try:
            self._check(self.lib.vgk_gapless_extend(self.h, index.h, gs.array.ctypes.data, gs.n, res.ctypes.data, ext.ctypes.data, gs.ext_cap,
                                                    nodes.ctypes.data, gs.node_cap, mism.ctypes.data, gs.mism_cap, ctypes.byref(written)),
                        "vgk_gapless_extend")
        finally:
            if defer and gs.n:
                gs.array["flags"][0] &= ~np.uint32(VGK_GAPLESS_DEFER)
        if defer:
            self._deferred_keep = (res, ext, nodes, mism)          # the engine still writes into them: alive until the deferral is finished
        return res, ext[:written[0]], nodes[:written[1]], mism[:written[2]]

    def minimizer_index(self, nodes, threads, k=29, w=11):
        return MinimizerIndex(self, nodes, threads, k, w)

    def minimizer_seeds(self, mindex, hindex, reads, read_off, hit_cap=500, keep_on_device=False):
        """vgk_minimizer_seeds: reads flat (uint8), read i = reads[read_off[i]:read_off[i+1]] -> (seed_off [n+1], seeds as SEED_DT, minimizers per read);
        keep_on_device: the seeds stay in HBM for gapless_extend_seeded (an empty seeds array comes back).  `self.minimizers_truncated`: per
        read, whether it reached the cap of 64 seeds with hits left unexamined (VGK_MINIMIZERS_TRUNCATED)"""
        reads = np.ascontiguousarray(reads, dtype=np.uint8); off = np.ascontiguousarray(read_off, dtype=np.uint64)
        n = len(off) - 1
        seed_off = self._out("mz_off", n + 1, np.uint32); mins = self._out("mz_mins", max(n, 1), np.uint32)
        cap = 0 if keep_on_device else 64 * max(n, 1)
        seeds = self._out("mz_seeds", max(cap, 1), SEED_DT)
        written = ctypes.c_size_t()
        self.lib.vgk_minimizer_seeds.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        self._check(self.lib.vgk_minimizer_seeds(self.h, mindex.h, hindex.h, reads.ctypes.data, off.ctypes.data, n, hit_cap, seed_off.ctypes.data, mins.ctypes.data,
                                                 None if keep_on_device else seeds.ctypes.data, cap, ctypes.byref(written)), "vgk_minimizer_seeds")
        self.minimizers_truncated = (mins[:n] & 0x80000000) != 0
        self.minimizers_policy_skipped = (mins[:n] & 0x40000000) != 0          # (VGK_MINIMIZERS_POLICY_SKIPPED: more than 64 minimizers, seeded without the policy)
        return seed_off, seeds[:0 if keep_on_device else written.value], mins[:n] & 0x3fffffff

    def minimizer_list(self, mindex, reads, read_off):
        """vgk_minimizer_list: every minimizer of every read, no caps -> (minimizer_off [n + 1] uint64, records READ_MINIMIZER_DT in read order)"""
        reads = np.ascontiguousarray(reads, dtype=np.uint8); off = np.ascontiguousarray(read_off, dtype=np.uint64); n = len(off) - 1
        moff = np.zeros(n + 1, dtype=np.uint64); written = ctypes.c_size_t()
        self.lib.vgk_minimizer_list.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        cap = max(16, int(len(reads)) // 4)
        for attempt in range(2):
            recs = np.zeros(cap, dtype=READ_MINIMIZER_DT)
            rc = self.lib.vgk_minimizer_list(self.h, mindex.h, reads.ctypes.data, off.ctypes.data, n, moff.ctypes.data, recs.ctypes.data, cap, ctypes.byref(written))
            if rc != VGK_EOPS:
                break
            cap = int(written.value)
        self._check(rc, "vgk_minimizer_list")
        return moff, recs[:written.value]

    def minimizer_seeds_of(self, mindex, minimizers, take):
        """vgk_minimizer_seeds_of: one seed per hit of the minimizers taken -> (seed_off [len(minimizers) + 1] uint64, seeds SEED_DT)"""
        recs = np.ascontiguousarray(minimizers, dtype=READ_MINIMIZER_DT); take = np.ascontiguousarray(take, dtype=np.uint8)
        assert len(take) == len(recs)
        soff = np.zeros(len(recs) + 1, dtype=np.uint64); written = ctypes.c_size_t()
        self.lib.vgk_minimizer_seeds_of.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        cap = max(16, int(recs["hits"][take != 0].sum()))
        seeds = np.zeros(cap, dtype=SEED_DT)
        self._check(self.lib.vgk_minimizer_seeds_of(self.h, mindex.h, recs.ctypes.data, take.ctypes.data, len(recs), soff.ctypes.data, seeds.ctypes.data, cap, ctypes.byref(written)), "vgk_minimizer_seeds_of")
        return soff, seeds[:written.value]

    def minimizer_choose(self, policy, k, reads, read_off, minimizer_off, minimizers):
        """vgk_minimizer_choose (include/vgk_engine.h): find_seeds' choice on the device over a list as minimizer_list answers it (any list: no index).
        policy: the keys of pipeline.GIRAFFE_LONG_READ_POLICY -> verdict per minimizer, uint8 (0 = taken, otherwise the SEED_* filter that dropped it)"""
        reads = np.ascontiguousarray(reads, dtype=np.uint8); off = np.ascontiguousarray(read_off, dtype=np.uint64); moff = np.ascontiguousarray(minimizer_off, dtype=np.uint64)
        recs = np.ascontiguousarray(minimizers, dtype=READ_MINIMIZER_DT); pol = find_seeds_policy(policy)
        verdict = np.zeros(max(len(recs), 1), dtype=np.uint8)
        self.lib.vgk_minimizer_choose.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.vgk_minimizer_choose(self.h, ctypes.byref(pol), k, reads.ctypes.data if len(reads) else None, off.ctypes.data, len(off) - 1, moff.ctypes.data,
                                                  recs.ctypes.data if len(recs) else None, verdict.ctypes.data), "vgk_minimizer_choose")
        return verdict[:len(recs)]

    def minimizer_find_seeds(self, mindex, policy, reads, read_off, cap_m=None, cap_s=None):
        """vgk_minimizer_find_seeds (include/vgk_engine.h): list -> find_seeds' choice -> the seeds of the taken, all on the device, one call.
        -> (minimizer_off [n + 1] uint64, records READ_MINIMIZER_DT, take uint8, seed_off [len(records) + 1] uint64, seeds SEED_DT).
        cap_m / cap_s: room to offer at first (default: a guess); too little costs a second call with the sizes the first one answered"""
        reads = np.ascontiguousarray(reads, dtype=np.uint8); off = np.ascontiguousarray(read_off, dtype=np.uint64); n = len(off) - 1
        pol = find_seeds_policy(policy)
        moff = np.zeros(n + 1, dtype=np.uint64); written = (ctypes.c_size_t * 2)()
        f = self.lib.vgk_minimizer_find_seeds
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        cap_m = max(16, int(len(reads)) // 4) if cap_m is None else int(cap_m); cap_s = 4 * cap_m if cap_s is None else int(cap_s)
        self.find_seeds_calls = 0
        for attempt in range(2):
            recs = np.zeros(max(cap_m, 1), dtype=READ_MINIMIZER_DT); take = np.zeros(max(cap_m, 1), dtype=np.uint8); soff = np.zeros(cap_m + 1, dtype=np.uint64); seeds = np.zeros(max(cap_s, 1), dtype=SEED_DT)
            rc = f(self.h, mindex.h, ctypes.byref(pol), reads.ctypes.data if len(reads) else None, off.ctypes.data, n, moff.ctypes.data, recs.ctypes.data, take.ctypes.data, cap_m,
                   soff.ctypes.data, seeds.ctypes.data, cap_s, written)
            self.find_seeds_calls += 1
            if rc != VGK_EOPS:
                break
            cap_m = max(cap_m, int(written[0])); cap_s = max(cap_s, int(written[1]))
        self._check(rc, "vgk_minimizer_find_seeds")
        m = int(written[0])
        return moff, recs[:m], take[:m], soff[:m + 1], seeds[:int(written[1])]

    def minimizer_choose_last_ms(self):
        self.lib.vgk_minimizer_choose_last_ms.restype = ctypes.c_double; self.lib.vgk_minimizer_choose_last_ms.argtypes = [ctypes.c_void_p]
        return self.lib.vgk_minimizer_choose_last_ms(self.h)

    def chain_items(self, scheme, anchor_off, anchors, cand_off, candidates, read_lookback=None, indel_limit=None):
        """vgk_chain_items (include/vgk_engine.h): find_best_chains on the device for a batch of (read, tree) problems.  scheme: the keys of
        CHAIN_SCHEME_DEFAULTS; anchors CHAIN_ANCHOR_DT in sort_anchor_indexes' order per problem; candidates CHAIN_CANDIDATE_DT in any order.
        -> dict(chain_off [n + 1], chains CHAIN_FOUND_DT, items, rec_right, rec_left, table_score, table_source (CHAIN_NOWHERE = from nowhere))"""
        rc, out = chain_items_call(self.lib.vgk_chain_items, (self.h,), scheme, anchor_off, anchors, cand_off, candidates, read_lookback, indel_limit)
        self._check(rc, "vgk_chain_items")
        return out

    def chain_items_limits(self):
        """-> (anchors of a problem whose table fits LDS, the largest indel limit, lanes per problem, 0)"""
        out = (ctypes.c_uint32 * 4)()
        self._check(self.lib.vgk_chain_items_limits(out), "vgk_chain_items_limits")
        return tuple(int(x) for x in out)

    def chain_items_last_ms(self):
        """device time of the last chain_items call: (legality + grouping, DP, traceback) in ms"""
        ms = (ctypes.c_double * 3)()
        self.lib.vgk_chain_items_last_ms.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.vgk_chain_items_last_ms(self.h, ms), "vgk_chain_items_last_ms")
        return tuple(float(x) for x in ms)

    def extension_anchors(self, index, seed_off, seeds, ext_off=None, extensions=None, full_length=None, nodes=None, mismatches=None, match=1, mismatch=4,
                          default_max_extension_mismatches=4, from_seeds=False, caps=None):
        """vgk_extension_anchors (include/vgk_engine.h): the anchors vgk_chain_items takes, from seeds (ANCHOR_SEED_DT) and the extensions vgk_gapless_extend
        wrote for them without trimming (EXT_DT with their nodes and mismatches; full_length = GAPLESS_RESULT_DT's per problem).  from_seeds: the seed anchors,
        sorted (do_gapless_extension == false).  caps = (anchors, represented) offers less room than the call's bounds: VgkError on VGK_EOPS unless enough.
        -> dict(anchor_off, anchors CHAIN_ANCHOR_DT, origins ANCHOR_ORIGIN_DT, rep_off, represented, status, written)"""
        rc, out = extension_anchors_call(self.lib.vgk_extension_anchors, (self.h, index.h), match, mismatch,
                                         VGK_ANCHORS_FROM_SEEDS if from_seeds else 0, default_max_extension_mismatches, seed_off, seeds, ext_off, extensions, full_length, nodes, mismatches, caps=caps)
        self._check(rc, "vgk_extension_anchors")
        return out

    def extension_anchors_limits(self):
        """-> (seeds of a problem whose working arrays fit LDS, lanes per problem, extensions of a problem whose order fits LDS, 0)"""
        out = (ctypes.c_uint32 * 4)()
        self._check(self.lib.vgk_extension_anchors_limits(out), "vgk_extension_anchors_limits")
        return tuple(int(x) for x in out)

    def extension_anchors_last_ms(self):
        """device time of the last extension_anchors call: (seed anchors + diagonal sort, the extensions' seed lists, the order-dependent part + sort) in ms"""
        ms = (ctypes.c_double * 3)()
        self.lib.vgk_extension_anchors_last_ms.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.vgk_extension_anchors_last_ms(self.h, ms), "vgk_extension_anchors_last_ms")
        return tuple(float(x) for x in ms)

    def read_alignments(self, index, reads, read_off, results, extensions, nodes, mismatches, tails=None, ops=None, extension_score_threshold=1,
                        max_local_extensions=0xffffffff, window_length=39, caps=None):
        """vgk_read_alignments (include/vgk_engine.h): per read the alignments giraffe makes of its extension set — one per leading full extension of a
        full-length set, otherwise the best and the second best of find_optimal_tail_alignments — from the set (GAPLESS_RESULT_DT, EXT_DT with their nodes
        and mismatches, as gapless_extend returns them) and the tails' alignments (TAIL_ALIGNMENT_DT, OP_DT, as tail_stage_aligned returns them).
        window_length: k + w - 1 of the minimizer index (k with syncmers).  caps = (alignments, mappings, edit runs) offers that much room: VgkError on
        VGK_EOPS.  -> dict(aln_off, alignments READ_ALIGNMENT_DT, mappings CHAIN_MAPPING_DT, edits, written)"""
        rc, out = read_alignments_call(self.lib.vgk_read_alignments, (self.h, index.h), reads, read_off, results, extensions, nodes, mismatches,
                                       tails, ops, extension_score_threshold, max_local_extensions, window_length, caps)
        self.read_alignments_written = out["written"]
        self._check(rc, "vgk_read_alignments")
        return out

    def tail_stage_composed(self, index, n_reads, n_ext, ops_per_problem=32, extension_score_threshold=1, max_local_extensions=0xffffffff, window_length=39, caps=None):
        """vgk_tail_stage_composed (include/vgk_engine.h): the tail stage over the sets the last gapless_extend / gapless_extend_seeded call left on the device,
        and the reads' alignments composed there from the tails' winners: neither tails nor ops come down.  caps = (alignments, mappings, edit runs): the
        room offered; None: n_ext + 2 n_reads alignments (which always suffices) with 8 mappings and 12 edit runs each.  Too little room: VgkError
        (VGK_EOPS) with self.read_alignments_written = what is needed — ext_total and read_score are complete by then; extend again and call with that room.
        -> (ext_total, read_score, dict(aln_off, alignments READ_ALIGNMENT_DT, mappings CHAIN_MAPPING_DT, edits, written), stats)"""
        ext_total = self._out("ts_ext", max(n_ext, 1), np.int32); read_score = self._out("ts_read", max(n_reads, 1), np.int32); stats = np.zeros(4, dtype=np.uint64)
        cap = caps if caps is not None else (n_ext + 2 * n_reads + 1, 8 * (n_ext + 2 * n_reads) + 16, 12 * (n_ext + 2 * n_reads) + 16)
        aln = self._out("tc_aln", max(cap[0], 1), READ_ALIGNMENT_DT); maps = self._out("tc_maps", max(cap[1], 1), CHAIN_MAPPING_DT); edits = self._out("tc_edits", max(cap[2], 1), np.uint32)
        aln_off = np.zeros(n_reads + 1, dtype=np.uint64); written = (ctypes.c_size_t * 3)()
        policy = ReadAlignmentsPolicy(int(extension_score_threshold), int(max_local_extensions), int(window_length), 0)
        fn = self.lib.vgk_tail_stage_composed
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                       ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        rc = fn(self.h, index.h, ops_per_problem, ctypes.byref(policy), ext_total.ctypes.data, len(ext_total), read_score.ctypes.data, aln_off.ctypes.data,
                aln.ctypes.data, cap[0], maps.ctypes.data, cap[1], edits.ctypes.data, cap[2], written, stats.ctypes.data)
        w = tuple(int(x) for x in written)
        self.read_alignments_written = w
        self._check(rc, "vgk_tail_stage_composed")
        return ext_total[:n_ext], read_score[:n_reads], dict(aln_off=aln_off, alignments=aln[:w[0]], mappings=maps[:w[1]], edits=edits[:w[2]], written=w), tuple(int(x) for x in stats)

    def read_alignments_limits(self):
        """-> (extensions of a set the selection keeps in LDS, lanes per read in the selection, lanes per read in count and emit, 0)"""
        out = (ctypes.c_uint32 * 4)()
        self._check(self.lib.vgk_read_alignments_limits(out), "vgk_read_alignments_limits")
        return tuple(int(x) for x in out)

    def read_alignments_last_ms(self):
        """device time of the last read_alignments call: (selection, count + prefix sums, emit) in ms"""
        ms = (ctypes.c_double * 3)()
        self.lib.vgk_read_alignments_last_ms.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.vgk_read_alignments_last_ms(self.h, ms), "vgk_read_alignments_last_ms")
        return tuple(float(x) for x in ms)

    def minimizer_regions(self, k, w, read_off, minimizer_off, minimizers):
        """vgk_minimizer_regions (include/vgk_engine.h): the agglomeration of every minimizer of a list as minimizer_list / minimizer_find_seeds answer it
        -> MINIMIZER_REGION_DT per minimizer (start, length in read bases)"""
        rc, regions = minimizer_regions_call(self.lib.vgk_minimizer_regions, (self.h,), k, w, read_off, minimizer_off, minimizers)
        self._check(rc, "vgk_minimizer_regions")
        return regions

    def read_mapq(self, scheme, score_off, scores, minimizer_off, minimizers, regions, explored, read_off, quality=None, multiplicity=None, unmapped=None):
        """vgk_read_mapq (include/vgk_engine.h): per read the mapping quality of its alignments' scores, capped by faster_cap over its explored minimizers.
        scheme: a ReadMapqScheme -> READ_MAPQ_RESULT_DT per read (mapq, status, uncapped, explored_cap)"""
        rc, out = read_mapq_call(self.lib.vgk_read_mapq, (self.h,), scheme, score_off, scores, minimizer_off, minimizers, regions, explored, read_off,
                                 quality, multiplicity, unmapped)
        self._check(rc, "vgk_read_mapq")
        return out

    def read_mapq_limits(self):
        """-> (explored minimizers of a read swept in LDS, lanes per read, lanes per minimizer in minimizer_regions, 0)"""
        out = (ctypes.c_uint32 * 4)()
        self._check(self.lib.vgk_read_mapq_limits(out), "vgk_read_mapq_limits")
        return tuple(int(x) for x in out)

    def read_mapq_last_ms(self):
        """device time of the last minimizer_regions | read_mapq call in ms"""
        ms = (ctypes.c_double * 2)()
        self.lib.vgk_read_mapq_last_ms.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.vgk_read_mapq_last_ms(self.h, ms), "vgk_read_mapq_last_ms")
        return tuple(float(x) for x in ms)

    def read_mapq_last_launches(self):
        """reads of the last read_mapq call: (swept in LDS, swept over the slab, refused by the checks)"""
        reads = (ctypes.c_uint64 * 3)()
        self.lib.vgk_read_mapq_last_launches.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.vgk_read_mapq_last_launches(self.h, reads), "vgk_read_mapq_last_launches")
        return tuple(int(x) for x in reads)

    def funnel_clusters(self, policy, reads, read_off, minimizer_off, minimizers, minimizer_score, cluster_off, cluster_seed_off, sources, rng_state=None, cap=None):
        """vgk_funnel_clusters (include/vgk_engine.h): per cluster score, covered, coverage, verdict, rank, better_or_equal; per read the clusters extended, in
        that order.  policy: a FunnelPolicy; rng_state: uint32 per read, updated in place (None: nothing shuffled) -> (rc, dict), rc VGK_OK or VGK_EOPS"""
        rc, out = funnel_clusters_call(self.lib.vgk_funnel_clusters, (self.h,), policy, reads, read_off, minimizer_off, minimizers, minimizer_score, cluster_off, cluster_seed_off,
                                       sources, rng_state, cap=cap)
        if rc != VGK_EOPS:
            self._check(rc, "vgk_funnel_clusters")
        return rc, out

    def funnel_extension_sets(self, policy, reads, read_off, set_off, results, extensions, kept_off, kept, cluster_seed_off, sources, minimizer_off, rng_state=None, cap=None):
        """vgk_funnel_extension_sets: per set estimate, verdict, rank, better_or_equal; per read the sets aligned, in that order, and the explored minimizers"""
        rc, out = funnel_extension_sets_call(self.lib.vgk_funnel_extension_sets, (self.h,), policy, reads, read_off, set_off, results, extensions, kept_off, kept,
                                             cluster_seed_off, sources, minimizer_off, rng_state, cap=cap)
        if rc != VGK_EOPS:
            self._check(rc, "vgk_funnel_extension_sets")
        return rc, out

    def funnel_winners(self, policy, reads, read_off, aligned_off, aln_off, aln_score, aln_mappings, rng_state=None, cap=None):
        """vgk_funnel_winners: per read every kept score in the winner walk's order, where each came from, how many are mappings, and whether the read is unmapped"""
        rc, out = funnel_winners_call(self.lib.vgk_funnel_winners, (self.h,), policy, reads, read_off, aligned_off, aln_off, aln_score, aln_mappings, rng_state, cap=cap)
        if rc != VGK_EOPS:
            self._check(rc, "vgk_funnel_winners")
        return rc, out

    def funnel_limits(self):
        """-> what a lane keeps in LDS: (minimizers of a read, bases of a read, items of a walk, extensions of a set)"""
        out = (ctypes.c_uint32 * 4)()
        self._check(self.lib.vgk_funnel_limits(out), "vgk_funnel_limits")
        return tuple(int(x) for x in out)

    def funnel_last_ms(self):
        """device time of the last funnel_clusters | funnel_extension_sets | funnel_winners call in ms"""
        ms = (ctypes.c_double * 3)()
        self.lib.vgk_funnel_last_ms.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.vgk_funnel_last_ms(self.h, ms), "vgk_funnel_last_ms")
        return tuple(float(x) for x in ms)

    def funnel_last_launches(self):
        """reads of the last funnel call: (everything in LDS, something over the slab, refused by the checks)"""
        reads = (ctypes.c_uint64 * 3)()
        self.lib.vgk_funnel_last_launches.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.vgk_funnel_last_launches(self.h, reads), "vgk_funnel_last_launches")
        return tuple(int(x) for x in reads)

    def chain_links(self, scheme, reads, read_off, anchor_off, anchors, sites, items, dist_off, dist, chains, caps=None, want_seqs=True):
        """vgk_chain_links (include/vgk_engine.h): per chain its links (mode, route, end points, slice of the read, graph distance), its kept anchors and their
        score.  scheme: a ChainLinksScheme; anchors CHAIN_ANCHOR_DT with sites CHAIN_SITE_DT beside them; items as vgk_chain_items leaves them; dist
        CHAIN_CANDIDATE_DT ascending by (from, to) per set; chains CHAIN_PROBLEM_DT -> (rc, dict), rc VGK_OK or VGK_EOPS"""
        rc, out = chain_links_call(self.lib.vgk_chain_links, (self.h,), scheme, reads, read_off, anchor_off, anchors, sites, items, dist_off, dist, chains, caps=caps, want_seqs=want_seqs)
        if rc != VGK_EOPS:
            self._check(rc, "vgk_chain_links")
        return rc, out

    def chain_links_last_ms(self):
        """device time of the last chain_links call in ms: checks + walk | counts, prefix sums and write-out | sequences"""
        ms = (ctypes.c_double * 3)()
        self.lib.vgk_chain_links_last_ms.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.vgk_chain_links_last_ms(self.h, ms), "vgk_chain_links_last_ms")
        return tuple(float(x) for x in ms)

    def pick_mappings(self, scheme, reads, read_off, chain_off, chains, aln_off, alns, mappings, edits, rng_state=None, cap=None):
        """vgk_pick_mappings (include/vgk_engine.h): per read the alignments picked as mappings or counted beyond the cut, their scores and multiplicities in walk
        order, the unmapped flag; per alignment identity, unique fraction and fate.  scheme: a PickScheme; chains PICK_CHAIN_DT; alns PICK_ALIGNMENT_DT over
        mappings CHAIN_MAPPING_DT and edit runs as vgk_chain_stitch leaves them -> (rc, dict), rc VGK_OK or VGK_EOPS"""
        rc, out = pick_mappings_call(self.lib.vgk_pick_mappings, (self.h,), scheme, reads, read_off, chain_off, chains, aln_off, alns, mappings, edits, rng_state=rng_state, cap=cap)
        if rc != VGK_EOPS:
            self._check(rc, "vgk_pick_mappings")
        return rc, out

    def pick_mappings_last_ms(self):
        """device time of the last pick_mappings call in ms: checks | statistics | multiplicities and sort scores | the pick"""
        ms = (ctypes.c_double * 4)()
        self.lib.vgk_pick_mappings_last_ms.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.vgk_pick_mappings_last_ms(self.h, ms), "vgk_pick_mappings_last_ms")
        return tuple(float(x) for x in ms)

    def pick_mappings_last_launches(self):
        """reads of the last pick_mappings call by where the pick ran: in LDS | over the slab | refused by the checks"""
        reads = (ctypes.c_uint64 * 3)()
        self.lib.vgk_pick_mappings_last_launches.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.vgk_pick_mappings_last_launches(self.h, reads), "vgk_pick_mappings_last_launches")
        return tuple(int(x) for x in reads)

    def pick_mappings_limits(self):
        """(nodes in the LDS table, its slots, alignments whose order lies in LDS, lanes per read)"""
        out = (ctypes.c_uint32 * 4)()
        self.lib.vgk_pick_mappings_limits.argtypes = [ctypes.c_void_p]
        self._check(self.lib.vgk_pick_mappings_limits(out), "vgk_pick_mappings_limits")
        return tuple(int(x) for x in out)

    def pair_mapq(self, scheme, cand_off, candidates, counts, **rest):
        """vgk_pair_mapq (include/vgk_engine.h): per pair both mates' mapping qualities from its candidate pairings — pair scores, their order, the caps both
        mates share.  scheme: a PairMapqScheme; rest: pair_mapq_call's optional arrays (unpaired_off, unpaired_scores; given_cap, or the sweep's minimizer_off,
        minimizers, regions, explored, read_off, quality) -> (PAIR_MAPQ_RESULT_DT per pair, pair_score per candidate, order per candidate)"""
        rc, out, pair_score, order = pair_mapq_call(self.lib.vgk_pair_mapq, (self.h,), scheme, cand_off, candidates, counts, **rest)
        self._check(rc, "vgk_pair_mapq")
        return out, pair_score, order

    def pair_mapq_limits(self):
        """-> (candidates of a pair ordered in LDS, lanes per pair, lanes per candidate in the score kernel, 0)"""
        out = (ctypes.c_uint32 * 4)()
        self._check(self.lib.vgk_pair_mapq_limits(out), "vgk_pair_mapq_limits")
        return tuple(int(x) for x in out)

    def pair_mapq_last_ms(self):
        """device time of the last pair_mapq call in ms: the mates' sweep | the score and pair kernels"""
        ms = (ctypes.c_double * 2)()
        self.lib.vgk_pair_mapq_last_ms.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.vgk_pair_mapq_last_ms(self.h, ms), "vgk_pair_mapq_last_ms")
        return tuple(float(x) for x in ms)

    def pair_mapq_last_launches(self):
        """pairs of the last pair_mapq call: (in LDS, over the slab, refused by the checks)"""
        pairs = (ctypes.c_uint64 * 3)()
        self.lib.vgk_pair_mapq_last_launches.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.vgk_pair_mapq_last_launches(self.h, pairs), "vgk_pair_mapq_last_launches")
        return tuple(int(x) for x in pairs)

    def pair_mapq_last_kernel_launches(self):
        """kernels the last pair_mapq call launched: (the mates' sweep, the score and pair kernels)"""
        out = (ctypes.c_uint32 * 2)()
        self.lib.vgk_pair_mapq_last_kernel_launches.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.vgk_pair_mapq_last_kernel_launches(self.h, out), "vgk_pair_mapq_last_kernel_launches")
        return tuple(int(x) for x in out)

    def minimizer_last_ms(self):
        self.lib.vgk_minimizer_last_ms.restype = ctypes.c_double; self.lib.vgk_minimizer_last_ms.argtypes = [ctypes.c_void_p]
        return self.lib.vgk_minimizer_last_ms(self.h)

    def tail_forest(self, index, problems):
        """vgk_tail_forest: problems = numpy array of TAIL_DT (search state node / lo / hi, cut offset, walk distance) or a list of
        such tuples.  -> (results as TAIL_RESULT_DT, Forest)"""
        pr = np.ascontiguousarray(problems, dtype=TAIL_DT) if isinstance(problems, np.ndarray) else np.array([tuple(p) for p in problems], dtype=TAIL_DT)
        res = np.zeros(max(len(pr), 1), dtype=TAIL_RESULT_DT)
        h = ctypes.c_void_p()
        self.lib.vgk_tail_forest.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.vgk_tail_forest(self.h, index.h, pr.ctypes.data, len(pr), res.ctypes.data, ctypes.byref(h)), "vgk_tail_forest")
        return res[:len(pr)], Forest(self, h)

    def tail_stage(self, index, n_reads, n_ext, ops_per_problem=32):
        """vgk_tail_stage over the sets the last gapless_extend / gapless_extend_seeded call left on the device
        -> (ext_total [n_ext], read_score [n_reads], (tails, trees, tree nodes, declined))"""
        ext_total = self._out("ts_ext", max(n_ext, 1), np.int32); read_score = self._out("ts_read", max(n_reads, 1), np.int32); stats = np.zeros(4, dtype=np.uint64)
        self.lib.vgk_tail_stage.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.vgk_tail_stage(self.h, index.h, ops_per_problem, ext_total.ctypes.data, len(ext_total), read_score.ctypes.data, stats.ctypes.data), "vgk_tail_stage")
        return ext_total[:n_ext], read_score[:n_reads], tuple(int(x) for x in stats)

    def tail_stage_aligned(self, index, n_reads, n_ext, ops_per_problem=32):
        """vgk_tail_stage_aligned -> (ext_total, read_score, tails as TAIL_ALIGNMENT_DT, ops as OP_DT, stats)"""
        ext_total = self._out("ts_ext", max(n_ext, 1), np.int32); read_score = self._out("ts_read", max(n_reads, 1), np.int32); stats = np.zeros(4, dtype=np.uint64)
        tails_cap = 2 * max(n_ext, 1)
        tails = self._out("ts_tails", tails_cap, TAIL_ALIGNMENT_DT); ops = self._out("ts_ops", tails_cap * ops_per_problem + 1, OP_DT)
        written = (ctypes.c_size_t * 2)()
        self.lib.vgk_tail_stage_aligned.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.vgk_tail_stage_aligned(self.h, index.h, ops_per_problem, ext_total.ctypes.data, len(ext_total), read_score.ctypes.data,
                                                    tails.ctypes.data, tails_cap, ops.ctypes.data, len(ops), ctypes.byref(written), stats.ctypes.data), "vgk_tail_stage_aligned")
        return ext_total[:n_ext], read_score[:n_reads], tails[:written[0]], ops[:written[1]], tuple(int(x) for x in stats)

    def tail_stage_last_ms(self):
        self.lib.vgk_tail_stage_last_ms.restype = ctypes.c_double; self.lib.vgk_tail_stage_last_ms.argtypes = [ctypes.c_void_p, ctypes.c_int]
        return [self.lib.vgk_tail_stage_last_ms(self.h, k) for k in range(4)]

    def tail_last_ms(self):
        self.lib.vgk_tail_last_ms.restype = ctypes.c_double; self.lib.vgk_tail_last_ms.argtypes = [ctypes.c_void_p]
        return self.lib.vgk_tail_last_ms(self.h)

    def gapless_extend_seeded(self, index, n_reads, n_seeds, max_mismatches=4, overlap_threshold=0.8, trim=True, read_len=150, defer=False):
        """vgk_gapless_extend_seeded: extend the clusters the last minimizer_seeds call left on the device -> as gapless_extend.
        defer (VGK_GAPLESS_DEFER): the arrays come back sized but are FILLED only when the next tail_stage / tail_stage_aligned call (or
        gapless_fetch_deferred) returns"""
        res = self._out("gs_res", max(n_reads, 1), GAPLESS_RESULT_DT)
        ext_cap = n_seeds + 1; node_cap = n_seeds * 16 + 1024; mism_cap = n_seeds * 12 + 1024
        ext = self._out("gs_ext", ext_cap, EXT_DT); nodes = self._out("gs_nodes", node_cap, np.uint32); mism = self._out("gs_mism", mism_cap, np.uint32)
        written = (ctypes.c_size_t * 3)()
        self.lib.vgk_gapless_extend_seeded.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_double, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                                       ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        self._check(self.lib.vgk_gapless_extend_seeded(self.h, index.h, max_mismatches, overlap_threshold, (VGK_GAPLESS_TRIM if trim else 0) | (VGK_GAPLESS_DEFER if defer else 0), res.ctypes.data,
                                                       ext.ctypes.data, ext_cap, nodes.ctypes.data, node_cap, mism.ctypes.data, mism_cap, ctypes.byref(written)),
                    "vgk_gapless_extend_seeded")
        if defer:
            self._deferred_keep = (res, ext, nodes, mism)          # the engine still writes into them: alive until the deferral is finished
        return res[:n_reads], ext[:written[0]], nodes[:written[1]], mism[:written[2]]

    def gapless_fetch_deferred(self):
        self.lib.vgk_gapless_fetch_deferred.argtypes = [ctypes.c_void_p]
        self._check(self.lib.vgk_gapless_fetch_deferred(self.h), "vgk_gapless_fetch_deferred")

    def gapless_last_ms(self):
        return self.lib.vgk_gapless_last_ms(self.h)

    def gapless_last_redone(self):
        """seeds of the last extension call whose search branched on the merged-run index and ran again on the original one"""
        self.lib.vgk_gapless_last_redone.restype = ctypes.c_uint64; self.lib.vgk_gapless_last_redone.argtypes = [ctypes.c_void_p]
        return int(self.lib.vgk_gapless_last_redone(self.h))

    def gapless_last_retried(self):
        self.lib.vgk_gapless_last_retried.restype = ctypes.c_uint64
        self.lib.vgk_gapless_last_retried.argtypes = [ctypes.c_void_p]
        return self.lib.vgk_gapless_last_retried(self.h)

    def wfa_extend(self, index, problems, error_model=None):
        """problems: a WfaSet, or a list of dicts {seq, mode: "connect"|"suffix"|"prefix", from: (oriented node, offset),
        to: (oriented node, offset)}; error_model: four (per_base, min, max) rows or None for the reference's default.
        -> (results, paths, edits) as numpy arrays laid out like include/vgk.h."""
        ws = problems if isinstance(problems, WfaSet) else WfaSet.from_lists(problems)
        res = np.zeros(ws.n, dtype=WFA_RESULT_DT)
        paths = np.zeros(ws.path_cap, dtype=np.uint32); edits = np.zeros(ws.edit_cap, dtype=np.uint32)
        model = None
        if error_model is not None:
            model = np.zeros(4, dtype=WFA_EVENT_DT)
            for i, row in enumerate(error_model):
                model[i] = tuple(row)
        written = (ctypes.c_size_t * 2)()
        self._check(self.lib.vgk_wfa_extend(self.h, index.h, model.ctypes.data if model is not None else None, ws.array.ctypes.data, ws.n,
                                            res.ctypes.data, paths.ctypes.data, ws.path_cap, edits.ctypes.data, ws.edit_cap,
                                            ctypes.byref(written)), "vgk_wfa_extend")
        return res, paths[:written[0]], edits[:written[1]]

    def chain_stitch(self, index, pieces, piece_off, nodes=None, mappings=None, edits=None, mapping_cap=None, edit_cap=None):
        """vgk_chain_stitch: pieces (CHAIN_PIECE_DT; LINK pieces name results of the last wfa_extend on this engine with `index`), piece_off (n_reads + 1),
        the arrays ALIGNMENT / PATH pieces point into -> (results CHAIN_RESULT_DT, mappings CHAIN_MAPPING_DT, edits uint32: length << 2 | WFA_*).
        Without caps the call is made twice when the first guess is too small."""
        pieces = np.ascontiguousarray(pieces, dtype=CHAIN_PIECE_DT); piece_off = np.ascontiguousarray(piece_off, dtype=np.uint64)
        nodes = np.ascontiguousarray(nodes if nodes is not None else [], dtype=np.uint32)
        mappings = np.ascontiguousarray(mappings if mappings is not None else [], dtype=CHAIN_MAPPING_DT)
        edits = np.ascontiguousarray(edits if edits is not None else [], dtype=np.uint32)
        n = len(piece_off) - 1
        res = np.zeros(n, dtype=CHAIN_RESULT_DT)
        retry = mapping_cap is None and edit_cap is None
        mcap = mapping_cap if mapping_cap is not None else 4 * len(pieces) + len(nodes) + len(mappings) + 16
        ecap = edit_cap if edit_cap is not None else 4 * len(pieces) + len(nodes) + len(edits) + 16
        while True:
            om = np.zeros(mcap, dtype=CHAIN_MAPPING_DT); oe = np.zeros(ecap, dtype=np.uint32)
            written = (ctypes.c_size_t * 2)()
            rc = self.lib.vgk_chain_stitch(self.h, index.h, pieces.ctypes.data if len(pieces) else None, piece_off.ctypes.data, n, nodes.ctypes.data if len(nodes) else None, len(nodes),
                                           mappings.ctypes.data if len(mappings) else None, len(mappings), edits.ctypes.data if len(edits) else None, len(edits),
                                           res.ctypes.data, om.ctypes.data, mcap, oe.ctypes.data, ecap, ctypes.byref(written))
            if rc == VGK_EOPS and retry:
                mcap, ecap, retry = int(written[0]) + 1, int(written[1]) + 1, False
                continue
            if rc != VGK_EOPS:
                self._check(rc, "vgk_chain_stitch")
            return res, om[:min(written[0], mcap)], oe[:min(written[1], ecap)]

    def wfa_set_cost_hints(self, extra_bases):
        """vgk_wfa_set_cost_hints: per problem of the NEXT wfa_extend, bases to add to its length when the hand-out order is made (order only)"""
        a = np.ascontiguousarray(extra_bases, dtype=np.uint32)
        self.lib.vgk_wfa_set_cost_hints.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
        self._check(self.lib.vgk_wfa_set_cost_hints(self.h, a.ctypes.data, len(a)), "vgk_wfa_set_cost_hints")

    def wfa_set_point_budgets(self, connect_points, tail_points):
        self.lib.vgk_wfa_set_point_budgets.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
        self._check(self.lib.vgk_wfa_set_point_budgets(self.h, connect_points, tail_points), "vgk_wfa_set_point_budgets")

    def wfa_set_point_budget(self, points):
        """problems that store more than `points` wavefront points are declined (VGK_ETOOBIG) early; 0 = the kernel's table size"""
        self.lib.vgk_wfa_set_point_budget.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        self._check(self.lib.vgk_wfa_set_point_budget(self.h, points), "vgk_wfa_set_point_budget")

    def wfa_rerun(self):
        self._check(self.lib.vgk_wfa_rerun(self.h), "vgk_wfa_rerun")

    def wfa_last_ms(self):
        return self.lib.vgk_wfa_last_ms(self.h)

    def wfa_last_wave(self):
        """(ms of the first launch — the hybrid's pair when its kernels ran at once —, ms of the wavefront kernel when it followed the thread
        kernel, problems handed over / outgrown)"""
        self.lib.vgk_wfa_last_wave.restype = ctypes.c_double; self.lib.vgk_wfa_last_wave.argtypes = [ctypes.c_void_p, ctypes.c_int]
        return tuple(self.lib.vgk_wfa_last_wave(self.h, k) for k in range(3))


TAIL_DT = np.dtype([("node", "<u4"), ("lo", "<i4"), ("hi", "<i4"), ("offset", "<u4"), ("walk_distance", "<u4")])
TAIL_RESULT_DT = np.dtype([("status", "<i4"), ("first_node", "<u4"), ("n_nodes", "<u4"), ("n_trees", "<u4"), ("root_trim", "<u4"), ("bases", "<u4")])


class Forest:
    """vgk_forest: the tail forests of a batch of tails, resident in HBM; `.graph` is the forest as one ResidentGraph-like handle
    whose windows are the trees (usable with Engine.pack_windows / align_windows)."""

    class _Graph:
        def __init__(self, h):
            self.h = h

    def __init__(self, eng, h):
        self.eng = eng; self.h = h
        lib = eng.lib
        lib.vgk_forest_size.restype = ctypes.c_uint64; lib.vgk_forest_size.argtypes = [ctypes.c_void_p]
        lib.vgk_forest_graph.restype = ctypes.c_void_p; lib.vgk_forest_graph.argtypes = [ctypes.c_void_p]
        lib.vgk_forest_fetch.argtypes = [ctypes.c_void_p] * 4
        lib.vgk_forest_destroy.argtypes = [ctypes.c_void_p]; lib.vgk_forest_destroy.restype = None
        self.size = int(lib.vgk_forest_size(h))
        g = lib.vgk_forest_graph(h)
        self.graph = Forest._Graph(ctypes.c_void_p(g)) if g else None
        eng._indexes.add(self)

    def fetch(self):
        """-> (parent, node, length) per tree node: parent = index in the forest or -1, node = oriented node of the index"""
        parent = np.zeros(max(self.size, 1), dtype=np.int32); node = np.zeros(max(self.size, 1), dtype=np.uint32); length = np.zeros(max(self.size, 1), dtype=np.uint32)
        self.eng._check(self.eng.lib.vgk_forest_fetch(self.h, parent.ctypes.data, node.ctypes.data, length.ctypes.data), "vgk_forest_fetch")
        return parent[:self.size], node[:self.size], length[:self.size]

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.eng, "h", None):
                self.eng.lib.vgk_forest_destroy(self.h)
            self.h = None; self.graph = None

    __del__ = close


class MinimizerIndex:
    """vgk_minimizer_index: the (k, w)-minimizers of the haplotype threads with their graph positions, resident in HBM."""

    def __init__(self, eng, nodes, threads, k=29, w=11):
        self.eng = eng; self.k, self.w = k, w
        if isinstance(nodes, tuple):
            self._len = np.ascontiguousarray(nodes[0], dtype=np.uint32); self._seq = np.ascontiguousarray(nodes[1], dtype=np.uint8); nodes = self._len
        else:
            self._len = np.array([len(s) for s in nodes], dtype=np.uint32)
            self._seq = np.frombuffer("".join(nodes).encode(), dtype=np.uint8).copy()
        self._toff = np.concatenate([[0], np.cumsum([len(t) for t in threads])]).astype(np.uint32)
        self._tn = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.uint32) for t in threads]) if len(threads) and self._toff[-1] else np.zeros(1, np.uint32), dtype=np.uint32)
        d = Haplotypes(len(nodes), self._len.ctypes.data, self._seq.ctypes.data, len(threads), self._toff.ctypes.data, self._tn.ctypes.data)
        h = ctypes.c_void_p()
        eng.lib.vgk_minimizer_index_create.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
        eng._check(eng.lib.vgk_minimizer_index_create(eng.h, ctypes.byref(d), k, w, ctypes.byref(h)), "vgk_minimizer_index_create")
        self.h = h
        eng.lib.vgk_minimizer_index_keys.restype = ctypes.c_uint64; eng.lib.vgk_minimizer_index_keys.argtypes = [ctypes.c_void_p]
        self.keys = int(eng.lib.vgk_minimizer_index_keys(h))
        eng._indexes.add(self)

    def set_policy(self, hit_cap=10, hard_hit_cap=500, score_fraction=0.9, on=True, paired=False):
        """vgk_minimizer_set_policy: find_seeds' choice of minimizers (giraffe's short-read defaults) for the following minimizer_seeds calls;
        on=False: none"""
        class Policy(ctypes.Structure):
            _fields_ = [("hit_cap", ctypes.c_uint32), ("hard_hit_cap", ctypes.c_uint32), ("minimizer_score_fraction", ctypes.c_double), ("paired", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]
        self.eng.lib.vgk_minimizer_set_policy.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        p = Policy(hit_cap, hard_hit_cap, score_fraction, 1 if paired else 0, 0)
        self.eng._check(self.eng.lib.vgk_minimizer_set_policy(self.h, ctypes.byref(p) if on else None), "vgk_minimizer_set_policy")

    def fetch(self):
        """vgk_minimizer_index_fetch: every indexed occurrence as (key, oriented node, offset), sorted"""
        lib = self.eng.lib
        lib.vgk_minimizer_index_hits.restype = ctypes.c_uint64; lib.vgk_minimizer_index_hits.argtypes = [ctypes.c_void_p]
        n = int(lib.vgk_minimizer_index_hits(self.h))
        hits = np.zeros(max(n, 1), dtype=MINIMIZER_HIT_DT)
        lib.vgk_minimizer_index_fetch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        self.eng._check(lib.vgk_minimizer_index_fetch(self.h, hits.ctypes.data, n), "vgk_minimizer_index_fetch")
        return hits[:n]

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.eng, "h", None):
                self.eng.lib.vgk_minimizer_index_destroy.argtypes = [ctypes.c_void_p]; self.eng.lib.vgk_minimizer_index_destroy.restype = None
                self.eng.lib.vgk_minimizer_index_destroy(self.h)
            self.h = None

    __del__ = close


class ResidentGraph:
    """vgk_dgraph: one topologically ordered DAG kept in HBM; problems name windows (runs of consecutive nodes) of it."""

    def __init__(self, eng, node_len, seq, pred_off, pred_idx):
        self.eng = eng
        self.node_len = np.ascontiguousarray(node_len, dtype=np.uint32)
        self.seq = np.ascontiguousarray(seq, dtype=np.uint8)
        self.pred_off = np.ascontiguousarray(pred_off, dtype=np.uint32)
        self.pred_idx = np.ascontiguousarray(pred_idx if len(pred_idx) else np.zeros(1, np.uint32), dtype=np.uint32)
        self.col = np.concatenate([[0], np.cumsum(self.node_len, dtype=np.int64)])
        g = np.zeros(1, dtype=GRAPH_DT)
        g["n_nodes"] = len(self.node_len); g["node_len"] = self.node_len.ctypes.data; g["seq"] = self.seq.ctypes.data
        g["pred_off"] = self.pred_off.ctypes.data; g["pred_idx"] = self.pred_idx.ctypes.data
        h = ctypes.c_void_p()
        eng._check(eng.lib.vgk_graph_create(eng.h, g.ctypes.data, ctypes.byref(h)), "vgk_graph_create")
        self.h = h
        eng._indexes.add(self)

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.eng, "h", None):
                self.eng.lib.vgk_graph_destroy(self.h)
            self.h = None

    __del__ = close


class WindowSet:
    """A batch of window problems (vgk_window_problem): reads in one flat ASCII array, read i = reads[read_off[i]:read_off[i+1]],
    aligned against nodes [first_node[i], first_node[i] + n_nodes[i]) of a ResidentGraph."""

    def __init__(self, reads, read_off, first_node, n_nodes, flags, max_gap=None, cols=None):
        self.reads = np.ascontiguousarray(reads, dtype=np.uint8)
        self.read_off = np.asarray(read_off, dtype=np.int64)
        n = self.n = len(self.read_off) - 1
        arr = np.zeros(n, dtype=WINDOW_DT)
        arr["read_off"] = self.read_off[:-1]; arr["read_len"] = np.diff(self.read_off)
        arr["flags"] = flags; arr["first_node"] = first_node; arr["n_nodes"] = n_nodes
        if max_gap is not None:
            arr["max_gap_length"] = np.asarray(max_gap, dtype=np.uint32)
        self.array = arr
        self.cols = None if cols is None else np.asarray(cols, dtype=np.int64)      # graph bases per window (sizes the default op array)

    @property
    def seq_off(self):
        c = self.cols if self.cols is not None else np.zeros(self.n, dtype=np.int64)
        return np.concatenate([[0], np.cumsum(c)])


class ExtensionSet:
    """A batch of extension windows (vgk_extension_problem): one pass of a seeded X-drop alignment from a position inside a window."""

    def __init__(self, reads, read_off, first_node, n_nodes, flags, max_gap, start_node, start_offset, query_offset, leftward, cols=None):
        self.reads = np.ascontiguousarray(reads, dtype=np.uint8)
        self.read_off = np.asarray(read_off, dtype=np.int64)
        n = self.n = len(self.read_off) - 1
        arr = np.zeros(n, dtype=EXTENSION_DT)
        arr["read_off"] = self.read_off[:-1]; arr["read_len"] = np.diff(self.read_off)
        for k, v in (("flags", flags), ("first_node", first_node), ("n_nodes", n_nodes), ("max_gap_length", max_gap), ("start_node", start_node),
                     ("start_offset", start_offset), ("query_offset", query_offset), ("leftward", leftward)):
            arr[k] = np.asarray(v, dtype=np.uint32)
        self.array = arr
        self.cols = None if cols is None else np.asarray(cols, dtype=np.int64)

    @property
    def seq_off(self):
        c = self.cols if self.cols is not None else np.zeros(self.n, dtype=np.int64)
        return np.concatenate([[0], np.cumsum(c)])


class GaplessSet:
    """A batch of gapless-extension problems (vgk_gapless_problem) over shared numpy arenas."""

    def __init__(self, reads, read_off, seeds, seed_off, max_mismatches=4, overlap_threshold=0.8, trim=True, node_cap=None, mism_cap=None):
        self.reads = np.ascontiguousarray(reads, dtype=np.uint8)
        self.read_off = np.asarray(read_off, dtype=np.int64)
        self.seeds = np.ascontiguousarray(seeds, dtype=SEED_DT)
        self.seed_off = np.asarray(seed_off, dtype=np.int64)
        n = self.n = len(self.read_off) - 1
        arr = np.zeros(n, dtype=GAPLESS_DT)
        arr["read"] = self.reads.ctypes.data + self.read_off[:-1]
        arr["read_len"] = np.diff(self.read_off)
        arr["n_seeds"] = np.diff(self.seed_off)
        arr["seeds"] = self.seeds.ctypes.data + 8 * self.seed_off[:-1]
        arr["max_mismatches"] = max_mismatches
        arr["flags"] = np.where(np.broadcast_to(np.asarray(trim), (n,)), VGK_GAPLESS_TRIM, 0)
        arr["overlap_threshold"] = overlap_threshold
        self.array = arr
        rl = np.diff(self.read_off); ns = np.diff(self.seed_off)
        self.ext_cap = int(ns.sum()) + 1
        self.node_cap = int(node_cap if node_cap is not None else (ns * (rl + 2)).sum()) + 1
        self.mism_cap = int(mism_cap if mism_cap is not None else (ns * rl).sum()) + 1

    @classmethod
    def from_lists(cls, problems):
        reads = [np.frombuffer(p["read"].encode(), dtype=np.uint8) for p in problems]
        read_off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
        read_buf = np.concatenate(reads) if len(reads) and read_off[-1] else np.zeros(1, np.uint8)
        seed_off = np.concatenate([[0], np.cumsum([len(p["seeds"]) for p in problems])]).astype(np.int64)
        seeds = np.zeros(max(int(seed_off[-1]), 1), dtype=SEED_DT)
        k = 0
        for p in problems:
            for node, diff in p["seeds"]:
                seeds[k] = (node, diff); k += 1
        return cls(read_buf, read_off, seeds, seed_off, [p.get("max_mismatches", 4) for p in problems],
                   [p.get("overlap_threshold", 0.8) for p in problems], [p.get("trim", True) for p in problems])


class WfaSet:
    """A batch of WFA problems (vgk_wfa_problem) over one shared numpy arena of sequences."""

    def __init__(self, seqs, seq_off, mode, from_node, from_offset, to_node, to_offset, path_cap=None, edit_cap=None):
        self.seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        self.seq_off = np.asarray(seq_off, dtype=np.int64)
        n = self.n = len(self.seq_off) - 1
        arr = np.zeros(n, dtype=WFA_DT)
        arr["seq"] = self.seqs.ctypes.data + self.seq_off[:-1]
        arr["seq_len"] = np.diff(self.seq_off)
        arr["mode"] = mode
        arr["from_node"] = from_node; arr["from_offset"] = from_offset
        arr["to_node"] = to_node; arr["to_offset"] = to_offset
        self.array = arr
        sl = np.diff(self.seq_off)
        self.path_cap = int(path_cap if path_cap is not None else (4 * sl + 64).sum()) + 1
        self.edit_cap = int(edit_cap if edit_cap is not None else (2 * sl + 8).sum()) + 1

    @classmethod
    def from_lists(cls, problems):
        modes = {"connect": WFA_CONNECT, "suffix": WFA_SUFFIX, "prefix": WFA_PREFIX}
        seqs = [np.frombuffer(p["seq"].encode(), dtype=np.uint8) for p in problems]
        seq_off = np.concatenate([[0], np.cumsum([len(r) for r in seqs])]).astype(np.int64)
        buf = np.concatenate(seqs) if len(seqs) and seq_off[-1] else np.zeros(1, np.uint8)
        none = (WFA_NO_NODE, 0)
        return cls(buf, seq_off, [modes[p.get("mode", "connect")] for p in problems],
                   [(p.get("from") or none)[0] for p in problems], [(p.get("from") or none)[1] for p in problems],
                   [(p.get("to") or none)[0] for p in problems], [(p.get("to") or none)[1] for p in problems])


class HaploIndex:
    """The haplotype index the gapless extender walks (stands in for vg's GBWTGraph)."""

    def __init__(self, eng, nodes, threads=None, gbwt=None):
        """threads: [[oriented node]]; or gbwt: the bytes of a GBWT file (vgk_haplo_create_gbwt)"""
        self.eng = eng
        if isinstance(nodes, tuple):                                   # (node lengths, concatenated forward bases) as arrays: graphs with millions of nodes
            self.nodes = None
            self._len = np.ascontiguousarray(nodes[0], dtype=np.uint32); self._seq = np.ascontiguousarray(nodes[1], dtype=np.uint8)
            nodes = self._len
        else:
            self.nodes = list(nodes)
            self._len = np.array([len(s) for s in nodes], dtype=np.uint32)
            self._seq = np.frombuffer("".join(nodes).encode(), dtype=np.uint8).copy()
        if gbwt is not None:
            h = ctypes.c_void_p()
            eng.lib.vgk_haplo_create_gbwt.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
            eng._check(eng.lib.vgk_haplo_create_gbwt(eng.h, bytes(gbwt), len(gbwt), len(nodes), self._len.ctypes.data, self._seq.ctypes.data, ctypes.byref(h)),
                       "vgk_haplo_create_gbwt")
            self.h = h
            eng._indexes.add(self)
            return
        self._toff = np.concatenate([[0], np.cumsum([len(t) for t in threads])]).astype(np.uint32)
        self._tn = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.uint32) for t in threads]) if len(threads) and self._toff[-1] else np.zeros(1, np.uint32), dtype=np.uint32)
        d = Haplotypes(len(nodes), self._len.ctypes.data, self._seq.ctypes.data, len(threads), self._toff.ctypes.data, self._tn.ctypes.data)
        h = ctypes.c_void_p()
        eng._check(eng.lib.vgk_haplo_create(eng.h, ctypes.byref(d), ctypes.byref(h)), "vgk_haplo_create")
        self.h = h
        eng._indexes.add(self)

    def run_nodes(self):
        """nodes of the index's merged-run form, which the WFA wavefront kernel walks (= the graph's nodes when nothing merged)"""
        self.eng.lib.vgk_haplo_run_nodes.restype = ctypes.c_uint64; self.eng.lib.vgk_haplo_run_nodes.argtypes = [ctypes.c_void_p]
        return int(self.eng.lib.vgk_haplo_run_nodes(self.h))

    def search_nodes(self):
        """nodes of the index the gapless search walks (unary runs merged at build; = the graph's nodes when nothing merged)"""
        self.eng.lib.vgk_haplo_search_nodes.restype = ctypes.c_uint64; self.eng.lib.vgk_haplo_search_nodes.argtypes = [ctypes.c_void_p]
        return int(self.eng.lib.vgk_haplo_search_nodes(self.h))

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.eng, "h", None):
                self.eng.lib.vgk_haplo_destroy(self.h)
            self.h = None

    __del__ = close


class Batch:
    def __init__(self, eng, h, ps, ops_per_problem):
        self.eng, self.h, self.ps, self.ops_per = eng, h, ps, ops_per_problem

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()

    def free(self):
        if self.h:
            self.eng.lib.vgk_batch_free(self.h); self.h = None

    def run(self):
        self.eng._check(self.eng.lib.vgk_gssw_run(self.h), "vgk_gssw_run")

    def sync(self):
        self.eng._check(self.eng.lib.vgk_batch_sync(self.h), "vgk_batch_sync")

    def kernel_ms(self, which=-1):
        return self.eng.lib.vgk_batch_kernel_ms(self.h, which)

    def cells(self):
        return self.eng.lib.vgk_batch_cells(self.h)

    def alg_bytes(self):
        return self.eng.lib.vgk_batch_alg_bytes(self.h)

    def device_bytes(self):
        return self.eng.lib.vgk_batch_device_bytes(self.h)

    def lane(self):
        """launch lane (stream) of this batch: consecutive batches of a context alternate between two"""
        self.eng.lib.vgk_batch_lane.argtypes = [ctypes.c_void_p]
        return self.eng.lib.vgk_batch_lane(self.h)

    def wave_steps(self):
        return self.eng.lib.vgk_batch_wave_steps(self.h)

    def refill_stats(self):
        """the last speculative run's second fill, read back from the device: dict of `waves` filled a second time, their `steps` summed,
        `missed` reads, `bounded` (missed reads whose second fill began right of column 0) and `broken` (walks that asked for a code
        left of where their read's fill began: always 0).  All 0 when the last run did not speculate.  Engine library only."""
        f = self.eng.lib.vgk_batch_refill_stats
        f.restype = ctypes.c_int; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        out = (ctypes.c_uint64 * 5)()
        self.eng._check(f(self.h, out), "vgk_batch_refill_stats")
        return dict(zip(("waves", "steps", "missed", "bounded", "broken"), (int(v) for v in out)))

    def row_offset(self):
        """the constant (times the score scale) that the rows of this batch's speculative first fill carry in their offset form; 0 when the
        batch does not speculate or that fill runs the saturating rows.  Engine library only."""
        f = self.eng.lib.vgk_batch_row_offset
        f.restype = ctypes.c_uint32; f.argtypes = [ctypes.c_void_p]
        return int(f(self.h))

    def speculated(self):
        """did the last run fill without traceback codes first (the speculative fill; the context's feedback decides per run)"""
        self.eng.lib.vgk_batch_speculated.argtypes = [ctypes.c_void_p]
        return bool(self.eng.lib.vgk_batch_speculated(self.h))

    def fetch(self, into=None):
        """-> (results, ops).  `into` = (results, ops) arrays of an earlier fetch of a batch of the same shape, written again
        (a streaming caller keeps its output buffers; fresh numpy arrays cost a page fault per 4 KB touched)."""
        n = self.ps.n
        if self.ops_per:
            cap = n * self.ops_per
        else:
            cap = int(np.diff(self.ps.read_off).sum() + np.diff(self.ps.seq_off).sum() + 2 * n)
        if into is not None:
            res, ops = into[0], (into[1].base if into[1].base is not None else into[1])
            assert len(res) == n and len(ops) >= max(cap, 1)
        else:
            res = np.zeros(n, dtype=RESULT_DT)
            ops = np.zeros(max(cap, 1), dtype=OP_DT)
        written = ctypes.c_size_t()
        self.eng._check(self.eng.lib.vgk_gssw_fetch(self.h, res.ctypes.data, ops.ctypes.data, cap, ctypes.byref(written)),
                        "vgk_gssw_fetch")
        return res, ops[:written.value]


def cigar_string(res_row, ops):
    """'offset@node:3M1D,node:...' for debugging / comparison."""
    o = ops[res_row["ops_begin"]:res_row["ops_begin"] + res_row["n_ops"]]
    parts, cur = [], None
    for e in o:
        if cur != e["node"]:
            parts.append("%d:" % e["node"]); cur = e["node"]
        parts[-1] += "%d%s" % (e["len"], OP_CHARS[e["op"]])
    return "%d@%s" % (res_row["first_offset"], ",".join(parts))
