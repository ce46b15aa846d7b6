// scratch_slots.hpp — who owns which of the context's cached device buffers (vgk_ctx::scratch, ctx.hpp).  One enumerator per buffer, grouped by
// the C-ABI file that uses it and numbered by the compiler: a family that needs another buffer adds a name to its group.  Two names share a
// buffer only through the aliases behind SLOT_COUNT.  "Never aliased": a later call reads what these slots hold through the ctx-> record named.
#pragma once

enum Slot : int {
    // ---- banded_api.cpp.  Never aliased: banded_last (vgk_banded_rerun) points into set 0 and BANDED_SCORES.
    // Two sub-batches in flight: a buffer is BANDED<set>_PROBS + S_*, the file's own index enum (a static_assert there ties the runs to it)
    BANDED0_PROBS, BANDED0_ORDER, BANDED0_NODES, BANDED0_SEEDS, BANDED0_POOL, BANDED0_STARTS, BANDED0_READS, BANDED0_QUALS, BANDED0_GRAPH, BANDED0_MAT,
    BANDED0_TB, BANDED0_LAST, BANDED0_OPS, BANDED0_DENSE, BANDED0_RESULTS, BANDED0_END,
    BANDED1_PROBS = BANDED0_END, BANDED1_ORDER, BANDED1_NODES, BANDED1_SEEDS, BANDED1_POOL, BANDED1_STARTS, BANDED1_READS, BANDED1_QUALS, BANDED1_GRAPH, BANDED1_MAT,
    BANDED1_TB, BANDED1_LAST, BANDED1_OPS, BANDED1_DENSE, BANDED1_RESULTS, BANDED1_END,
    BANDED_SCORES = BANDED1_END,       // k-best mode: the full score matrices
    // the device-geometry path's raw arrays, per sub-batch in flight: BGEOM<set>_PROBS + G_*
    BGEOM0_PROBS, BGEOM0_NODELEN, BGEOM0_PREDOFF, BGEOM0_PREDIDX, BGEOM0_TMP, BGEOM0_OUT, BGEOM0_END,
    BGEOM1_PROBS = BGEOM0_END, BGEOM1_NODELEN, BGEOM1_PREDOFF, BGEOM1_PREDIDX, BGEOM1_TMP, BGEOM1_OUT, BGEOM1_END,
    BKBEST_SUMS = BGEOM1_END, BKBEST_PRES, BKBEST_POPS,      // the k-best walk on the device: what it does not share (BKBEST_* aliases below)
    // ---- gapless_api.cpp.  Never aliased: ctx->sets (vgk_tail_stage reads the descriptors, the masked reads and the ordered sets here) and
    // gapless_last (vgk_gapless_rerun).  Both entry points use one name per purpose; the seeded one leaves READS and SEEDS alone.
    GAPLESS_SCRATCH, GAPLESS_COLD, GAPLESS_PROBS, GAPLESS_READS, GAPLESS_SEEDS, GAPLESS_SORT, GAPLESS_RESULTS, GAPLESS_EXT, GAPLESS_NODES, GAPLESS_MISM,
    GAPLESS_COUNTERS, GAPLESS_WINNERS, GAPLESS_RETRY, GAPLESS_TAB, GAPLESS_RES_OUT, GAPLESS_EXT_OUT, GAPLESS_NODES_OUT, GAPLESS_READ_OF,
    // ---- wfa_api.cpp.  Never aliased: ctx->wfa_out (vgk_chain_stitch's LINK pieces read results, paths and edit runs here), wfa_last and
    // wfa_wave_last (vgk_wfa_rerun).  WFA_RAW, WFA_SRC_OFF: the sequences as the caller holds them, their offsets
    WFA_SCRATCH, WFA_PROBS, WFA_SEQS, WFA_ORDER, WFA_RESULTS, WFA_PATHS, WFA_EDITS, WFA_COUNTERS,
    WFA_HANDED_OVER, WFA_SLABS, WFA_DECLINED, WFA_STATS, WFA_PRODUCERS_DONE, WFA_RAW, WFA_SRC_OFF,
    // ---- gssw_multi_api.cpp (the k-best pinned path; nothing stays for a later call): the matrices' inputs, then the walk on the device
    MULTI_PROBS, MULTI_READS, MULTI_QUALS, MULTI_GRAPH, MULTI_NODES, MULTI_PREDS, MULTI_MAT, MULTI_CELLS,
    MULTI_PINNING, MULTI_POOL, MULTI_ORDER, MULTI_RESULTS, MULTI_N_ALIGNMENTS, MULTI_STATUS, MULTI_OPS, MULTI_OPS_OFF, MULTI_OFFS, MULTI_SUMS, MULTI_PRES, MULTI_POPS,
    // ---- xdrop_band_api.cpp (nothing stays).  Two sub-batches in flight: set 0 is the XBAND0_* aliases below plus these three, set 1 the run
    // XBAND1_PROBS + D_*, the file's own index enum (a static_assert there ties both sets to it)
    XBAND0_FMAX, XBAND0_STATS, XBAND0_FRONT,
    XBAND1_PROBS, XBAND1_READS, XBAND1_QUALS, XBAND1_GRAPH, XBAND1_NODES, XBAND1_PREDS, XBAND1_MAT, XBAND1_CELLS, XBAND1_FMAX, XBAND1_STATS, XBAND1_FRONT,
    XBAND1_ORDER, XBAND1_RES, XBAND1_OPS, XBAND1_OPSOFF, XBAND1_WANT, XBAND1_OFFS, XBAND1_SUMS, XBAND1_PRES, XBAND1_POPS, XBAND1_END,
    // ---- tail_api.cpp: the forest's per-call tables (the forest itself is owned by its graph)
    TAIL_PROBS = XBAND1_END, TAIL_RES, TAIL_COUNTS, TAIL_SCRATCH, TAIL_TMP,
    // ---- minimizer_api.cpp.  Never aliased: ctx->seeded (vgk_gapless_extend_seeded takes reads, offsets and seeds from the SEEDED_* slots, and
    // ctx->sets.reads then points there too).  MZLIST_*: vgk_minimizer_list and vgk_minimizer_seeds_of (nothing stays)
    SEEDED_READS, SEEDED_READ_OFF, SEEDED_TAB, SEEDED_SEEDS,
    MZLIST_READS, MZLIST_READ_OFF, MZLIST_TAB, MZLIST_ITEMS, MZLIST_MINIMIZERS, MZLIST_TAKE, MZLIST_SEED_TAB, MZLIST_SEEDS,
    // vgk_minimizer_choose / vgk_minimizer_find_seeds (nothing stays): they work on the MZLIST_* buffers — the reads, the list, MZLIST_TAKE for the
    // verdicts — plus the minimizers' offsets per read, the score table, the reads of a launch and the slab of the reads too large for LDS
    MZCHOOSE_MIN_OFF, MZCHOOSE_TAB, MZCHOOSE_IDS, MZCHOOSE_SLAB,
    // ---- gssw_wide_api.cpp, chain_api.cpp (nothing stays)
    WIDE_PROBS, WIDE_ORDER, WIDE_COLINFO, WIDE_PROF, WIDE_NODES, WIDE_PREDS, WIDE_SCRATCH, WIDE_CARRY, WIDE_TB, WIDE_BEST, WIDE_RESULTS, WIDE_OPS,
    CHAIN_UP, CHAIN_TAB, CHAIN_RES, CHAIN_WORK_M, CHAIN_WORK_E, CHAIN_OUT_M, CHAIN_OUT_E,
    // ---- chain_items_api.cpp (nothing stays): the problems and their inputs, the jump tables, the launch's problem numbers; per candidate the
    // indel; per anchor the group counts, their prefix sums and the scatter's cursors; the groups; the error flag; the table and the outputs; the slabs
    CITEMS_PROBS, CITEMS_CAND_OFF, CITEMS_ANCHORS, CITEMS_CANDS, CITEMS_JUMP, CITEMS_IDS, CITEMS_INDEL, CITEMS_COUNT, CITEMS_FIRST, CITEMS_CURSOR, CITEMS_GROUPED,
    CITEMS_FLAGS, CITEMS_TSCORE, CITEMS_TSOURCE, CITEMS_CHAINS, CITEMS_NCHAINS, CITEMS_ITEMS, CITEMS_REC_RIGHT, CITEMS_REC_LEFT, CITEMS_SLAB,
    // ---- extension_anchors_api.cpp (nothing stays): the problems and their inputs (seeds, extensions, path nodes, mismatches, the problem of each
    // extension), the launch's problem numbers; per seed its anchor and its place in the diagonal order; per extension the number of seeds it contains,
    // the prefix sums, the lists; the error flag; the anchors as made and sorted with their origins, the represented seeds, the per-problem counts; the slabs
    EANCH_PROBS, EANCH_SEEDS, EANCH_EXT, EANCH_NODES, EANCH_MISM, EANCH_PROB_OF_EXT, EANCH_IDS, EANCH_SEED_ANCHOR, EANCH_SORTED, EANCH_EXT_COUNT, EANCH_EXT_FIRST,
    EANCH_EXT_SEEDS, EANCH_FLAGS, EANCH_MADE, EANCH_MADE_ORIGIN, EANCH_ANCHORS, EANCH_ORIGINS, EANCH_REP, EANCH_N_ANCHORS, EANCH_N_REP, EANCH_STATUS, EANCH_SLAB,
    // ---- read_alignments_api.cpp (nothing stays): the reads and their inputs (offsets, gapless results, extensions, path nodes, mismatches, tails, ops, the
    // tails of each extension, the validation's verdicts), the launches' reads and the large sets' slab; per read the choice and the alignments it has,
    // their prefix sums; per alignment the mappings and edit runs it has, their prefix sums and 64-bit totals; the headers, mappings and edit runs
    READALN_READS, READALN_READ_OFF, READALN_RES, READALN_EXT, READALN_NODES, READALN_MISM, READALN_TAILS, READALN_OPS, READALN_TAIL_OF, READALN_STATUS,
    READALN_IDS, READALN_WORK_OFF, READALN_WORK, READALN_CHOICE, READALN_ALN_COUNT, READALN_ALN_FIRST, READALN_MAP_COUNT, READALN_EDIT_COUNT,
    READALN_MAP_FIRST, READALN_EDIT_FIRST, READALN_OUT, READALN_MAPPINGS, READALN_EDITS, READALN_TOTALS,
    // ---- read_mapq_api.cpp.  Never aliased: ctx->mapq_tables (the two probability tables go up once per context and stay in READMAPQ_TABLES).  The
    // rest is per call: offsets of reads, scores and minimizers; the scores, multiplicities and unmapped bytes; the list, its regions, the explored
    // bytes and the qualities; the checks' verdicts, the launches' reads, the large reads' slices and their slab; the 24-byte results
    READMAPQ_TABLES, READMAPQ_READ_OFF, READMAPQ_SCORE_OFF, READMAPQ_MIN_OFF, READMAPQ_SCORES, READMAPQ_MULT, READMAPQ_UNMAPPED, READMAPQ_MINS, READMAPQ_REGIONS,
    READMAPQ_EXPLORED, READMAPQ_QUAL, READMAPQ_STATUS, READMAPQ_IDS, READMAPQ_WORK_OFF, READMAPQ_WORK, READMAPQ_OUT,
    // ---- pair_mapq_api.cpp (nothing stays).  Without given caps the mates' sweep runs over the READMAPQ_* inputs above (the two calls never overlap
    // under the context lock) and leaves every read's cap and verdict in PAIRMAPQ_CAPS / PAIRMAPQ_CAP_STATUS for the pair kernels; given caps go up
    // into PAIRMAPQ_CAPS.  The rest: the pairs' offsets, candidates and counts, the mates' unpaired scores, the checks' verdicts, the launches' pairs,
    // the large pairs' slices and their slab; per candidate its pair score and its place in the order; the 80-byte results
    PAIRMAPQ_CAND_OFF, PAIRMAPQ_CANDS, PAIRMAPQ_COUNTS, PAIRMAPQ_UNP_OFF, PAIRMAPQ_UNP_SCORES, PAIRMAPQ_CAPS, PAIRMAPQ_CAP_STATUS, PAIRMAPQ_STATUS, PAIRMAPQ_IDS,
    PAIRMAPQ_WORK_OFF, PAIRMAPQ_WORK, PAIRMAPQ_SCORE, PAIRMAPQ_ORDER, PAIRMAPQ_OUT,
    // ---- read_funnel_api.cpp (nothing stays): the reads, their offsets and generators, the checks' verdicts; the minimizers' offsets, list and scores; the
    // clusters' offsets, seed offsets and sources; the kept clusters, the sets' results and extensions; the aligned sets' offsets, the alignments' offsets,
    // scores and mapping counts, the winner walk's flat lists; the per-item outputs; a walk's accepted items, their counts and prefix sums, the two laid-out
    // outputs; the scoring launches' items, slices and slab, and the walk launches'
    FUNNEL_READS, FUNNEL_READ_OFF, FUNNEL_RNG, FUNNEL_STATUS, FUNNEL_MIN_OFF, FUNNEL_MINS, FUNNEL_MIN_SCORE, FUNNEL_CLUSTER_OFF, FUNNEL_SEED_OFF, FUNNEL_SOURCES,
    FUNNEL_KEPT_OFF, FUNNEL_KEPT, FUNNEL_RES, FUNNEL_EXT, FUNNEL_ALIGNED_OFF, FUNNEL_ALN_OFF, FUNNEL_ALN_SCORE, FUNNEL_ALN_MAPPINGS, FUNNEL_FLAT_OFF, FUNNEL_FLAT_SCORE,
    FUNNEL_FLAT_PICK, FUNNEL_SORTED_SCORE, FUNNEL_SORTED_PICK, FUNNEL_CLUSTERS, FUNNEL_SETS, FUNNEL_EXPLORED, FUNNEL_N_REPORTED, FUNNEL_UNMAPPED, FUNNEL_TMP, FUNNEL_COUNT,
    FUNNEL_FIRST, FUNNEL_OUT0, FUNNEL_OUT1, FUNNEL_IDS, FUNNEL_WORK_OFF, FUNNEL_WORK, FUNNEL_WALK_IDS, FUNNEL_WALK_WORK_OFF, FUNNEL_WALK_WORK,
    // ---- chain_links_api.cpp (nothing stays): the reads and their offsets; the sets' offsets, anchors, sites and the item array; the distances and their
    // offsets; the chains and their first item slots; a set's verdict, the kept bytes and the route bytes (one block, zeroed together); the three counts per
    // link slot, their prefix sums, the 64-bit totals; the results, links, kept anchors, sequence offsets and sequences on their way back
    CHAINLINKS_READS, CHAINLINKS_READ_OFF, CHAINLINKS_ANCHOR_OFF, CHAINLINKS_ANCHORS, CHAINLINKS_SITES, CHAINLINKS_ITEMS, CHAINLINKS_DIST_OFF, CHAINLINKS_DIST,
    CHAINLINKS_CHAINS, CHAINLINKS_SLOT_OFF, CHAINLINKS_BYTES, CHAINLINKS_COUNT, CHAINLINKS_FIRST, CHAINLINKS_TOTALS, CHAINLINKS_RES, CHAINLINKS_LINKS,
    CHAINLINKS_KEPT, CHAINLINKS_SEQ_OFF, CHAINLINKS_SEQS,
    // ---- pick_mappings_api.cpp (nothing stays): the reads, their offsets and generators; the chains and alignments with their offsets; the mappings and
    // edit runs; an alignment's first mapping slot; a slot's from_length, an alignment's two sums, multiplicity and sort score; the results and verdicts;
    // the picked alignments, scores and multiplicities on their way back; the pick's reads and its slab
    PICK_READS, PICK_READ_OFF, PICK_RNG, PICK_CHAIN_OFF, PICK_CHAINS, PICK_ALN_OFF, PICK_ALNS, PICK_MAPPINGS, PICK_EDITS, PICK_SLOT_OFF, PICK_FROM_LEN, PICK_SUMS,
    PICK_ALN_MULT, PICK_ALN_SORT, PICK_RES, PICK_VERDICTS, PICK_PICKED, PICK_SCORES, PICK_OUT_MULT, PICK_IDS, PICK_SLAB,
    // ---- gssw_wide_window_api.cpp (nothing stays): the call's problems, reads and verdicts; a sub-batch's windows, per-node temporaries, sizes, their
    // sums, the order's keys; the results and ops packed for the way back.  The arenas the wide kernels read are the WIDE_* buffers (aliases below)
    WIDEWIN_PROBLEMS, WIDEWIN_READS, WIDEWIN_META, WIDEWIN_SUB, WIDEWIN_STORE, WIDEWIN_NODE_FLAGS, WIDEWIN_SLOT_AT, WIDEWIN_PRED_AT, WIDEWIN_WIN_SLOTS,
    WIDEWIN_SIZES, WIDEWIN_OFFS, WIDEWIN_KEY, WIDEWIN_IDX, WIDEWIN_KEY_SORTED, WIDEWIN_IDX_SORTED, WIDEWIN_KEY2, WIDEWIN_OPS_OFFS, WIDEWIN_OPS_SUMS,
    WIDEWIN_RES_OUT, WIDEWIN_OPS_OUT,
    SLOT_COUNT,                        // sizes vgk_ctx::scratch; only aliases follow

    // ---- deliberate sharing: a second name for a buffer above, so that a context which uses both paths keeps one set of buffers in HBM.
    // Safe for both: the two calls never overlap under the context lock (vgk_ctx::mu), and neither leaves state behind for a later call.
    // xdrop set 0 over the k-best pinned path's buffers
    XBAND0_PROBS = MULTI_PROBS, XBAND0_READS = MULTI_READS, XBAND0_QUALS = MULTI_QUALS, XBAND0_GRAPH = MULTI_GRAPH, XBAND0_NODES = MULTI_NODES,
    XBAND0_PREDS = MULTI_PREDS, XBAND0_MAT = MULTI_MAT, XBAND0_CELLS = MULTI_CELLS, XBAND0_ORDER = MULTI_OFFS, XBAND0_RES = MULTI_PINNING,
    XBAND0_OPS = MULTI_POOL, XBAND0_OPSOFF = MULTI_ORDER, XBAND0_WANT = MULTI_RESULTS, XBAND0_OFFS = MULTI_N_ALIGNMENTS, XBAND0_SUMS = MULTI_STATUS,
    XBAND0_PRES = MULTI_OPS, XBAND0_POPS = MULTI_OPS_OFF,
    // the banded k-best walk over the gssw k-best walk's buffers
    BKBEST_POOL = MULTI_PINNING, BKBEST_ORDER = MULTI_POOL, BKBEST_SP_OFF = MULTI_ORDER, BKBEST_SP_LEN = MULTI_RESULTS, BKBEST_PREFIX = MULTI_N_ALIGNMENTS,
    BKBEST_HOST_ONLY = MULTI_STATUS, BKBEST_RESULTS = MULTI_OPS, BKBEST_N_ALIGNMENTS = MULTI_OPS_OFF, BKBEST_OPS = MULTI_OFFS, BKBEST_OPS_OFF = MULTI_SUMS,
    BKBEST_STATUS = MULTI_PRES, BKBEST_OFFS = MULTI_POPS,
    // the wide window route over the wide route's arenas: both feed the same kernels
    WIDEWIN_PROBS = WIDE_PROBS, WIDEWIN_ORDER = WIDE_ORDER, WIDEWIN_COLINFO = WIDE_COLINFO, WIDEWIN_PROF = WIDE_PROF, WIDEWIN_NODES = WIDE_NODES,
    WIDEWIN_PREDS = WIDE_PREDS, WIDEWIN_SCRATCH = WIDE_SCRATCH, WIDEWIN_CARRY = WIDE_CARRY, WIDEWIN_TB = WIDE_TB, WIDEWIN_BEST = WIDE_BEST,
    WIDEWIN_RESULTS = WIDE_RESULTS, WIDEWIN_OPS = WIDE_OPS,
};
constexpr Slot operator+(Slot base, int k) { return (Slot)((int)base + k); }      // a buffer of a run: its first name + the family's index
