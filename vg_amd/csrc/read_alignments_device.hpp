// read_alignments_device.hpp — giraffe's alignments of a short read from its extension set and the tails' alignments (vgk_read_alignments,
// include/vgk_engine.h): what MinimizerMapper::map_from_extensions makes of a set at src/minimizer_mapper.cpp:934-1000.  The lane code of the kernels in
// backend_hip.hip, and ra_read_one: the same rule stated serially, what the kernels are checked against without a GPU
// (tests/emu/read_alignments_driver.cpp).
//
// The rule, piece by piece:
//   ra_frontier      find_pareto_frontier (:5266-5283): sort by (cost ascending, value descending), the scan, the final sort by (value, cost)
//   ra_flank         flank_penalty (:5301-5311) over gap_penalty (:5286, :5296) and mismatch_penalty (:5291)
//   ra_select_one    a full-length set: the leading extensions that are full on both sides (:939-969).  Any other set: min_tails (:5376-5384), the
//                    frontiers (:5397-5419), the extensions by score descending — a stable sort: the reference shuffles the tie at the top with the
//                    read's generator [PARITY-UNPINNED], here ties stay in extension order —, process_until_threshold_e
//                    (src/minimizer_mapper.hpp:1580-1659; `unskipped` counts the items the estimate drops too, the lambda returns true there), the
//                    estimate's skip (:5463-5479), the totals and the replace rules (:5545-5590) with node id = (oriented node >> 1) + 1
//   ra_extension     GaplessExtension::to_path (src/gbwt_extender.cpp:119-156)
//   ra_tail          a tail's Path as get_best_alignment_against_any_tree returns it (:5626-5743): the soft clip at the default position, or the ops
//                    grouped by node as GSSWAligner::ops_to_alignment groups them, M runs re-split by comparing bases; a left tail comes out flipped
//                    (reverse_complement_path, src/path.cpp:1863-1882) by walking groups, ops and bases from the last to the first
//   RaOut::begin     add_to_path (:5318-5367)
//   RaOut::finish    identity(path) (src/path.cpp:2316-2335) as numerator and denominator
//
// MI355X-first: a lane per read.  The selection is serial by nature (every step depends on the winner so far) and cheap; its working arrays — the
// order and both frontiers, 9 n + 4 words for n extensions — lie in LDS at an odd stride for sets of up to RA_LDS_EXT extensions,
// larger sets run in a second launch over a slab in HBM that only their lane touches, so that no wavefront of the first
// launch waits on a large set.  Count and emit run the one composer twice, first counting, then writing at the prefix sums: the sizes are exact.
#pragma once
#include <cstdint>
#include "../../include/vgk_engine.h"
#include "pk16.hpp"

namespace vgk {

constexpr uint32_t RA_NONE = 0xffffffffu;
constexpr uint32_t RA_LDS_EXT = 6;                      // a set within it is selected in LDS
constexpr uint32_t RA_LDS_STRIDE = 59;                  // words per lane there: 9 * 6 + 4 = 58, odd so that the 64 lanes' slices start in different banks
VGK_HD uint64_t ra_work_words(uint64_t n_ext) { return 9u * n_ext + 4u; }      // order [n] | left frontier 2 (2 n + 1) | right frontier 2 (2 n + 1)

struct RaChoice { uint32_t ext[2]; int32_t score[2]; };          // a set that is not full-length: BEST and SECOND (extension within the set, RA_NONE = empty)

struct RaParams {
    int32_t match, mismatch, gap_open, gap_extend, bonus;
    uint32_t threshold, max_local, window_length;
    uint32_t n_reads, n_oriented;
    const uint64_t* node_tab; const char* seq;      // the index: per oriented node the offset of its bases in `seq` (low word) | its length (high word)
    const char* reads; const uint64_t* read_off;
    const uint32_t* prob_words; uint32_t prob_stride;      // the resident form instead of read_off: read r begins at prob_words[r * stride] and has prob_words[r * stride + 1] bases
    const vgk_gapless_result* res; const vgk_extension* ext; const uint32_t* nodes; const uint32_t* mism;
    const vgk_tail_alignment* tails; const vgk_op* ops;
    const uint32_t* tail_of;                        // [2 * extensions] the right | left tail of an extension (RA_NONE: none given)
    uint32_t* tail_of_out; uint32_t n_tails;        // ... made on the device from the tails (RA_RUN_TAILS; the table filled with RA_NONE before)
    const int32_t* status;                          // [n_reads] what the validation found; nullptr: the gapless results' own status (the engine's own sets)
    unsigned long long* totals;                     // [2] mappings and edit runs of all alignments in 64 bits: what the count adds up beside the 32-bit prefix sums
    const uint32_t* ids; uint32_t n;                // the reads of a selection launch
    const uint64_t* work_off; uint32_t* work;       // ... over the slab: where a read's working words begin (work nullptr: LDS; work_off nullptr: 9 ext_begin + 4 r)
    RaChoice* choice; uint32_t* aln_count; const uint32_t* aln_first;      // [n_reads] | [n_reads + 1] alignments per read, their exclusive prefix sums
    uint32_t* map_count; uint32_t* edit_count; const uint32_t* map_first; const uint32_t* edit_first;      // [alignments + 1]
    vgk_read_alignment* out; vgk_chain_mapping* mappings; uint32_t* edits;
};
enum { RA_RUN_SELECT = 0, RA_RUN_COUNT = 1, RA_RUN_EMIT = 2, RA_RUN_TAILS = 3 };      // Backend::run_read_alignments' stages

VGK_HD uint32_t ra_len(const RaParams& P, uint32_t o) { return (uint32_t)(P.node_tab[o] >> 32); }
VGK_HD char ra_node_base(const RaParams& P, uint32_t o, uint32_t at) { return P.seq[(uint32_t)P.node_tab[o] + at]; }
VGK_HD const char* ra_read(const RaParams& P, uint32_t r, uint32_t& length) {
    if (P.prob_words) { length = P.prob_words[(uint64_t)r * P.prob_stride + 1]; return P.reads + P.prob_words[(uint64_t)r * P.prob_stride]; }
    length = (uint32_t)(P.read_off[r + 1] - P.read_off[r]); return P.reads + P.read_off[r];
}
VGK_HD int32_t ra_status(const RaParams& P, uint32_t r) { return P.status ? P.status[r] : P.res[r].status; }
#if defined(__HIP_DEVICE_COMPILE__)
VGK_HD void ra_add64(unsigned long long* p, unsigned long long v) { atomicAdd(p, v); }
#else
VGK_HD void ra_add64(unsigned long long* p, unsigned long long v) { *p += v; }
#endif
VGK_HD bool ra_full(const vgk_extension& e) { return e.left_full && e.right_full; }
VGK_HD int32_t ra_gap(const RaParams& P, uint32_t length) { return length == 0 ? 0 : P.gap_open + (int32_t)(length - 1) * P.gap_extend; }
VGK_HD int32_t ra_gap_between(const RaParams& P, uint32_t start, uint32_t limit) { return start >= limit ? P.gap_open : P.gap_open + (int32_t)(limit - start - 1) * P.gap_extend; }
VGK_HD int32_t ra_mismatches(const RaParams& P, uint32_t n) { return (int32_t)n * (P.match + P.mismatch); }

// find_pareto_frontier over n points (value, cost) at pts[2 i], pts[2 i + 1]; -> the points left
VGK_HD uint32_t ra_frontier(uint32_t* pts, uint32_t n) {
    if (!n) return 0;
    for (uint32_t i = 1; i < n; ++i) {                              // (cost ascending, value descending)
        const uint32_t v = pts[2 * i]; const int32_t c = (int32_t)pts[2 * i + 1];
        uint32_t j = i;
        for (; j > 0; --j) {
            const uint32_t pv = pts[2 * j - 2]; const int32_t pc = (int32_t)pts[2 * j - 1];
            if (!(c < pc || (c == pc && v > pv))) break;
            pts[2 * j] = pv; pts[2 * j + 1] = (uint32_t)pc;
        }
        pts[2 * j] = v; pts[2 * j + 1] = (uint32_t)c;
    }
    uint32_t tail = 1;
    for (uint32_t i = 1; i < n; ++i) {
        if (pts[2 * i] <= pts[2 * tail - 2]) continue;
        pts[2 * tail] = pts[2 * i]; pts[2 * tail + 1] = pts[2 * i + 1];
        ++tail;
    }
    for (uint32_t i = 1; i < tail; ++i) {                           // (value, cost) ascending
        const uint32_t v = pts[2 * i]; const int32_t c = (int32_t)pts[2 * i + 1];
        uint32_t j = i;
        for (; j > 0; --j) {
            const uint32_t pv = pts[2 * j - 2]; const int32_t pc = (int32_t)pts[2 * j - 1];
            if (!(v < pv || (v == pv && c < pc))) break;
            pts[2 * j] = pv; pts[2 * j + 1] = (uint32_t)pc;
        }
        pts[2 * j] = v; pts[2 * j + 1] = (uint32_t)c;
    }
    return tail;
}

VGK_HD int32_t ra_flank(const RaParams& P, uint32_t length, const uint32_t* pts, uint32_t n) {
    int32_t result = ra_gap(P, length);
    for (uint32_t i = 0; i < n; ++i) {
        const int32_t candidate = (int32_t)pts[2 * i + 1] + ra_gap_between(P, pts[2 * i], length);
        result = candidate < result ? candidate : result;
        if (pts[2 * i] >= length) break;
    }
    return result;
}

// the tail of extension x (number in the call) on one side: its record, or nullptr for the soft clip
VGK_HD const vgk_tail_alignment* ra_tail_of(const RaParams& P, uint32_t x, uint32_t left) {
    const uint32_t t = P.tail_of[2 * (uint64_t)x + left];
    if (t == RA_NONE) return nullptr;
    const vgk_tail_alignment* a = P.tails + t;
    return a->n_ops ? a : nullptr;
}
// node ids of an alignment's first and last mapping (:5545-5556): the tail's outermost mapping where there is one, the extension's end otherwise
VGK_HD uint32_t ra_end_id(const RaParams& P, const vgk_extension& e, uint32_t x, uint32_t left) {
    const uint32_t own = left ? P.nodes[e.path_begin] : P.nodes[e.path_begin + e.path_len - 1];
    const vgk_tail_alignment* t = (left ? e.left_full : e.right_full) ? nullptr : ra_tail_of(P, x, left);
    const uint32_t o = t ? P.ops[t->ops_begin + t->n_ops - 1].node : own;      // (a left tail's ops run outwards: its last op is the path's first mapping)
    return (o >> 1) + 1u;
}

// The alignments of read r: how many, and for a set that is not full-length which extensions.  work: 9 n + 4 words, stride 1.
VGK_HD void ra_select_one(const RaParams& P, uint32_t r, uint32_t* work) {
    RaChoice ch; ch.ext[0] = ch.ext[1] = RA_NONE; ch.score[0] = ch.score[1] = 0;
    const vgk_gapless_result g = P.res[r];
    if (ra_status(P, r) != VGK_OK) { P.choice[r] = ch; P.aln_count[r] = 1; return; }
    const vgk_extension* e = P.ext + g.ext_begin; const uint32_t n = g.n_ext;
    if (g.full_length) {
        uint32_t k = 0;
        while (k < n && ra_full(e[k])) ++k;
        P.choice[r] = ch; P.aln_count[r] = k; return;
    }
    uint32_t L; ra_read(P, r, L);
    uint32_t min_tails = 1;
    for (uint32_t x = 0; x < n; ++x) if (ra_full(e[x])) ++min_tails;
    if (min_tails < 2) min_tails = 2;
    uint32_t* order = work; uint32_t* lf = work + n; uint32_t* rf = lf + 2u * (2u * n + 1u);
    uint32_t nl = 0, nr = 0;
    for (uint32_t x = 0; x < n; ++x) {
        if (ra_full(e[x])) continue;
        const int32_t left_penalty = ra_gap(P, e[x].read_begin), mid_penalty = ra_mismatches(P, e[x].n_mismatches), right_penalty = ra_gap(P, L - e[x].read_end);
        lf[2 * nl] = e[x].read_end; lf[2 * nl + 1] = (uint32_t)(mid_penalty + left_penalty); ++nl;
        rf[2 * nr] = L - e[x].read_begin; rf[2 * nr + 1] = (uint32_t)(mid_penalty + right_penalty); ++nr;
        if (e[x].n_mismatches) {
            lf[2 * nl] = P.mism[e[x].mism_begin]; lf[2 * nl + 1] = (uint32_t)left_penalty; ++nl;
            rf[2 * nr] = L - P.mism[e[x].mism_begin + e[x].n_mismatches - 1] - 1u; rf[2 * nr + 1] = (uint32_t)right_penalty; ++nr;
        }
    }
    lf[2 * nl] = P.window_length - 1u; lf[2 * nl + 1] = 0; ++nl;
    rf[2 * nr] = P.window_length - 1u; rf[2 * nr + 1] = 0; ++nr;
    nl = ra_frontier(lf, nl); nr = ra_frontier(rf, nr);
    for (uint32_t x = 0; x < n; ++x) {                              // score descending, ties in extension order
        uint32_t j = x;
        for (; j > 0 && e[order[j - 1]].score < e[x].score; --j) order[j] = order[j - 1];
        order[j] = x;
    }
    const int64_t cutoff = n ? (int64_t)e[order[0]].score - (int64_t)P.threshold : 0;
    uint32_t unskipped = 0, w_start = 0, w_end = 0;
    bool partial_aligned = false; int32_t threshold = -1;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t x = order[i]; const vgk_extension& ex = e[x];
        if (P.threshold != 0 && (int64_t)ex.score <= cutoff) { if (!(unskipped < min_tails)) continue; }
        else if (!(unskipped < P.max_local || P.max_local == 0xffffffffu)) continue;
        ++unskipped;
        if (threshold < 0) threshold = (int32_t)((uint32_t)ex.score - P.threshold);
        if (!ra_full(ex)) {
            if (partial_aligned && ex.score <= threshold) {
                int32_t estimate = (int32_t)L * P.match + 2 * P.bonus - ra_mismatches(P, ex.n_mismatches);
                if (!ex.left_full) estimate -= ra_flank(P, ex.read_begin, lf, nl);
                if (!ex.right_full) estimate -= ra_flank(P, L - ex.read_end, rf, nr);
                if (estimate <= ch.score[0]) continue;
            }
            partial_aligned = true;
        }
        const vgk_tail_alignment* lt = ex.left_full ? nullptr : ra_tail_of(P, g.ext_begin + x, 1);
        const vgk_tail_alignment* rt = ex.right_full ? nullptr : ra_tail_of(P, g.ext_begin + x, 0);
        const int32_t total = ex.score + (lt ? lt->score : 0) + (rt ? rt->score : 0);
        const uint32_t winning_start = ch.score[0] == 0 ? 0u : w_start, winning_end = ch.score[0] == 0 ? 0u : w_end;
        const uint32_t current_start = ra_end_id(P, ex, g.ext_begin + x, 1), current_end = ra_end_id(P, ex, g.ext_begin + x, 0);
        const bool different = winning_start != current_start && winning_end != current_end;
        if (total > ch.score[0] || ch.score[0] == 0) {
            if (ch.score[0] != 0 && different) { ch.score[1] = ch.score[0]; ch.ext[1] = ch.ext[0]; }
            ch.score[0] = total; ch.ext[0] = x; w_start = current_start; w_end = current_end;
        } else if ((total > ch.score[1] || ch.score[1] == 0) && different) { ch.score[1] = total; ch.ext[1] = x; }
    }
    P.choice[r] = ch; P.aln_count[r] = 2;
}

// One alignment under construction: mappings and edits counted, and written when there is room to write to (maps != nullptr)
struct RaOut {
    vgk_chain_mapping* maps; uint32_t* edits;
    uint32_t n_maps = 0, n_edits = 0, from_length = 0, to_length = 0, matched = 0;
    uint32_t cur_first = 0;                 // the open mapping's first edit (kind, RA_NONE while it has none)
    uint32_t cur_node = 0, cur_edits = 0, cur_begin = 0;
    uint32_t first_edit = 0, last_edit = 0;
    VGK_HD RaOut(vgk_chain_mapping* m, uint32_t* e) : maps(m), edits(e) {}
    VGK_HD bool cur_total_insertion() const { return cur_edits == 1 && cur_first == VGK_WFA_INSERTION; }
    // add_to_path for a mapping at (node, offset) that `total_insertion` describes; joined = false: the mapping is taken as it is (the left tail's)
    VGK_HD void begin(uint32_t node, uint32_t offset, bool total_insertion, bool joined) {
        if (joined && n_maps && (node >> 1) == (cur_node >> 1)) {
            bool combine = false;
            if (offset != 0) combine = true;
            else if (cur_total_insertion() || total_insertion) {
                combine = true;
                if (cur_total_insertion()) { cur_node = node; if (maps) { maps[n_maps - 1].node = node; maps[n_maps - 1].offset = offset; } }
            }
            if (combine) return;
        }
        if (maps) { maps[n_maps].node = node; maps[n_maps].offset = offset; maps[n_maps].edit_begin = n_edits; maps[n_maps].n_edits = 0; }
        ++n_maps; cur_node = node; cur_edits = 0; cur_first = RA_NONE; cur_begin = n_edits;
    }
    VGK_HD void edit(uint32_t kind, uint32_t length) {
        if (!length) return;
        const uint32_t word = length << 2 | kind;
        if (edits) edits[n_edits] = word;
        if (!n_edits) first_edit = word;
        last_edit = word;
        if (!cur_edits) cur_first = kind;
        ++cur_edits; ++n_edits;
        if (maps) maps[n_maps - 1].n_edits = cur_edits;
        if (kind != VGK_WFA_INSERTION) from_length += length;
        if (kind != VGK_WFA_DELETION) to_length += length;
        if (kind == VGK_WFA_MATCH) matched += length;
    }
    // identity(path): matched / (read bases - the insertion that is the very first edit - the one that is the very last)
    VGK_HD void identity(uint32_t& num, uint32_t& den) const {
        uint32_t total = to_length;
        if (n_edits && (first_edit & 3u) == VGK_WFA_INSERTION) total -= first_edit >> 2;
        if (n_edits > 1 && (last_edit & 3u) == VGK_WFA_INSERTION) total -= last_edit >> 2;
        num = total ? matched : 0u; den = total;
    }
};

// GaplessExtension::to_path
VGK_HD void ra_extension(const RaParams& P, const vgk_extension& e, RaOut& out) {
    uint32_t m = 0, read_offset = e.read_begin, node_offset = e.offset;
    for (uint32_t i = 0; i < e.path_len; ++i) {
        const uint32_t node = P.nodes[e.path_begin + i];
        const uint64_t reach = (uint64_t)read_offset + ra_len(P, node) - node_offset;
        const uint32_t limit = reach < e.read_end ? (uint32_t)reach : e.read_end;
        out.begin(node, node_offset, false, true);
        while (m < e.n_mismatches && P.mism[e.mism_begin + m] < limit) {
            const uint32_t at = P.mism[e.mism_begin + m];
            out.edit(VGK_WFA_MATCH, at - read_offset);
            out.edit(VGK_WFA_MISMATCH, 1);
            read_offset = at + 1; ++m;
        }
        out.edit(VGK_WFA_MATCH, limit - read_offset);
        read_offset = limit; node_offset = 0;
    }
}

VGK_HD bool ra_acgt(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
VGK_HD char ra_complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N'; }
// base q of the sequence a tail was aligned as: the read's bases behind the extension, or the reverse complement of those before it.  0: never matches
VGK_HD char ra_tail_base(const char* read, const vgk_tail_alignment& t, uint32_t q) {
    const char c = t.left ? read[t.read_end - 1u - q] : read[t.read_begin + q];
    if (!ra_acgt(c)) return 0;
    return t.left ? ra_complement(c) : c;
}
// Group `want` of a tail's ops: ops [i, j) on one visit of a node, beginning at offset `from` of it and at base `q` of the tail's sequence, spending
// `from_len` bases of the node.  A visit ends where the node changes, or where its bases are spent and an M or D op follows.  false: there is none
struct RaGroup { uint32_t i, j, from, q, from_len, node; };
VGK_HD bool ra_group(const RaParams& P, const vgk_tail_alignment& t, uint32_t want, RaGroup& g) {
    const vgk_op* ops = P.ops + t.ops_begin;
    uint32_t i = 0, q = 0, from = t.first_offset;
    for (uint32_t at = 0; i < t.n_ops; ++at) {
        const uint32_t node = ops[i].node, node_len = ra_len(P, node);
        uint32_t j = i, pos = from, q_end = q;
        while (j < t.n_ops && ops[j].node == node) {
            const uint32_t op = ops[j].op;
            if (j > i && pos >= node_len && (op == VGK_OP_M || op == VGK_OP_D)) break;
            if (op == VGK_OP_M || op == VGK_OP_D) pos += ops[j].len;
            if (op != VGK_OP_D) q_end += ops[j].len;
            ++j;
        }
        if (at == want) { g.i = i; g.j = j; g.from = from; g.q = q; g.from_len = pos - from; g.node = node; return true; }
        i = j; q = q_end; from = 0;
    }
    return false;
}
VGK_HD uint32_t ra_groups(const RaParams& P, const vgk_tail_alignment& t) {
    RaGroup g{}; uint32_t n = 0;
    while (ra_group(P, t, n, g)) ++n;
    return n;
}
// One tail's Path onto `out`.  e: its extension; t: its alignment (nullptr: the soft clip); [begin, end): the tail's read bases.
VGK_HD void ra_tail(const RaParams& P, const char* read, const vgk_extension& e, const vgk_tail_alignment* t, uint32_t left, uint32_t begin, uint32_t end, RaOut& out) {
    if (begin >= end) return;
    if (!t) {
        uint32_t node = P.nodes[e.path_begin], offset = e.offset;
        if (!left) {
            uint64_t tail_offset = (uint64_t)e.offset + (e.read_end - e.read_begin);
            for (uint32_t i = 0; i + 1 < e.path_len; ++i) tail_offset -= ra_len(P, P.nodes[e.path_begin + i]);
            node = P.nodes[e.path_begin + e.path_len - 1]; offset = (uint32_t)tail_offset;
        }
        out.begin(node, offset, true, !left);
        out.edit(VGK_WFA_INSERTION, end - begin);
        return;
    }
    const vgk_op* ops = P.ops + t->ops_begin;
    const uint32_t n_groups = ra_groups(P, *t);
    for (uint32_t k = 0; k < n_groups; ++k) {
        RaGroup g{};
        ra_group(P, *t, left ? n_groups - 1u - k : k, g);
        const bool total_insertion = g.j - g.i == 1 && (ops[g.i].op == VGK_OP_I || ops[g.i].op == VGK_OP_S);
        if (left) out.begin(g.node ^ 1u, ra_len(P, g.node) - (g.from + g.from_len), total_insertion, false);
        else out.begin(g.node, g.from, total_insertion, true);
        // where the group ends, for the walk from its last op to its first
        uint32_t pos = g.from, q = g.q;
        if (left) for (uint32_t o = g.i; o < g.j; ++o) { if (ops[o].op == VGK_OP_M || ops[o].op == VGK_OP_D) pos += ops[o].len; if (ops[o].op != VGK_OP_D) q += ops[o].len; }
        for (uint32_t kk = 0; kk < g.j - g.i; ++kk) {
            const vgk_op op = left ? ops[g.j - 1u - kk] : ops[g.i + kk];
            const uint32_t len = op.len;
            if (op.op == VGK_OP_M) {
                if (left) { pos -= len; q -= len; }
                uint32_t run = 0;
                for (uint32_t s = 0; s < len; ++s) {
                    const uint32_t at = left ? len - 1u - s : s;
                    const char c = ra_tail_base(read, *t, q + at);
                    if (c && c == ra_node_base(P, g.node, pos + at)) { ++run; continue; }
                    out.edit(VGK_WFA_MATCH, run); run = 0;
                    out.edit(VGK_WFA_MISMATCH, 1);
                }
                out.edit(VGK_WFA_MATCH, run);
                if (!left) { pos += len; q += len; }
            } else if (op.op == VGK_OP_D) {
                out.edit(VGK_WFA_DELETION, len);
                if (left) pos -= len; else pos += len;
            } else {
                out.edit(VGK_WFA_INSERTION, len);
                if (left) q -= len; else q += len;
            }
        }
    }
}

// alignment k of read r: counted (mappings == nullptr), or written with its header at P.out[a]
VGK_HD void ra_compose(const RaParams& P, uint32_t r, uint32_t k, uint32_t a, bool write) {
    const vgk_gapless_result g = P.res[r];
    uint32_t L; const char* read = ra_read(P, r, L);
    const int32_t status = ra_status(P, r);
    vgk_read_alignment h;
    h.status = status; h.mapping_begin = write ? P.map_first[a] : 0u; h.edit_begin = write ? P.edit_first[a] : 0u;
    h.n_mappings = h.n_edits = h.from_length = h.to_length = 0; h.read = r; h.kind = VGK_READ_ALN_DIRECT; h.extension = RA_NONE; h.score = 0;
    h.identity_num = h.identity_den = 0; h.reserved = 0;
    RaOut out(write ? P.mappings + h.mapping_begin : nullptr, write ? P.edits + h.edit_begin : nullptr);
    if (status == VGK_OK) {
        uint32_t x = k;
        if (!g.full_length) { h.kind = k ? VGK_READ_ALN_SECOND : VGK_READ_ALN_BEST; x = P.choice[r].ext[k]; h.score = P.choice[r].score[k]; }
        if (x != RA_NONE) {
            const vgk_extension& e = P.ext[g.ext_begin + x];
            h.extension = g.ext_begin + x;
            if (g.full_length) {
                ra_extension(P, e, out);
                h.score = e.score; h.identity_num = L - e.n_mismatches; h.identity_den = L;
            } else {
                if (!e.left_full) ra_tail(P, read, e, ra_tail_of(P, h.extension, 1), 1, 0, e.read_begin, out);
                ra_extension(P, e, out);
                if (!e.right_full) ra_tail(P, read, e, ra_tail_of(P, h.extension, 0), 0, e.read_end, L, out);
                out.identity(h.identity_num, h.identity_den);
            }
        }
    }
    if (write) {
        // (the edits' offsets count from the alignment's first edit while it is made; the caller's arrays hold all alignments behind each other)
        for (uint32_t m = 0; m < out.n_maps; ++m) P.mappings[h.mapping_begin + m].edit_begin += h.edit_begin;
        h.n_mappings = out.n_maps; h.n_edits = out.n_edits; h.from_length = out.from_length; h.to_length = out.to_length;
        P.out[a] = h;
    } else { P.map_count[a] = out.n_maps; P.edit_count[a] = out.n_edits; if (P.totals) { ra_add64(P.totals, out.n_maps); ra_add64(P.totals + 1, out.n_edits); } }
}
// One stage of the call for read r — what a lane does, and all there is to the serial statement.  work: the selection's working words
VGK_HD void ra_read_one(const RaParams& P, int what, uint32_t r, uint32_t* work) {
    if (what == RA_RUN_SELECT) { ra_select_one(P, r, work); return; }
    if (what == RA_RUN_TAILS) { P.tail_of_out[2 * (uint64_t)P.tails[r].ext + P.tails[r].left] = r; return; }      // (r: a tail)
    const uint32_t a0 = P.aln_first[r], n = P.aln_first[r + 1] - a0;
    for (uint32_t k = 0; k < n; ++k) ra_compose(P, r, k, a0 + k, what == RA_RUN_EMIT);
}

// ---- what the call checks per read before any lane sees it (read_alignments_api.cpp, and the serial driver): VGK_OK, the gapless result's own
// status, or VGK_EINVAL.  tail_of as in RaParams; a slot holding RA_NONE - 1 marks an end that two tails claim.
constexpr uint32_t RA_TWICE = RA_NONE - 1u;
// tail_of [2 * n_ext] from the tails; false: a tail names an extension the call does not have, or a side that is neither 0 nor 1
inline bool ra_tail_table(const vgk_tail_alignment* tails, uint64_t n_tails, uint64_t n_ext, uint32_t* tail_of) {
    for (uint64_t k = 0; k < 2 * n_ext; ++k) tail_of[k] = RA_NONE;
    for (uint64_t t = 0; t < n_tails; ++t) {
        if (tails[t].ext >= n_ext || tails[t].left > 1u) return false;
        uint32_t& slot = tail_of[2 * (uint64_t)tails[t].ext + tails[t].left];
        slot = slot == RA_NONE ? (uint32_t)t : RA_TWICE;
    }
    return true;
}
inline int32_t ra_validate_read(const RaParams& P, uint32_t r, uint64_t n_ext, uint64_t n_nodes, uint64_t n_mism, uint64_t n_ops) {
    const vgk_gapless_result g = P.res[r];
    if (g.status != VGK_OK) return g.status;
    if ((uint64_t)g.ext_begin + g.n_ext > n_ext) return VGK_EINVAL;
    const uint64_t L = P.read_off[r + 1] - P.read_off[r];
    for (uint32_t x = 0; x < g.n_ext; ++x) {
        const vgk_extension& e = P.ext[g.ext_begin + x];
        if (!e.path_len || (uint64_t)e.path_begin + e.path_len > n_nodes || (uint64_t)e.mism_begin + e.n_mismatches > n_mism) return VGK_EINVAL;
        if (e.read_begin >= e.read_end || e.read_end > L) return VGK_EINVAL;
        uint64_t bases = 0;
        for (uint32_t i = 0; i < e.path_len; ++i) {
            const uint32_t o = P.nodes[e.path_begin + i];
            if (o >= P.n_oriented) return VGK_EINVAL;
            if (i + 1 < e.path_len) bases += ra_len(P, o);
        }
        const uint64_t span = (uint64_t)e.offset + (e.read_end - e.read_begin);
        if (e.offset >= ra_len(P, P.nodes[e.path_begin]) || span <= bases || span - bases > ra_len(P, P.nodes[e.path_begin + e.path_len - 1])) return VGK_EINVAL;
        for (uint32_t i = 0; i < e.n_mismatches; ++i) {
            const uint32_t m = P.mism[e.mism_begin + i];
            if (m < e.read_begin || m >= e.read_end || (i && m <= P.mism[e.mism_begin + i - 1])) return VGK_EINVAL;
        }
        if ((e.left_full != 0) != (e.read_begin == 0) || (e.right_full != 0) != (e.read_end == L)) return VGK_EINVAL;
        for (uint32_t left = 0; left < 2; ++left) {
            const uint32_t ti = P.tail_of[2 * ((uint64_t)g.ext_begin + x) + left];
            if (ti == RA_NONE) continue;
            if (ti == RA_TWICE || (left ? e.left_full : e.right_full)) return VGK_EINVAL;
            const vgk_tail_alignment& t = P.tails[ti];
            if (t.read_begin != (left ? 0u : e.read_end) || t.read_end != (left ? e.read_begin : (uint32_t)L)) return VGK_EINVAL;
            if ((uint64_t)t.ops_begin + t.n_ops > n_ops) return VGK_EINVAL;
            uint64_t read_bases = 0, pos = t.first_offset;
            for (uint32_t k = 0; k < t.n_ops; ++k) {
                const vgk_op& op = P.ops[t.ops_begin + k];
                if (!op.len || op.op > VGK_OP_S || op.node >= P.n_oriented) return VGK_EINVAL;
                const bool graph = op.op == VGK_OP_M || op.op == VGK_OP_D;
                if (k && (op.node != P.ops[t.ops_begin + k - 1].node || (graph && pos >= ra_len(P, op.node)))) pos = 0;      // (ra_group's visits)
                if (graph) pos += op.len;
                if (op.op != VGK_OP_D) read_bases += op.len;
                if (pos > ra_len(P, op.node)) return VGK_EINVAL;
            }
            if (read_bases > (uint64_t)t.read_end - t.read_begin) return VGK_EINVAL;
        }
    }
    if (g.full_length && (!g.n_ext || !ra_full(P.ext[g.ext_begin]))) return VGK_EINVAL;
    return VGK_OK;
}

}  // namespace vgk
