// pick_mappings_device.hpp — a long read's mappings: the end of MinimizerMapper::do_alignment_on_chains (the multiplicity fix-up,
// src/minimizer_mapper_from_chains.cpp:2241-2262, with chain_ranges_are_equivalent :100-191) and pick_mappings_from_alignments (:2265-2493).  Stated
// serially here and called by the kernels as they stand:
//
//   pick_ranges_equivalent  :100-191 over the four GIVEN numbers of each chain: different components: no; chain 1 in a root snarl and child_start1 !=
//                           child_start2 or child_start1 != child_end1 or child_start2 != child_end2: no; each pair of offsets swapped into order;
//                           disjoint: no; one contains the other: yes; otherwise overlap > min(len1, len2) / 2, integer division, uint64.
//   pick_check_one          a lane per alignment and per chain: source inside the read's chains, the result's mappings inside the array, a finite chain
//                           multiplicity — else VGK_EINVAL for the read alone.
//   pick_stat_one           a lane per mapping slot (the alignments' mappings back to back, slot_off[]): the mapping's from_length (match + mismatch +
//                           deletion runs; 0 without a node), matched bases and to_length; a mapping whose runs lie outside `edits` refuses its read.
//                           The two sums per alignment are integers: whatever order they are added in, one sum.
//   pick_alignment_one      a lane per alignment: count = item_count less one for every other alignment j of the read with estimate[source] >=
//                           estimate[source[j]] and equivalent ranges, multiplicity = chain multiplicity + (count >= A ? (double)count - (double)A : 0);
//                           identity (src/path.cpp:2316-2335) = matched / (to_length less an insertion that is the path's very first or very last
//                           edit — one that is both: once), 0.0 when that length is 0; sort = (double)score + identity, or (double)estimate[source].
//                           THE WRAP: count is the reference's size_t and is a uint64 here: it wraps below 0 as there, and (double)count is then
//                           about 2^64.  Kept, because the reference's mapping qualities come out of it.
//   pick_read_one           the walk: rf_walk (read_funnel_device.hpp, process_until_threshold_e as it stands) with before(a, b) = sort(a) > sort(b),
//                           threshold 0, min 1, max max_multimaps.  Processed (:2334-2404): score <= 0 fails; fraction unique = (double)(total - used)
//                           / total (1.0 when total is 0) < min_unique_node_fraction fails; neither counts; otherwise the alignment's oriented nodes
//                           are marked, score and multiplicity appended, a mapping.  Beyond the cut (:2405-2466): the same filters, no marking,
//                           survivors append score and multiplicity.  No mapping: one entry of score 0, multiplicity 0, unmapped (:2480-2486).
//
// pick_read_one runs on `co.lanes` lanes at once, all of them through the same walk (every decision is taken from values all lanes hold alike): they
// share out an alignment's mappings when its fraction is computed and its nodes are marked, and lane 0 writes.  The serial form is one lane.  The used
// set is an open-addressed table of oriented nodes, `slots` a power of two, a node's first slot pick_hash(node, slots) = (node * 2654435761 mod 2^32)
// >> (32 - log2 slots), then the next slot round the table; PICK_EMPTY is VGK_WFA_NO_NODE, which is never entered.  Inserted with compare-and-swap,
// probed with plain loads behind a barrier.  PICK_LDS_NODES nodes at most go into the PICK_LDS_SLOTS slots of LDS (half full at most); a read
// whose accepted alignments may hold more — the sum of the mapping counts of its max_multimaps largest alignments — or which has more than
// FN_LDS_ITEMS alignments runs over a slab in HBM with a table of twice its bound.
// The walk's order: rf_walk sorts by insertion, A^2 / 2 steps at worst, and every lane takes every step; the lanes of a wavefront store one value
// to one address in one instruction, which the memory pipeline sends on as one request, so the slab sees a lane's traffic, not 64 times it.  What
// remains is the dependent chain of A^2 / 2 slab accesses of a read with A > FN_LDS_ITEMS.  A is the number of chains do_alignment_on_chains
// aligned, at most max_alignments (single digits to a few tens in giraffe's presets); this form is meant for A up to a few hundred — some 10^4
// dependent accesses, as §38's slab walks have them.  Thousands of alignments in one read stay correct and turn quadratic: a sort by lane 0 into LDS
// pieces was not written, and no shape with A > FN_LDS_ITEMS was timed.
#pragma once
#include <stdint.h>
#include "read_funnel_device.hpp"

namespace vgk {

constexpr uint32_t PICK_LDS_NODES = 1024;                        // distinct oriented nodes of a read's accepted alignments whose used set lies in LDS
constexpr uint32_t PICK_LDS_SLOTS = 2048;                        // slots of that table
constexpr uint32_t PICK_EMPTY = VGK_WFA_NO_NODE;
enum { PICK_RUN_CHECK, PICK_RUN_STATS, PICK_RUN_ALIGNMENTS, PICK_RUN_PICK };

struct PickParams {
    vgk_pick_scheme sch;
    uint32_t n_reads, n_alns, n_chains, n_slots; uint64_t n_mappings, n_edits;
    const char* reads; const uint64_t* read_off; uint32_t* rng_state;      // rng_state null: no generator, nothing shuffled
    const uint64_t* chain_off; const vgk_pick_chain* chains; const uint64_t* aln_off; const vgk_pick_alignment* alns;
    const vgk_chain_mapping* mappings; const uint32_t* edits;
    const uint64_t* slot_off;                                    // [n_alns + 1] an alignment's first mapping slot (no slots where its mappings lie outside the array)
    unsigned long long* from_len;                                // [n_slots] per mapping slot
    unsigned long long* sums;                                    // [2 n_alns] per alignment: matched bases | to_length (zeroed before the statistics)
    double* aln_mult; double* aln_sort;                          // [n_alns]
    vgk_pick_result* res; vgk_pick_verdict* verdicts;            // res: status as the host's checks left it, every other field 0; verdicts: 0
    uint32_t* picked; int32_t* scores; double* out_mult;         // [aln_off[n_reads] + n_reads]
    const uint32_t* ids; uint32_t n;                             // the reads of a pick launch
    char* slab; uint64_t slab_stride; uint32_t slab_items, slab_slots;      // the slab launch: per block order[slab_items] | table[slab_slots]
};

VGK_HD uint32_t pick_kind(uint32_t e) { return e & 3u; }
VGK_HD uint32_t pick_len(uint32_t e) { return e >> 2; }
VGK_HD uint32_t pick_hash(uint32_t node, uint32_t slots) { return slots > 1 ? (node * 2654435761u) >> (uint32_t)__builtin_clz(slots - 1) : 0u; }
VGK_HD double pick_not_evaluated() { const unsigned long long bits = VGK_PICK_NOT_EVALUATED; double d; __builtin_memcpy(&d, &bits, 8); return d; }
VGK_HD bool pick_refused(const PickParams& P, uint32_t r) { return P.res[r].status != VGK_OK; }
// an alignment's mappings lie inside the array
VGK_HD bool pick_range_ok(const vgk_chain_result& g, uint64_t n_mappings) { return (uint64_t)g.mapping_begin + g.n_mappings <= n_mappings; }
// the most distinct nodes the accepted alignments of a read can hold: counts[0 .. n) are its alignments' mapping counts (reordered here)
inline uint64_t pick_node_bound(uint32_t* counts, uint32_t n, uint32_t max_multimaps) {
    const uint32_t top = n < max_multimaps ? n : max_multimaps;
    uint64_t sum = 0;
    for (uint32_t k = 0; k < top; ++k) {                         // a selection: top is small
        uint32_t best = k;
        for (uint32_t j = k + 1; j < n; ++j) if (counts[j] > counts[best]) best = j;
        const uint32_t t = counts[k]; counts[k] = counts[best]; counts[best] = t;
        sum += counts[k];
    }
    return sum;
}
VGK_HD uint32_t pick_slots_for(uint64_t bound) { uint32_t s = PICK_LDS_SLOTS; while ((uint64_t)s < 2 * bound) s <<= 1; return s; }

// ---- the checks (host): the call's own ---------------------------------------------------------------------------------------------------------------
inline int pick_check_call(const vgk_pick_scheme* s, uint32_t n, const char* reads, const uint64_t* read_off, const uint32_t* rng_state, const uint64_t* chain_off,
                           const uint64_t* aln_off, uint64_t n_mappings, uint64_t n_edits) {
    if (!s || (s->flags & ~(uint32_t)VGK_PICK_SORT_BY_CHAIN_SCORE) || !s->max_multimaps || s->min_unique_node_fraction != s->min_unique_node_fraction) return VGK_EINVAL;
    if (!n) return VGK_OK;
    if (n > INDEX_MOST || n_mappings > INDEX_MOST || n_edits > INDEX_MOST) return VGK_ETOOBIG;
    if (rng_state && !reads) return VGK_EINVAL;
    int rc;
    if ((rng_state && (rc = rf_check_reads(read_off, n))) || (rc = rf_check_offsets(chain_off, n)) || (rc = rf_check_offsets(aln_off, n))) return rc;
    return aln_off[n] + n > INDEX_MOST ? VGK_ETOOBIG : VGK_OK;
}

// ---- equivalence ---------------------------------------------------------------------------------------------------------------------------------------
VGK_HD bool pick_ranges_equivalent(const vgk_chain_range& a, const vgk_chain_range& b) {
    if (a.component != b.component) return false;
    if ((a.flags & VGK_CHAIN_RANGE_ROOT_SNARL) && (a.child_start != b.child_start || a.child_start != a.child_end || b.child_start != b.child_end)) return false;
    uint64_t s1 = a.offset_start, e1 = a.offset_end, s2 = b.offset_start, e2 = b.offset_end;
    if (s1 > e1) { const uint64_t t = s1; s1 = e1; e1 = t; }
    if (s2 > e2) { const uint64_t t = s2; s2 = e2; e2 = t; }
    if (s1 > e2 || s2 > e1) return false;
    if ((s1 <= s2 && e1 >= e2) || (s2 <= s1 && e2 >= e1)) return true;
    if (s1 > s2) { uint64_t t = s1; s1 = s2; s2 = t; t = e1; e1 = e2; e2 = t; }
    const uint64_t overlap = e1 - s2, l1 = e1 - s1, l2 = e2 - s2;
    return overlap > (l1 < l2 ? l1 : l2) / 2;
}

// ---- checks: item i < n_alns an alignment, the others a chain --------------------------------------------------------------------------------------------
VGK_HD void pick_check_one(const PickParams& P, uint64_t i) {
    if (i < P.n_alns) {
        const uint32_t r = mq_read_of(P.aln_off, P.n_reads, i);
        const vgk_pick_alignment a = P.alns[i];
        if ((uint64_t)a.source >= P.chain_off[r + 1] - P.chain_off[r] || !pick_range_ok(a.result, P.n_mappings)) P.res[r].status = VGK_EINVAL;
    } else {
        const uint64_t c = i - P.n_alns;
        if (!rf_finite(P.chains[c].multiplicity)) P.res[mq_read_of(P.chain_off, P.n_reads, c)].status = VGK_EINVAL;
    }
}

// ---- statistics: mapping slot s of alignment *aln; out: matched bases and to_length of the mapping ---------------------------------------------------------
VGK_HD void pick_stat_one(const PickParams& P, uint32_t s, uint32_t* aln, unsigned long long out[2]) {
    const uint32_t i = mq_read_of(P.slot_off, P.n_alns, s);
    *aln = i; out[0] = out[1] = 0;
    const vgk_chain_mapping m = P.mappings[P.alns[i].result.mapping_begin + (s - P.slot_off[i])];
    unsigned long long from = 0;
    if ((uint64_t)m.edit_begin + m.n_edits > P.n_edits) P.res[mq_read_of(P.aln_off, P.n_reads, i)].status = VGK_EINVAL;
    else for (uint32_t x = 0; x < m.n_edits; ++x) {
        const uint32_t e = P.edits[m.edit_begin + x], k = pick_kind(e), len = pick_len(e);
        if (k == (uint32_t)VGK_WFA_MATCH) out[0] += len;
        if (k != (uint32_t)VGK_WFA_INSERTION) from += len;
        if (k != (uint32_t)VGK_WFA_DELETION) out[1] += len;
    }
    P.from_len[s] = m.node == VGK_WFA_NO_NODE ? 0ull : from;
}

// ---- an alignment's multiplicity, identity and sort score ---------------------------------------------------------------------------------------------------
VGK_HD void pick_alignment_one(const PickParams& P, uint32_t i) {
    const uint32_t r = mq_read_of(P.aln_off, P.n_reads, i);
    if (pick_refused(P, r)) return;
    const uint64_t lo = P.aln_off[r], A = P.aln_off[r + 1] - lo;
    const vgk_pick_chain* ch = P.chains + P.chain_off[r];
    const vgk_pick_alignment a = P.alns[i];
    const vgk_pick_chain mine = ch[a.source];
    uint64_t count = a.item_count;                               // (:2244-2257; wraps as the reference's size_t does)
    for (uint64_t j = lo; j < lo + A; ++j) {
        if (j == i) continue;
        const vgk_pick_chain& other = ch[P.alns[j].source];
        if (mine.score_estimate >= other.score_estimate && pick_ranges_equivalent(mine.range, other.range)) --count;
    }
    P.aln_mult[i] = mine.multiplicity + (count >= A ? (double)count - (double)A : 0.0);      // (:2258-2262)
    uint64_t total = P.sums[2 * (uint64_t)i + 1];
    const uint32_t M = a.result.n_mappings;
    if (M) {                                                     // (src/path.cpp:2325-2330)
        const vgk_chain_mapping m0 = P.mappings[a.result.mapping_begin], ml = P.mappings[a.result.mapping_begin + M - 1];
        if (m0.n_edits && pick_kind(P.edits[m0.edit_begin]) == (uint32_t)VGK_WFA_INSERTION) total -= pick_len(P.edits[m0.edit_begin]);
        if (ml.n_edits && !(M == 1 && ml.n_edits == 1)) {
            const uint32_t e = P.edits[ml.edit_begin + ml.n_edits - 1];
            if (pick_kind(e) == (uint32_t)VGK_WFA_INSERTION) total -= pick_len(e);
        }
    }
    const double identity = total == 0 ? 0.0 : (double)P.sums[2 * (uint64_t)i] / (double)total;
    P.verdicts[i].identity = identity;
    P.aln_sort[i] = (P.sch.flags & VGK_PICK_SORT_BY_CHAIN_SCORE) ? (double)mine.score_estimate : (double)a.score + identity;
}

// ---- the pick --------------------------------------------------------------------------------------------------------------------------------------------
// one lane alone: the serial form
struct PickOneLane {
    uint32_t lane = 0, lanes = 1;
    VGK_HD unsigned long long sum(unsigned long long x) const { return x; }
    VGK_HD void sync() const {}
    VGK_HD uint32_t load(const uint32_t* p) const { return *p; }
    VGK_HD void store(uint32_t* p, uint32_t v) const { *p = v; }
    VGK_HD uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) const { const uint32_t old = *p; if (old == expect) *p = v; return old; }
};
template <class Coop> VGK_HD bool pick_used(const Coop& co, uint32_t* table, uint32_t slots, uint32_t node) {
    for (uint32_t h = pick_hash(node, slots);; h = (h + 1u) & (slots - 1u)) {
        const uint32_t at = co.load(table + h);
        if (at == node) return true;
        if (at == PICK_EMPTY) return false;
    }
}
template <class Coop> VGK_HD void pick_mark(const Coop& co, uint32_t* table, uint32_t slots, uint32_t node) {
    for (uint32_t h = pick_hash(node, slots);; h = (h + 1u) & (slots - 1u)) {
        const uint32_t was = co.cas(table + h, PICK_EMPTY, node);
        if (was == PICK_EMPTY || was == node) return;
    }
}
template <class Coop> VGK_HD void pick_read_one(const PickParams& P, uint32_t r, uint32_t* order, uint32_t* table, uint32_t slots, const Coop& co) {
    if (pick_refused(P, r)) return;
    const uint64_t lo = P.aln_off[r]; const uint32_t A = (uint32_t)(P.aln_off[r + 1] - lo), first = (uint32_t)(lo + r);
    const vgk_pick_alignment* al = P.alns + lo; vgk_pick_verdict* vd = P.verdicts + lo;
    const double* sort = P.aln_sort + lo;
    for (uint32_t s = co.lane; s < slots; s += co.lanes) co.store(table + s, PICK_EMPTY);
    co.sync();
    RfRng rng; rng.on = P.rng_state != nullptr; rng.x = rng.on ? P.rng_state[r] : 0u; rng.seq = rng.on ? P.reads + P.read_off[r] : nullptr;
    rng.L = rng.on ? (uint32_t)(P.read_off[r + 1] - P.read_off[r]) : 0u;
    uint32_t n_scores = 0, n_mappings = 0; bool marked = false;
    // both filters (:2338-2380 and :2411-2457); -> the alignment survives
    auto filters = [&](uint32_t a) {
        if (al[a].score <= 0) {
            if (co.lane == 0) { vd[a].fraction_unique = pick_not_evaluated(); vd[a].fate = VGK_PICK_FAIL_SCORE; }
            return false;
        }
        const vgk_chain_mapping* mp = P.mappings + al[a].result.mapping_begin; const unsigned long long* from = P.from_len + P.slot_off[lo + a];
        unsigned long long total = 0, used = 0;
        for (uint32_t k = co.lane; k < al[a].result.n_mappings; k += co.lanes) {
            const uint32_t node = mp[k].node;
            if (node == VGK_WFA_NO_NODE) continue;
            total += from[k];
            if (marked && pick_used(co, table, slots, node)) used += from[k];
        }
        total = co.sum(total); used = co.sum(used);
        const double fraction = total > 0 ? (double)(total - used) / (double)total : 1.0;
        const bool fails = fraction < P.sch.min_unique_node_fraction;
        if (co.lane == 0) { vd[a].fraction_unique = fraction; if (fails) vd[a].fate = VGK_PICK_FAIL_UNIQUE; }
        return !fails;
    };
    auto append = [&](uint32_t a, uint32_t fate) {
        if (co.lane == 0) { vd[a].fate = fate; P.picked[first + n_scores] = a; P.scores[first + n_scores] = al[a].score; P.out_mult[first + n_scores] = P.aln_mult[lo + a]; }
        ++n_scores;
    };
    rf_walk(A, order,
        [&](uint32_t a, uint32_t b) { return sort[a] > sort[b]; },
        [&](uint32_t a) { return sort[a]; }, 0.0, 1u, P.sch.max_multimaps, rng,
        [&](uint32_t, uint32_t, uint32_t) {},
        [&](uint32_t a) {
            if (!filters(a)) return false;
            const vgk_chain_mapping* mp = P.mappings + al[a].result.mapping_begin;
            for (uint32_t k = co.lane; k < al[a].result.n_mappings; k += co.lanes) if (mp[k].node != VGK_WFA_NO_NODE) pick_mark(co, table, slots, mp[k].node);
            co.sync();
            marked = true;
            append(a, VGK_PICK_MAPPING); ++n_mappings;
            return true;
        },
        [&](uint32_t a) { if (filters(a)) append(a, VGK_PICK_BEYOND_CUT); },
        [&](uint32_t) {});
    if (co.lane != 0) return;
    if (rng.on) P.rng_state[r] = rng.x;
    vgk_pick_result out = P.res[r];
    out.first = first; out.unmapped = 0;
    if (!n_mappings) { P.picked[first] = FN_NONE; P.scores[first] = 0; P.out_mult[first] = 0.0; n_scores = 1; out.unmapped = 1; }      // (:2480-2486)
    out.n_scores = n_scores; out.n_mappings = n_mappings;
    P.res[r] = out;
}

}  // namespace vgk
