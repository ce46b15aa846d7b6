// chain_links_device.hpp — a chain's links: the walk of MinimizerMapper::find_chain_alignment over a chosen chain that decides WHAT gets aligned, and
// how (reference: src/minimizer_mapper_from_chains.cpp:2576-3292, its decisions only, no alignment).  Stated serially here, once, and called by the
// kernels as it stands; the serial driver (tests/emu/chain_links_driver.cpp) composes the same functions in loops.
//
// A chain is a read, an anchor set and the chain's item numbers, left to right.  The walk keeps a cursor `here` and looks for `next`:
//   left tail   here.read_start bases before the first item (:2611-2745): at most max_tail_length -> WFA (prefix); at most max_tail_dp_length -> DP;
//               longer -> SOFTCLIP, an insertion without a position, score 0 (:2667-2680)
//   next        every item that overlaps `here` in the read (next.read_start < here.read_end) is passed over (:2758-2778); none left: the chain ends
//   skip        past repetitive anchors (:2786-2863), the loop as the reference has it: total = dist(here, next), gap = |total - read distance|;
//               skip_to = next; while skip_to is skippable, is not the chain's last item and total + cur < max_skipped_bases (cur = dist(skip_to,
//               skip_to + 1) + skip_to.length): gap += |cur_read - cur|, total += cur, ++skip_to; where it stops: gap > min_indel_avoid_bases -> next =
//               skip_to.  The chain's last item is never skipped (its cur is SIZE_MAX and the second test fails)
//   link        link_length = next.read_start - here.read_end, graph_dist = dist(here, next) (:2909-3001, :3044-3051):
//               both 0 -> EMPTY; 0 < link_length <= max_chain_connection and graph_dist * link_length <= max_dp_cells -> WFA (connect);
//               else link_length > max_middle_dp_length or graph_dist * link_length > max_dp_cells -> REFUSED: no link, the chain is cut at `here`,
//               whose right tail is the rest of the read; else -> DP (a DP link may have length 0: a pure deletion)
//   right tail  read_length - here.read_end bases (:3152-3283), classed as the left one
// Kept anchors are `here` at every step (:2892, :3147: the item a cut chain ends at was appended before its link was refused, and is not appended
// again).  anchor_score = sum over the kept anchors of match * length, + full_length_bonus for an anchor that starts at read base 0, + the same for one
// that ends at the read's end (to_wfa_alignment, :4083-4104; plain scoring).
//
// Distances are GIVEN, as vgk_chain_items is given its transitions: dist(a, b) = the graph_distance of the set's entry (a, b), found by binary search
// in the set's list (strictly ascending by (from, to)); a pair that is absent, or given as UINT32_MAX, is unreachable = UINT64_MAX.
//
// THE WRAP.  The reference computes in size_t and lets three expressions wrap; they are restated in uint64 WITH the wrap:
//   graph_dist * link_length               an unreachable pair times a link of L bases is 2^64 - L: with the default max_dp_cells = SIZE_MAX nothing exceeds
//                                          it, so an unreachable pair whose link is 1 .. max_chain_connection bases still goes to WFA — kept as it is;
//                                          with a finite max_dp_cells such a link is REFUSED (2^64 - L is above any sensible limit)
//   total_graph_distance + cur_graph_distance   (and cur itself: SIZE_MAX + length) inside the skip loop — an unreachable neighbour wraps to a SMALL sum
//   the read distance of overlapping neighbours inside the skip loop: get_read_distance answers SIZE_MAX, + length wraps
//
// Work split (backend_hip.hip): only the walk is serial — a lane per chain, which writes per item one byte (kept) and per link slot one byte (route + 1)
// and the chain's few words; everything per link is a lane per LINK SLOT.  Chain c with n items has n + 1 link slots, slot_off[c] + c + j: j = 0 the
// left tail, j = k + 1 the link that follows item k (the right tail behind the last kept item).  A slot's lane finds its chain by binary search, its
// `next` by scanning the kept bytes forward, looks its own distance up again, and writes its descriptor at the prefix sum of the slots before it.
#pragma once
#include <stdint.h>
#include "pk16.hpp"
#include "../../include/vgk_engine.h"

namespace vgk {

constexpr uint64_t CL_UNREACHABLE = ~0ull;
constexpr uint32_t CL_REFUSED = 0xffu;                           // (cl_link_route's answer for a refused link; never stored)
enum { CL_RUN_CHECK = 0, CL_RUN_WALK = 1, CL_RUN_COUNT = 2, CL_RUN_WRITE = 3, CL_RUN_SEQS = 4 };      // Backend::run_chain_links

struct ClParams {
    vgk_chain_links_scheme sch;
    uint32_t n_reads, n_sets, n_chains, n_slots;                 // n_slots: item slots = the sum of n_items over the chains whose range the host accepted
    uint64_t n_dist;
    const char* reads; const uint64_t* read_off;
    const uint64_t* anchor_off; const vgk_chain_anchor* anchors; const vgk_chain_site* sites; const uint32_t* items;
    const uint64_t* dist_off; const vgk_chain_candidate* dist;
    const vgk_chain_problem* chains;
    const uint32_t* slot_off;                                    // [n_chains + 1]: a chain's first item slot (a refused range: no slots)
    uint8_t* set_bad;                                            // [n_sets]: the set's distance list is out of order or names anchors outside it
    uint8_t* keep;                                               // [n_slots]: the item is kept
    uint8_t* route;                                              // [n_slots + n_chains]: VGK_CHAIN_ROUTE_* + 1 of the link slot, 0 = no link
    uint32_t* cnt; uint32_t* first;                              // 3 x (link slots + 1): links | kept anchors | sequence bytes per link slot; their prefix sums
    unsigned long long* totals;                                  // [3], in 64 bits
    vgk_chain_links_result* res; vgk_chain_link* links; uint32_t* kept; uint64_t* seq_off; char* seqs;
    uint32_t n_links;                                            // (for the sequence copy) links written
};

VGK_HD uint32_t cl_link_slots(const ClParams& P) { return P.n_slots + P.n_chains; }
VGK_HD uint64_t cl_absdiff(uint64_t a, uint64_t b) { return a > b ? a - b : b - a; }

// the last c in [0, n) with off[c] + c * per <= x (off ascends; per = 1 makes the keys strictly ascending)
VGK_HD uint32_t cl_owner(const uint32_t* off, uint32_t n, uint32_t per, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (off[mid] + mid * per <= x) lo = mid; else hi = mid; }
    return lo;
}
VGK_HD uint32_t cl_owner64(const uint64_t* off, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (off[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}

// get_graph_distance(a, b) of anchors a, b of set s, as given
VGK_HD uint64_t cl_dist(const ClParams& P, uint32_t s, uint32_t a, uint32_t b) {
    uint64_t lo = P.dist_off[s], hi = P.dist_off[s + 1];
    const uint64_t key = (uint64_t)a << 32 | b;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const vgk_chain_candidate e = P.dist[mid];
        const uint64_t k = (uint64_t)e.from << 32 | e.to;
        if (k == key) return e.graph_distance == 0xffffffffu ? CL_UNREACHABLE : (uint64_t)e.graph_distance;
        if (k < key) lo = mid + 1; else hi = mid;
    }
    return CL_UNREACHABLE;
}

VGK_HD uint32_t cl_tail_route(const vgk_chain_links_scheme& sch, uint64_t length) {
    return length <= sch.max_tail_length ? VGK_CHAIN_ROUTE_WFA : length <= sch.max_tail_dp_length ? VGK_CHAIN_ROUTE_DP : VGK_CHAIN_ROUTE_SOFTCLIP;
}
// :2928-2946, :3044 — the product wraps
VGK_HD uint32_t cl_link_route(const vgk_chain_links_scheme& sch, uint64_t link_length, uint64_t graph_dist) {
    const uint64_t cells = graph_dist * link_length;
    if (link_length == 0 && graph_dist == 0) return VGK_CHAIN_ROUTE_EMPTY;
    if (link_length > 0 && link_length <= sch.max_chain_connection && cells <= sch.max_dp_cells) return VGK_CHAIN_ROUTE_WFA;
    if (link_length > sch.max_middle_dp_length || cells > sch.max_dp_cells) return CL_REFUSED;
    return VGK_CHAIN_ROUTE_DP;
}

// ---- the call's own checks, on the host, every sum in 64 bits: offsets ascend from 0, every chain names a read and a set of the batch; a chain
// without items or with items beyond `items` keeps VGK_EINVAL and gets no item slots; bound[] = link slots, item slots, the chains' reads' bases.
// -> VGK_OK, VGK_EINVAL, or VGK_ETOOBIG when anything is beyond `most` (2^32 - 16)
inline int cl_plan_call(uint32_t n_reads, const uint64_t* read_off, uint32_t n_sets, const uint64_t* anchor_off, uint64_t n_items, const uint64_t* dist_off,
                        uint32_t n_chains, const vgk_chain_problem* chains, uint64_t most, uint32_t* slot_off, int32_t* status, uint64_t bound[3]) {
    bound[0] = bound[1] = bound[2] = 0;
    if ((n_reads && read_off[0] != 0) || (n_sets && (anchor_off[0] != 0 || dist_off[0] != 0))) return VGK_EINVAL;
    for (uint32_t r = 0; r < n_reads; ++r) if (read_off[r + 1] < read_off[r]) return VGK_EINVAL;
    for (uint32_t s = 0; s < n_sets; ++s) if (anchor_off[s + 1] < anchor_off[s] || dist_off[s + 1] < dist_off[s]) return VGK_EINVAL;
    if (n_chains > most || n_items > most || (n_reads && read_off[n_reads] > most) || (n_sets && (anchor_off[n_sets] > most || dist_off[n_sets] > most))) return VGK_ETOOBIG;
    uint64_t slots = 0, bases = 0;
    for (uint32_t c = 0; c < n_chains; ++c) {
        const vgk_chain_problem ch = chains[c];
        if (ch.read >= n_reads || ch.anchor_set >= n_sets) return VGK_EINVAL;
        const bool ok = ch.n_items != 0 && (uint64_t)ch.item_begin + ch.n_items <= n_items;
        status[c] = ok ? VGK_OK : VGK_EINVAL;
        if (slots > most) return VGK_ETOOBIG;
        slot_off[c] = (uint32_t)slots;
        if (ok) { slots += ch.n_items; bases += read_off[ch.read + 1] - read_off[ch.read]; }
    }
    if (slots + n_chains > most || bases > most) return VGK_ETOOBIG;
    slot_off[n_chains] = (uint32_t)slots;
    bound[0] = slots + n_chains; bound[1] = slots; bound[2] = bases;
    return VGK_OK;
}

// ---- the checks that need no walk: a lane per item slot, then a lane per distance entry ---------------------------------------------------------------
// item slot: the item is an anchor of its set, does not start before its predecessor, and its site's end_offset is past the end (>= 1)
// distance entry: both anchors in the set, the list strictly ascending by (from, to)
VGK_HD void cl_check_one(const ClParams& P, uint64_t i) {
    if (i < P.n_slots) {
        const uint32_t c = cl_owner(P.slot_off, P.n_chains, 0, (uint32_t)i), k = (uint32_t)i - P.slot_off[c];
        const vgk_chain_problem ch = P.chains[c];
        const uint64_t a0 = P.anchor_off[ch.anchor_set], A = P.anchor_off[ch.anchor_set + 1] - a0;
        const uint32_t a = P.items[(uint64_t)ch.item_begin + k];
        bool bad = a >= A;
        if (!bad && P.sites[a0 + a].end_offset == 0) bad = true;
        if (!bad && k) { const uint32_t b = P.items[(uint64_t)ch.item_begin + k - 1]; if (b < A && P.anchors[a0 + b].read_start > P.anchors[a0 + a].read_start) bad = true; }
        if (bad) P.res[c].status = VGK_EINVAL;
        return;
    }
    const uint64_t d = i - P.n_slots;
    if (d >= P.n_dist) return;
    const uint32_t s = cl_owner64(P.dist_off, P.n_sets, d);
    const uint64_t A = P.anchor_off[s + 1] - P.anchor_off[s];
    const vgk_chain_candidate e = P.dist[d];
    bool bad = e.from >= A || e.to >= A;
    if (!bad && d > P.dist_off[s]) { const vgk_chain_candidate p = P.dist[d - 1]; if (((uint64_t)p.from << 32 | p.to) >= ((uint64_t)e.from << 32 | e.to)) bad = true; }
    if (bad) P.set_bad[s] = 1;
}

// ---- the walk: a lane per chain ----------------------------------------------------------------------------------------------------------------------
// keep[] and route[] are zero when it starts; a chain that fails (a bad set; a kept anchor that ends past its read) leaves them zero
VGK_HD void cl_walk_one(const ClParams& P, uint32_t c) {
    if (P.res[c].status != VGK_OK) return;
    const vgk_chain_problem ch = P.chains[c];
    const uint32_t s = ch.anchor_set, n = ch.n_items;
    if (P.set_bad[s]) { P.res[c].status = VGK_EINVAL; return; }
    const vgk_chain_links_scheme& sch = P.sch;
    const uint64_t read_len = P.read_off[ch.read + 1] - P.read_off[ch.read];
    const vgk_chain_anchor* anc = P.anchors + P.anchor_off[s];
    const vgk_chain_site* site = P.sites + P.anchor_off[s];
    const uint32_t* it = P.items + ch.item_begin;
    uint8_t* keep = P.keep + P.slot_off[c];
    uint8_t* route = P.route + P.slot_off[c] + c;                // [0]: the left tail; [k + 1]: the link behind item k

    uint32_t here = 0, next = 1, flags = 0;
    uint64_t here_end = (uint64_t)anc[it[0]].read_start + anc[it[0]].length, longest = 0;
    const uint64_t left = anc[it[0]].read_start;
    if (left > 0) route[0] = (uint8_t)(cl_tail_route(sch, left) + 1);
    bool ok = true;
    for (;;) {
        if (here_end > read_len) { ok = false; break; }
        keep[here] = 1;
        while (next < n && anc[it[next]].read_start < here_end) ++next;               // overlap: keep here, pass next over (:2762-2773)
        if (next == n) break;
        // past repetitive anchors (:2786-2863)
        const uint64_t first_dist = cl_dist(P, s, it[here], it[next]);
        uint64_t total = first_dist, gap = cl_absdiff(total, (uint64_t)anc[it[next]].read_start - here_end);
        const uint32_t first_next = next;
        uint32_t skip_to = next;
        for (;;) {
            const vgk_chain_anchor st = anc[it[skip_to]];
            const bool last = skip_to + 1 == n;
            uint64_t cur_graph = CL_UNREACHABLE;
            if (!last) cur_graph = cl_dist(P, s, it[skip_to], it[skip_to + 1]) + st.length;
            if ((site[it[skip_to]].flags & VGK_CHAIN_SITE_SKIPPABLE) && !last && total + cur_graph < sch.max_skipped_bases) {
                const uint64_t st_end = (uint64_t)st.read_start + st.length, nx = anc[it[skip_to + 1]].read_start;
                const uint64_t cur_read = (nx < st_end ? CL_UNREACHABLE : nx - st_end) + st.length;
                gap += cl_absdiff(cur_read, cur_graph);
                total += cur_graph;
                ++skip_to;
            } else {
                if (gap > sch.min_indel_avoid_bases) next = skip_to;
                break;
            }
        }
        const uint64_t link_length = (uint64_t)anc[it[next]].read_start - here_end;
        const uint64_t graph_dist = next == first_next ? first_dist : cl_dist(P, s, it[here], it[next]);
        const uint32_t r = cl_link_route(sch, link_length, graph_dist);
        if (r == CL_REFUSED) { flags |= VGK_CHAIN_LINKS_CUT; break; }
        if (r == VGK_CHAIN_ROUTE_WFA && link_length > longest) longest = link_length;
        route[here + 1] = (uint8_t)(r + 1);
        here = next; next = here + 1;
        here_end = (uint64_t)anc[it[here]].read_start + anc[it[here]].length;
    }
    if (!ok) {
        for (uint32_t k = 0; k < n; ++k) { keep[k] = 0; route[k] = 0; }
        route[n] = 0;
        P.res[c].status = VGK_EINVAL;
        return;
    }
    const uint64_t right = read_len - here_end;
    if (right > 0) route[here + 1] = (uint8_t)(cl_tail_route(sch, right) + 1);
    P.res[c].flags = flags; P.res[c].left_tail_length = (uint32_t)left; P.res[c].longest_attempted_connection = (uint32_t)longest;
}

// ---- a link slot, from the walk's bytes ------------------------------------------------------------------------------------------------------------------
struct ClSlot {
    uint32_t c, j;                                               // chain, slot within it
    bool has_link, has_kept;
    vgk_chain_link link;                                         // (has_link) complete when `full`, else only .length
    uint32_t kept_anchor; int64_t kept_score;                    // (has_kept) the anchor number within its set; what it adds to anchor_score
};
VGK_HD ClSlot cl_slot(const ClParams& P, uint32_t ls, bool full) {
    ClSlot o{};
    const uint32_t c = cl_owner(P.slot_off, P.n_chains, 1, ls), j = ls - P.slot_off[c] - c;
    o.c = c; o.j = j;
    const uint32_t r = P.route[ls];
    o.has_link = r != 0;
    const uint8_t* keep = P.keep + P.slot_off[c];
    o.has_kept = j >= 1 && keep[j - 1];
    if (!o.has_link && !o.has_kept) return o;
    const vgk_chain_problem ch = P.chains[c];
    const uint32_t n = P.slot_off[c + 1] - P.slot_off[c], s = ch.anchor_set;
    const uint64_t read_len = P.read_off[ch.read + 1] - P.read_off[ch.read];
    const vgk_chain_anchor* anc = P.anchors + P.anchor_off[s];
    const vgk_chain_site* site = P.sites + P.anchor_off[s];
    const uint32_t* it = P.items + ch.item_begin;
    vgk_chain_link& L = o.link;
    L.chain = c; L.route = r - 1;
    L.from_node = L.to_node = VGK_WFA_NO_NODE;
    if (j == 0) {                                                // the left tail: a prefix that ends before the first item's start
        const uint32_t a = it[0];
        L.mode = VGK_WFA_PREFIX; L.read_begin = 0; L.length = anc[a].read_start; L.graph_distance = L.length;
        if (full) { L.to_node = site[a].start_node; L.to_offset = site[a].start_offset; }
        return o;
    }
    const uint32_t a = it[j - 1];
    const uint64_t here_end = (uint64_t)anc[a].read_start + anc[a].length;
    if (o.has_kept) {
        o.kept_anchor = a;
        o.kept_score = (int64_t)P.sch.match * (int64_t)anc[a].length + (anc[a].read_start == 0 ? P.sch.full_length_bonus : 0) + (here_end == read_len ? P.sch.full_length_bonus : 0);
    }
    if (!o.has_link) return o;
    uint32_t k = j;
    while (k < n && !keep[k]) ++k;                               // the next kept item, if the chain has one
    L.read_begin = (uint32_t)here_end;
    if (full) { L.from_node = site[a].end_node; L.from_offset = site[a].end_offset - 1; }      // graph_end with its offset walked back (:2949-2950, :3162)
    if (k == n) {
        L.mode = VGK_WFA_SUFFIX; L.length = (uint32_t)(read_len - here_end); L.graph_distance = L.length;
    } else {
        const uint32_t b = it[k];
        L.mode = VGK_WFA_CONNECT; L.length = (uint32_t)(anc[b].read_start - here_end);
        if (full) {
            const uint64_t d = cl_dist(P, s, a, b);
            L.graph_distance = d > 0xffffffffull ? 0xffffffffu : (uint32_t)d;
            L.to_node = site[b].start_node; L.to_offset = site[b].start_offset;
        }
    }
    return o;
}

// the three counts of a link slot (entry `link slots` of each is 0, set by the caller)
VGK_HD void cl_count_one(const ClParams& P, uint32_t ls, uint32_t out[3]) {
    const ClSlot o = cl_slot(P, ls, false);
    const uint32_t LS1 = cl_link_slots(P) + 1;
    out[0] = o.has_link; out[1] = o.has_kept; out[2] = o.has_link ? o.link.length : 0;
    P.cnt[ls] = out[0]; P.cnt[LS1 + ls] = out[1]; P.cnt[2 * (uint64_t)LS1 + ls] = out[2];
}

// the write-out of a link slot at its prefix sums; -> what its kept anchor adds to its chain's anchor_score (the caller sums: a segmented sum over the
// wavefront's lanes of one chain, one atomic per wavefront per chain)
VGK_HD int64_t cl_write_one(const ClParams& P, uint32_t ls, uint32_t* chain) {
    const ClSlot o = cl_slot(P, ls, true);
    const uint32_t LS1 = cl_link_slots(P) + 1;
    const uint32_t* f_link = P.first; const uint32_t* f_kept = P.first + LS1; const uint32_t* f_seq = P.first + 2 * (uint64_t)LS1;
    *chain = o.c;
    if (o.has_link) { P.links[f_link[ls]] = o.link; if (P.seq_off) P.seq_off[f_link[ls]] = f_seq[ls]; }
    if (o.has_kept) P.kept[f_kept[ls]] = o.kept_anchor;
    if (o.j == 0 && P.res[o.c].status == VGK_OK) {
        const uint32_t end = P.slot_off[o.c + 1] + o.c + 1;                                    // the next chain's first link slot
        vgk_chain_links_result& R = P.res[o.c];
        R.link_begin = f_link[ls]; R.n_links = f_link[end] - f_link[ls]; R.kept_begin = f_kept[ls]; R.n_kept = f_kept[end] - f_kept[ls]; R.seq_begin = f_seq[ls];
    }
    if (ls == 0 && P.seq_off) P.seq_off[f_link[LS1 - 1]] = f_seq[LS1 - 1];
    return o.has_kept ? o.kept_score : 0;
}

}  // namespace vgk
