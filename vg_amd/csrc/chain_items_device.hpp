// chain_items_device.hpp — choosing chains of anchors (vgk_chain_items, include/vgk_engine.h): algorithms::find_best_chains of the reference
// (src/algorithms/chain_items.cpp:735-877) over an explicit list of candidate transitions.  The lane code of the kernels in backend_hip.hip,
// and ci_problem_one: the same rule stated serially, what the kernels are checked against without a GPU (tests/emu/chain_items_driver.cpp).
//
// The rule, piece by piece (the host shim's vg_amd/host/chain_items.cpp states it in the reference's loop shape):
//   ci_legal         add_transition_if_legal (:270-355): the five drops, the indel of what is left
//   jump table       (int)(-score_chain_gap(indel, bsl) * gap_scale) (:365-373, :511), made on the host in double, one table per distinct bsl
//   ci_candidate     the score a destination gets from one source, the evaluation bonus it is compared with (:511-550), set_shared_paths (:71-94)
//   the winner       per destination the maximum of (score + bonus, score, source), from nowhere = the largest source (:464-476, :544-550).  A
//                    maximum: the order of a destination's transitions cannot matter, so they are grouped with atomics and reduced across lanes
//   ci_start_before  the order tracebacks start in; ci_walk the tracebacks with the penalty correction (:650-719); ci_rec_passes (:793-868)
// rec_num of TracedScore is not kept: nothing the call answers depends on it (a chain's recombinations come from ci_rec_passes).
//
// MI355X-first: a destination's table entry depends on finished entries of smaller anchor numbers only (a legal source ends at or before the
// destination's start and is at least one base long), so a wavefront takes a problem's destinations in anchor order, its 64 lanes stride over
// the destination's incoming transitions, and the table (score, paths) stays in LDS: 12 B per anchor, up to CI_LDS_MAX anchors; above that in
// a slab in HBM that only this wavefront touches.
#pragma once
#include <cstdint>
#include <algorithm>
#include <vector>
#include "../../include/vgk_engine.h"
#include "pk16.hpp"

namespace vgk {

constexpr uint32_t CI_NOWHERE = 0xffffffffu, CI_DROPPED = 0xffffffffu;
constexpr uint32_t CI_LDS_MAX = 2048;           // anchors of a problem whose tables the kernels keep in LDS (DP: 24 KiB, traceback: 36.3 KiB)
constexpr uint32_t CI_MAX_INDEL = 65536;        // the largest indel limit a jump table is made for
enum { CI_NOT_REACHABLE = 1, CI_TOO_FAR = 2, CI_OVERLAPPED = 3, CI_BACKED_OUT = 4, CI_INDEL = 5 };      // add_transition_if_legal's drops, in its order

struct CiProb { uint64_t a_off, slot; uint32_t n, lookback, limit, jump_off; };      // a problem: its anchors, its first chain's slot, its limits, its jump table
struct CiEdge { uint32_t from; int32_t jump; };                                       // a legal transition in its destination's group

struct CiParams {
    int32_t item_bonus, recombination_penalty, consistency_bonus; uint32_t max_chains;
    uint32_t n_problems; uint64_t n_cands, n_anchors;
    const CiProb* probs; const uint64_t* cand_off; const vgk_chain_anchor* anchors; const vgk_chain_candidate* cands; const int32_t* jump;
    uint32_t* indel;                            // [n_cands] CI_DROPPED, or the indel of a legal transition
    uint32_t* count; const uint32_t* first;     // [n_anchors + 1] legal transitions into each anchor (numbered through the call), their exclusive prefix sums
    uint32_t* cursor; CiEdge* grouped;          // [n_anchors] zeroed: the scatter's positions; [legal transitions] grouped by destination
    uint32_t* flags;                            // [1] bit 0: a candidate names an anchor outside its problem
    int32_t* t_score; uint32_t* t_source;       // [n_anchors] the DP table
    vgk_chain_found* chains; uint32_t* n_chains; uint32_t* items; uint32_t* rec_right; uint32_t* rec_left;      // chains at a problem's slot, their number per problem
    const uint32_t* ids; uint32_t n;            // the problems of a launch
    uint32_t lds_np;                            // ... in LDS: the largest of them, rounded up to a power of two (sizes the dynamic LDS)
    char* slab; uint64_t slab_stride; uint32_t slab_n, slab_np;      // ... over slabs: one per workgroup, sized for slab_n anchors (slab_np: rounded up to a power of two)
};

enum { CI_RUN_LEGAL = 0, CI_RUN_SCATTER = 1, CI_RUN_DP = 2, CI_RUN_TRACE = 3 };      // Backend::run_chain_items' stages
// LDS of a launch whose largest problem has np anchors (a power of two): the DP keeps (paths, score), the traceback score, source, penalties,
// the used bits and four 16-bit index arrays (backend_hip.hip: chain_items_dp_kernel, chain_items_trace_kernel)
VGK_HD uint32_t ci_dp_lds_bytes(uint32_t np) { return 12u * np; }
VGK_HD uint32_t ci_trace_lds_bytes(uint32_t np) { return 12u * np + 4u * (np / 32u + 1u) + 2u * (4u * np + 2u); }
// a slab of the kernels for problems of up to n anchors (np: n rounded up to a power of two), either kernel
VGK_HD uint64_t ci_slab_bytes(uint64_t n, uint64_t np) {
    const uint64_t dp = 12u * n, trace = 4u * (n + n / 32u + 1u + np + n + n + n + 2u);
    return ((dp > trace ? dp : trace) + 63u) & ~63ull;
}

// add_transition_if_legal (:282-354): the indel of a legal transition, or CI_DROPPED with the drop in *why
VGK_HD uint32_t ci_legal(const vgk_chain_anchor& f, const vgk_chain_anchor& t, uint32_t graph_distance, uint32_t lookback, uint32_t limit, uint32_t* why) {
    const uint64_t f_end = (uint64_t)f.read_start + f.length;
    if ((uint64_t)t.read_start < f_end) { *why = CI_NOT_REACHABLE; return CI_DROPPED; }
    const uint64_t read_distance = (uint64_t)t.read_start - f_end;
    if (read_distance > lookback) { *why = CI_TOO_FAR; return CI_DROPPED; }               // (UINT32_MAX = none: no read distance is above it)
    if (f_end + f.margin_after > (uint64_t)t.read_start - (uint64_t)t.margin_before) { *why = CI_OVERLAPPED; return CI_DROPPED; }     // (size_t arithmetic, as there)
    const uint64_t remove = (uint64_t)t.start_hint_offset + f.end_hint_offset;
    if (remove > graph_distance) { *why = CI_BACKED_OUT; return CI_DROPPED; }
    const uint64_t g = graph_distance - remove, indel = read_distance > g ? read_distance - g : g - read_distance;
    if (indel > limit) { *why = CI_INDEL; return CI_DROPPED; }
    *why = 0;
    return (uint32_t)indel;
}

struct CiKey { int32_t eval, score; uint32_t source; };          // what a destination's winner is the maximum of
VGK_HD bool ci_key_greater(const CiKey& a, const CiKey& b) {
    return a.eval > b.eval || (a.eval == b.eval && (a.score > b.score || (a.score == b.score && a.source > b.source)));
}
// set_shared_paths (:71-94) of a source's paths with a destination's (start, end) paths
VGK_HD uint64_t ci_paths_after(uint64_t source_paths, uint64_t start, uint64_t end) {
    if (start != end) return end;                                  // an internally recombinant anchor resets to its end paths
    return (source_paths & start) ? (source_paths & start) : start;
}
// one source for one destination (:511-542): points = the destination's score + item_bonus
VGK_HD CiKey ci_candidate(int32_t source_score, uint64_t source_paths, uint32_t from, int32_t jump, int32_t points, uint64_t start, uint64_t end,
                          int32_t recombination_penalty, int32_t consistency_bonus) {
    const bool recombination = (source_paths & start) == 0;
    const int32_t score = source_score + jump - (recombination ? recombination_penalty : 0) + points;
    int32_t bonus = 0;
    if (consistency_bonus > 0 && !recombination)                   // (no recombination: the source has paths)
        bonus = consistency_bonus * (int32_t)__builtin_popcountll(ci_paths_after(source_paths, start, end)) / (int32_t)__builtin_popcountll(source_paths);
    return CiKey{score + bonus, score, from};
}
VGK_HD CiKey ci_from_nowhere(int32_t points, int32_t consistency_bonus) { return CiKey{points + consistency_bonus, points, CI_NOWHERE}; }

// the order tracebacks start in [PARITY-UNPINNED beyond the score]: score descending, source descending (nowhere largest), anchor ascending
VGK_HD bool ci_start_before(int32_t sa, uint32_t src_a, uint32_t ia, int32_t sb, uint32_t src_b, uint32_t ib) {
    return sa > sb || (sa == sb && (src_a > src_b || (src_a == src_b && ia < ib)));
}
// chain_items_traceback's walks (:674-718) from the starts in `order`: traceback k's anchors lie right to left in tmp[begin[k] .. begin[k + 1]),
// its penalty in pen[k]; -> the number of tracebacks.  used: a bit per anchor, zeroed.  IDX: uint16_t in LDS, uint32_t elsewhere
template <class IDX> VGK_HD uint32_t ci_walk(uint32_t n, const IDX* order, const int32_t* score, const uint32_t* source, const vgk_chain_anchor* a, int32_t item_bonus,
                                             int32_t best, uint32_t* used, IDX* tmp, int32_t* pen, IDX* begin) {
    uint32_t n_tb = 0, at = 0;
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t from = order[s];
        if ((used[from >> 5] >> (from & 31)) & 1u) continue;
        begin[n_tb] = (IDX)at;
        int32_t penalty = best - score[from];
        uint32_t here = from;
        tmp[at++] = (IDX)here;
        for (;;) {
            used[here >> 5] |= 1u << (here & 31);
            const uint32_t next = source[here];
            if (next == CI_NOWHERE) break;
            if ((used[next >> 5] >> (next & 31)) & 1u) { penalty += score[here] - (a[here].score + item_bonus); break; }      // stopped at a used item
            tmp[at++] = (IDX)next;
            here = next;
        }
        pen[n_tb++] = penalty;
    }
    begin[n_tb] = (IDX)at;
    return n_tb;
}
// the recombination passes over one chain, left to right in items[0 .. len) (:797-856): right[] = rec_positions, left[] = the backward pass'
// boundaries, both in chain order
VGK_HD void ci_rec_passes(const vgk_chain_anchor* a, const uint32_t* items, uint32_t len, uint32_t* right, uint32_t* left, uint32_t* n_right, uint32_t* n_left) {
    uint32_t nr = 0, nl = 0;
    if (len) {
        uint64_t cur = a[items[0]].end_paths;
        for (uint32_t k = 1; k < len; ++k) {
            const uint64_t s = a[items[k]].start_paths, e = a[items[k]].end_paths;
            if (s == e) { if ((cur & s) == 0) { right[nr++] = items[k]; cur = s; } else cur &= s; }
            else cur = e;
        }
    }
    if (len > 1) {
        uint64_t cur = a[items[len - 1]].start_paths;
        for (uint32_t k = len - 1; k > 0; --k) {
            const uint64_t s = a[items[k - 1]].start_paths, e = a[items[k - 1]].end_paths;
            if (s == e) { if ((cur & e) == 0) { left[nl++] = items[k - 1]; cur = e; } else cur &= e; }
            else cur = s;
        }
        for (uint32_t x = 0, y = nl; x + 1 < y; ++x) { --y; const uint32_t t = left[x]; left[x] = left[y]; left[y] = t; }
    }
    *n_right = nr; *n_left = nl;
}
// the problem a candidate belongs to: the last p with cand_off[p] <= c
VGK_HD uint32_t ci_problem_of(const uint64_t* cand_off, uint32_t n_problems, uint64_t c) {
    uint32_t lo = 0, hi = n_problems;                              // cand_off[lo] <= c < cand_off[hi]
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (cand_off[mid] <= c) lo = mid; else hi = mid; }
    return lo;
}
// ---- the serial statement of the device's rule for problem p: legality, grouping (a stable counting sort by destination), the DP in anchor
// order, the tracebacks, the chains.  Host code; P's arrays are host arrays, `first` must hold the prefix sums of the counts this function
// itself leaves in `count` for its problem — so it groups privately instead and leaves count / first / cursor / grouped alone.
inline void ci_problem_one(const CiParams& P, uint32_t p) {
    const CiProb q = P.probs[p];
    const uint32_t n = q.n; const vgk_chain_anchor* a = P.anchors + q.a_off;
    vgk_chain_found* out = P.chains + q.slot;
    const uint32_t base = (uint32_t)q.a_off;
    if (!n) { out[0] = vgk_chain_found{0, base, 0, base, 0, 0}; P.n_chains[p] = 1; return; }
    // legality and grouping
    std::vector<uint32_t> first((size_t)n + 1, 0);
    for (uint64_t c = P.cand_off[p]; c < P.cand_off[p + 1]; ++c) {
        const vgk_chain_candidate e = P.cands[c]; uint32_t why = 0;
        if (e.from >= n || e.to >= n) { P.indel[c] = CI_DROPPED; P.flags[0] |= 1u; continue; }
        P.indel[c] = ci_legal(a[e.from], a[e.to], e.graph_distance, q.lookback, q.limit, &why);
        if (P.indel[c] != CI_DROPPED) ++first[e.to + 1];
    }
    for (uint32_t i = 0; i < n; ++i) first[i + 1] += first[i];
    std::vector<CiEdge> grouped(first[n]); std::vector<uint32_t> cursor(first.begin(), first.end() - 1);
    for (uint64_t c = P.cand_off[p]; c < P.cand_off[p + 1]; ++c)
        if (P.indel[c] != CI_DROPPED) grouped[cursor[P.cands[c].to]++] = CiEdge{P.cands[c].from, P.jump[q.jump_off + P.indel[c]]};
    // the DP, destinations in anchor order
    std::vector<int32_t> score(n); std::vector<uint32_t> source(n); std::vector<uint64_t> paths(n);
    for (uint32_t t = 0; t < n; ++t) {
        const int32_t points = a[t].score + P.item_bonus;
        CiKey best = ci_from_nowhere(points, P.consistency_bonus);
        for (uint32_t g = first[t]; g < first[t + 1]; ++g) {
            const CiEdge e = grouped[g];
            const CiKey k = ci_candidate(score[e.from], paths[e.from], e.from, e.jump, points, a[t].start_paths, a[t].end_paths, P.recombination_penalty, P.consistency_bonus);
            if (ci_key_greater(k, best)) best = k;
        }
        score[t] = best.score; source[t] = best.source;
        paths[t] = best.source == CI_NOWHERE ? a[t].end_paths : ci_paths_after(paths[best.source], a[t].start_paths, a[t].end_paths);
        P.t_score[q.a_off + t] = best.score; P.t_source[q.a_off + t] = best.source;
    }
    int32_t best_score = score[0];                                 // the first largest
    for (uint32_t t = 1; t < n; ++t) if (score[t] > best_score) best_score = score[t];
    // the tracebacks
    std::vector<uint32_t> order(n), tmp(n), begin((size_t)n + 1), used((n + 31) / 32, 0u); std::vector<int32_t> pen(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return ci_start_before(score[x], source[x], x, score[y], source[y], y); });
    const uint32_t n_tb = ci_walk<uint32_t>(n, order.data(), score.data(), source.data(), a, P.item_bonus, best_score, used.data(), tmp.data(), pen.data(), begin.data());
    std::vector<uint32_t> by_penalty(n_tb);
    for (uint32_t k = 0; k < n_tb; ++k) by_penalty[k] = k;
    std::sort(by_penalty.begin(), by_penalty.end(), [&](uint32_t x, uint32_t y) { return pen[x] < pen[y] || (pen[x] == pen[y] && x < y); });
    const uint32_t n_out = n_tb < P.max_chains ? n_tb : P.max_chains;
    if (!n_out) { out[0] = vgk_chain_found{0, base, 0, base, 0, 0}; P.n_chains[p] = 1; return; }
    uint32_t at = base;
    for (uint32_t k = 0; k < n_out; ++k) {
        const uint32_t tb = by_penalty[k], len = begin[tb + 1] - begin[tb];
        for (uint32_t i = 0; i < len; ++i) P.items[at + i] = tmp[begin[tb] + len - 1 - i];
        uint32_t nr = 0, nl = 0;
        ci_rec_passes(a, P.items + at, len, P.rec_right + at, P.rec_left + at, &nr, &nl);
        out[k] = vgk_chain_found{best_score - pen[tb], at, len, at, nr, nl};
        at += len;
    }
    P.n_chains[p] = n_out;
}

}  // namespace vgk
