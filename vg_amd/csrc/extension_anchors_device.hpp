// extension_anchors_device.hpp — anchors for chaining from seeds and their gapless extensions (vgk_extension_anchors, include/vgk_engine.h): the
// block of MinimizerMapper::map_from_chains between the extension and the chaining (src/minimizer_mapper_from_chains.cpp:1380-1596).  The lane code
// of the kernels in backend_hip.hip, and ea_problem_one: the same rule stated serially, what the kernels are checked against without a GPU
// (tests/emu/extension_anchors_driver.cpp).
//
// The rule, piece by piece (the host shim's vg_amd/host/extension_anchors.cpp states it in the reference's loop shape):
//   ea_seed_anchor   to_anchor of one seed (:3978-4038)
//   ea_diag_before   the order that puts a problem's seeds diagonal by diagonal, each in stapled order [PARITY-UNPINNED beyond that: seed number]
//   ea_ext_seeds     the seeds an extension contains (extend_seed_group, src/minimizer_mapper.cpp:4881-5000): per path node its read interval and
//                    diagonal (for_each_read_interval, src/gbwt_extender.cpp:23-39), a binary search, the run of stapled bases inside the interval
//   ea_ext_before    the order extensions are taken in (:1472-1479) [PARITY-UNPINNED: equal scores by number]
//   ea_extension     one extension in its turn (:1484-1586): find_anchor_intervals (:480-706) as a sweep that hands every interval on the moment it
//                    is closed — an interval ends before the seed that closes it, so marking its seeds cannot change what the sweep has yet to
//                    see —, the mismatches and unused seeds inside it, the composite anchor (to_anchor, :4040-4081; Anchor(first, last, ...),
//                    src/algorithms/chain_items.hpp:249-262)
//   ea_anchor_before sort_anchor_indexes [PARITY-UNPINNED: equal start and end in order of creation]
//
// MI355X-first: the seed anchors, the diagonal sort (a bitonic sort per problem) and the extensions' seed lists are data-parallel and leave their
// results in HBM; what depends on the order of the extensions — the used flags — runs one wavefront per problem: the extensions and later the
// anchors are ordered by bitonic sorts across the 64 lanes, the sweep itself is lane 0's (profiles/r08_extension_anchors/NOTES.md gives its share).
// Used flags, sort keys: LDS up to EA_LDS_SEEDS seeds and EA_LDS_EXT extensions, a slab in HBM that only the problem's wavefront touches above.
#pragma once
#include <cstdint>
#include <algorithm>
#include <vector>
#include "../../include/vgk_engine.h"
#include "pk16.hpp"

namespace vgk {

constexpr uint32_t EA_LDS_SEEDS = 2048, EA_LDS_EXT = 1024;      // a problem within both runs in LDS (8.3 KiB at most)
constexpr uint32_t EA_NONE = 0xffffffffu;
enum { EA_BAD_SEED = 1 };                                       // flags[0]

struct EaProb { uint64_t s_off, e_off; uint32_t n_seeds, n_ext, full_length, pad; };      // a problem: its seeds (and its slot of anchors), its extensions

struct EaParams {
    int32_t match, mismatch; uint32_t from_seeds, max_mismatches;
    uint32_t n_problems, n_oriented; uint64_t n_seeds, n_ext;
    const uint64_t* node_tab;                   // the index: per oriented node its length in the high word (gapless_device.hpp GIndex)
    const EaProb* probs; const vgk_anchor_seed* seeds; const vgk_extension* ext; const uint32_t* nodes; const uint32_t* mism;
    const uint32_t* prob_of_ext;                // [n_ext] the problem an extension belongs to
    vgk_chain_anchor* seed_anchor;              // [n_seeds] every seed's own anchor
    uint32_t* sorted;                           // [n_seeds] per problem its seed numbers in ea_diag_before's order
    uint32_t* ext_count; const uint32_t* ext_first; uint32_t* ext_seeds;      // [n_ext + 1] seeds each extension contains, their exclusive prefix sums; the lists
    uint32_t* flags;                            // [1] EA_BAD_SEED
    vgk_chain_anchor* made; vgk_anchor_origin* made_origin;      // [n_seeds] anchors in order of creation, at the problem's seed offset
    vgk_chain_anchor* anchors; vgk_anchor_origin* origins;       // [n_seeds] ... sorted
    uint32_t* rep;                              // [n_seeds + n_ext] a problem's stretch at s_off + e_off
    uint32_t* n_anchors; uint32_t* n_rep; uint32_t* status;      // [n_problems]
    const uint32_t* ids; uint32_t n;            // the problems of a launch
    uint32_t lds_np;                            // ... in LDS: the largest power of two its sorts need (sizes the dynamic LDS)
    char* slab; uint64_t slab_stride; uint32_t slab_np, slab_seeds;      // ... over slabs: one per workgroup
};
enum { EA_RUN_SEEDS = 0, EA_RUN_SORT = 1, EA_RUN_COUNT = 2, EA_RUN_EMIT = 3, EA_RUN_ANCHORS = 4 };      // Backend::run_extension_anchors' stages
// working memory of a problem whose sorts need np entries (a power of two) and that has n seeds: the order array, the used bits
VGK_HD uint64_t ea_work_bytes(uint64_t np, uint64_t n_seeds) { return (4u * np + 4u * (n_seeds / 32u + 1u) + 63u) & ~63ull; }

// to_anchor (:3978-4038) for one seed on a node of node_len bases; false = the seed is malformed (VGK_EINVAL)
VGK_HD bool ea_seed_anchor(const vgk_anchor_seed& s, uint32_t n_oriented, const uint64_t* node_tab, int32_t match, vgk_chain_anchor* out) {
    if (s.node >= n_oriented || !s.length || s.is_reverse > 1u || s.stapled > 0x3fffffffu) return false;
    const uint32_t node_len = (uint32_t)(node_tab[s.node] >> 32), k = s.length;
    const int64_t offset = (int64_t)s.stapled - s.diff;
    if (offset < 0 || offset >= (int64_t)node_len) return false;
    vgk_chain_anchor a;
    if (s.is_reverse) {
        if (s.stapled + 1u < k) return false;
        a.length = k < (uint32_t)offset + 1u ? k : (uint32_t)offset + 1u;
        a.margin_before = k - a.length; a.margin_after = 0; a.read_start = s.stapled + 1u - a.length; a.start_hint_offset = a.length - 1u;
    } else {
        const uint32_t room = node_len - (uint32_t)offset;
        a.length = k < room ? k : room;
        a.margin_before = 0; a.margin_after = k - a.length; a.read_start = s.stapled; a.start_hint_offset = 0;
    }
    a.end_hint_offset = a.length - a.start_hint_offset; a.base_seed_length = k; a.score = match * (int32_t)k; a.start_paths = a.end_paths = s.paths;
    *out = a;
    return true;
}
// seeds x before y: diagonal by diagonal, stapled ascending, then seed number [PARITY-UNPINNED]
VGK_HD bool ea_diag_before(const vgk_anchor_seed* s, uint32_t x, uint32_t y) {
    const vgk_anchor_seed& a = s[x]; const vgk_anchor_seed& b = s[y];
    if (a.node != b.node) return a.node < b.node;
    if (a.diff != b.diff) return (uint32_t)a.diff < (uint32_t)b.diff;
    if (a.stapled != b.stapled) return a.stapled < b.stapled;
    return x < y;
}
// the seeds extension e contains, in its order (path node by path node, each run in stapled order): take(seed number) for each; -> their number
template <class TAKE> VGK_HD uint32_t ea_ext_seeds(const vgk_extension& e, const uint32_t* nodes, const uint64_t* node_tab, const vgk_anchor_seed* s, const uint32_t* sorted, uint32_t n_seeds, TAKE take) {
    uint32_t read_offset = e.read_begin, node_offset = e.offset, found = 0;
    for (uint32_t i = 0; i < e.path_len; ++i) {
        const uint32_t node = nodes[e.path_begin + i], node_len = (uint32_t)(node_tab[node] >> 32);
        const uint32_t left = e.read_end - read_offset, len = node_len - node_offset < left ? node_len - node_offset : left;
        const uint32_t diff = read_offset - node_offset;           // (as the seeds' int32, compared as bits)
        uint32_t lo = 0, hi = n_seeds;                              // the first seed not before (node, diff, read_offset)
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2; const vgk_anchor_seed& m = s[sorted[mid]];
            const bool before = m.node != node ? m.node < node : ((uint32_t)m.diff != diff ? (uint32_t)m.diff < diff : m.stapled < read_offset);
            if (before) lo = mid + 1; else hi = mid;
        }
        for (; lo < n_seeds; ++lo) {
            const vgk_anchor_seed& m = s[sorted[lo]];
            if (m.node != node || (uint32_t)m.diff != diff || m.stapled >= read_offset + len) break;
            take(sorted[lo]); ++found;
        }
        read_offset += len; node_offset = 0;
    }
    return found;
}
// extension x is taken before y: (read_end - read_begin) - 5 * mismatches descending, then number [PARITY-UNPINNED]
VGK_HD int32_t ea_ext_score(const vgk_extension& e) { return (int32_t)(e.read_end - e.read_begin) - 5 * (int32_t)e.n_mismatches; }
VGK_HD bool ea_ext_before(const vgk_extension* e, uint32_t x, uint32_t y) { const int32_t a = ea_ext_score(e[x]), b = ea_ext_score(e[y]); return a > b || (a == b && x < y); }
// sort_anchor_indexes: read start ascending, read end descending, then order of creation [PARITY-UNPINNED]
VGK_HD bool ea_anchor_before(const vgk_chain_anchor* a, uint32_t x, uint32_t y) {
    if (a[x].read_start != a[y].read_start) return a[x].read_start < a[y].read_start;
    if (a[x].length != a[y].length) return a[x].length > a[y].length;
    return x < y;
}
VGK_HD bool ea_used(const uint32_t* used, uint32_t i) { return (used[i >> 5] >> (i & 31u)) & 1u; }

// what a problem's anchors are written through, in order of creation
struct EaOut { vgk_chain_anchor* made; vgk_anchor_origin* origin; uint32_t* rep; uint32_t n_made, n_rep; };

// one anchor interval [a, b) of extension x (:1518-1585): the mismatches inside it, the unused seeds stapled inside it (marked used), the welded anchor
struct EaCursor { uint32_t m_it, s_it; };
VGK_HD void ea_interval(uint32_t a, uint32_t b, uint32_t x, const uint32_t* mm, uint32_t M, const uint32_t* list, uint32_t S, const vgk_anchor_seed* s,
                        const vgk_chain_anchor* seed_anchor, uint32_t* used, int32_t match, int32_t mismatch, EaCursor& c, EaOut& out) {
    while (c.m_it < M && mm[c.m_it] < a) ++c.m_it;
    const uint32_t m0 = c.m_it;
    while (c.m_it < M && mm[c.m_it] < b) ++c.m_it;
    const uint32_t n_mm = c.m_it - m0;
    while (c.s_it < S && s[list[c.s_it]].stapled < a) ++c.s_it;
    uint32_t first = EA_NONE, last = EA_NONE; const uint32_t rep0 = out.n_rep;
    while (c.s_it < S && s[list[c.s_it]].stapled < b) {
        const uint32_t i = list[c.s_it];
        if (!ea_used(used, i)) { used[i >> 5] |= 1u << (i & 31u); if (first == EA_NONE) first = i; last = i; out.rep[out.n_rep++] = i; }
        ++c.s_it;
    }
    if (first == EA_NONE) return;                                   // every seed of the interval stands in an earlier anchor
    const vgk_chain_anchor& f = seed_anchor[first]; const vgk_chain_anchor& l = seed_anchor[last];
    vgk_chain_anchor w;
    w.read_start = f.read_start; w.length = l.read_start + l.length - f.read_start;
    w.margin_before = f.margin_before + ((f.read_start - f.margin_before) - a);                   // (wraps as the reference's size_t does)
    w.margin_after = l.margin_after + (b - (l.read_start + l.length + l.margin_after));
    w.score = match * (int32_t)(b - a - n_mm) - mismatch * (int32_t)n_mm;
    w.start_hint_offset = f.start_hint_offset; w.end_hint_offset = l.end_hint_offset; w.base_seed_length = (f.base_seed_length + l.base_seed_length) / 2u;
    w.start_paths = f.start_paths; w.end_paths = l.end_paths;
    out.made[out.n_made] = w;
    out.origin[out.n_made] = vgk_anchor_origin{first, last, f.read_start + f.length <= l.read_start ? 2u : 1u, rep0, out.n_rep - rep0, x, a, b};
    ++out.n_made;
}
// extension x in its turn: its seeds list[0 .. S) (ea_ext_seeds' order), its mismatches mm[0 .. M)
VGK_HD void ea_extension(const vgk_extension& e, uint32_t x, const uint32_t* mm, const uint32_t* list, uint32_t S, const vgk_anchor_seed* s, const vgk_chain_anchor* seed_anchor,
                         uint32_t* used, int32_t match, int32_t mismatch, EaOut& out) {
    const uint32_t M = e.n_mismatches, rb = e.read_begin, re = e.read_end;
    uint32_t si = 0;                                                // the sweep's seed: the next unused one of the list
    while (si < S && ea_used(used, list[si])) ++si;
    if (si == S) return;                                            // no distinct seeds left
    EaCursor c{0, 0};
    if (!M) { ea_interval(rb, re, x, mm, M, list, S, s, seed_anchor, used, match, mismatch, c, out); return; }
    uint32_t mi = 0, after_prev = M, before_cur = M, interval_start = rb; bool have_prev = false;        // (M = the past-end mismatch)
    for (;;) {
        const bool at_end = si == S;
        if (!at_end && mi < M && mm[mi] < s[list[si]].stapled) {    // next is a mismatch
            if (have_prev && after_prev == M) after_prev = mi;
            before_cur = mi; ++mi;
            continue;
        }
        if (at_end && mi < M) { if (have_prev && after_prev == M) after_prev = mi; before_cur = mi; ++mi; continue; }
        // next is a seed, or the end seed that finishes the last interval
        if (!have_prev) {                                           // the first seed: trim from the left end
            int32_t score = 0, best = 0; uint32_t here = before_cur, cut = here;
            if (here != M) {
                while (here != 0) { const uint32_t next = here - 1; score += (int32_t)(mm[here] - mm[next] - 1u) - 4; if (score > best) { best = score; cut = next; } here = next; }
                score += (int32_t)(mm[here] - rb) - 4;
                if (score > best) { best = score; cut = M; }
            }
            if (cut != M) interval_start = mm[cut] + 1u;
        } else if (after_prev != M) {                               // the first seed after some mismatches: close the previous seed's interval
            const uint32_t split = at_end ? M : after_prev + (before_cur - after_prev + 1u) / 2u;
            int32_t score = 0, best = 0; uint32_t here = after_prev, cut = here;
            while (here != split) {
                const uint32_t next = here + 1;
                score += (int32_t)((next == M ? re : mm[next]) - mm[here] - 1u) - 4;
                if (score > best) { best = score; cut = next; }
                here = next;
            }
            const uint32_t interval_end = cut == M ? re : mm[cut];
            ea_interval(interval_start, interval_end, x, mm, M, list, S, s, seed_anchor, used, match, mismatch, c, out);
            if (!at_end) {
                score = 0; best = 0; here = before_cur; cut = here;
                while (here != split) { const uint32_t next = here - 1; score += (int32_t)(mm[here] - mm[next] - 1u) - 4; if (score > best) { best = score; cut = next; } here = next; }
                interval_start = mm[cut] + 1u;
            }
        } else if (at_end) ea_interval(interval_start, re, x, mm, M, list, S, s, seed_anchor, used, match, mismatch, c, out);
        if (at_end) break;
        have_prev = true; after_prev = M;
        ++si; while (si < S && ea_used(used, list[si])) ++si;
    }
}
// the full-length shortcut (:1408-1464): the good extensions' numbers into rep, ascending; -> their number (0: no shortcut)
VGK_HD uint32_t ea_full_length(const EaProb& q, const vgk_extension* e, uint32_t max_mismatches, uint32_t* rep) {
    uint32_t n = 0;
    if (q.full_length) for (uint32_t x = 0; x < q.n_ext; ++x) if (e[x].left_full && e[x].right_full && e[x].n_mismatches <= max_mismatches) rep[n++] = x;
    return n;
}
// the seeds-only mode: seed i's anchor as anchor i
VGK_HD void ea_from_seed(const vgk_chain_anchor& a, uint32_t i, vgk_chain_anchor* made, vgk_anchor_origin* origin, uint32_t* rep) {
    made[i] = a; rep[i] = i;
    origin[i] = vgk_anchor_origin{i, i, 1u, i, 1u, EA_NONE, a.read_start - a.margin_before, a.read_start + a.length + a.margin_after};
}

// ---- the serial statement of the device's rule for problem p.  Host code; P's arrays are host arrays; sorted / ext_count / ext_first / ext_seeds
// are left alone (the lists are made privately).
inline void ea_problem_one(const EaParams& P, uint32_t p) {
    const EaProb q = P.probs[p];
    const vgk_anchor_seed* s = P.seeds + q.s_off; const vgk_extension* e = P.ext + q.e_off;
    vgk_chain_anchor* sa = P.seed_anchor + q.s_off;
    uint32_t* rep = P.rep + q.s_off + q.e_off;
    P.n_anchors[p] = 0; P.n_rep[p] = 0; P.status[p] = 0;
    for (uint32_t i = 0; i < q.n_seeds; ++i) if (!ea_seed_anchor(s[i], P.n_oriented, P.node_tab, P.match, &sa[i])) { P.flags[0] |= EA_BAD_SEED; return; }
    EaOut out{P.made + q.s_off, P.made_origin + q.s_off, rep, 0, 0};
    if (P.from_seeds) {
        for (uint32_t i = 0; i < q.n_seeds; ++i) ea_from_seed(sa[i], i, out.made, out.origin, rep);
        out.n_made = out.n_rep = q.n_seeds;
    } else {
        const uint32_t n_full = ea_full_length(q, e, P.max_mismatches, rep);
        if (n_full) { P.status[p] = VGK_ANCHORS_FULL_LENGTH; P.n_rep[p] = n_full; return; }
        std::vector<uint32_t> sorted(q.n_seeds), order(q.n_ext), used(q.n_seeds / 32 + 1, 0u);
        for (uint32_t i = 0; i < q.n_seeds; ++i) sorted[i] = i;
        std::sort(sorted.begin(), sorted.end(), [&](uint32_t x, uint32_t y) { return ea_diag_before(s, x, y); });
        std::vector<std::vector<uint32_t>> lists(q.n_ext);
        for (uint32_t x = 0; x < q.n_ext; ++x) ea_ext_seeds(e[x], P.nodes, P.node_tab, s, sorted.data(), q.n_seeds, [&](uint32_t i) { lists[x].push_back(i); });
        for (uint32_t x = 0; x < q.n_ext; ++x) order[x] = x;
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return ea_ext_before(e, x, y); });
        for (uint32_t k = 0; k < q.n_ext; ++k) {
            const uint32_t x = order[k];
            ea_extension(e[x], x, P.mism + e[x].mism_begin, lists[x].data(), (uint32_t)lists[x].size(), s, sa, used.data(), P.match, P.mismatch, out);
        }
    }
    std::vector<uint32_t> by(out.n_made);
    for (uint32_t k = 0; k < out.n_made; ++k) by[k] = k;
    std::sort(by.begin(), by.end(), [&](uint32_t x, uint32_t y) { return ea_anchor_before(out.made, x, y); });
    for (uint32_t k = 0; k < out.n_made; ++k) { P.anchors[q.s_off + k] = out.made[by[k]]; P.origins[q.s_off + k] = out.origin[by[k]]; }
    P.n_anchors[p] = out.n_made; P.n_rep[p] = out.n_rep;
}

}  // namespace vgk
