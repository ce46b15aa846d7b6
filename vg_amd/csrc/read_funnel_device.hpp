// read_funnel_device.hpp — a short read's funnel: the three decisions MinimizerMapper::map_from_extensions makes between the stages the engine already
// runs (src/minimizer_mapper.cpp:650-1128, find_supplementaries == false).  Stated serially here and called by the kernels as they stand:
//
//   rf_walk                process_until_threshold_e (src/minimizer_mapper.hpp:1580-1659) with the escape always false: the items in std::stable_sort
//                          order by a strict comparator; the run of w >= 2 items at the top that the first one does not beat shuffled as
//                          deterministic_shuffle does it (src/utility.hpp:721-728: for i = 1 .. w - 1: swap(x[rng() % (i + 1)], x[i]), w - 1 draws) when the
//                          read has a generator; better_or_equal of position i = one past the end of the run of positions from i on in which no item
//                          beats its successor; cutoff = score(first) - threshold; an item with threshold != 0 && score <= cutoff is processed only while
//                          fewer than min_count items were accepted, otherwise discarded by score; any other item is processed while fewer than max_count
//                          were accepted, otherwise discarded by count; only the items process() answers true for count.
//   rf_cluster_score_one   score_cluster (:4738-4770): present = the distinct minimizers of the cluster's seeds; score = their scores added in ascending
//                          minimizer number; covered = the read bases under some present k-mer (a union, in a bitmap); coverage = covered / length.
//   rf_clusters_one        :650-832: best and second best score, cutoff = best - cluster_score_threshold moved down to min(cutoff, second) when
//                          cutoff - pad_cluster_score_threshold < second (strict); the walk by coverage descending then score descending with
//                          cluster_coverage_threshold, min_extensions, max_extensions; a processed cluster with cluster_score_threshold != 0 &&
//                          score < cutoff && kept >= min_extensions fails the score filter (and does not count); the others are kept, in that order.
//   rf_set_estimate_one    score_extension_group (:5022-5243) as a quadratic recurrence over the set's extensions in the extender's order:
//                          chain[j] = score[j] + max(0, chain[i] for end_i == begin_j, chain[i] - open - extend (begin_j - end_i - 1) for end_i < begin_j,
//                          chain[i] - open - extend (end_i - begin_j) for begin_i < begin_j < end_i), the estimate max(0, chain[]).  Equal to the
//                          reference's sweep (host shim: score_extension_group) on sets sorted by read_begin with non-empty intervals, which the checks demand.
//   rf_sets_one            :887-1063: the walk by estimate descending with extension_set_score_threshold, min_extension_sets, max_alignments; a
//                          processed set whose estimate is below extension_set_min_score is discarded without counting; a set whose gapless result
//                          failed has estimate 0 and is never aligned; the minimizers with a seed in an aligned set's cluster are explored (:1036-1043).
//   rf_winners_one         :1025 per aligned set in walk order: its alignments are kept while the score is non-zero and >= 0.8 x the set's first score
//                          (in double), stopping at the first that fails; nothing kept: one unaligned entry of score 0 (:1065-1068); then the walk of
//                          :1095-1128 by score descending with threshold 0, min 1, max max_multimaps: every score in walk order, the first
//                          min(count, max_multimaps) are the mappings; unmapped = the first one has no mappings (:1146).
//
// The generator: one uint32 per read, the state of its std::minstd_rand; 0 = not made yet, made at the first draw from the read's bytes exactly as
// find_seeds' sort makes it (minimizer_device.hpp: mz_shuffle_seed, mz_minstd_first).  Without one nothing is shuffled.
//
// Working words: a cluster's present bits and covered bitmap ((M + 31) / 32 + (L + 31) / 32 words), a set's chain[] (n_ext words), a walk's order (one
// word per item) — a lane's slice of LDS up to the FN_LDS_* limits (FN_LDS_STRIDE words, odd: the 64 slices start in different banks), a slice of a
// slab in HBM beyond them.
#pragma once
#include <stdint.h>
#include "launch_split.hpp"
#include "read_mapq_device.hpp"
#include "../../include/vgk_engine.h"

namespace vgk {

constexpr uint32_t FN_LDS_MINIMIZERS = 128;                      // minimizers of a read whose clusters' present bits lie in LDS (4 words)
constexpr uint32_t FN_LDS_BASES = 896;                           // bases of a read whose clusters' covered bitmap lies in LDS (28 words)
constexpr uint32_t FN_LDS_ITEMS = 32;                            // items of a walk (clusters, sets, alignments of a read) whose order lies in LDS
constexpr uint32_t FN_LDS_EXT = 32;                              // extensions of a set whose chain[] lies in LDS
constexpr uint32_t FN_LDS_STRIDE = 33;                           // words of a lane's slice
constexpr uint32_t FN_NONE = 0xffffffffu;
enum { FN_RUN_CLUSTER_SCORE, FN_RUN_CLUSTER_WALK, FN_RUN_SET_ESTIMATE, FN_RUN_SET_WALK, FN_RUN_WINNER_WALK, FN_RUN_GATHER };

VGK_HD uint64_t fn_cluster_words(uint64_t minimizers, uint64_t bases) { return (minimizers + 31) / 32 + (bases + 31) / 32; }
VGK_HD bool fn_cluster_large(uint64_t minimizers, uint64_t bases) { return minimizers > FN_LDS_MINIMIZERS || bases > FN_LDS_BASES; }

struct FnParams {
    vgk_funnel_policy pol; int32_t gap_open, gap_extend; int what;
    uint32_t n_reads;
    const char* reads; const uint64_t* read_off; uint32_t* rng_state;      // rng_state null: no generator, nothing shuffled
    const int32_t* status;                                       // the checks' verdicts per read (null: every read passed)
    const uint64_t* min_off; const vgk_read_minimizer* mins; const double* min_score;
    const uint64_t* cluster_off; const uint64_t* cluster_seed_off; const uint32_t* sources; vgk_funnel_cluster* clusters;
    const uint64_t* kept_off; const uint32_t* kept;              // the set call: a read's sets are its kept clusters, set s of cluster kept[s]
    const vgk_gapless_result* res; const vgk_extension* ext; vgk_funnel_set* sets; uint8_t* explored;
    const uint64_t* aligned_off; const uint64_t* aln_off; const int32_t* aln_score; const uint32_t* aln_mappings;      // the winner call
    const uint64_t* flat_off; int32_t* flat_score; vgk_funnel_pick* flat_pick; int32_t* sorted_score; vgk_funnel_pick* sorted_pick;
    uint32_t* n_reported; uint8_t* unmapped;
    uint32_t* tmp; uint32_t* count;                              // a walk's accepted items at the read's first item, and their number
    // FN_RUN_GATHER: per read count[r] elements of `gather_words` words from src + gather_words * src_off[r] to dst + gather_words * first[r]
    const uint64_t* src_off; const uint32_t* first; const uint32_t* src; uint32_t* dst; uint32_t gather_words;
    const uint32_t* ids; uint32_t n;                             // the items of a launch
    uint32_t* work; const uint64_t* work_off;                    // the slab of the items beyond the LDS limits, a slice per item of the launch
};

// ---- the generator ----------------------------------------------------------------------------------------------------------------------------------
struct RfRng {
    bool on; uint32_t x; const char* seq; uint32_t L;
    VGK_HD uint32_t draw() {
        if (!x) { bool masked; x = mz_minstd_first(mz_shuffle_seed(seq, L, masked)); }
        x = mz_minstd_next(x);
        return x;
    }
};
VGK_HD RfRng rf_rng_of(const FnParams& P, uint32_t r) {
    RfRng g; g.on = P.rng_state != nullptr; g.x = g.on ? P.rng_state[r] : 0u; g.seq = P.reads ? P.reads + P.read_off[r] : nullptr; g.L = (uint32_t)(P.read_off[r + 1] - P.read_off[r]);
    return g;
}
VGK_HD void rf_rng_keep(const FnParams& P, uint32_t r, const RfRng& g) { if (g.on) P.rng_state[r] = g.x; }

// ---- the walk ---------------------------------------------------------------------------------------------------------------------------------------
// before(a, b): item a must come before item b; score(a): what the threshold is held against; placed(item, position, better_or_equal) for every item
// in walk order, just before its fate: process(item) -> accepted, by_count(item) or by_score(item)
template <class Before, class Score, class Placed, class Process, class ByCount, class ByScore>
VGK_HD void rf_walk(uint32_t n, uint32_t* order, Before before, Score score, double threshold, uint32_t min_count, uint32_t max_count, RfRng& rng,
                    Placed placed, Process process, ByCount by_count, ByScore by_score) {
    for (uint32_t i = 0; i < n; ++i) {                           // std::stable_sort's result: an item moves past those it beats, and no further
        uint32_t j = i;
        while (j > 0 && before(i, order[j - 1])) { order[j] = order[j - 1]; --j; }
        order[j] = i;
    }
    uint32_t ties = 0;
    while (ties < n && !before(order[0], order[ties])) ++ties;
    if (rng.on) for (uint32_t i = 1; i < ties; ++i) { const uint32_t j = rng.draw() % (i + 1u); const uint32_t t = order[j]; order[j] = order[i]; order[i] = t; }
    const double cutoff = n ? score(order[0]) - threshold : 0.0;
    uint32_t unskipped = 0, run_end = 0;                         // run_end: better_or_equal of the positions before it
    for (uint32_t i = 0; i < n; ++i) {
        if (i >= run_end) { run_end = i + 1; while (run_end < n && !before(order[run_end - 1], order[run_end])) ++run_end; }
        const uint32_t item = order[i];
        placed(item, i, run_end);
        if (threshold != 0 && score(item) <= cutoff) {
            if (unskipped < min_count) unskipped += process(item) ? 1u : 0u;
            else by_score(item);
        } else {
            if (unskipped < max_count) unskipped += process(item) ? 1u : 0u;
            else by_count(item);
        }
    }
}

VGK_HD uint32_t rf_length(const FnParams& P, const vgk_read_minimizer& m) { return (P.pol.flags & VGK_FUNNEL_OWN_LENGTH) ? m.reserved : P.pol.k; }
VGK_HD bool rf_finite(double x) { return x - x == 0.0; }
VGK_HD bool rf_refused(const FnParams& P, uint32_t r) { return P.status && P.status[r] != VGK_OK; }

// ---- the checks (host): a call's own — the policy, then offsets that ascend from 0 and carry no more than a 32-bit index holds ---------------------------
inline int rf_check_policy(const vgk_funnel_policy* p) {
    if (!p || (p->flags & ~(uint32_t)VGK_FUNNEL_OWN_LENGTH)) return VGK_EINVAL;
    if (!rf_finite(p->cluster_score_threshold) || !rf_finite(p->pad_cluster_score_threshold) || !rf_finite(p->cluster_coverage_threshold) || !rf_finite(p->extension_set_score_threshold)) return VGK_EINVAL;
    return VGK_OK;
}
inline int rf_check_offsets(const uint64_t* off, uint64_t n) {                          // off[0 .. n]
    if (!off || off[0] != 0) return VGK_EINVAL;
    for (uint64_t i = 0; i < n; ++i) if (off[i + 1] < off[i]) return VGK_EINVAL;
    return off[n] > INDEX_MOST ? VGK_ETOOBIG : VGK_OK;
}
inline int rf_check_reads(const uint64_t* read_off, uint32_t n) {
    const int rc = rf_check_offsets(read_off, n);
    for (uint32_t r = 0; !rc && r < n; ++r) if (read_off[r + 1] - read_off[r] > 0x3fffffffull) return VGK_ETOOBIG;
    return rc;
}
inline int rf_check_clusters_call(const vgk_funnel_policy* p, uint32_t n, const char* reads, const uint64_t* read_off, const uint64_t* minimizer_off,
                                  const uint64_t* cluster_off, const uint64_t* cluster_seed_off, const uint32_t* rng_state) {
    int rc = rf_check_policy(p);
    if (rc || !n) return rc;
    if (n > INDEX_MOST) return VGK_ETOOBIG;
    if (rng_state && !reads) return VGK_EINVAL;
    if ((rc = rf_check_reads(read_off, n)) || (rc = rf_check_offsets(minimizer_off, n)) || (rc = rf_check_offsets(cluster_off, n))) return rc;
    return rf_check_offsets(cluster_seed_off, cluster_off[n]);
}
inline int rf_check_sets_call(const vgk_funnel_policy* p, uint32_t n, const char* reads, const uint64_t* read_off, const uint64_t* set_off, const uint64_t* kept_off,
                              const uint64_t* cluster_seed_off, uint64_t n_clusters, uint64_t n_extensions, const uint64_t* minimizer_off, const uint32_t* rng_state) {
    int rc = rf_check_policy(p);
    if (rc || !n) return rc;
    if (n > INDEX_MOST || n_clusters > INDEX_MOST || n_extensions > INDEX_MOST) return VGK_ETOOBIG;
    if (rng_state && !reads) return VGK_EINVAL;
    if ((rc = rf_check_reads(read_off, n)) || (rc = rf_check_offsets(minimizer_off, n)) || (rc = rf_check_offsets(kept_off, n)) || (rc = rf_check_offsets(set_off, n))) return rc;
    for (uint32_t r = 0; r <= n; ++r) if (set_off[r] != kept_off[r]) return VGK_EINVAL;
    return rf_check_offsets(cluster_seed_off, n_clusters);
}
inline int rf_check_winners_call(const vgk_funnel_policy* p, uint32_t n, const char* reads, const uint64_t* read_off, const uint64_t* aligned_off, const uint64_t* aln_off,
                                 const uint32_t* rng_state) {
    int rc = rf_check_policy(p);
    if (rc) return rc;
    if (!p->max_multimaps) return VGK_EINVAL;                    // (the reference stops on a read without a mapping)
    if (!n) return VGK_OK;
    if (n > INDEX_MOST) return VGK_ETOOBIG;
    if (rng_state && !reads) return VGK_EINVAL;
    if ((rc = rf_check_reads(read_off, n)) || (rc = rf_check_offsets(aligned_off, n))) return rc;
    if ((rc = rf_check_offsets(aln_off, aligned_off[n]))) return rc;
    return aln_off[aligned_off[n]] + n > INDEX_MOST ? VGK_ETOOBIG : VGK_OK;      // (every read may add its one unaligned entry)
}
// ---- what must hold before any lane touches read r -------------------------------------------------------------------------------------------------------
inline int32_t rf_validate_clusters_read(const FnParams& P, uint32_t r) {
    const uint64_t L = P.read_off[r + 1] - P.read_off[r], mlo = P.min_off[r], M = P.min_off[r + 1] - mlo;
    if (P.cluster_off[r + 1] > P.cluster_off[r] && !L) return VGK_EINVAL;                 // (the reference would divide by 0)
    for (uint64_t j = 0; j < M; ++j) {
        if (!rf_finite(P.min_score[mlo + j])) return VGK_EINVAL;
        if ((uint64_t)P.mins[mlo + j].offset + rf_length(P, P.mins[mlo + j]) > L) return VGK_EINVAL;
    }
    for (uint64_t s = P.cluster_seed_off[P.cluster_off[r]]; s < P.cluster_seed_off[P.cluster_off[r + 1]]; ++s) if (P.sources[s] >= M) return VGK_EINVAL;
    return VGK_OK;
}
inline int32_t rf_validate_sets_read(const FnParams& P, uint32_t r, uint64_t n_extensions, uint64_t n_clusters) {
    const uint64_t L = P.read_off[r + 1] - P.read_off[r], M = P.min_off[r + 1] - P.min_off[r];
    for (uint64_t s = P.kept_off[r]; s < P.kept_off[r + 1]; ++s) {
        const uint32_t c = P.kept[s];
        if (c >= n_clusters) return VGK_EINVAL;
        for (uint64_t q = P.cluster_seed_off[c]; q < P.cluster_seed_off[c + 1]; ++q) if (P.sources[q] >= M) return VGK_EINVAL;
        const vgk_gapless_result g = P.res[s];
        if (g.status != VGK_OK) continue;
        if ((uint64_t)g.ext_begin + g.n_ext > n_extensions) return VGK_EINVAL;
        for (uint32_t x = 0; x < g.n_ext; ++x) {
            const vgk_extension& e = P.ext[g.ext_begin + x];
            if (e.read_begin >= e.read_end || e.read_end > L || (x && e.read_begin < P.ext[g.ext_begin + x - 1].read_begin)) return VGK_EINVAL;
        }
    }
    return VGK_OK;
}

// ---- clusters -----------------------------------------------------------------------------------------------------------------------------------------
VGK_HD void rf_cluster_score_one(const FnParams& P, uint32_t c, uint32_t* work) {
    const uint32_t r = mq_read_of(P.cluster_off, P.n_reads, c);
    vgk_funnel_cluster out; out.score = 0.0; out.coverage = 0.0; out.covered = 0; out.rank = 0; out.better_or_equal = 0; out.verdict = VGK_FUNNEL_UNDECIDED;
    if (rf_refused(P, r)) { P.clusters[c] = out; return; }
    const uint64_t mlo = P.min_off[r]; const uint32_t M = (uint32_t)(P.min_off[r + 1] - mlo), L = (uint32_t)(P.read_off[r + 1] - P.read_off[r]);
    const uint32_t pw = (M + 31) / 32, cw = (L + 31) / 32;
    uint32_t* present = work; uint32_t* covered = work + pw;
    for (uint32_t i = 0; i < pw + cw; ++i) work[i] = 0;
    for (uint64_t s = P.cluster_seed_off[c]; s < P.cluster_seed_off[c + 1]; ++s) { const uint32_t src = P.sources[s]; present[src >> 5] |= 1u << (src & 31u); }
    for (uint32_t j = 0; j < M; ++j) {
        if (!(present[j >> 5] >> (j & 31u) & 1u)) continue;
        out.score += P.min_score[mlo + j];
        const vgk_read_minimizer m = P.mins[mlo + j];
        const uint32_t len = rf_length(P, m);
        if (!len) continue;
        const uint32_t first = m.offset, last = m.offset + len - 1;                      // (the checks: last < L)
        for (uint32_t w = first >> 5; w <= last >> 5; ++w) {
            uint32_t mask = 0xffffffffu;
            if (w == first >> 5) mask &= 0xffffffffu << (first & 31u);
            if (w == last >> 5) mask &= 0xffffffffu >> (31u - (last & 31u));
            covered[w] |= mask;
        }
    }
    for (uint32_t w = 0; w < cw; ++w) out.covered += (uint32_t)__builtin_popcount(covered[w]);
    out.coverage = (double)out.covered / (double)L;
    P.clusters[c] = out;
}

VGK_HD void rf_clusters_one(const FnParams& P, uint32_t r, uint32_t* order) {
    const uint64_t lo = P.cluster_off[r]; const uint32_t C = (uint32_t)(P.cluster_off[r + 1] - lo);
    P.count[r] = 0;
    if (rf_refused(P, r)) return;
    vgk_funnel_cluster* cl = P.clusters + lo;
    double best = 0.0, second = 0.0;                             // (:655-671)
    for (uint32_t i = 0; i < C; ++i) {
        if (cl[i].score > best) { second = best; best = cl[i].score; }
        else if (cl[i].score > second) second = cl[i].score;
    }
    double cutoff = best - P.pol.cluster_score_threshold;        // (:685-688)
    if (cutoff - P.pol.pad_cluster_score_threshold < second) cutoff = cutoff < second ? cutoff : second;
    RfRng rng = rf_rng_of(P, r);
    uint32_t kept = 0;
    rf_walk(C, order,
        [&](uint32_t a, uint32_t b) { return cl[a].coverage > cl[b].coverage || (cl[a].coverage == cl[b].coverage && cl[a].score > cl[b].score); },
        [&](uint32_t a) { return cl[a].coverage; }, P.pol.cluster_coverage_threshold, P.pol.min_extensions, P.pol.max_extensions, rng,
        [&](uint32_t a, uint32_t at, uint32_t boe) { cl[a].rank = at; cl[a].better_or_equal = boe; },
        [&](uint32_t a) {
            if (P.pol.cluster_score_threshold != 0 && cl[a].score < cutoff && kept >= P.pol.min_extensions) { cl[a].verdict = VGK_FUNNEL_FAIL_SCORE; return false; }      // (:746-747)
            cl[a].verdict = VGK_FUNNEL_EXTEND; P.tmp[lo + kept] = (uint32_t)(lo + a); ++kept;
            return true;
        },
        [&](uint32_t a) { cl[a].verdict = VGK_FUNNEL_FAIL_MAX_EXTENSIONS; },
        [&](uint32_t a) { cl[a].verdict = VGK_FUNNEL_FAIL_COVERAGE; });
    rf_rng_keep(P, r, rng);
    P.count[r] = kept;
}

// ---- extension sets -----------------------------------------------------------------------------------------------------------------------------------
VGK_HD void rf_set_estimate_one(const FnParams& P, uint32_t s, uint32_t* work) {
    const uint32_t r = mq_read_of(P.kept_off, P.n_reads, s);
    vgk_funnel_set out; out.estimate = 0; out.rank = 0; out.better_or_equal = 0; out.verdict = VGK_FUNNEL_UNDECIDED;
    if (rf_refused(P, r)) { P.sets[s] = out; return; }
    const vgk_gapless_result g = P.res[s];
    const uint32_t L = (uint32_t)(P.read_off[r + 1] - P.read_off[r]);
    if (g.status != VGK_OK) out.verdict = VGK_FUNNEL_SET_FAILED;
    else if (!g.n_ext) out.estimate = 0;
    else if (g.full_length) out.estimate = P.ext[g.ext_begin].score;
    else if (L) {
        const vgk_extension* e = P.ext + g.ext_begin;
        int32_t* chain = (int32_t*)work; int64_t best_ever = 0;
        for (uint32_t j = 0; j < g.n_ext; ++j) {
            int64_t best = 0; const int64_t b = e[j].read_begin;
            for (uint32_t i = 0; i < j; ++i) {
                const int64_t bi = e[i].read_begin, ei = e[i].read_end; int64_t via;
                if (ei == b) via = chain[i];
                else if (ei < b) via = (int64_t)chain[i] - P.gap_open - (int64_t)P.gap_extend * (b - ei - 1);
                else if (bi < b) via = (int64_t)chain[i] - P.gap_open - (int64_t)P.gap_extend * (ei - b);
                else continue;
                if (via > best) best = via;
            }
            chain[j] = (int32_t)(best + e[j].score);
            if (chain[j] > best_ever) best_ever = chain[j];
        }
        out.estimate = (int32_t)best_ever;
    }
    P.sets[s] = out;
}

VGK_HD void rf_sets_one(const FnParams& P, uint32_t r, uint32_t* order) {
    const uint64_t lo = P.kept_off[r]; const uint32_t S = (uint32_t)(P.kept_off[r + 1] - lo);
    P.count[r] = 0;
    for (uint64_t j = P.min_off[r]; j < P.min_off[r + 1]; ++j) P.explored[j] = 0;
    if (rf_refused(P, r)) return;
    vgk_funnel_set* st = P.sets + lo;
    RfRng rng = rf_rng_of(P, r);
    uint32_t aligned = 0;
    rf_walk(S, order,
        [&](uint32_t a, uint32_t b) { return st[a].estimate > st[b].estimate; },
        [&](uint32_t a) { return (double)st[a].estimate; }, P.pol.extension_set_score_threshold, P.pol.min_extension_sets, P.pol.max_alignments, rng,
        [&](uint32_t a, uint32_t at, uint32_t boe) { st[a].rank = at; st[a].better_or_equal = boe; },
        [&](uint32_t a) {
            if (st[a].verdict == VGK_FUNNEL_SET_FAILED) return false;
            if (st[a].estimate < P.pol.extension_set_min_score) { st[a].verdict = VGK_FUNNEL_SET_FAIL_MIN_SCORE; return false; }      // (:912-916)
            st[a].verdict = VGK_FUNNEL_SET_ALIGN; P.tmp[lo + aligned] = (uint32_t)(lo + a); ++aligned;
            const uint32_t c = P.kept[lo + a];
            for (uint64_t q = P.cluster_seed_off[c]; q < P.cluster_seed_off[c + 1]; ++q) P.explored[P.min_off[r] + P.sources[q]] = 1;      // (:1036-1043)
            return true;
        },
        [&](uint32_t a) { if (st[a].verdict != VGK_FUNNEL_SET_FAILED) st[a].verdict = VGK_FUNNEL_SET_FAIL_MAX_ALIGNMENTS; },
        [&](uint32_t a) { if (st[a].verdict != VGK_FUNNEL_SET_FAILED) st[a].verdict = VGK_FUNNEL_SET_FAIL_SCORE; });
    rf_rng_keep(P, r, rng);
    P.count[r] = aligned;
}

// ---- winners --------------------------------------------------------------------------------------------------------------------------------------------
// the most items read r's winner walk can have: the alignments of its aligned sets, or the one unaligned entry
VGK_HD uint64_t rf_winner_bound(const uint64_t* aligned_off, const uint64_t* aln_off, uint32_t r) {
    const uint64_t most = aln_off[aligned_off[r + 1]] - aln_off[aligned_off[r]];
    return most ? most : 1;
}
VGK_HD void rf_winners_one(const FnParams& P, uint32_t r, uint32_t* order) {
    const uint64_t f = P.flat_off[r];
    uint32_t A = 0;
    for (uint64_t j = P.aligned_off[r]; j < P.aligned_off[r + 1]; ++j) {                // (:1025)
        const uint64_t lo = P.aln_off[j], hi = P.aln_off[j + 1];
        for (uint64_t t = lo; t < hi; ++t) {
            const int32_t sc = P.aln_score[t];
            if (!(sc != 0 && (double)sc >= (double)P.aln_score[lo] * 0.8)) break;
            P.flat_score[f + A] = sc; P.flat_pick[f + A].set = (uint32_t)j; P.flat_pick[f + A].alignment = (uint32_t)(t - lo); ++A;
        }
    }
    if (!A) { P.flat_score[f] = 0; P.flat_pick[f].set = FN_NONE; P.flat_pick[f].alignment = FN_NONE; A = 1; }      // (:1065-1068)
    RfRng rng = rf_rng_of(P, r);
    uint32_t reported = 0;
    rf_walk(A, order,
        [&](uint32_t a, uint32_t b) { return P.flat_score[f + a] > P.flat_score[f + b]; },
        [&](uint32_t a) { return (double)P.flat_score[f + a]; }, 0.0, 1u, P.pol.max_multimaps, rng,
        [&](uint32_t a, uint32_t at, uint32_t) { P.sorted_score[f + at] = P.flat_score[f + a]; P.sorted_pick[f + at] = P.flat_pick[f + a]; },
        [&](uint32_t) { ++reported; return true; },
        [&](uint32_t) {},
        [&](uint32_t) {});
    rf_rng_keep(P, r, rng);
    const vgk_funnel_pick top = P.sorted_pick[f];
    P.unmapped[r] = top.set == FN_NONE || P.aln_mappings[P.aln_off[top.set] + top.alignment] == 0 ? 1 : 0;      // (:1146)
    P.n_reported[r] = reported;
    P.count[r] = A;
}

VGK_HD void rf_gather_one(const FnParams& P, uint32_t r) {
    const uint32_t w = P.gather_words;
    const uint32_t* from = P.src + (uint64_t)w * P.src_off[r]; uint32_t* to = P.dst + (uint64_t)w * P.first[r];
    for (uint64_t i = 0; i < (uint64_t)w * P.count[r]; ++i) to[i] = from[i];
}

// one item of a launch: a cluster, a set or a read, by P.what
VGK_HD void rf_item_one(const FnParams& P, uint32_t item, uint32_t* work) {
    switch (P.what) {
        case FN_RUN_CLUSTER_SCORE: rf_cluster_score_one(P, item, work); break;
        case FN_RUN_CLUSTER_WALK: rf_clusters_one(P, item, work); break;
        case FN_RUN_SET_ESTIMATE: rf_set_estimate_one(P, item, work); break;
        case FN_RUN_SET_WALK: rf_sets_one(P, item, work); break;
        case FN_RUN_WINNER_WALK: rf_winners_one(P, item, work); break;
        default: break;
    }
}

}  // namespace vgk
