// read_mapq_device.hpp — a read's mapping quality: what both mapping routes close with (MinimizerMapper::map, src/minimizer_mapper.cpp:1143-1188;
// map_from_chains, src/minimizer_mapper_from_chains.cpp:957-1057).  Two rules, each stated serially here and called by the kernels as they stand:
//
//   mq_region_one   a minimizer's agglomeration — the stretch of consecutive windows in which that instance is the window's minimizer
//                   (src/minimizer_mapper.hpp:565-600, filled at src/minimizer_mapper.cpp:3927-3957) — from the list alone.  Window s is k-mers
//                   [s, s + w); its minimizer is the leftmost smallest canonical hash among its valid k-mers (minimizer_device.hpp), and every winner is
//                   in the list.  The winners' offsets never decrease from window to window, so an instance's windows are one run, bounded by its
//                   two neighbours in the list: instance i at k-mer b_i wins from window
//                       first_i = max(0, b_i - w + 1, hash_i < hash_{i-1} ? 0 : b_{i-1} + 1)
//                   (the first window that holds it; behind its predecessor unless it beats it — and then no earlier instance is in that window
//                   either: one with a hash <= hash_i would have kept every window that also holds i - 1) until
//                       last_i = min(b_i, first_{i+1} - 1, last window).
//                   Nothing depends on how the list was scanned (the list kernel cuts long reads into stretches of windows).
//   mq_read_one     the mapping quality of the alignments' scores (MappingQualityCalculator::maximum_mapping_quality_exact,
//                   src/mapping_quality_calculator.cpp:26-139), capped by faster_cap over the explored minimizers (src/minimizer_mapper.cpp:2946-3260), the
//                   escape bonus, round, clamp.  faster_cap's sweep (for_each_agglomeration_interval) keeps a deque of open agglomerations: in the
//                   explored order — by (agglomeration end, start) — the open set is always a contiguous range, so the deque is a pair of indices.
//   mq_cap_one      that cap alone, with the sweep's verdict, for the paired rule (pair_mapq_device.hpp), which sums two reads' caps and has no scores
//                   of a read's own; the quality formula is stated once, as a running sum (mq_sum_*), for both rules.
//
// Arithmetic: phred_to_prob and prob_for_at_least_one are tables the HOST makes with the shim's own expressions (read_mapq_tables below) and hands
// over; no pow is evaluated here.  The OR chain p + q - p q and the column products are not contracted to FMA (MQ_NO_CONTRACT: hipcc contracts by
// default in device code), so that shim, serial statement and kernel agree bit for bit up to log10 (one per interval) and the exp / log1p / log of
// the score half, which are the platform's library's.
//
// Working words of a read with E explored minimizers (mq_work_words): order[E] — bucket << 24 | index in the read's list, bucket = the hash's top
// 8 bits, which is all prob_for_at_least_one reads of it — then c[E + 1] as pairs of 32-bit words (a lane's slice starts at an odd word).
#pragma once
#include <math.h>
#include <stdint.h>
#include "minimizer_device.hpp"
#include "../../include/vgk_engine.h"

#if defined(__clang__)
#define MQ_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MQ_NO_CONTRACT
#endif

namespace vgk {

constexpr uint32_t MQ_LDS_EXPLORED = 64;                         // explored minimizers of a read swept in LDS (the short-read seeding cap)
constexpr uint32_t MQ_LDS_STRIDE = 3 * MQ_LDS_EXPLORED + 3;      // words of a lane's slice: order, c[] as pairs, one pad — odd, so that the 64 slices start in different banks
constexpr uint32_t MQ_MAX_EVENTS = 32, MQ_PRECISION = 8;         // src/statistics.hpp:176-178
constexpr uint32_t MQ_MAX_READ_MINIMIZERS = 1u << 24;            // (an order word holds the index in 24 bits)
constexpr uint32_t MQ_PHRED_ENTRIES = 256, MQ_EVENT_ENTRIES = (MQ_MAX_EVENTS + 1) << MQ_PRECISION;
constexpr int32_t MQ_INT32_MAX = 0x7fffffff;
VGK_HD uint64_t mq_work_words(uint64_t explored) { return 3 * explored + 2; }

struct MqRegionParams {
    uint32_t k, w, n_reads;
    uint64_t n_minimizers;
    const uint64_t* read_off; const uint64_t* min_off; const vgk_read_minimizer* mins;
    vgk_minimizer_region* out;
};

struct MqParams {
    double log_base, score_scale, quality_scale;                 // quality_scale = 10 / ln 10, as the host's library rounds it
    uint32_t score_window, k, flags, n_reads;
    const uint64_t* score_off; const int32_t* scores; const double* mult; const uint8_t* unmapped;
    const uint64_t* min_off; const vgk_read_minimizer* mins; const vgk_minimizer_region* regions; const uint8_t* explored;
    const uint64_t* read_off; const uint8_t* qual;
    const double* phred; const double* events;                   // read_mapq_tables
    const int32_t* status;                                       // mq_validate_read's verdicts
    const uint32_t* ids; uint32_t n;                             // the reads of a launch
    uint32_t* work; const uint64_t* work_off;                    // the slab of the reads beyond MQ_LDS_EXPLORED, a slice per read of the launch
    vgk_read_mapq_result* out;
    double* cap_out; int32_t* cap_status;                        // a cap-only launch (mq_cap_one): per read the cap and the sweep's verdict, left in HBM
};

// ---- agglomerations ---------------------------------------------------------------------------------------------------------------------------------
// the first window instance j of its read's list wins, given its predecessor (has_prev) — header
VGK_HD uint32_t mq_first_window(const vgk_read_minimizer& m, uint32_t w, bool has_prev, const vgk_read_minimizer& prev) {
    uint32_t first = m.offset + 1 >= w ? m.offset + 1 - w : 0;
    if (has_prev && !(mz_hash(m.key) < mz_hash(prev.key)) && prev.offset + 1 > first) first = prev.offset + 1;      // it took over when its predecessor slid out
    return first;
}
// the read a minimizer belongs to: the last r with min_off[r] <= j
VGK_HD uint32_t mq_read_of(const uint64_t* min_off, uint32_t n_reads, uint64_t j) {
    uint32_t lo = 0, hi = n_reads;
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (min_off[mid] <= j) lo = mid; else hi = mid; }
    return lo;
}
VGK_HD void mq_region_one(const MqRegionParams& P, uint64_t j) {
    const uint32_t r = mq_read_of(P.min_off, P.n_reads, j);
    const uint64_t lo = P.min_off[r], hi = P.min_off[r + 1];
    const uint32_t L = (uint32_t)(P.read_off[r + 1] - P.read_off[r]);
    const uint32_t windows = L - P.k - P.w + 2;                  // (the call's checks: L >= k + w - 1 wherever there is a minimizer)
    const vgk_read_minimizer m = P.mins[j];
    const uint32_t first = mq_first_window(m, P.w, j > lo, P.mins[j > lo ? j - 1 : j]);
    uint32_t end = m.offset < windows - 1 ? m.offset + 1 : windows;      // one past the last window it wins: it slides out, or the read ends
    if (j + 1 < hi) { const uint32_t next = mq_first_window(P.mins[j + 1], P.w, true, m); if (next < end) end = next; }
    vgk_minimizer_region g;
    g.start = first;
    g.length = end > first ? (end - 1 + P.w + P.k - 1) - first : 0;     // (an instance that wins nothing is in no list the list call makes)
    P.out[j] = g;
}

// ---- the mapping quality ----------------------------------------------------------------------------------------------------------------------------
VGK_HD double mq_bits_to_double(uint32_t lo, uint32_t hi) { union { uint64_t u; double d; } x; x.u = (uint64_t)hi << 32 | lo; return x.d; }
VGK_HD double mq_c_get(const uint32_t* c, uint32_t i) { return mq_bits_to_double(c[2 * i], c[2 * i + 1]); }
VGK_HD void mq_c_set(uint32_t* c, uint32_t i, double v) { union { uint64_t u; double d; } x; x.d = v; c[2 * i] = (uint32_t)x.u; c[2 * i + 1] = (uint32_t)(x.u >> 32); }
VGK_HD double mq_infinity() { return mq_bits_to_double(0u, 0x7ff00000u); }
VGK_HD double mq_lowest() { return mq_bits_to_double(0xffffffffu, 0xffefffffu); }            // std::numeric_limits<double>::lowest()
VGK_HD bool mq_is_inf(double x) { return x == mq_infinity() || x == -mq_infinity(); }

VGK_HD uint32_t mq_length(const MqParams& P, const vgk_read_minimizer& m) { return (P.flags & VGK_READ_MAPQ_OWN_LENGTH) ? m.reserved : P.k; }

// What must hold before a lane sweeps read r: the verdict is the read's status, and a read that fails is not swept.  The sweep's own half (all a
// cap-only launch checks: pair_mapq_device.hpp), then the read's
VGK_HD int32_t mq_validate_sweep(const MqParams& P, uint32_t r) {
    if ((P.flags & VGK_READ_MAPQ_NO_EXPLORED_CAP) || !P.qual) return VGK_OK;
    const uint64_t L = P.read_off[r + 1] - P.read_off[r];
    for (uint64_t j = P.min_off[r]; j < P.min_off[r + 1]; ++j) {
        if (!P.explored[j]) continue;
        const uint32_t len = mq_length(P, P.mins[j]);
        if (len == 0 || len > MQ_MAX_EVENTS) return VGK_EINVAL;                               // "minimizer with no sequence" | beyond prob_for_at_least_one's table
        if (P.regions[j].start > L) return VGK_EINVAL;                                        // (the sweep would read qualities behind the read's)
    }
    return VGK_OK;
}
VGK_HD int32_t mq_validate_read(const MqParams& P, uint32_t r) {
    const bool unmapped = P.unmapped && P.unmapped[r];
    if (!unmapped && P.score_off[r + 1] == P.score_off[r]) return VGK_EINVAL;                 // (crash_unless(!mappings.empty()))
    return mq_validate_sweep(P, r);
}
VGK_HD uint32_t mq_count_explored(const MqParams& P, uint32_t r) {
    uint32_t e = 0;
    for (uint64_t j = P.min_off[r]; j < P.min_off[r + 1]; ++j) e += P.explored[j] ? 1u : 0u;
    return e;
}

// MappingQualityCalculator::maximum_mapping_quality_exact over log_base * (scaled score), backwards; first: to_score is the first score's
VGK_HD double mq_add_log(double x, double y) { return x > y ? x + log1p(exp(y - x)) : y + log1p(exp(x - y)); }
// The formula as a running sum, for any list handed over from its LAST score to its first (a read's scores here; a pair's ordered scores, its score
// groups and its mates' unpaired scores in pair_mapq_device.hpp): score = log_base * (the score), m = its multiplicity (1.0: none)
struct MqSum { double log_sum_exp, to_score, front, front_mult; uint64_t n; };
VGK_HD MqSum mq_sum_begin() { MqSum s; s.log_sum_exp = mq_lowest(); s.to_score = mq_lowest(); s.front = 0.0; s.front_mult = 1.0; s.n = 0; return s; }
VGK_HD void mq_sum_add(MqSum& s, double score, double m, bool first) {
    MQ_NO_CONTRACT
    s.front = score; s.front_mult = m; ++s.n;                                                 // (the last one handed over is the list's first)
    if (!first && score >= s.to_score) s.to_score = score;
    if (m > 1.0) score = score + log(m);
    s.log_sum_exp = mq_add_log(s.log_sum_exp, score);
}
// -> the quality after compute_*_mapping_quality's (int32_t): INT32_MAX when infinite — and for a list without scores
VGK_HD double mq_sum_quality(const MqSum& s, bool first, double quality_scale) {
    MQ_NO_CONTRACT
    double log_sum_exp = s.log_sum_exp, to_score = s.to_score;
    if (s.n == 1 && !(s.front_mult > 1.0)) log_sum_exp = mq_add_log(log_sum_exp, 0.0);      // the null alignment
    if (first) to_score = s.front;
    const double direct = -quality_scale * (0.0 + log1p(-exp((to_score - log_sum_exp) - 0.0)));
    const double q = mq_is_inf(direct) ? (double)MQ_INT32_MAX : direct;
    return (double)(int32_t)q;                                                                // compute_*_mapping_quality returns int32_t
}
VGK_HD double mq_uncapped(const MqParams& P, uint32_t r) {
    MQ_NO_CONTRACT
    if (P.unmapped && P.unmapped[r]) return 0.0;                                              // not the 50 % the formula would give
    const uint64_t lo = P.score_off[r], n = P.score_off[r + 1] - lo;
    const uint64_t L = P.read_off[r + 1] - P.read_off[r];
    const bool first = (P.flags & VGK_READ_MAPQ_FIRST) != 0;
    MqSum sum = mq_sum_begin();
    for (uint64_t i = n; i-- > 0;) {
        double scaled = (double)P.scores[lo + i];
        if (P.score_window > 0) scaled = scaled * (double)P.score_window / (double)L;       // (:961-964)
        scaled = scaled * P.score_scale;
        mq_sum_add(sum, P.log_base * scaled, P.mult ? P.mult[lo + i] : 1.0, first);
    }
    return mq_sum_quality(sum, first, P.quality_scale);
}

// the order word of list entry `idx` (relative to the read's first minimizer)
VGK_HD uint32_t mq_order_word(const vgk_read_minimizer& m, uint32_t idx) { return (uint32_t)(mz_hash(m.key) >> (64 - MQ_PRECISION)) << 24 | idx; }
// by agglomeration end, then start (:2957-2962); ties keep list order
VGK_HD bool mq_before(const vgk_minimizer_region* g, uint32_t a, uint32_t b) {
    const uint64_t ae = (uint64_t)g[a].start + g[a].length, be = (uint64_t)g[b].start + g[b].length;
    if (ae != be) return ae < be;
    if (g[a].start != g[b].start) return g[a].start < g[b].start;
    return a < b;
}

// get_prob_of_disruption_in_column (:3203-3260): an error at read base `index` disrupts every one of the open minimizers order[bottom, top)
VGK_HD double mq_column(const MqParams& P, const vgk_read_minimizer* mins, const vgk_minimizer_region* g, const uint8_t* qual, const uint32_t* order,
                        uint32_t bottom, uint32_t top, uint32_t index) {
    MQ_NO_CONTRACT
    double p = P.phred[qual[index]];
    for (uint32_t k = bottom; k < top; ++k) {
        const uint32_t word = order[k], idx = word & 0xffffffu;
        const uint32_t off = mins[idx].offset, len = mq_length(P, mins[idx]);
        if (off <= index && (uint64_t)index < (uint64_t)off + len) continue;                 // inside the k-mer: the error itself disrupts it
        const uint32_t start = g[idx].start, before = index - start + 1;
        const uint64_t after = ((uint64_t)start + g[idx].length) - index;
        uint32_t possible = len < before ? len : before;
        if (after < possible) possible = (uint32_t)after;
        p = p * P.events[(possible << MQ_PRECISION) + (word >> 24)];
    }
    return p;
}

// faster_cap (:2946-3090) with for_each_agglomeration_interval (:3092-3161) inlined: -> the cap; *status = VGK_EINVAL where the reference stops
VGK_HD double mq_explored_cap(const MqParams& P, uint32_t r, uint32_t* work, int32_t* status) {
    MQ_NO_CONTRACT
    if (!P.qual) return mq_infinity();
    const uint64_t lo = P.min_off[r];
    const uint32_t n_min = (uint32_t)(P.min_off[r + 1] - lo), L = (uint32_t)(P.read_off[r + 1] - P.read_off[r]);
    const vgk_read_minimizer* mins = P.mins + lo; const vgk_minimizer_region* g = P.regions + lo; const uint8_t* qual = P.qual + P.read_off[r];
    // the explored minimizers in their order: insertion from the back (lists come nearly sorted: agglomerations advance with the offsets)
    uint32_t E = 0;
    for (uint32_t j = 0; j < n_min; ++j) {
        if (!P.explored[lo + j]) continue;
        uint32_t at = E++;
        while (at > 0 && mq_before(g, j, work[at - 1] & 0xffffffu)) { work[at] = work[at - 1]; --at; }
        work[at] = mq_order_word(mins[j], j);
    }
    const uint32_t* order = work; uint32_t* c = work + E;
    // c[i + 1] = log10 probability that minimizers 0 .. i were all created by errors (:2996-3000)
    mq_c_set(c, 0, 0.0);
    for (uint32_t i = 1; i <= E; ++i) mq_c_set(c, i, -mq_infinity());
    if (E) {
        uint32_t bottom = 0, pushed = 1;                                                      // the open agglomerations: order[bottom, pushed)
        uint32_t left = g[order[0] & 0xffffffu].start;
        for (uint32_t k = 1; k <= E; ++k) {
            if (k < E && pushed == bottom) { *status = VGK_EINVAL; return 0.0; }              // "minimizers not stacked up properly"
            const uint32_t right = k < E ? g[order[k] & 0xffffffu].start : L;
            while (left < right) {                                                            // emit every interval before `right`
                const uint32_t front = order[bottom] & 0xffffffu;
                const uint64_t first_end = (uint64_t)g[front].start + g[front].length;
                const bool closes = first_end <= right;
                if (closes && first_end < left) { *status = VGK_EINVAL; return 0.0; }         // "minimizers not sorted properly"
                const uint32_t to = closes ? (uint32_t)first_end : right, top = pushed;
                double p_here = 0.0;                                                          // a 0-length interval needs no disruption
                if (left != to) {
                    double p = mq_column(P, mins, g, qual, order, bottom, top, left);
                    for (uint32_t i = left + 1; i < to; ++i) { const double q = mq_column(P, mins, g, qual, order, bottom, top, i); p = p + q - p * q; }      // OR, assuming independence
                    p_here = log10(p);
                }
                if (mq_is_inf(p_here)) { *status = VGK_EINVAL; return 0.0; }                  // "minimizers seem impossible to disrupt in a region"
                const double here = mq_c_get(c, bottom) + p_here;
                for (uint32_t i = bottom + 1; i < top + 1; ++i) if (mq_c_get(c, i) < here) mq_c_set(c, i, here);
                if (closes) { left = (pushed - bottom == 1) ? right : (uint32_t)first_end; ++bottom; }      // a single open item: a gap follows it
                else left = right;
            }
            if (k < E) ++pushed;
        }
    }
    const double last = mq_c_get(c, E);
    if (mq_is_inf(last)) { *status = VGK_EINVAL; return 0.0; }                                // "minimizers seem impossible to disrupt"
    return -last * 10.0;
}

// One read: its 24 bytes.  work: mq_work_words(explored minimizers of the read) words of its own; never read for a read that failed the checks
VGK_HD void mq_read_one(const MqParams& P, uint32_t r, uint32_t* work) {
    MQ_NO_CONTRACT
    vgk_read_mapq_result o;
    o.mapq = 0; o.status = P.status[r]; o.uncapped = 0.0; o.explored_cap = 0.0;
    if (o.status == VGK_OK) {
        o.uncapped = mq_uncapped(P, r);
        const double bonus = o.uncapped < (double)MQ_INT32_MAX ? 1.0 : 2.0;                  // the escape bonus
        o.explored_cap = (P.flags & VGK_READ_MAPQ_NO_EXPLORED_CAP) ? mq_infinity() : mq_explored_cap(P, r, work, &o.status);
        if (o.status == VGK_OK) {
            // :1177-1188 is max(min(round(min(cap', min(mapq, 60))), 60), 0) and :1042-1057 max(min(round(min(cap', mapq)), 60), 0) with cap' = bonus * cap
            // (without the cap: mapq, an integer already); 60 is an integer and round is monotone, so both are this one expression
            const double capped = bonus * o.explored_cap;
            double q = round(capped < o.uncapped ? capped : o.uncapped);
            q = q < 0.0 ? 0.0 : q; q = q > 60.0 ? 60.0 : q;
            o.mapq = (int32_t)q;
        } else { o.uncapped = 0.0; o.explored_cap = 0.0; }
    }
    P.out[r] = o;
}
// One read's explored cap alone, as mq_read_one makes it, for a caller that has no scores of the read's own (a pair's mates): P.status holds
// mq_validate_sweep's verdicts.  A read that is refused or on which the sweep stops: cap 0, its verdict in cap_status
VGK_HD void mq_cap_one(const MqParams& P, uint32_t r, uint32_t* work) {
    int32_t status = P.status[r];
    double cap = 0.0;
    if (status == VGK_OK) {
        cap = (P.flags & VGK_READ_MAPQ_NO_EXPLORED_CAP) ? mq_infinity() : mq_explored_cap(P, r, work, &status);
        if (status != VGK_OK) cap = 0.0;
    }
    P.cap_out[r] = cap; P.cap_status[r] = status;
}

// The tables, made on the host with the expressions of vg_amd/host/mapq_cap.cpp (phred_to_prob, prob_for_at_least_one): phred[256],
// events[(MQ_MAX_EVENTS + 1) << MQ_PRECISION]
inline void read_mapq_tables(double* phred, double* events) {
    for (uint32_t q = 0; q < MQ_PHRED_ENTRIES; ++q) phred[q] = pow(10.0, -(double)(uint8_t)q / 10.0);
    const size_t values = (size_t)1 << MQ_PRECISION;
    for (size_t q = 0; q < values; ++q) events[q] = 0.0;
    for (size_t k = 1; k <= MQ_MAX_EVENTS; ++k)
        for (size_t q = 0; q < values; ++q) events[(k << MQ_PRECISION) + q] = 1.0 - pow(1.0 - (2 * q + 1) / (2.0 * values), (double)k);      // the middle of the bucket
}

}  // namespace vgk
