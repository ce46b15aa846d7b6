// pair_mapq_device.hpp — a pair's mapping qualities: what MinimizerMapper::map_paired closes with (src/minimizer_mapper.cpp:2476-2765, with
// score_alignment_pair :6017-6028).  Two rules, each stated serially here and called by the kernels as they stand:
//
//   pm_candidate_score  the score of one candidate pairing: the mates' scores plus the fragment length's log likelihood under N(mean, sd) in the
//                       scorer's log base, never below the worse mate's score — or the mapped mate's score alone where rescue found nothing.
//                       IEEE basic operations only (+ - * / and conversions): every statement of it gives the same bits.
//   pm_pair_one         the candidates in score order (process_until_threshold_a with threshold 0: descending, equal scores in candidate order), the
//                       max_multimaps cut, the quality of all the ordered scores (under the rescue multiplicities when no candidate is PAIRED), the
//                       fragment-cluster cap, the score groups, and per mate the cap both mates share — the two explored caps summed —, the
//                       unpaired cap, the halving for unreachable mates and max(min(capped, 120) / 2, 0).
//
// The quality formula is read_mapq_device.hpp's running sum (mq_sum_*), handed each list from its last score to its first.  The mates' explored caps
// are read from HBM: given by the caller, or left there by a cap-only launch of that header's sweep (mq_cap_one) with each read's verdict.
//
// Working words of a pair with C candidates (pm_work_words): order[C] — the candidate numbers in score order — then the ordered scores as pairs of
// 32-bit words (a lane's slice starts at an odd stride).
#pragma once
#include "read_mapq_device.hpp"

namespace vgk {

constexpr uint32_t PM_LDS_CANDIDATES = 64;                       // candidates of a pair ordered in LDS
constexpr uint32_t PM_LDS_STRIDE = 3 * PM_LDS_CANDIDATES + 1;    // words of a lane's slice: order, the scores as pairs, one pad — odd; 64 slices are 49 408 bytes, three workgroups a CU
constexpr int64_t PM_UNREACHABLE = 0x7fffffffffffffffll;         // std::numeric_limits<int64_t>::max()
VGK_HD uint64_t pm_work_words(uint64_t candidates) { return 3 * candidates; }

struct PmParams {
    double log_base, mean, sd, quality_scale;                    // quality_scale = 10 / ln 10, as the host's library rounds it
    uint32_t max_multimaps, max_rescue_attempts, n_pairs;
    uint64_t n_candidates;
    const uint64_t* cand_off; const vgk_pair_candidate* cands; const vgk_pair_counts* counts;
    const uint64_t* unp_off; const int32_t* unp_scores;          // either null: no mate has unpaired scores
    const double* caps; const int32_t* cap_status;               // per read; caps null: +infinity; cap_status null: the caps were given
    const int32_t* status;                                       // pm_validate_pair's verdicts
    const uint32_t* ids; uint32_t n;                             // the pairs of a launch
    uint32_t* work; const uint64_t* work_off;                    // the slab of the pairs beyond PM_LDS_CANDIDATES, a slice per pair of the launch
    double* pair_score; uint32_t* order; vgk_pair_mapq_result* out;
};

VGK_HD bool pm_is_rescued(uint32_t type) { return type == VGK_PAIR_RESCUED_FROM_FIRST || type == VGK_PAIR_RESCUED_FROM_SECOND; }
VGK_HD uint32_t pm_mapped_mate(uint32_t type) { return type == VGK_PAIR_RESCUED_FROM_FIRST ? 0u : 1u; }      // the mate rescue started from; the other one was rescued
VGK_HD bool pm_aligned(const vgk_pair_candidate& c, uint32_t r) { return ((c.aligned >> r) & 1u) != 0; }
VGK_HD int64_t pm_distance(const vgk_pair_candidate& c) { return c.type == VGK_PAIR_UNPAIRED ? PM_UNREACHABLE : c.distance; }
VGK_HD uint32_t pm_rescue_attempts(const PmParams& P, const vgk_pair_counts& n, uint32_t side) {
    return n.rescued_count[side] < P.max_rescue_attempts ? n.rescued_count[side] : P.max_rescue_attempts;
}

// :2386-2391 | score_alignment_pair (:6017-6028); 0 for a type that is none
VGK_HD double pm_candidate_score(const PmParams& P, const vgk_pair_candidate& c) {
    MQ_NO_CONTRACT
    if (c.type > VGK_PAIR_RESCUED_FROM_SECOND) return 0.0;
    if (pm_is_rescued(c.type) && !pm_aligned(c, 1u - pm_mapped_mate(c.type))) return (double)c.score[pm_mapped_mate(c.type)];       // no rescue result
    const double dev = (double)pm_distance(c) - P.mean;
    const double log_likelihood = (-dev * dev / (2.0 * P.sd * P.sd)) / P.log_base;
    const int32_t both = (int32_t)((uint32_t)c.score[0] + (uint32_t)c.score[1]);                 // the integer sum first, as aln1.score() + aln2.score()
    const double score = (double)both + log_likelihood;
    const double worse_score = (double)(c.score[1] < c.score[0] ? c.score[1] : c.score[0]);
    return score < worse_score ? worse_score : score;                                            // std::max(score, worse_score)
}

// What must hold before a lane takes pair p: the verdict is the pair's status, and a pair that fails is not ordered
VGK_HD int32_t pm_validate_pair(const PmParams& P, uint32_t p) {
    const vgk_pair_counts n = P.counts[p];
    for (uint64_t j = P.cand_off[p]; j < P.cand_off[p + 1]; ++j) {
        const vgk_pair_candidate c = P.cands[j];
        if (c.type > VGK_PAIR_RESCUED_FROM_SECOND) return VGK_EINVAL;
        if (!pm_is_rescued(c.type)) continue;
        if (pm_rescue_attempts(P, n, pm_mapped_mate(c.type)) == 0) return VGK_EINVAL;             // a rescued pair from a side that rescued nothing: its multiplicity divides by 0
        if (!pm_aligned(c, 1u - pm_mapped_mate(c.type)) && c.distance != PM_UNREACHABLE) return VGK_EINVAL;      // (:2390)
    }
    return VGK_OK;
}

// :2660-2685, for the candidate types that have passed pm_validate_pair
VGK_HD double pm_multiplicity(const PmParams& P, const vgk_pair_counts& n, uint32_t type) {
    if (!pm_is_rescued(type)) return 1.0;
    const uint32_t side = pm_mapped_mate(type);
    return n.unpaired_count[side] > 0 ? (double)n.unpaired_count[side] / (double)pm_rescue_attempts(P, n, side) : 1.0;
}

// One pair: its 80 bytes and its stretch of `order`.  work: pm_work_words(candidates of the pair) words of its own; never touched for a pair that is refused
VGK_HD void pm_pair_one(const PmParams& P, uint32_t p, uint32_t* work) {
    MQ_NO_CONTRACT
    const uint64_t lo = P.cand_off[p];
    const uint32_t C = (uint32_t)(P.cand_off[p + 1] - lo);
    vgk_pair_mapq_result o;
    o.mapq[0] = 0; o.mapq[1] = 0; o.status = P.status[p]; o.n_chosen = 0; o.uncapped = 0.0; o.fragment_cluster_cap = 0.0;
    for (uint32_t r = 0; r < 2; ++r) { o.explored_cap[r] = 0.0; o.score_group[r] = 0.0; o.applied_cap[r] = 0.0; }
    if (o.status == VGK_OK && P.cap_status && (P.cap_status[2 * (uint64_t)p] != VGK_OK || P.cap_status[2 * (uint64_t)p + 1] != VGK_OK)) o.status = VGK_EINVAL;      // the sweep stopped on a mate
    if (o.status != VGK_OK) {
        for (uint32_t i = 0; i < C; ++i) P.order[lo + i] = i;
        P.out[p] = o;
        return;
    }
    // the candidates in score order: insertion from the back, an equal score stays behind the earlier candidate
    uint32_t* order = work; uint32_t* sorted = work + C;
    for (uint32_t j = 0; j < C; ++j) {
        const double s = P.pair_score[lo + j];
        uint32_t at = j;
        while (at > 0 && mq_c_get(sorted, at - 1) < s) { order[at] = order[at - 1]; mq_c_set(sorted, at, mq_c_get(sorted, at - 1)); --at; }
        order[at] = j; mq_c_set(sorted, at, s);
    }
    for (uint32_t i = 0; i < C; ++i) P.order[lo + i] = order[i];
    o.n_chosen = C < P.max_multimaps ? C : P.max_multimaps;
    for (uint32_t r = 0; r < 2; ++r) { o.explored_cap[r] = P.caps ? P.caps[2 * (uint64_t)p + r] : mq_infinity(); o.score_group[r] = (double)MQ_INT32_MAX; }
    o.fragment_cluster_cap = mq_infinity();
    if (C) {
        const uint32_t winner = order[0];
        const vgk_pair_candidate win = P.cands[lo + winner];
        const vgk_pair_counts counts = P.counts[p];
        bool found_pair = false;
        for (uint32_t j = 0; j < C; ++j) found_pair = found_pair || P.cands[lo + j].type == VGK_PAIR_PAIRED;
        // :2686-2690: all the scores, under the multiplicities when every pair was rescued (or unpaired)
        const double best = mq_c_get(sorted, 0);
        if (best != 0.0) {
            MqSum sum = mq_sum_begin();
            for (uint32_t i = C; i-- > 0;) mq_sum_add(sum, P.log_base * mq_c_get(sorted, i), found_pair ? 1.0 : pm_multiplicity(P, counts, P.cands[lo + order[i]].type), false);
            o.uncapped = mq_sum_quality(sum, false, P.quality_scale);
        }
        // :2692-2697
        if (win.better_cluster_count > 1) o.fragment_cluster_cap = -10.0 * log10(1.0 - (1.0 / (double)win.better_cluster_count));
        // :2524-2546, :2704: the winner's score, then the other pairs that share its alignment of mate r
        for (uint32_t r = 0; r < 2; ++r) {
            MqSum group = mq_sum_begin();
            if (found_pair) {
                if (win.type == VGK_PAIR_PAIRED)
                    for (uint32_t j = C; j-- > 0;) {
                        const vgk_pair_candidate c = P.cands[lo + j];
                        if (j != winner && c.type == VGK_PAIR_PAIRED && c.aln[r] == win.aln[r]) mq_sum_add(group, P.log_base * P.pair_score[lo + j], 1.0, false);
                    }
                mq_sum_add(group, P.log_base * best, 1.0, false);
            }
            o.score_group[r] = mq_sum_quality(group, false, P.quality_scale);
        }
        // :2727-2765
        const double escape_bonus = o.uncapped < (double)MQ_INT32_MAX ? 1.0 : 2.0;
        const double explored = (o.explored_cap[0] + o.explored_cap[1]) * escape_bonus;
        for (uint32_t r = 0; r < 2; ++r) {
            double mapq_cap = explored < o.fragment_cluster_cap ? explored : o.fragment_cluster_cap;
            if (win.type == VGK_PAIR_UNPAIRED) {                                                 // from two fragment clusters: this mate's unpaired alignments alone
                MqSum alone = mq_sum_begin();
                if (P.unp_off && P.unp_scores)
                    for (uint64_t i = P.unp_off[2 * (uint64_t)p + r + 1]; i-- > P.unp_off[2 * (uint64_t)p + r];) mq_sum_add(alone, P.log_base * (double)P.unp_scores[i], 1.0, false);
                const double q = mq_sum_quality(alone, false, P.quality_scale);
                mapq_cap = q < mapq_cap ? q : mapq_cap;
            }
            o.applied_cap[r] = mapq_cap;
            double capped = o.uncapped < mapq_cap ? o.uncapped : mapq_cap;
            if (pm_distance(win) == PM_UNREACHABLE) capped = capped / 2.0;                      // the two reads are not reachable: lower
            double q = 120.0 < capped ? 120.0 : capped;
            q = q / 2.0;
            q = q < 0.0 ? 0.0 : q;
            o.mapq[r] = pm_aligned(win, r) && q == q ? (int32_t)q : 0;                           // an unaligned read always has 0
        }
    }
    P.out[p] = o;
}

}  // namespace vgk
