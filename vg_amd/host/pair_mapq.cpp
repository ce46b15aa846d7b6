// pair_mapq.cpp — see pair_mapq.hpp.
#include "pair_mapq.hpp"
#include <algorithm>
#include <cmath>
#include <functional>
#include <limits>
#include <numeric>
#include "vg_standin/mapping_quality.hpp"

namespace vgamd {

double score_alignment_pair(const PairMapqScheme& scheme, int32_t score1, int32_t score2, int64_t fragment_distance) {
    //Score a pair of alignments
    double dev = fragment_distance - scheme.fragment_mean;
    double fragment_length_log_likelihood = (-dev * dev / (2.0 * scheme.fragment_sd * scheme.fragment_sd)) / scheme.log_base;
    double score = (int32_t)((uint32_t)score1 + (uint32_t)score2) + fragment_length_log_likelihood;       // (int32 + int32, as aln1.score() + aln2.score())
    //Don't let the fragment length log likelihood bring score down below the score of the best alignment
    double worse_score = std::min(score1, score2);
    return std::max(score, worse_score);
}

double pair_candidate_score(const PairMapqScheme& scheme, const PairCandidate& c) {
    if (c.type == rescued_from_first || c.type == rescued_from_second) {
        const size_t mapped = c.type == rescued_from_first ? 0 : 1;
        // If there's no rescue result, the score of the pair is the score of the one actually-aligned read
        if (!c.aligned[1 - mapped]) return c.score[mapped];
    }
    if (c.type < paired || c.type > rescued_from_second) return 0.0;
    return score_alignment_pair(scheme, c.score[0], c.score[1], c.type == unpaired ? std::numeric_limits<int64_t>::max() : c.fragment_distance);
}

namespace {
// process_until_threshold_a (src/minimizer_mapper.hpp:1580-1659) with threshold 0 and min_count 1: the items in descending score order — ties in index
// order, where the reference shuffles them —, the first max_count processed, the others discarded by count
void process_until_threshold(size_t items, const std::function<double(size_t)>& get_score, size_t max_count,
                             const std::function<bool(size_t)>& process_item, const std::function<void(size_t)>& discard_item_by_count) {
    std::vector<size_t> indexes_in_order(items);
    std::iota(indexes_in_order.begin(), indexes_in_order.end(), (size_t)0);
    std::stable_sort(indexes_in_order.begin(), indexes_in_order.end(), [&](size_t a, size_t b) { return get_score(a) > get_score(b); });
    size_t unskipped = 0;
    for (size_t i = 0; i < indexes_in_order.size(); i++) {
        size_t item_num = indexes_in_order[i];
        if (unskipped < max_count) unskipped += (size_t)process_item(item_num);
        else discard_item_by_count(item_num);
    }
}
}  // namespace

PairMapq pair_mapq(const PairMapqScheme& scheme, const std::vector<PairCandidate>& candidates, const std::array<size_t, 2>& unpaired_count,
                   const std::array<size_t, 2>& rescued_count, const std::array<std::vector<double>, 2>& unpaired_scores, const std::array<double, 2>& explored_caps) {
    PairMapq out;
    out.order.resize(candidates.size());
    std::iota(out.order.begin(), out.order.end(), (size_t)0);
    std::vector<double> paired_scores; std::vector<int64_t> fragment_distances; std::vector<int> pair_types; std::vector<size_t> better_cluster_count_by_pairs;
    bool found_pair = false;
    for (const PairCandidate& c : candidates) {
        paired_scores.push_back(pair_candidate_score(scheme, c));
        fragment_distances.push_back(c.type == unpaired ? std::numeric_limits<int64_t>::max() : c.fragment_distance);
        pair_types.push_back(c.type);
        better_cluster_count_by_pairs.push_back(c.better_cluster_count);
        found_pair = found_pair || c.type == paired;
    }
    out.paired_scores = paired_scores;
    auto stop = [&](const std::string& why) { out.stopped = true; out.why = why; return out; };
    for (const PairCandidate& c : candidates) {
        if (c.type < paired || c.type > rescued_from_second) return stop("a pair type that is none");
        if (c.type == rescued_from_first || c.type == rescued_from_second) {
            const size_t mapped = c.type == rescued_from_first ? 0 : 1;
            if (std::min(rescued_count[mapped], scheme.max_rescue_attempts) == 0) return stop("a rescued pair from a read that rescued nothing");
            if (!c.aligned[1 - mapped] && c.fragment_distance != std::numeric_limits<int64_t>::max()) return stop("no rescue result, yet a fragment distance");
        }
    }

    // Grab all the scores in order for MAPQ computation.
    std::vector<double> scores;
    std::array<std::vector<double>, 2> scores_group;
    std::vector<int64_t> distances;
    std::vector<int> types;
    std::vector<size_t> better_cluster_count_by_mappings;
    std::vector<size_t> mappings, in_order;
    process_until_threshold(candidates.size(), [&](size_t i) -> double { return paired_scores[i]; }, scheme.max_multimaps, [&](size_t alignment_num) {
        // This alignment makes it.  Called in score order
        scores.emplace_back(paired_scores[alignment_num]);
        distances.emplace_back(fragment_distances[alignment_num]);
        types.emplace_back(pair_types[alignment_num]);
        better_cluster_count_by_mappings.emplace_back(better_cluster_count_by_pairs[alignment_num]);
        mappings.emplace_back(alignment_num); in_order.emplace_back(alignment_num);
        if (mappings.size() == 1 && found_pair) {
            //If this is the best pair of alignments that we're going to return and we didn't attempt rescue, get the group scores for mapq
            for (auto r : {0, 1}) scores_group[r].push_back(paired_scores[alignment_num]);
            //The pairs with the same first/second read as this (alignment_groups: only a paired pair joins its alignments' groups)
            if (pair_types[alignment_num] == paired)
                for (auto r : {0, 1})
                    for (size_t other_alignment_num = 0; other_alignment_num < candidates.size(); ++other_alignment_num)
                        if (other_alignment_num != alignment_num && pair_types[other_alignment_num] == paired
                            && candidates[other_alignment_num].alignment[r] == candidates[alignment_num].alignment[r]) scores_group[r].push_back(paired_scores[other_alignment_num]);
        }
        return true;
    }, [&](size_t alignment_num) {
        // We already have enough alignments, although this one has a good score.  Remember the score at its rank anyway
        scores.emplace_back(paired_scores[alignment_num]);
        distances.emplace_back(fragment_distances[alignment_num]);
        types.emplace_back(pair_types[alignment_num]);
        better_cluster_count_by_mappings.emplace_back(better_cluster_count_by_pairs[alignment_num]);
        in_order.emplace_back(alignment_num);
    });
    out.order = in_order; out.n_chosen = mappings.size();

    const MappingQualityCalculator mapq_calc(1.0, 4.0, scheme.log_base);
    std::array<double, 2> mapq_explored_caps = explored_caps;
    std::array<double, 2> mapq_score_groups;
    // We also have one fragment_cluster_cap across both ends.
    double fragment_cluster_cap = std::numeric_limits<float>::infinity();
    // And one base uncapped MAPQ
    double uncapped_mapq = 0;
    out.explored_cap = mapq_explored_caps; out.fragment_cluster_cap = fragment_cluster_cap;
    for (auto r : {0, 1}) out.score_group[r] = mapq_calc.compute_max_mapping_quality(scores_group[r], false);
    if (mappings.empty()) return out;            //If we didn't get an alignment, return empty alignments: mapping quality 0

    //Get the multiplicities for mapq calculation.  We're only using multiplicities if the alignments were rescued
    std::vector<double> paired_multiplicities;
    bool all_rescued = true;
    for (int type : types) {
        switch (type) {
            case paired: paired_multiplicities.push_back(1.0); all_rescued = false; break;
            case unpaired: paired_multiplicities.push_back(1.0); break;
            case rescued_from_first: case rescued_from_second: {
                const size_t r = type == rescued_from_first ? 0 : 1;
                paired_multiplicities.push_back(unpaired_count[r] > 0 ? (double)unpaired_count[r] / std::min(rescued_count[r], scheme.max_rescue_attempts) : 1.0);
                break;
            }
        }
    }
    const std::vector<double>* multiplicities = all_rescued ? &paired_multiplicities : nullptr;
    // Compute base MAPQ if not unmapped. Otherwise use 0 instead of the 50% this would give us.
    uncapped_mapq = scores[0] == 0 ? 0 : mapq_calc.compute_max_mapping_quality(scores, false, multiplicities);
    //Cap mapq at 1 - 1 / # equivalent or better fragment clusters, including self
    if (better_cluster_count_by_mappings.front() > 1) fragment_cluster_cap = -10.0 * std::log10(1.0 - (1.0 / (double)better_cluster_count_by_mappings.front()));      // prob_to_phred
    for (auto r : {0, 1}) mapq_score_groups[r] = mapq_calc.compute_max_mapping_quality(scores_group[r], false);
    out.uncapped = uncapped_mapq; out.fragment_cluster_cap = fragment_cluster_cap; out.score_group = mapq_score_groups;

    for (auto r : {0, 1}) {
        // Compute the overall cap for just this read, now that the individual cap components are filled in for both reads.
        double escape_bonus = uncapped_mapq < std::numeric_limits<int32_t>::max() ? 1.0 : 2.0;
        double mapq_cap = std::min(fragment_cluster_cap, ((mapq_explored_caps[0] + mapq_explored_caps[1]) * escape_bonus));
        if (types.front() == unpaired) {
            //If this pair came from two different fragment cluster, then cap mapq at the mapq from only unpaired alignments of this read
            mapq_cap = std::min(mapq_cap, (double)mapq_calc.compute_max_mapping_quality(unpaired_scores[r], false));
        }
        double read_mapq = uncapped_mapq;
        out.applied_cap[r] = mapq_cap;
        // Apply the cap, and limit to 0-60
        double capped_mapq = std::min(mapq_cap, read_mapq);
        if (distances.front() == std::numeric_limits<int64_t>::max()) {
            //If the two reads are not reachable, lower cap
            capped_mapq = capped_mapq / 2.0;
        }
        read_mapq = std::max(std::min(capped_mapq, 120.0) / 2.0, 0.0);
        // Unaligned reads always have MAPQ 0, even if they're the obvious right answer given pairing constraints.
        if (!candidates[mappings.front()].aligned[r] || std::isnan(read_mapq)) read_mapq = 0;
        out.mapq[r] = (int32_t)read_mapq;
    }
    return out;
}

}  // namespace vgamd
