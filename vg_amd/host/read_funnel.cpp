// read_funnel.cpp — see read_funnel.hpp.
#include "read_funnel.hpp"
#include <algorithm>

namespace vgamd {

void process_until_threshold_e(size_t items, const std::function<double(size_t)>& get_score, const std::function<bool(size_t, size_t)>& comparator,
                               double threshold, size_t min_count, size_t max_count, ReadRng* rng, const std::function<void(size_t, size_t, size_t)>& placed,
                               const std::function<bool(size_t)>& process_item, const std::function<void(size_t)>& discard_item_by_count,
                               const std::function<void(size_t)>& discard_item_by_score) {
    std::vector<size_t> indexes_in_order(items);
    for (size_t i = 0; i < items; ++i) indexes_in_order[i] = i;
    // sort_shuffling_ties (src/utility.hpp:771-794): everything sorted, then the run the first item does not beat shuffled
    std::stable_sort(indexes_in_order.begin(), indexes_in_order.end(), comparator);
    size_t ties_end = 0;
    while (ties_end < items && !comparator(indexes_in_order[0], indexes_in_order[ties_end])) ++ties_end;
    if (rng) for (size_t i = 1; i < ties_end; ++i) std::swap(indexes_in_order[(*rng)() % (i + 1)], indexes_in_order[i]);      // deterministic_shuffle (:721-728)
    std::vector<size_t> better_or_equal_count(items, items);     // (:1603-1614)
    for (size_t i = items; i-- > 1;) better_or_equal_count[i - 1] = comparator(indexes_in_order[i - 1], indexes_in_order[i]) ? i : better_or_equal_count[i];
    const double cutoff = items == 0 ? 0 : get_score(indexes_in_order[0]) - threshold;
    size_t unskipped = 0;
    for (size_t i = 0; i < items; ++i) {                         // (:1623-1658)
        const size_t item_num = indexes_in_order[i];
        placed(item_num, i, better_or_equal_count[i]);
        if (threshold != 0 && get_score(item_num) <= cutoff) {
            if (unskipped < min_count) unskipped += (size_t)process_item(item_num);
            else discard_item_by_score(item_num);
        } else {
            if (unskipped < max_count) unskipped += (size_t)process_item(item_num);
            else discard_item_by_count(item_num);
        }
    }
}

std::vector<size_t> funnel_clusters(const FunnelPolicy& P, size_t read_length, const std::vector<PolicyMinimizer>& minimizers, const std::vector<std::vector<size_t>>& clusters,
                                    ReadRng* rng, std::vector<FunnelCluster>& out) {
    out.assign(clusters.size(), FunnelCluster());
    double best_cluster_score = 0.0, second_best_cluster_score = 0.0;
    for (size_t i = 0; i < clusters.size(); ++i) {               // (:656-671)
        const ClusterScore c = score_cluster(clusters[i], minimizers, read_length);
        out[i].score = c.score; out[i].coverage = c.coverage;
        std::vector<uint8_t> covered(read_length, 0);            // (the count behind the fraction)
        for (size_t j = 0; j < minimizers.size(); ++j)
            if (c.present[j]) for (size_t b = minimizers[j].forward_offset; b < minimizers[j].forward_offset + minimizers[j].length && b < read_length; ++b) covered[b] = 1;
        out[i].covered = (uint32_t)std::count(covered.begin(), covered.end(), (uint8_t)1);
        if (c.score > best_cluster_score) { second_best_cluster_score = best_cluster_score; best_cluster_score = c.score; }
        else if (c.score > second_best_cluster_score) second_best_cluster_score = c.score;
    }
    double cluster_score_cutoff = best_cluster_score - P.cluster_score_threshold;      // (:685-688)
    if (cluster_score_cutoff - P.pad_cluster_score_threshold < second_best_cluster_score) cluster_score_cutoff = std::min(cluster_score_cutoff, second_best_cluster_score);
    std::vector<size_t> kept;
    process_until_threshold_e(clusters.size(), [&](size_t i) { return out[i].coverage; },
        [&](size_t a, size_t b) { return out[a].coverage > out[b].coverage || (out[a].coverage == out[b].coverage && out[a].score > out[b].score); },
        P.cluster_coverage_threshold, P.min_extensions, P.max_extensions, rng,
        [&](size_t c, size_t at, size_t count) { out[c].rank = (uint32_t)at; out[c].better_or_equal = (uint32_t)count; },
        [&](size_t c) {
            if (P.cluster_score_threshold != 0 && out[c].score < cluster_score_cutoff && kept.size() >= P.min_extensions) { out[c].verdict = FUNNEL_FAIL_SCORE; return false; }      // (:746-761)
            out[c].verdict = FUNNEL_EXTEND; kept.push_back(c);
            return true;
        },
        [&](size_t c) { out[c].verdict = FUNNEL_FAIL_MAX_EXTENSIONS; },
        [&](size_t c) { out[c].verdict = FUNNEL_FAIL_COVERAGE; });
    return kept;
}

std::vector<size_t> funnel_extension_sets(const FunnelPolicy& P, size_t read_length, const std::vector<FunnelSetIn>& sets, int gap_open, int gap_extend, ReadRng* rng,
                                          std::vector<FunnelSet>& out, std::vector<uint8_t>& explored) {
    out.assign(sets.size(), FunnelSet());
    for (size_t s = 0; s < sets.size(); ++s)                     // score_extensions (:5245-5262); a failed search has nothing to score
        out[s].estimate = sets[s].failed ? 0 : score_extension_group(read_length, sets[s].extensions, sets[s].full_length, gap_open, gap_extend);
    std::vector<size_t> aligned;
    auto fate = [&](size_t s, uint32_t verdict) { out[s].verdict = sets[s].failed ? (uint32_t)FUNNEL_SET_FAILED : verdict; };
    process_until_threshold_e(sets.size(), [&](size_t i) { return (double)out[i].estimate; }, [&](size_t a, size_t b) { return out[a].estimate > out[b].estimate; },
        P.extension_set_score_threshold, P.min_extension_sets, P.max_alignments, rng,
        [&](size_t s, size_t at, size_t count) { out[s].rank = (uint32_t)at; out[s].better_or_equal = (uint32_t)count; },
        [&](size_t s) {
            if (sets[s].failed) { fate(s, FUNNEL_SET_FAILED); return false; }
            if (out[s].estimate < P.extension_set_min_score) { fate(s, FUNNEL_SET_FAIL_MIN_SCORE); return false; }      // (:912-916)
            fate(s, FUNNEL_SET_ALIGN); aligned.push_back(s);
            if (sets[s].sources) for (size_t source : *sets[s].sources) explored.at(source) = 1;      // (:1036-1043)
            return true;
        },
        [&](size_t s) { fate(s, FUNNEL_SET_FAIL_MAX_ALIGNMENTS); },
        [&](size_t s) { fate(s, FUNNEL_SET_FAIL_SCORE); });
    return aligned;
}

FunnelWinners funnel_winners(const FunnelPolicy& P, const std::vector<std::vector<FunnelAlignment>>& set_alignments, ReadRng* rng) {
    std::vector<FunnelAlignment> alignments; std::vector<FunnelPick> origin;
    for (size_t s = 0; s < set_alignments.size(); ++s) {
        const std::vector<FunnelAlignment>& best_alignments = set_alignments[s];
        for (size_t a = 0; a < best_alignments.size() && best_alignments[a].score != 0 && best_alignments[a].score >= best_alignments[0].score * 0.8; ++a) {      // (:1025)
            alignments.push_back(best_alignments[a]); origin.push_back(FunnelPick{(uint32_t)s, (uint32_t)a});
        }
    }
    if (alignments.empty()) { alignments.push_back(FunnelAlignment()); origin.push_back(FunnelPick()); }      // (:1065-1068)
    FunnelWinners w;
    process_until_threshold_e(alignments.size(), [&](size_t i) { return (double)alignments[i].score; }, [&](size_t a, size_t b) { return alignments[a].score > alignments[b].score; },
        0, 1, P.max_multimaps, rng, [](size_t, size_t, size_t) {},
        [&](size_t a) { w.scores.push_back(alignments[a].score); w.picks.push_back(origin[a]); if (!w.n_reported) w.unmapped = alignments[a].n_mappings == 0; ++w.n_reported; return true; },
        [&](size_t a) { w.scores.push_back(alignments[a].score); w.picks.push_back(origin[a]); },
        [](size_t) {});
    return w;
}

}  // namespace vgamd
