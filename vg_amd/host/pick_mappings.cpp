// pick_mappings.cpp — see pick_mappings.hpp.
#include "pick_mappings.hpp"
#include <algorithm>
#include <limits>
#include <unordered_set>

namespace vgamd {

bool chain_ranges_are_equivalent(const ChainRange& range1, const ChainRange& range2) {
    if (range1.component != range2.component) return false;      // different connected components
    if (range1.root_snarl) {
        if (range1.child_start != range2.child_start || range1.child_start != range1.child_end || range2.child_start != range2.child_end) return false;      // different children of the snarl
    }
    size_t offset_start1 = range1.offset_start, offset_end1 = range1.offset_end, offset_start2 = range2.offset_start, offset_end2 = range2.offset_end;
    if (offset_start1 > offset_end1) std::swap(offset_start1, offset_end1);
    if (offset_start2 > offset_end2) std::swap(offset_start2, offset_end2);
    if (offset_start1 > offset_end2 || offset_start2 > offset_end1) return false;      // disconnected
    if ((offset_start1 <= offset_start2 && offset_end1 >= offset_end2) || (offset_start2 <= offset_start1 && offset_end2 >= offset_end1)) return true;      // one contains the other
    if (offset_start1 > offset_start2) { std::swap(offset_start1, offset_start2); std::swap(offset_end1, offset_end2); }      // range1 first
    const size_t overlap_size = offset_end1 - offset_start2;
    return overlap_size > (std::min(offset_end1 - offset_start1, offset_end2 - offset_start2) / 2);
}

double identity(const std::vector<PickMapping>& path) {
    size_t total_length = 0, matched_length = 0;
    for (const PickMapping& mapping : path) for (const PickEdit& edit : mapping.edits) total_length += edit.to_length;      // path_to_length
    for (size_t i = 0; i < path.size(); ++i) {
        const PickMapping& mapping = path[i];
        for (size_t j = 0; j < mapping.edits.size(); ++j) {
            const PickEdit& edit = mapping.edits[j];
            if (edit.match) matched_length += edit.from_length;
            else if (edit.from_length == 0) {                    // an insertion (a run of length 0 takes nothing off either way)
                const bool is_first_edit = i == 0 && j == 0, is_last_edit = i == path.size() - 1 && j == mapping.edits.size() - 1;
                if (is_first_edit || is_last_edit) total_length -= edit.to_length;
            }
        }
    }
    return total_length == 0 ? 0.0 : (double)matched_length / (double)total_length;
}

std::vector<double> fix_up_multiplicities(const std::vector<size_t>& alignments_to_source, const std::vector<int>& chain_score_estimates, const std::vector<ChainRange>& chain_ranges,
                                          const std::vector<double>& multiplicity_by_chain, std::vector<size_t> chain_count_by_alignment) {
    std::vector<double> multiplicity_by_alignment(chain_count_by_alignment.size());
    for (size_t i = 0; i < multiplicity_by_alignment.size(); ++i) multiplicity_by_alignment[i] = multiplicity_by_chain[alignments_to_source[i]];
    for (size_t i = 0; i < chain_count_by_alignment.size(); ++i) {
        const size_t chain_i = alignments_to_source[i];
        for (size_t j = 0; j < chain_count_by_alignment.size(); ++j) {
            const size_t chain_j = alignments_to_source[j];
            if (i != j && chain_score_estimates[chain_i] >= chain_score_estimates[chain_j] && chain_ranges_are_equivalent(chain_ranges[chain_i], chain_ranges[chain_j]))
                --chain_count_by_alignment[i];                   // (size_t: below 0 it wraps, as in the reference)
        }
    }
    const size_t alignments = chain_count_by_alignment.size();
    for (size_t i = 0; i < multiplicity_by_alignment.size(); ++i)
        multiplicity_by_alignment[i] += (chain_count_by_alignment[i] >= alignments ? ((double)chain_count_by_alignment[i] - (double)alignments) : 0.0);
    return multiplicity_by_alignment;
}

namespace {
struct NodeKeyHash { size_t operator()(const std::pair<int64_t, bool>& k) const { return std::hash<int64_t>()(k.first * 2 + (k.second ? 1 : 0)); } };
size_t mapping_from_length(const PickMapping& mapping) { size_t l = 0; for (const PickEdit& e : mapping.edits) l += e.from_length; return l; }
}  // namespace

PickedMappings pick_mappings_from_alignments(const PickScheme& scheme, const std::vector<PickAlignment>& alignments, const std::vector<double>& multiplicity_by_alignment,
                                             const std::vector<size_t>& alignments_to_source, const std::vector<int>& chain_score_estimates, ReadRng* rng) {
    PickedMappings out;
    const size_t A = alignments.size();
    out.identity.assign(A, 0.0); out.fraction_unique.assign(A, 0.0); out.evaluated.assign(A, 0); out.fate.assign(A, 0);
    for (size_t i = 0; i < A; ++i) out.identity[i] = identity(alignments[i].path);
    std::unordered_set<std::pair<int64_t, bool>, NodeKeyHash> used_nodes;
    auto get_fraction_unique = [&](size_t alignment_num) {
        size_t from_length_from_used = 0, from_length_total = 0;
        for (const PickMapping& mapping : alignments[alignment_num].path) {
            if (!mapping.has_position) continue;                 // (no node: no from_length, never in the set)
            const size_t from_length = mapping_from_length(mapping);
            if (used_nodes.count({mapping.node_id, mapping.is_reverse})) from_length_from_used += from_length;
            from_length_total += from_length;
        }
        return from_length_total > 0 ? ((double)(from_length_total - from_length_from_used) / from_length_total) : 1.0;
    };
    auto mark_nodes_used = [&](size_t alignment_num) {
        for (const PickMapping& mapping : alignments[alignment_num].path) if (mapping.has_position) used_nodes.insert({mapping.node_id, mapping.is_reverse});
    };
    auto get_sorting_score = [&](size_t alignment_number) -> double {
        if (scheme.sort_by_chain_score) return chain_score_estimates.at(alignments_to_source.at(alignment_number));
        return alignments.at(alignment_number).score + out.identity[alignment_number];
    };
    // both filters, in order; -> the alignment passes
    auto filters = [&](size_t alignment_num) {
        if (alignments[alignment_num].score <= 0) { out.fate[alignment_num] = PICK_FAIL_SCORE; return false; }
        const double unique_node_fraction = get_fraction_unique(alignment_num);
        out.fraction_unique[alignment_num] = unique_node_fraction; out.evaluated[alignment_num] = 1;
        if (unique_node_fraction < scheme.min_unique_node_fraction) { out.fate[alignment_num] = PICK_FAIL_UNIQUE; return false; }
        return true;
    };
    process_until_threshold_e(A, get_sorting_score, [&](size_t a, size_t b) { return get_sorting_score(a) > get_sorting_score(b); }, 0, 1, scheme.max_multimaps, rng,
        [](size_t, size_t, size_t) {},
        [&](size_t alignment_num) {
            if (!filters(alignment_num)) return false;
            mark_nodes_used(alignment_num);
            out.scores.emplace_back(alignments[alignment_num].score);
            out.picked.emplace_back(alignment_num); ++out.n_mappings;
            out.multiplicity_by_mapping.emplace_back(multiplicity_by_alignment[alignment_num]);
            out.fate[alignment_num] = PICK_MAPPING;
            return true;
        }, [&](size_t alignment_num) {
            if (!filters(alignment_num)) return;                 // fails a filter: no secondary for MAPQ
            out.scores.emplace_back(alignments[alignment_num].score);
            out.picked.emplace_back(alignment_num);
            out.multiplicity_by_mapping.emplace_back(multiplicity_by_alignment[alignment_num]);
            out.fate[alignment_num] = PICK_BEYOND_CUT;
        }, [](size_t) {});
    if (out.n_mappings == 0) {                                   // (:2480-2486)
        out.scores.emplace_back(0); out.picked.emplace_back(std::numeric_limits<size_t>::max()); out.multiplicity_by_mapping.emplace_back(0);
        out.unmapped = true;
    }
    return out;
}

}  // namespace vgamd
