// pick_mappings.hpp — how MinimizerMapper::map_from_chains turns a read's chain alignments into mappings, scores and multiplicities (reference
// src/minimizer_mapper_from_chains.cpp): the multiplicity fix-up at the end of do_alignment_on_chains (:2241-2262) with chain_ranges_are_equivalent
// (:100-191) over the four GIVEN numbers of a chain's range, then pick_mappings_from_alignments (:2265-2493) with identity (src/path.cpp:2316-2335).
// Written in the reference's shape: a std::unordered_set of (node, is_reverse), three callbacks into process_until_threshold_e's statement
// (read_funnel.hpp), the O(A^2) loop over size_t counts that wrap where the original's do.  The checker and CPU baseline of vgk_pick_mappings
// (include/vgk_engine.h), whose rule is stated a second time, serially, in vg_amd/csrc/pick_mappings_device.hpp.  [PARITY-UNPINNED: the reference
// holds no test that names these loops; tests/test_pick_mappings.py holds them to a statement of the cited lines in another shape.]
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "read_funnel.hpp"

namespace vgamd {

struct PickScheme { double min_unique_node_fraction = 0.0; size_t max_multimaps = 1; bool sort_by_chain_score = false; };
// what the zip codes of a chain's first and last seed say about it
struct ChainRange { uint64_t component = 0; bool root_snarl = false; uint32_t child_start = 0, child_end = 0; size_t offset_start = 0, offset_end = 0; };
bool chain_ranges_are_equivalent(const ChainRange& range1, const ChainRange& range2);

struct PickEdit { size_t from_length = 0, to_length = 0; bool match = false; };
struct PickMapping { bool has_position = false; int64_t node_id = 0; bool is_reverse = false; std::vector<PickEdit> edits; };
struct PickAlignment { int score = 0; std::vector<PickMapping> path; };
double identity(const std::vector<PickMapping>& path);

// :2244-2262 — chain_count_by_alignment holds the better_or_equal_counts on entry; -> multiplicity_by_alignment
std::vector<double> fix_up_multiplicities(const std::vector<size_t>& alignments_to_source, const std::vector<int>& chain_score_estimates, const std::vector<ChainRange>& chain_ranges,
                                          const std::vector<double>& multiplicity_by_chain, std::vector<size_t> chain_count_by_alignment);

enum PickFate : uint32_t { PICK_MAPPING = 1, PICK_BEYOND_CUT = 2, PICK_FAIL_SCORE = 3, PICK_FAIL_UNIQUE = 4 };
struct PickedMappings {
    std::vector<size_t> picked; std::vector<int> scores; std::vector<double> multiplicity_by_mapping;      // in walk order; picked SIZE_MAX: the unmapped entry
    size_t n_mappings = 0; bool unmapped = false;
    std::vector<double> identity, fraction_unique; std::vector<uint8_t> evaluated; std::vector<uint32_t> fate;      // per alignment
};
PickedMappings pick_mappings_from_alignments(const PickScheme& scheme, const std::vector<PickAlignment>& alignments, const std::vector<double>& multiplicity_by_alignment,
                                             const std::vector<size_t>& alignments_to_source, const std::vector<int>& chain_score_estimates, ReadRng* rng);

}  // namespace vgamd
