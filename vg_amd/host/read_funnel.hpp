// read_funnel.hpp — the decisions MinimizerMapper::map_from_extensions makes between its stages (reference src/minimizer_mapper.cpp:650-1128,
// find_supplementaries == false): which clusters are extended, which extension sets are aligned, which alignments are reported and which
// minimizers count as explored.  Written in the reference's loop shape — three sets of callbacks into one process_until_threshold_e
// (src/minimizer_mapper.hpp:1580-1659) — over score_cluster (seed_policy.hpp), score_extension_group (extension_scoring.hpp) and ReadRng.
// The checker and CPU baseline of vgk_funnel_clusters / vgk_funnel_extension_sets / vgk_funnel_winners (include/vgk_engine.h), whose rule is
// stated a second time, serially, in vg_amd/csrc/read_funnel_device.hpp.  [PARITY-UNPINNED: the reference holds no test of these loops;
// tests/test_read_funnel.py holds them to a statement of the cited lines in another shape.]
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>
#include "extension_scoring.hpp"
#include "seed_policy.hpp"

namespace vgamd {

struct FunnelPolicy {                    // MinimizerMapper's fields of the same names, giraffe's defaults
    double cluster_score_threshold = 50, pad_cluster_score_threshold = 20, cluster_coverage_threshold = 0.3;
    double extension_set_score_threshold = 20;
    int extension_set_min_score = 20;
    size_t min_extensions = 2, max_extensions = 800, min_extension_sets = 2, max_alignments = 8, max_multimaps = 1;
};
enum FunnelVerdict : uint32_t { FUNNEL_UNDECIDED = 0, FUNNEL_EXTEND = 1, FUNNEL_FAIL_COVERAGE = 2, FUNNEL_FAIL_SCORE = 3, FUNNEL_FAIL_MAX_EXTENSIONS = 4 };
enum FunnelSetVerdict : uint32_t { FUNNEL_SET_ALIGN = 1, FUNNEL_SET_FAIL_SCORE = 2, FUNNEL_SET_FAIL_MIN_SCORE = 3, FUNNEL_SET_FAIL_MAX_ALIGNMENTS = 4, FUNNEL_SET_FAILED = 5 };

// process_until_threshold_e with threshold_escape always false.  rng null: the top ties are not shuffled.  placed(item, position,
// better_or_equal_count) is told every item in walk order just before its fate (the reference hands the count to process_item only).
void process_until_threshold_e(size_t items, const std::function<double(size_t)>& get_score, const std::function<bool(size_t, size_t)>& comparator,
                               double threshold, size_t min_count, size_t max_count, ReadRng* rng, const std::function<void(size_t, size_t, size_t)>& placed,
                               const std::function<bool(size_t)>& process_item, const std::function<void(size_t)>& discard_item_by_count,
                               const std::function<void(size_t)>& discard_item_by_score);

struct FunnelCluster { double score = 0, coverage = 0; uint32_t covered = 0, rank = 0, better_or_equal = 0, verdict = FUNNEL_UNDECIDED; };
// clusters[c] = the sources (minimizer numbers within the read) of cluster c's seeds -> per cluster `out`, and the clusters extended in that order
std::vector<size_t> funnel_clusters(const FunnelPolicy& policy, size_t read_length, const std::vector<PolicyMinimizer>& minimizers_in_read_order,
                                    const std::vector<std::vector<size_t>>& clusters, ReadRng* rng, std::vector<FunnelCluster>& out);

struct FunnelSetIn { bool failed = false, full_length = false; std::vector<ScoredInterval> extensions; const std::vector<size_t>* sources = nullptr; };
struct FunnelSet { int estimate = 0; uint32_t rank = 0, better_or_equal = 0, verdict = FUNNEL_UNDECIDED; };
// the sets of the kept clusters in kept order -> per set `out`, the sets aligned in that order, and explored[] per minimizer of the read
std::vector<size_t> funnel_extension_sets(const FunnelPolicy& policy, size_t read_length, const std::vector<FunnelSetIn>& sets, int gap_open, int gap_extend,
                                          ReadRng* rng, std::vector<FunnelSet>& out, std::vector<uint8_t>& explored);

struct FunnelAlignment { int score = 0; size_t n_mappings = 0; };
struct FunnelPick { uint32_t set = 0xffffffffu, alignment = 0xffffffffu; };
struct FunnelWinners { std::vector<int> scores; std::vector<FunnelPick> picks; size_t n_reported = 0; bool unmapped = true; };
// the alignments of the aligned sets in walk order -> every kept score in the winner walk's order, where each came from, how many are mappings
FunnelWinners funnel_winners(const FunnelPolicy& policy, const std::vector<std::vector<FunnelAlignment>>& set_alignments, ReadRng* rng);

}  // namespace vgamd
