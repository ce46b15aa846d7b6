// chain_items.hpp — choosing chains of anchors: algorithms::find_best_chains (reference src/algorithms/chain_items.cpp:735-877) with its DP
// chain_items_dp (:385-648), the multi-chain traceback chain_items_traceback (:650-733), the recombination positions (:793-868) and the filter
// add_transition_if_legal (:270-355) — over an explicit list of candidate transitions (from, to, graph distance) instead of a
// transition_iterator: what the reference's iterators hand to add_transition_if_legal IS such a list (zip_tree_transition_iterator collects
// generate_zip_tree_transitions' triples, :108-268), and nothing behind it looks at the distance index or the graph again.
// Host logic, the checker of the engine's vgk_chain_items (include/vgk_engine.h): same rule, the reference's loop shape.
//
// Pinned: find_best_chain, by the reference's four unit tests (src/unittest/chain_items.cpp:94-153; tests/test_chain_items.py).
// [PARITY-UNPINNED] what std::sort leaves open there and is fixed here: traceback starts are ordered by score descending, then source
// descending (nowhere is the largest source), then anchor index ascending; chains by penalty ascending, then order of creation.  The
// reference holds no test for several chains, recombination penalties or the consistency bonus; tests/test_chain_items.py holds those to a
// definition-level restatement.
#pragma once
#include <cstddef>
#include <cstdint>
#include <limits>
#include <utility>
#include <vector>

namespace vgamd {

using path_flags_t = uint64_t;

struct Anchor {                          // what chaining reads of algorithms::Anchor (src/algorithms/chain_items.hpp:50-290)
    size_t start = 0, size = 0;          // read_start(), length()
    size_t margin_before = 0, margin_after = 0;
    int points = 0;                      // score()
    size_t start_offset = 0, end_offset = 0;      // start_hint_offset(), end_hint_offset()
    size_t seed_length = 0;              // base_seed_length()
    path_flags_t start_paths = 0, end_paths = 0;
    size_t read_start() const { return start; }
    size_t read_end() const { return start + size; }
    size_t read_exclusion_start() const { return start - margin_before; }
    size_t read_exclusion_end() const { return read_end() + margin_after; }
};

struct TracedScore {                     // src/algorithms/chain_items.hpp:296-372
    int score = 0; size_t source = nowhere(); path_flags_t paths = 0; size_t rec_num = 0;
    static size_t nowhere() { return std::numeric_limits<size_t>::max(); }
    static TracedScore unset() { return {0, nowhere(), 0, 0}; }
    void max_in(const std::vector<TracedScore>& options, size_t option_number);
    static TracedScore score_from(const std::vector<TracedScore>& options, size_t option_number);
    TracedScore add_points(int adjustment) const { return {score + adjustment, source, paths, rec_num}; }
    TracedScore set_shared_paths(const std::pair<path_flags_t, path_flags_t>& new_paths) const;
    bool operator>(const TracedScore& o) const { return score > o.score || (score == o.score && source > o.source); }
};

struct ChainScoringScheme { int item_bonus = 0; double gap_scale = 1.0; int recombination_penalty = 0; int consistency_bonus = 0; };

struct transition_info { size_t from_anchor, to_anchor, indel_size; };
struct candidate_transition { size_t from_anchor, to_anchor, graph_distance; };

struct ChainWithRec {
    std::pair<int, std::vector<size_t>> scored_chain;
    std::vector<size_t> rec_positions;           // anchors that introduce a recombination, chain order
    std::vector<size_t> left_rec_positions;      // the backward pass' boundaries, chain order (the reference keeps them only paired, as rec_intervals)
    std::vector<std::pair<size_t, size_t>> rec_intervals;
};
struct ChainsResult { std::vector<ChainWithRec> chains; };

// -> 0 when the transition was added, otherwise which of the five conditions dropped it (1 not reachable in the read, 2 beyond the read
// lookback, 3 exclusion zones overlap, 4 more to back out than the distance, 5 indel above the limit)
int add_transition_if_legal(std::vector<transition_info>& transitions, const std::vector<Anchor>& to_chain, size_t max_read_lookback_bases, size_t max_indel_bases,
                            size_t from_anchor, size_t to_anchor, size_t graph_distance);
int score_chain_gap(size_t distance_difference, size_t base_seed_length);
TracedScore chain_items_dp(std::vector<TracedScore>& chain_scores, const std::vector<Anchor>& to_chain, const std::vector<candidate_transition>& candidates,
                           const ChainScoringScheme& scheme, size_t max_read_lookback_bases, size_t max_indel_bases);
std::vector<std::pair<std::vector<size_t>, int>> chain_items_traceback(const std::vector<TracedScore>& chain_scores, const std::vector<Anchor>& to_chain,
                                                                      const TracedScore& best_past_ending_score_ever, const ChainScoringScheme& scheme, size_t max_tracebacks);
// table (nullable): the DP table as chain_items_dp leaves it
ChainsResult find_best_chains(const std::vector<Anchor>& to_chain, const std::vector<candidate_transition>& candidates, const ChainScoringScheme& scheme,
                              size_t max_chains, size_t max_read_lookback_bases, size_t max_indel_bases, std::vector<TracedScore>* table = nullptr);
std::pair<int, std::vector<size_t>> find_best_chain(const std::vector<Anchor>& to_chain, const std::vector<candidate_transition>& candidates, const ChainScoringScheme& scheme,
                                                    size_t max_read_lookback_bases, size_t max_indel_bases);

}  // namespace vgamd
