// extension_anchors.hpp — anchors for chaining from a tree's seeds and their gapless extensions: the block of MinimizerMapper::map_from_chains
// between extend_seed_group and find_best_chains (reference src/minimizer_mapper_from_chains.cpp:1380-1596) with to_anchor for a seed (:3978-4038)
// and for an interval of an extension (:4040-4081), find_anchor_intervals (:480-706), the mapping of an extension back to the seeds it contains
// (extend_seed_group, src/minimizer_mapper.cpp:4881-5000 over GaplessExtension::for_each_read_interval, src/gbwt_extender.cpp:23-39) and
// sort_anchor_indexes.  Host logic, the checker of the engine's vgk_extension_anchors (include/vgk_engine.h): same rule, the reference's loop shape.
//
// Pinned: the seed anchors, by the reference's unit test of fragments on a 13-base stick (src/unittest/minimizer_mapper.cpp:997-1003, :1050-1128;
// tests/test_extension_anchors.py).  The reference holds no test of find_anchor_intervals; tests/test_extension_anchors.py holds it to a
// definition-level restatement and to the contract of its comment (:464-479).
// [PARITY-UNPINNED] what the reference's sorts leave open and is fixed here: seeds of one diagonal with the same stapled base by seed number;
// extensions of equal score by number; anchors with equal read start and end in order of creation.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>
#include "chain_items.hpp"

namespace vgamd {

struct AnchorSeed {                      // what the block reads of a Seed and its Minimizer
    uint32_t node = 0; int32_t diff = 0;         // GaplessExtender::seed_type: (oriented node, read_offset - node_offset)
    size_t stapled = 0, length = 0; bool is_reverse = false;      // Minimizer::pin_offset(), length, value.is_reverse
    path_flags_t paths = 0;
    size_t offset() const { return (size_t)((int64_t)stapled - diff); }      // in the node
};
struct Extension {                       // what the block reads of a GaplessExtension
    std::vector<uint32_t> path; size_t offset = 0;
    std::pair<size_t, size_t> read_interval;
    std::vector<size_t> mismatch_positions;
    bool left_full = false, right_full = false;
    bool full() const { return left_full && right_full; }
    size_t mismatches() const { return mismatch_positions.size(); }
};
struct AnchorOrigin { std::vector<size_t> seed_sequence, represented_seeds; size_t extension = 0; std::pair<size_t, size_t> interval; size_t created = 0; };      // created: its place in order of creation
struct ExtensionAnchors {
    bool full_length = false; std::vector<size_t> full_length_extensions;      // the shortcut: no anchors
    std::vector<Anchor> anchors; std::vector<AnchorOrigin> origins;            // in sort_anchor_indexes' order
};

// to_anchor of one seed on a node of node_length bases (:3978-4038); score = match * length of the minimizer
Anchor seed_to_anchor(const AnchorSeed& seed, size_t node_length, int match);
std::vector<std::pair<size_t, size_t>> find_anchor_intervals(const std::pair<size_t, size_t>& read_interval, const std::vector<size_t>& mismatch_positions,
                                                             const std::vector<size_t>& seed_positions);
// the seeds each extension contains, in stapled order (extend_seed_group's seeds_used)
std::vector<std::vector<size_t>> seeds_for_extensions(const std::vector<AnchorSeed>& seeds, const std::vector<Extension>& extensions, const uint32_t* oriented_node_length);
// the whole block for one (read, tree): do_gapless_extension == false -> the seed anchors, sorted
ExtensionAnchors extension_anchors(const std::vector<AnchorSeed>& seeds, const std::vector<Extension>& extensions, bool set_is_full_length, const uint32_t* oriented_node_length,
                                   int match, int mismatch, size_t default_max_extension_mismatches, bool do_gapless_extension);

}  // namespace vgamd
