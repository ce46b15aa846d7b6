// chain_links.hpp — the walk of MinimizerMapper::find_chain_alignment over a chosen chain (reference src/minimizer_mapper_from_chains.cpp:2576-3292):
// which stretches of the read get aligned, by what, between which graph positions, and which anchors are kept — its decisions only, no alignment.
// Written in the reference's loop shape: the iterators here_it / next_it / skip_to_it, the while loops and breaks of the original, size_t arithmetic
// that wraps where the original's does.  The checker and CPU baseline of vgk_chain_links (include/vgk_engine.h), whose rule is stated a second
// time, serially and slot by slot, in vg_amd/csrc/chain_links_device.hpp.  [PARITY-UNPINNED: the reference holds no test that names
// find_chain_alignment; tests/test_chain_links.py holds the walk to a statement of the cited lines in another shape.]
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <limits>
#include <vector>

namespace vgamd {

struct ChainLinksScheme {                // MinimizerMapper's fields of the same names, its defaults
    size_t max_chain_connection = 100, max_tail_length = 100;
    size_t max_middle_dp_length = (size_t)std::numeric_limits<int32_t>::max(), max_tail_dp_length = 30000;
    size_t max_dp_cells = std::numeric_limits<size_t>::max();
    size_t max_skipped_bases = 0, min_indel_avoid_bases = 0;
    int match = 1, full_length_bonus = 5;
};
struct GraphPos { uint32_t node = 0xffffffffu, offset = 0; };       // an oriented node and a base offset; node 0xffffffff: none
// algorithms::Anchor as the walk reads it
struct LinkAnchor {
    size_t start = 0, size = 0; GraphPos start_pos, end_pos; bool skippable = false;
    size_t read_start() const { return start; }
    size_t length() const { return size; }
    size_t read_end() const { return start + size; }
    GraphPos graph_start() const { return start_pos; }
    GraphPos graph_end() const { return end_pos; }                  // past the end within its node
    bool is_skippable() const { return skippable; }
};
enum LinkMode : uint32_t { LINK_CONNECT = 0, LINK_SUFFIX = 1, LINK_PREFIX = 2 };                      // VGK_WFA_*
enum LinkRoute : uint32_t { LINK_WFA = 0, LINK_DP = 1, LINK_EMPTY = 2, LINK_SOFTCLIP = 3 };            // VGK_CHAIN_ROUTE_*
struct ChainLink { LinkMode mode; LinkRoute route; GraphPos from, to; size_t read_begin, length, graph_distance; };
struct ChainLinks {
    bool ok = true;                      // false: an anchor the walk kept ends past the read (the reference would read beyond the sequence)
    bool cut = false;                    // the walk left the loop at a link it refused (:3044-3051)
    std::vector<ChainLink> links; std::vector<size_t> kept;        // in read order; kept: item VALUES (anchor numbers)
    size_t left_tail_length = 0, longest_attempted_connection = 0;
    int64_t anchor_score = 0;
};

// algorithms::get_read_distance (src/algorithms/chain_items.hpp): SIZE_MAX when `to` starts before `from` ends
size_t get_read_distance(const LinkAnchor& from, const LinkAnchor& to);

// to_chain: the anchors the chain's items number; chain: its items, left to right (not empty); get_graph_distance(a, b): end of anchor a to start of
// anchor b, SIZE_MAX unreachable
ChainLinks chain_links(const ChainLinksScheme& scheme, size_t read_length, const std::vector<LinkAnchor>& to_chain, const std::vector<size_t>& chain,
                       const std::function<size_t(size_t, size_t)>& get_graph_distance);

}  // namespace vgamd
