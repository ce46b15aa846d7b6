// chain_links.cpp — see chain_links.hpp.  Line numbers: reference src/minimizer_mapper_from_chains.cpp.
#include "chain_links.hpp"
#include <algorithm>

namespace vgamd {

size_t get_read_distance(const LinkAnchor& from, const LinkAnchor& to) {
    if (to.read_start() < from.read_end()) return std::numeric_limits<size_t>::max();
    return to.read_start() - from.read_end();
}

namespace {
// a tail of `length` bases: WFAExtender's prefix / suffix up to max_tail_length (:2619, :3163); the fallback up to max_tail_dp_length; beyond it an
// insertion without a position, score 0 (:2667-2680, :3217)
LinkRoute tail_route(const ChainLinksScheme& s, size_t length) {
    if (length <= s.max_tail_length) return LINK_WFA;
    if (length > s.max_tail_dp_length) return LINK_SOFTCLIP;
    return LINK_DP;
}
int64_t anchor_score(const ChainLinksScheme& s, const LinkAnchor& anchor, size_t read_length) {      // to_wfa_alignment, :4083-4104
    int64_t score = (int64_t)s.match * (int64_t)anchor.length();
    if (anchor.read_start() == 0) score += s.full_length_bonus;
    if (anchor.read_end() == read_length) score += s.full_length_bonus;
    return score;
}
}  // namespace

ChainLinks chain_links(const ChainLinksScheme& scheme, size_t read_length, const std::vector<LinkAnchor>& to_chain, const std::vector<size_t>& chain,
                       const std::function<size_t(size_t, size_t)>& get_graph_distance) {
    ChainLinks out;
    auto here_it = chain.begin();
    auto next_it = here_it;
    ++next_it;
    const LinkAnchor* here = &to_chain[*here_it];
    auto keep_here = [&]() {
        if (here->read_end() > read_length) { out.ok = false; return false; }
        out.kept.push_back(*here_it);
        out.anchor_score += anchor_score(scheme, *here, read_length);
        return true;
    };

    // Do the left tail, if any (:2611)
    size_t left_tail_length = here->read_start();
    out.left_tail_length = left_tail_length;
    if (left_tail_length > 0) {
        GraphPos right_anchor = here->graph_start();
        out.links.push_back(ChainLink{LINK_PREFIX, tail_route(scheme, left_tail_length), GraphPos{}, right_anchor, 0, left_tail_length, left_tail_length});
    }

    size_t longest_attempted_connection = 0;
    while (next_it != chain.end()) {
        const LinkAnchor* next = nullptr;
        while (next_it != chain.end()) {                                   // :2758
            next = &to_chain[*next_it];
            if (get_read_distance(*here, *next) == std::numeric_limits<size_t>::max()) {
                ++next_it;                                                 // overlap: keep here and skip next
            } else {
                break;
            }
        }
        if (next_it != chain.end()) {
            // skip seeds in repetitive regions that are involved in gaps (:2786)
            size_t total_graph_distance = get_graph_distance(*here_it, *next_it);
            size_t prev_read_distance = get_read_distance(*here, *next);
            size_t gap_lengths = std::max(total_graph_distance, prev_read_distance) - std::min(total_graph_distance, prev_read_distance);
            auto skip_to_it = next_it;
            while (skip_to_it != chain.end()) {
                const LinkAnchor* skip_to = &to_chain[*skip_to_it];
                size_t cur_graph_distance;
                if (skip_to_it + 1 == chain.end()) {
                    cur_graph_distance = std::numeric_limits<size_t>::max();      // we can't skip any further
                } else {
                    cur_graph_distance = get_graph_distance(*skip_to_it, *(skip_to_it + 1));
                    cur_graph_distance += skip_to->length();
                }
                if (skip_to->is_skippable() && skip_to_it + 1 != chain.end() && total_graph_distance + cur_graph_distance < scheme.max_skipped_bases) {
                    size_t cur_read_distance = get_read_distance(*skip_to, to_chain[*(skip_to_it + 1)]);
                    cur_read_distance += skip_to->length();
                    gap_lengths += std::max(cur_read_distance, cur_graph_distance) - std::min(cur_read_distance, cur_graph_distance);
                    total_graph_distance += cur_graph_distance;
                    ++skip_to_it;
                } else {
                    if (gap_lengths > scheme.min_indel_avoid_bases) {
                        next_it = skip_to_it;
                        next = skip_to;
                    }
                    break;
                }
            }
        }
        if (next_it == chain.end()) {
            break;                                                         // we couldn't find anything to connect to (:2865)
        }

        if (!keep_here()) return ChainLinks{false};                        // :2881-2893

        size_t link_start = here->read_end();                              // :2909
        size_t link_length = next->read_start() - link_start;
        size_t graph_dist = get_graph_distance(*here_it, *next_it);
        GraphPos left_anchor = here->graph_end();
        left_anchor.offset--;                                              // outside of the region to be aligned (:2949-2950)
        if (link_length == 0 && graph_dist == 0) {
            out.links.push_back(ChainLink{LINK_CONNECT, LINK_EMPTY, left_anchor, next->graph_start(), link_start, 0, 0});
        } else if (link_length > 0 && link_length <= scheme.max_chain_connection && graph_dist * link_length <= scheme.max_dp_cells) {
            out.links.push_back(ChainLink{LINK_CONNECT, LINK_WFA, left_anchor, next->graph_start(), link_start, link_length, graph_dist});
            longest_attempted_connection = std::max(longest_attempted_connection, link_length);
        } else {
            if (link_length > scheme.max_middle_dp_length || graph_dist * link_length > scheme.max_dp_cells) {
                out.cut = true;
                break;                                                     // just jump to right tail (:3051)
            }
            out.links.push_back(ChainLink{LINK_CONNECT, LINK_DP, left_anchor, next->graph_start(), link_start, link_length, graph_dist});
        }

        here_it = next_it;                                                 // :3116
        ++next_it;
        here = next;
    }

    if (next_it == chain.end()) {
        if (!keep_here()) return ChainLinks{false};                        // the final extension anchor (:3121-3149)
    }
    out.longest_attempted_connection = longest_attempted_connection;

    // Do the right tail, if any (:3152)
    size_t right_tail_length = read_length - here->read_end();
    if (right_tail_length > 0) {
        GraphPos left_anchor_excluded = here->graph_end();
        left_anchor_excluded.offset--;
        out.links.push_back(ChainLink{LINK_SUFFIX, tail_route(scheme, right_tail_length), left_anchor_excluded, GraphPos{}, here->read_end(), right_tail_length, right_tail_length});
    }
    return out;
}

}  // namespace vgamd
