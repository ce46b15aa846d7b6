// extension_anchors.cpp — see extension_anchors.hpp.  Line numbers: reference src/minimizer_mapper_from_chains.cpp unless another file is named.
#include "extension_anchors.hpp"
#include <algorithm>
#include <map>
#include <numeric>
#include <stdexcept>
#include <unordered_set>

namespace vgamd {

Anchor seed_to_anchor(const AnchorSeed& seed, size_t node_length, int match) {      // :3978-4038
    size_t length, read_start, hint_start, margin_left, margin_right;
    if (seed.is_reverse) {
        // the seed holds the last base of the match: how much of the node lies before the past-end position
        const size_t graph_end_offset = seed.offset() + 1;
        length = std::min(seed.length, graph_end_offset);
        margin_left = seed.length - length; margin_right = 0;
        read_start = seed.stapled + 1 - length;
        hint_start = length - 1;
    } else {
        length = std::min(seed.length, node_length - seed.offset());
        margin_left = 0; margin_right = seed.length - length;
        read_start = seed.stapled;
        hint_start = 0;
    }
    Anchor a;
    a.start = read_start; a.size = length; a.margin_before = margin_left; a.margin_after = margin_right;
    a.points = match * (int)(margin_left + length + margin_right);      // score_exact_match over the whole minimizer
    a.start_offset = hint_start; a.end_offset = length - hint_start; a.seed_length = margin_left + length + margin_right;
    a.start_paths = a.end_paths = seed.paths;
    return a;
}

std::vector<std::pair<size_t, size_t>> find_anchor_intervals(const std::pair<size_t, size_t>& read_interval, const std::vector<size_t>& mismatch_positions,
                                                             const std::vector<size_t>& seed_positions) {      // :480-706
    if (seed_positions.empty()) throw std::runtime_error("find_anchor_intervals: no seeds");
    std::vector<std::pair<size_t, size_t>> anchor_intervals;
    if (mismatch_positions.empty()) { anchor_intervals.push_back(read_interval); return anchor_intervals; }
    auto mismatch_it = mismatch_positions.begin();
    auto seed_it = seed_positions.begin();
    auto prev_seed = seed_positions.end();
    auto mismatch_after_prev_seed = mismatch_positions.end(), mismatch_before_current_seed = mismatch_positions.end();
    size_t interval_start = read_interval.first;

    auto visit_seed = [&]() {
        if (prev_seed == seed_positions.end()) {
            // the first seed: trim from the left end of the read interval
            int score = 0, max_score = 0;
            auto here = mismatch_before_current_seed; auto max_cut = here;
            if (here != mismatch_positions.end()) {
                while (here != mismatch_positions.begin()) {
                    auto next = here; --next;
                    score += (int)(*here - *next - 1); score -= 4;
                    if (score > max_score) { max_score = score; max_cut = next; }
                    here = next;
                }
                score += (int)(*here - read_interval.first); score -= 4;
                if (score > max_score) { max_score = score; max_cut = mismatch_positions.end(); }      // all the way to the bound
            }
            if (max_cut != mismatch_positions.end()) interval_start = *max_cut + 1;
        } else if (mismatch_after_prev_seed != mismatch_positions.end()) {
            // the first seed after some mismatches (or past everything): finish the previous seed's interval
            std::vector<size_t>::const_iterator split_mismatch;
            if (seed_it != seed_positions.end()) {
                const size_t separating_mismatches = mismatch_before_current_seed - mismatch_after_prev_seed + 1;
                split_mismatch = mismatch_after_prev_seed + separating_mismatches / 2;
            } else split_mismatch = mismatch_positions.end();
            int score = 0, max_score = 0;
            auto here = mismatch_after_prev_seed; auto max_cut = here;
            while (here != split_mismatch) {
                auto next = here; ++next;
                score += (int)((next == mismatch_positions.end() ? read_interval.second : *next) - *here - 1); score -= 4;
                if (score > max_score) { max_score = score; max_cut = next; }
                here = next;
            }
            anchor_intervals.emplace_back(interval_start, max_cut == mismatch_positions.end() ? read_interval.second : *max_cut);
            if (seed_it != seed_positions.end()) {
                score = 0; max_score = 0; here = mismatch_before_current_seed; max_cut = here;
                while (here != split_mismatch) {
                    auto next = here; --next;
                    score += (int)(*here - *next - 1); score -= 4;
                    if (score > max_score) { max_score = score; max_cut = next; }
                    here = next;
                }
                interval_start = *max_cut + 1;
            }
        } else if (seed_it == seed_positions.end()) anchor_intervals.emplace_back(interval_start, read_interval.second);
        prev_seed = seed_it;
        mismatch_after_prev_seed = mismatch_positions.end();
    };
    auto visit_mismatch = [&]() {
        if (prev_seed != seed_positions.end() && mismatch_after_prev_seed == mismatch_positions.end()) mismatch_after_prev_seed = mismatch_it;
        mismatch_before_current_seed = mismatch_it;
    };
    while (mismatch_it != mismatch_positions.end() && seed_it != seed_positions.end()) {
        if (*mismatch_it < *seed_it) { visit_mismatch(); ++mismatch_it; } else { visit_seed(); ++seed_it; }
    }
    while (mismatch_it != mismatch_positions.end()) { visit_mismatch(); ++mismatch_it; }
    while (seed_it != seed_positions.end()) { visit_seed(); ++seed_it; }
    visit_seed();                                                   // the end seed finishes the last interval
    if (anchor_intervals.empty()) throw std::runtime_error("find_anchor_intervals: no intervals");
    return anchor_intervals;
}

std::vector<std::vector<size_t>> seeds_for_extensions(const std::vector<AnchorSeed>& seeds, const std::vector<Extension>& extensions, const uint32_t* oriented_node_length) {
    // src/minimizer_mapper.cpp:4836-4860: the seeds of every diagonal, by stapled base [PARITY-UNPINNED: then by seed number]
    std::map<std::pair<uint32_t, int32_t>, std::vector<size_t>> extension_seed_to_seeds;
    for (size_t i = 0; i < seeds.size(); ++i) extension_seed_to_seeds[{seeds[i].node, seeds[i].diff}].push_back(i);
    for (auto& kv : extension_seed_to_seeds)
        std::stable_sort(kv.second.begin(), kv.second.end(), [&](size_t a, size_t b) { return seeds[a].stapled < seeds[b].stapled; });
    std::vector<std::vector<size_t>> seeds_used;
    for (const Extension& extension : extensions) {                 // :4883-5000
        seeds_used.emplace_back();
        std::vector<size_t>& seeds_in_extension = seeds_used.back();
        size_t read_offset = extension.read_interval.first, node_offset = extension.offset;      // for_each_read_interval
        for (uint32_t handle : extension.path) {
            const size_t len = std::min((size_t)oriented_node_length[handle] - node_offset, extension.read_interval.second - read_offset);
            auto found = extension_seed_to_seeds.find({handle, (int32_t)((int64_t)read_offset - (int64_t)node_offset)});
            if (found != extension_seed_to_seeds.end()) {
                const std::vector<size_t>& possible_seeds = found->second;
                auto cursor_it = std::partition_point(possible_seeds.begin(), possible_seeds.end(), [&](size_t seed_index) { return seeds[seed_index].stapled < read_offset; });
                for (; cursor_it != possible_seeds.end() && seeds[*cursor_it].stapled < read_offset + len; ++cursor_it) seeds_in_extension.push_back(*cursor_it);
            }
            read_offset += len; node_offset = 0;
        }
    }
    return seeds_used;
}

ExtensionAnchors extension_anchors(const std::vector<AnchorSeed>& seeds, const std::vector<Extension>& tree_extensions, bool set_is_full_length, const uint32_t* oriented_node_length,
                                   int match, int mismatch, size_t default_max_extension_mismatches, bool do_gapless_extension) {
    ExtensionAnchors result;
    std::vector<Anchor> seed_anchors;
    for (const AnchorSeed& seed : seeds) seed_anchors.push_back(seed_to_anchor(seed, oriented_node_length[seed.node], match));
    std::vector<Anchor> extension_anchors; std::vector<AnchorOrigin> extension_origins;
    std::vector<size_t> anchor_indexes;
    if (do_gapless_extension) {
        const std::vector<std::vector<size_t>> seeds_for_extension = seeds_for_extensions(seeds, tree_extensions, oriented_node_length);
        if (set_is_full_length) {                                   // :1408-1464
            for (size_t extension_i = 0; extension_i < tree_extensions.size(); ++extension_i)
                if (tree_extensions[extension_i].full() && tree_extensions[extension_i].mismatches() <= default_max_extension_mismatches) result.full_length_extensions.push_back(extension_i);
        }
        if (!result.full_length_extensions.empty()) { result.full_length = true; return result; }
        // :1472-1479: sort_permutation [PARITY-UNPINNED: stable]
        std::vector<size_t> extension_score_order(tree_extensions.size());
        std::iota(extension_score_order.begin(), extension_score_order.end(), (size_t)0);
        std::stable_sort(extension_score_order.begin(), extension_score_order.end(), [&](size_t x, size_t y) {
            const Extension& a = tree_extensions[x]; const Extension& b = tree_extensions[y];
            const int a_score = (int)(a.read_interval.second - a.read_interval.first) - (int)a.mismatch_positions.size() * 5;
            const int b_score = (int)(b.read_interval.second - b.read_interval.first) - (int)b.mismatch_positions.size() * 5;
            return a_score > b_score;
        });
        std::unordered_set<size_t> used_seeds;
        for (size_t extension_index : extension_score_order) {      // :1484-1586
            const Extension& extension = tree_extensions[extension_index];
            const std::vector<size_t>& extension_seeds = seeds_for_extension[extension_index];
            std::vector<size_t> seed_positions;
            for (size_t seed_index : extension_seeds) if (!used_seeds.count(seed_index)) seed_positions.push_back(seeds[seed_index].stapled);
            if (seed_positions.empty()) continue;
            const std::vector<std::pair<size_t, size_t>> anchor_intervals = find_anchor_intervals(extension.read_interval, extension.mismatch_positions, seed_positions);
            auto mismatch_it = extension.mismatch_positions.begin();
            auto seed_it = extension_seeds.begin();
            for (const auto& anchor_interval : anchor_intervals) {
                while (mismatch_it != extension.mismatch_positions.end() && *mismatch_it < anchor_interval.first) ++mismatch_it;
                const auto internal_mismatch_begin = mismatch_it;
                while (mismatch_it != extension.mismatch_positions.end() && *mismatch_it < anchor_interval.second) ++mismatch_it;
                const auto internal_mismatch_end = mismatch_it;
                std::vector<size_t> anchor_seeds;
                while (seed_it != extension_seeds.end() && seeds[*seed_it].stapled < anchor_interval.first) ++seed_it;
                while (seed_it != extension_seeds.end() && seeds[*seed_it].stapled < anchor_interval.second) {
                    if (used_seeds.insert(*seed_it).second) anchor_seeds.push_back(*seed_it);
                    ++seed_it;
                }
                if (anchor_seeds.empty()) continue;                 // all seeds of this piece stand in pieces of earlier extensions
                // to_anchor (:4040-4081): matches and mismatches of the interval under the plain scorer
                const size_t n_mismatches = internal_mismatch_end - internal_mismatch_begin;
                const int score = match * (int)(anchor_interval.second - anchor_interval.first - n_mismatches) - mismatch * (int)n_mismatches;
                const Anchor& left_anchor = seed_anchors.at(anchor_seeds.front()); const Anchor& right_anchor = seed_anchors.at(anchor_seeds.back());
                const size_t extra_left_margin = left_anchor.read_exclusion_start() - anchor_interval.first;
                const size_t extra_right_margin = anchor_interval.second - right_anchor.read_exclusion_end();
                Anchor welded;                                      // Anchor(first, last, extra margins, score), src/algorithms/chain_items.hpp:249-262
                welded.start = left_anchor.read_start(); welded.size = right_anchor.read_end() - left_anchor.read_start();
                welded.margin_before = left_anchor.margin_before + extra_left_margin; welded.margin_after = right_anchor.margin_after + extra_right_margin;
                welded.points = score; welded.start_offset = left_anchor.start_offset; welded.end_offset = right_anchor.end_offset;
                welded.seed_length = (left_anchor.seed_length + right_anchor.seed_length) / 2;
                welded.start_paths = left_anchor.start_paths; welded.end_paths = right_anchor.end_paths;
                if (welded.read_exclusion_start() != anchor_interval.first || welded.read_exclusion_end() != anchor_interval.second)
                    throw std::runtime_error("extension_anchors: a welded anchor's exclusion zone is not its interval");
                anchor_indexes.push_back(extension_anchors.size());
                extension_anchors.push_back(welded);
                AnchorOrigin origin;
                origin.seed_sequence.push_back(anchor_seeds.front());      // :1575-1580
                if (left_anchor.read_end() <= right_anchor.read_start()) origin.seed_sequence.push_back(anchor_seeds.back());
                origin.extension = extension_index; origin.interval = anchor_interval; origin.created = extension_origins.size();
                origin.represented_seeds = std::move(anchor_seeds);
                extension_origins.push_back(std::move(origin));
            }
        }
    } else {
        for (size_t i = 0; i < seeds.size(); ++i) {
            anchor_indexes.push_back(i);
            AnchorOrigin origin;
            origin.seed_sequence.push_back(i); origin.represented_seeds.push_back(i); origin.extension = std::numeric_limits<size_t>::max(); origin.created = i;
            origin.interval = {seed_anchors[i].read_exclusion_start(), seed_anchors[i].read_exclusion_end()};
            extension_origins.push_back(std::move(origin));
        }
    }
    const std::vector<Anchor>& anchors_to_chain = do_gapless_extension ? extension_anchors : seed_anchors;
    // sort_anchor_indexes [PARITY-UNPINNED: stable]
    std::stable_sort(anchor_indexes.begin(), anchor_indexes.end(), [&](size_t a, size_t b) {
        return anchors_to_chain[a].read_start() < anchors_to_chain[b].read_start()
            || (anchors_to_chain[a].read_start() == anchors_to_chain[b].read_start() && anchors_to_chain[a].read_end() > anchors_to_chain[b].read_end());
    });
    for (size_t index : anchor_indexes) { result.anchors.push_back(anchors_to_chain[index]); result.origins.push_back(extension_origins[index]); }
    return result;
}

}  // namespace vgamd
