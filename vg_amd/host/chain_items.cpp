// chain_items.cpp — see chain_items.hpp.  Line numbers: reference src/algorithms/chain_items.cpp.
#include "chain_items.hpp"
#include <algorithm>
#include <cmath>
#include <stdexcept>

namespace vgamd {

void TracedScore::max_in(const std::vector<TracedScore>& options, size_t option_number) {      // :48-57
    const TracedScore& option = options[option_number];
    if (option.score > score || source == nowhere()) { score = option.score; source = option_number; paths = option.paths; rec_num = option.rec_num; }
}
TracedScore TracedScore::score_from(const std::vector<TracedScore>& options, size_t option_number) {      // :59-65
    TracedScore got = options[option_number];
    got.source = option_number;
    return got;
}
TracedScore TracedScore::set_shared_paths(const std::pair<path_flags_t, path_flags_t>& new_paths) const {      // :71-94
    path_flags_t updated; size_t recs = rec_num;
    if (new_paths.first == new_paths.second) {
        if ((paths & new_paths.first) == 0) { updated = new_paths.first; ++recs; }      // a recombination between anchors: start over from the anchor's paths
        else updated = paths & new_paths.first;
    } else updated = new_paths.second;                                                  // an internally recombinant anchor: its end paths, not counted
    return {score, source, updated, recs};
}

static size_t get_read_distance(const Anchor& from, const Anchor& to) {                // :984-989
    if (to.read_start() < from.read_end()) return std::numeric_limits<size_t>::max();
    return to.read_start() - from.read_end();
}

int add_transition_if_legal(std::vector<transition_info>& transitions, const std::vector<Anchor>& to_chain, size_t max_read_lookback_bases, size_t max_indel_bases,
                            size_t from_anchor, size_t to_anchor, size_t graph_distance) {      // :270-355
    const Anchor& source_anchor = to_chain[from_anchor]; const Anchor& dest_anchor = to_chain[to_anchor];
    const size_t read_distance = get_read_distance(source_anchor, dest_anchor);
    if (read_distance == std::numeric_limits<size_t>::max()) return 1;
    if (read_distance > max_read_lookback_bases) return 2;
    if (source_anchor.read_exclusion_end() > dest_anchor.read_exclusion_start()) return 3;
    // the distance is between the two hint points; what lies between them and the anchors' facing ends is taken off
    const size_t distance_to_remove = dest_anchor.start_offset + source_anchor.end_offset;
    if (distance_to_remove > graph_distance) return 4;
    graph_distance -= distance_to_remove;
    const size_t indel_size = read_distance > graph_distance ? read_distance - graph_distance : graph_distance - read_distance;
    if (indel_size > max_indel_bases) return 5;
    transitions.push_back({from_anchor, to_anchor, indel_size});
    return 0;
}

int score_chain_gap(size_t distance_difference, size_t base_seed_length) {             // :365-373
    if (distance_difference == 0) return 0;
    return 0.01 * base_seed_length * distance_difference + 0.5 * log2(distance_difference);
}

TracedScore chain_items_dp(std::vector<TracedScore>& chain_scores, const std::vector<Anchor>& to_chain, const std::vector<candidate_transition>& candidates,
                           const ChainScoringScheme& scheme, size_t max_read_lookback_bases, size_t max_indel_bases) {      // :385-648
    if (scheme.recombination_penalty < 0 || scheme.consistency_bonus < 0) throw std::runtime_error("chain_items_dp: negative recombination_penalty or consistency_bonus");
    size_t base_seed_length = 0;
    for (const Anchor& anchor : to_chain) base_seed_length += anchor.seed_length;
    base_seed_length /= to_chain.size();
    chain_scores.resize(to_chain.size());
    // the bonus the current winner of each destination was chosen with; from nowhere every path is kept: the whole bonus
    std::vector<int> eval_bonuses(to_chain.size(), scheme.consistency_bonus);
    for (size_t i = 0; i < to_chain.size(); ++i) chain_scores[i] = {to_chain[i].points + scheme.item_bonus, TracedScore::nowhere(), to_chain[i].end_paths, 0};

    auto iteratee = [&](const transition_info& transition) {
        const Anchor& here = to_chain[transition.to_anchor];
        const int item_points = here.points + scheme.item_bonus;
        {   // from nowhere (:464-476)
            const TracedScore from_nowhere = {item_points, TracedScore::nowhere(), here.end_paths, 0};
            const int eval_nowhere = from_nowhere.score + scheme.consistency_bonus, eval_current = chain_scores[transition.to_anchor].score + eval_bonuses[transition.to_anchor];
            if (eval_nowhere > eval_current || (eval_nowhere == eval_current && from_nowhere > chain_scores[transition.to_anchor])) {
                chain_scores[transition.to_anchor] = from_nowhere; eval_bonuses[transition.to_anchor] = scheme.consistency_bonus;
            }
        }
        int jump_points = -score_chain_gap(transition.indel_size, base_seed_length) * scheme.gap_scale;      // :511
        const TracedScore source_score = TracedScore::score_from(chain_scores, transition.from_anchor);
        if ((source_score.paths & here.start_paths) == 0) jump_points -= scheme.recombination_penalty;       // check_recombination :377-383, :514
        const TracedScore from_source_score = source_score.add_points(jump_points + item_points).set_shared_paths({here.start_paths, here.end_paths});
        int eval_bonus_from = 0;                                                                             // :526-535
        if (scheme.consistency_bonus > 0) {
            const int pre_count = __builtin_popcountll(source_score.paths);
            if (pre_count > 0 && (source_score.paths & here.start_paths) != 0) eval_bonus_from = (scheme.consistency_bonus * __builtin_popcountll(from_source_score.paths)) / pre_count;
        }
        TracedScore& current_best = chain_scores[transition.to_anchor];
        const int eval_from = from_source_score.score + eval_bonus_from, eval_best = current_best.score + eval_bonuses[transition.to_anchor];
        if (eval_from > eval_best || (eval_from == eval_best && from_source_score > current_best)) { current_best = from_source_score; eval_bonuses[transition.to_anchor] = eval_bonus_from; }
    };

    // the transition iterator's part (:255-267): the legal ones, by destination read start, through the iteratee
    std::vector<transition_info> all_transitions;
    for (const candidate_transition& c : candidates) {
        if (c.from_anchor >= to_chain.size() || c.to_anchor >= to_chain.size()) throw std::runtime_error("chain_items_dp: transition outside the anchors");
        add_transition_if_legal(all_transitions, to_chain, max_read_lookback_bases, max_indel_bases, c.from_anchor, c.to_anchor, c.graph_distance);
    }
    std::stable_sort(all_transitions.begin(), all_transitions.end(), [&](const transition_info& a, const transition_info& b) {
        return to_chain[a.to_anchor].read_start() < to_chain[b.to_anchor].read_start();
    });
    for (const transition_info& transition : all_transitions) iteratee(transition);

    TracedScore best_score = TracedScore::unset();
    for (size_t to_anchor = 0; to_anchor < to_chain.size(); ++to_anchor) best_score.max_in(chain_scores, to_anchor);
    return best_score;
}

std::vector<std::pair<std::vector<size_t>, int>> chain_items_traceback(const std::vector<TracedScore>& chain_scores, const std::vector<Anchor>& to_chain,
                                                                      const TracedScore& best_past_ending_score_ever, const ChainScoringScheme& scheme, size_t max_tracebacks) {      // :650-733
    std::vector<std::pair<std::vector<size_t>, int>> tracebacks;
    tracebacks.reserve(chain_scores.size());
    std::vector<size_t> starts_in_score_order(chain_scores.size());
    for (size_t i = 0; i < starts_in_score_order.size(); ++i) starts_in_score_order[i] = i;
    // [PARITY-UNPINNED] the reference sorts by chain_scores[a] > chain_scores[b] alone (score, then source); equal ones by anchor index here
    std::sort(starts_in_score_order.begin(), starts_in_score_order.end(), [&](const size_t& a, const size_t& b) {
        return chain_scores[a] > chain_scores[b] || (!(chain_scores[b] > chain_scores[a]) && a < b);
    });
    std::vector<bool> item_is_used(chain_scores.size(), false);
    for (const size_t trace_from : starts_in_score_order) {
        if (item_is_used[trace_from]) continue;
        std::vector<size_t> traceback{trace_from};
        int penalty = best_past_ending_score_ever.score - chain_scores[trace_from].score;
        size_t here = trace_from;
        while (here != TracedScore::nowhere()) {
            item_is_used[here] = true;
            const size_t next = chain_scores[here].source;
            if (next != TracedScore::nowhere()) {
                if (item_is_used[next]) {      // stop early: give back what coming from there was worth, keep the item's own points
                    penalty += chain_scores[here].score;
                    penalty -= to_chain[here].points + scheme.item_bonus;
                    break;
                }
                traceback.push_back(next);
            }
            here = next;
        }
        tracebacks.emplace_back();
        tracebacks.back().second = penalty;
        tracebacks.back().first.assign(traceback.rbegin(), traceback.rend());
    }
    // [PARITY-UNPINNED] by penalty, equal ones in order of creation (the reference: std::sort by penalty alone)
    std::stable_sort(tracebacks.begin(), tracebacks.end(), [](const std::pair<std::vector<size_t>, int>& a, const std::pair<std::vector<size_t>, int>& b) { return a.second < b.second; });
    if (tracebacks.size() > max_tracebacks) tracebacks.resize(max_tracebacks);
    return tracebacks;
}

ChainsResult find_best_chains(const std::vector<Anchor>& to_chain, const std::vector<candidate_transition>& candidates, const ChainScoringScheme& scheme,
                              size_t max_chains, size_t max_read_lookback_bases, size_t max_indel_bases, std::vector<TracedScore>* table) {      // :735-877
    ChainsResult result;
    if (table) table->clear();
    if (to_chain.empty()) { result.chains.emplace_back(); return result; }
    std::vector<TracedScore> chain_scores;
    const TracedScore best_past_ending_score_ever = chain_items_dp(chain_scores, to_chain, candidates, scheme, max_read_lookback_bases, max_indel_bases);
    std::vector<std::pair<std::vector<size_t>, int>> tracebacks = chain_items_traceback(chain_scores, to_chain, best_past_ending_score_ever, scheme, max_chains);
    if (table) *table = chain_scores;
    if (tracebacks.empty()) { result.chains.emplace_back(); return result; }
    result.chains.reserve(tracebacks.size());
    for (auto& traceback : tracebacks) {
        ChainWithRec entry;
        const int score = best_past_ending_score_ever.score - traceback.second;
        std::vector<size_t> chain_indexes = std::move(traceback.first);
        // forward: the anchors that introduce a recombination, by set_shared_paths' rules (:797-828)
        if (!chain_indexes.empty()) {
            path_flags_t current_paths = to_chain[chain_indexes.front()].end_paths;
            for (size_t k = 1; k < chain_indexes.size(); ++k) {
                const Anchor& anchor = to_chain[chain_indexes[k]];
                if (anchor.start_paths == anchor.end_paths) {
                    if ((current_paths & anchor.start_paths) == 0) { entry.rec_positions.push_back(chain_indexes[k]); current_paths = anchor.start_paths; }
                    else current_paths &= anchor.start_paths;
                } else current_paths = anchor.end_paths;
            }
        }
        // backward: the left boundary of each (:834-856)
        if (chain_indexes.size() > 1) {
            path_flags_t current_paths = to_chain[chain_indexes.back()].start_paths;
            for (size_t k = chain_indexes.size() - 1; k > 0; --k) {
                const Anchor& anchor = to_chain[chain_indexes[k - 1]];
                if (anchor.start_paths == anchor.end_paths) {
                    if ((current_paths & anchor.end_paths) == 0) { entry.left_rec_positions.push_back(chain_indexes[k - 1]); current_paths = anchor.end_paths; }
                    else current_paths &= anchor.end_paths;
                } else current_paths = anchor.start_paths;
            }
            std::reverse(entry.left_rec_positions.begin(), entry.left_rec_positions.end());
        }
        if (entry.left_rec_positions.size() == entry.rec_positions.size())
            for (size_t i = 0; i < entry.rec_positions.size(); ++i) entry.rec_intervals.emplace_back(entry.left_rec_positions[i], entry.rec_positions[i]);
        entry.scored_chain = {score, std::move(chain_indexes)};
        result.chains.emplace_back(std::move(entry));
    }
    return result;
}

std::pair<int, std::vector<size_t>> find_best_chain(const std::vector<Anchor>& to_chain, const std::vector<candidate_transition>& candidates, const ChainScoringScheme& scheme,
                                                    size_t max_read_lookback_bases, size_t max_indel_bases) {      // :879-900
    return find_best_chains(to_chain, candidates, scheme, 1, max_read_lookback_bases, max_indel_bases).chains.front().scored_chain;
}

}  // namespace vgamd
