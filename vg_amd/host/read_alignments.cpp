// read_alignments.cpp — see read_alignments.hpp.  Reference line numbers are src/minimizer_mapper.cpp's unless a file is named.
#include "read_alignments.hpp"
#include <algorithm>
#include <functional>
#include <numeric>

namespace vgamd {
namespace {

typedef std::pair<uint32_t, int32_t> pareto_point;      // (value, cost)

void find_pareto_frontier(std::vector<pareto_point>& v) {
    if (v.empty()) return;
    std::sort(v.begin(), v.end(), [](pareto_point a, pareto_point b) { return (a.second < b.second || (a.second == b.second && a.first > b.first)); });
    size_t tail = 1;
    for (size_t i = 1; i < v.size(); i++) {
        if (v[i].first <= v[tail - 1].first) continue;
        v[tail] = v[i];
        tail++;
    }
    v.resize(tail);
    std::sort(v.begin(), v.end());
}
int32_t gap_penalty(size_t length, const TailScores& s) { return (length == 0 ? 0 : s.gap_open + (int32_t)(length - 1) * s.gap_extension); }
int32_t mismatch_penalty(size_t n, const TailScores& s) { return (int32_t)n * (s.match + s.mismatch); }
int32_t gap_penalty(size_t start, size_t limit, const TailScores& s) { return (start >= limit ? s.gap_open : s.gap_open + (int32_t)(limit - start - 1) * s.gap_extension); }
int32_t flank_penalty(size_t length, const std::vector<pareto_point>& frontier, const TailScores& s) {
    int32_t result = gap_penalty(length, s);
    for (size_t i = 0; i < frontier.size(); i++) {
        int32_t candidate = frontier[i].second + gap_penalty(frontier[i].first, length, s);
        result = std::min(result, candidate);
        if (frontier[i].first >= length) break;
    }
    return result;
}

bool mapping_is_total_insertion(const Mapping& m) { return m.edit.size() == 1 && edit_is_insertion(m.edit[0]); }

void add_to_path(Path* target, Path* to_append) {
    for (auto& mapping : to_append->mapping) {
        if (!target->mapping.empty()) {
            Mapping* prev_mapping = &target->mapping.back();
            if (mapping.position.node_id == prev_mapping->position.node_id) {
                bool can_combine = false;
                if (mapping.position.offset != 0) {
                    can_combine = true;
                } else {
                    bool prev_is_total_insert = mapping_is_total_insertion(*prev_mapping);
                    bool is_total_insert = mapping_is_total_insertion(mapping);
                    if (prev_is_total_insert || is_total_insert) {
                        can_combine = true;
                        if (prev_is_total_insert) prev_mapping->position = mapping.position;
                    }
                }
                if (can_combine) {
                    for (auto& edit : mapping.edit) prev_mapping->edit.push_back(std::move(edit));
                    continue;
                }
            }
        }
        target->mapping.push_back(std::move(mapping));
    }
}

Position position_of(uint32_t oriented, size_t offset) { Position p; p.node_id = (int64_t)(oriented >> 1) + 1; p.is_reverse = (oriented & 1u) != 0; p.offset = (int64_t)offset; return p; }
char complement(char c) { switch (c) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; default: return 'N'; } }
std::string reverse_complement(const std::string& s) { std::string r(s.rbegin(), s.rend()); for (char& c : r) c = complement(c); return r; }
bool is_acgt(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

// GSSWAligner::ops_to_alignment (vg_amd/host/aligner.cpp:68-114) over a tail's ops, whose nodes are oriented nodes of the graph already.  A visit of a node
// ends where the node changes, or where its bases are spent and an M or D op follows (a self-loop: the ops no longer tell the two tree nodes apart).
// node_of: the oriented node behind each mapping, for the flip
Path ops_to_path(const TailResult& tail, const std::string& to_seq, const OrientedGraph& graph, std::vector<uint32_t>& node_of) {
    Path path;
    size_t to_pos = 0, from_pos = tail.first_offset;
    size_t i = 0; bool first_node = true;
    while (i < tail.ops.size()) {
        uint32_t node = tail.ops[i].node;
        if (!first_node) from_pos = 0;
        first_node = false;
        path.mapping.emplace_back();
        Mapping& mapping = path.mapping.back();
        mapping.position = position_of(node, from_pos);
        node_of.push_back(node);
        size_t k = i;
        for (; k < tail.ops.size() && tail.ops[k].node == node; ++k) {
            const int32_t length = (int32_t)tail.ops[k].length;
            const bool on_graph = tail.ops[k].op == 0 || tail.ops[k].op == 2;
            if (k > i && on_graph && from_pos >= graph.get_length(node)) break;
            switch (tail.ops[k].op) {
                case 0: {
                    size_t hpos = from_pos, last_start = from_pos, q = to_pos;
                    for (; hpos < from_pos + length; ++hpos, ++q) {
                        if (!is_acgt(to_seq[q]) || graph.base(node, hpos) != to_seq[q]) {
                            if (hpos - last_start > 0) { Edit e; e.from_length = e.to_length = (int32_t)(hpos - last_start); mapping.edit.push_back(e); }
                            Edit e; e.from_length = e.to_length = 1; e.sequence = to_seq.substr(q, 1); mapping.edit.push_back(e);
                            last_start = hpos + 1;
                        }
                    }
                    if (hpos - last_start > 0) { Edit e; e.from_length = e.to_length = (int32_t)(hpos - last_start); mapping.edit.push_back(e); }
                    to_pos += length; from_pos += length;
                } break;
                case 2: { Edit e; e.from_length = length; e.to_length = 0; mapping.edit.push_back(e); from_pos += length; } break;
                default: { Edit e; e.from_length = 0; e.to_length = length; e.sequence = to_seq.substr(to_pos, length); mapping.edit.push_back(e); to_pos += length; } break;
            }
        }
        i = k;
    }
    return path;
}
// reverse_complement_path (src/path.cpp:1863-1882) with reverse_complement_mapping (:1791-1829)
Path reverse_complement_path(const Path& path, const std::vector<uint32_t>& node_of, const OrientedGraph& graph) {
    Path reversed;
    for (size_t i = path.mapping.size(); i-- > 0;) {
        const Mapping& m = path.mapping[i];
        Mapping r;
        const size_t used_bases = (size_t)mapping_from_length(m), unused_bases_after = (size_t)m.position.offset;
        r.position = m.position;
        r.position.offset = (int64_t)(graph.get_length(node_of[i]) - used_bases - unused_bases_after);
        r.position.is_reverse = !m.position.is_reverse;
        for (size_t k = m.edit.size(); k-- > 0;) { Edit e = m.edit[k]; e.sequence = reverse_complement(e.sequence); r.edit.push_back(e); }
        reversed.mapping.push_back(r);
    }
    for (size_t i = 0; i < reversed.mapping.size(); ++i) reversed.mapping[i].rank = (int64_t)i + 1;
    return reversed;
}
// get_best_alignment_against_any_tree (:5626-5743) with the trees' alignments already reduced to the winner: the soft clip unless a tree scored above 0
std::pair<Path, int64_t> best_tail_alignment(const TailResult& tail, const std::string& sequence, const Position& default_position, bool pin_left, const OrientedGraph& graph) {
    Path best_path; int32_t best_score = 0;
    if (!sequence.empty()) {
        best_path.mapping.emplace_back();
        Mapping& m = best_path.mapping.back();
        Edit e; e.from_length = 0; e.to_length = (int32_t)sequence.size(); e.sequence = sequence;
        m.edit.push_back(e); m.position = default_position;
        if (!tail.ops.empty()) {
            std::vector<uint32_t> node_of;
            best_path = ops_to_path(tail, pin_left ? sequence : reverse_complement(sequence), graph, node_of);
            if (!pin_left) best_path = reverse_complement_path(best_path, node_of, graph);
            best_score = tail.score;
        }
    }
    return std::make_pair(best_path, (int64_t)best_score);
}
size_t tail_offset(const SetExtension& x, const OrientedGraph& graph) {
    size_t result = x.offset + (x.read_interval.second - x.read_interval.first);
    for (size_t i = 0; i + 1 < x.path.size(); i++) result -= graph.get_length(x.path[i]);
    return result;
}
void set_identity(ReadAlignment& a) {       // identity(path), vg_standin/alignment.hpp:51-60, kept as its two integers
    const Path& p = a.alignment.path;
    size_t total = (size_t)path_to_length(p), matched = 0;
    for (size_t i = 0; i < p.mapping.size(); ++i) for (size_t j = 0; j < p.mapping[i].edit.size(); ++j) {
        const Edit& e = p.mapping[i].edit[j];
        if (edit_is_match(e)) matched += (size_t)e.from_length;
        else if (edit_is_insertion(e)) {
            const bool first = i == 0 && j == 0, last = i + 1 == p.mapping.size() && j + 1 == p.mapping[i].edit.size();
            if (first || last) total -= (size_t)e.to_length;
        }
    }
    a.identity_num = total ? (uint32_t)matched : 0u; a.identity_den = (uint32_t)total;
    a.alignment.identity = total ? (double)matched / (double)total : 0.0;
}

}  // namespace

Path extension_to_path(const SetExtension& x, const OrientedGraph& graph, const std::string& sequence) {
    Path result;
    auto mismatch = x.mismatch_positions.begin();
    size_t read_offset = x.read_interval.first, node_offset = x.offset;
    for (size_t i = 0; i < x.path.size(); i++) {
        size_t limit = std::min(read_offset + graph.get_length(x.path[i]) - node_offset, x.read_interval.second);
        result.mapping.emplace_back();
        Mapping& mapping = result.mapping.back();
        mapping.position = position_of(x.path[i], node_offset);
        while (mismatch != x.mismatch_positions.end() && *mismatch < limit) {
            if (read_offset < *mismatch) { Edit e; e.from_length = e.to_length = (int32_t)(*mismatch - read_offset); mapping.edit.push_back(e); }
            Edit e; e.from_length = e.to_length = 1; e.sequence = std::string(1, sequence[*mismatch]); mapping.edit.push_back(e);
            read_offset = *mismatch + 1;
            ++mismatch;
        }
        if (read_offset < limit) { Edit e; e.from_length = e.to_length = (int32_t)(limit - read_offset); mapping.edit.push_back(e); read_offset = limit; }
        mapping.rank = (int64_t)i + 1;
        node_offset = 0;
    }
    return result;
}

std::vector<ReadAlignment> read_alignments(const std::string& sequence, const std::vector<SetExtension>& extended_seeds, bool full_length_extensions, const OrientedGraph& graph,
                                           const TailScores& scorer, int extension_score_threshold, size_t max_local_extensions, size_t window_length) {
    std::vector<ReadAlignment> out;
    const size_t seq_len = sequence.size();
    if (full_length_extensions) {                                   // :939-969
        for (size_t k = 0; k < extended_seeds.size() && (k == 0 || extended_seeds[k].full()); ++k) {
            ReadAlignment a; a.kind = 0; a.extension = k;
            a.alignment.path = extension_to_path(extended_seeds[k], graph, sequence); a.alignment.score = extended_seeds[k].score;
            a.identity_num = (uint32_t)(seq_len - extended_seeds[k].mismatches()); a.identity_den = (uint32_t)seq_len;
            out.push_back(std::move(a));
        }
        return out;
    }
    size_t min_tails = 1;
    for (const SetExtension& extension : extended_seeds) if (extension.full()) min_tails++;
    if (min_tails < 2) min_tails = 2;
    std::vector<pareto_point> left_frontier, right_frontier;
    for (const SetExtension& extension : extended_seeds) {
        if (extension.full()) continue;
        int32_t left_penalty = gap_penalty(extension.read_interval.first, scorer);
        int32_t mid_penalty = mismatch_penalty(extension.mismatches(), scorer);
        int32_t right_penalty = gap_penalty(seq_len - extension.read_interval.second, scorer);
        left_frontier.push_back(pareto_point((uint32_t)extension.read_interval.second, mid_penalty + left_penalty));
        right_frontier.push_back(pareto_point((uint32_t)(seq_len - extension.read_interval.first), mid_penalty + right_penalty));
        if (extension.mismatches() > 0) {
            left_frontier.push_back(pareto_point((uint32_t)extension.mismatch_positions.front(), left_penalty));
            right_frontier.push_back(pareto_point((uint32_t)(seq_len - extension.mismatch_positions.back() - 1), right_penalty));
        }
    }
    left_frontier.push_back(pareto_point((uint32_t)(window_length - 1), 0));
    right_frontier.push_back(pareto_point((uint32_t)(window_length - 1), 0));
    find_pareto_frontier(left_frontier);
    find_pareto_frontier(right_frontier);

    Path winning_left, winning_middle, winning_right; int32_t winning_score = 0; size_t winning_extension = SIZE_MAX;
    Path second_left, second_middle, second_right; int32_t second_score = 0; size_t second_extension = SIZE_MAX;
    bool partial_extension_aligned = false;
    int32_t threshold = -1;
    auto process_item = [&](size_t extended_seed_num) -> bool {
        const SetExtension& extension = extended_seeds[extended_seed_num];
        if (threshold < 0) threshold = extension.score - extension_score_threshold;
        if (!extension.full()) {
            if (partial_extension_aligned && extension.score <= threshold) {
                int32_t score_estimate = (int32_t)seq_len * scorer.match + 2 * scorer.full_length_bonus - mismatch_penalty(extension.mismatches(), scorer);
                if (!extension.left_full) score_estimate -= flank_penalty(extension.read_interval.first, left_frontier, scorer);
                if (!extension.right_full) score_estimate -= flank_penalty(seq_len - extension.read_interval.second, right_frontier, scorer);
                if (score_estimate <= winning_score) return true;
            }
            partial_extension_aligned = true;
        }
        std::pair<Path, int64_t> left_tail_result{{}, 0}, right_tail_result{{}, 0};
        if (!extension.left_full)
            left_tail_result = best_tail_alignment(extension.left_tail, sequence.substr(0, extension.read_interval.first), position_of(extension.path.front(), extension.offset), false, graph);
        if (!extension.right_full)
            right_tail_result = best_tail_alignment(extension.right_tail, sequence.substr(extension.read_interval.second), position_of(extension.path.back(), tail_offset(extension, graph)), true, graph);
        int32_t total_score = extension.score + (int32_t)left_tail_result.second + (int32_t)right_tail_result.second;
        int64_t winning_start = winning_score == 0 ? 0 : (winning_left.mapping.empty() ? winning_middle.mapping.front().position.node_id : winning_left.mapping.front().position.node_id);
        int64_t current_start = left_tail_result.first.mapping.empty() ? (int64_t)(extension.path.front() >> 1) + 1 : left_tail_result.first.mapping.front().position.node_id;
        int64_t winning_end = winning_score == 0 ? 0 : (winning_right.mapping.empty() ? winning_middle.mapping.back().position.node_id : winning_right.mapping.back().position.node_id);
        int64_t current_end = right_tail_result.first.mapping.empty() ? (int64_t)(extension.path.back() >> 1) + 1 : right_tail_result.first.mapping.back().position.node_id;
        bool different_left = winning_start != current_start;
        bool different_right = winning_end != current_end;
        if (total_score > winning_score || winning_score == 0) {
            if (winning_score != 0 && different_left && different_right) {
                second_score = winning_score; second_extension = winning_extension;
                second_left = std::move(winning_left); second_middle = std::move(winning_middle); second_right = std::move(winning_right);
            }
            winning_score = total_score; winning_extension = extended_seed_num;
            winning_left = std::move(left_tail_result.first);
            winning_middle = extension_to_path(extension, graph, sequence);
            winning_right = std::move(right_tail_result.first);
        } else if ((total_score > second_score || second_score == 0) && different_left && different_right) {
            second_score = total_score; second_extension = extended_seed_num;
            second_left = std::move(left_tail_result.first);
            second_middle = extension_to_path(extension, graph, sequence);
            second_right = std::move(right_tail_result.first);
        }
        return true;
    };
    {   // process_until_threshold_e (src/minimizer_mapper.hpp:1580-1659); sort_shuffling_ties without the shuffle
        const size_t items = extended_seeds.size();
        std::vector<size_t> indexes_in_order(items);
        std::iota(indexes_in_order.begin(), indexes_in_order.end(), 0);
        std::stable_sort(indexes_in_order.begin(), indexes_in_order.end(), [&](size_t a, size_t b) { return extended_seeds[a].score > extended_seeds[b].score; });
        const double score_threshold = extension_score_threshold;
        double cutoff = items == 0 ? 0 : (double)extended_seeds[indexes_in_order[0]].score - score_threshold;
        size_t unskipped = 0;
        for (size_t i = 0; i < indexes_in_order.size(); i++) {
            size_t item_num = indexes_in_order[i];
            if (score_threshold != 0 && (double)extended_seeds[item_num].score <= cutoff) {
                if (unskipped < min_tails) unskipped += (size_t)process_item(item_num);
            } else if (unskipped < max_local_extensions) unskipped += (size_t)process_item(item_num);
        }
    }
    ReadAlignment best, second_best;
    best.kind = 1; best.extension = winning_extension; best.alignment.score = winning_score;
    second_best.kind = 2; second_best.extension = second_extension; second_best.alignment.score = second_score;
    best.alignment.path = std::move(winning_left);
    add_to_path(&best.alignment.path, &winning_middle);
    add_to_path(&best.alignment.path, &winning_right);
    set_identity(best);
    second_best.alignment.path = std::move(second_left);
    add_to_path(&second_best.alignment.path, &second_middle);
    add_to_path(&second_best.alignment.path, &second_right);
    set_identity(second_best);
    out.push_back(std::move(best)); out.push_back(std::move(second_best));
    return out;
}

}  // namespace vgamd
