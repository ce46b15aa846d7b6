// read_alignments.hpp — giraffe's alignments of a short read from one extension set and its tails' alignments: what MinimizerMapper::map_from_extensions
// does with a set at reference src/minimizer_mapper.cpp:934-1000 — extension_to_alignment (:3905-3914) for the leading full extensions of a full-length
// set, find_optimal_tail_alignments (:5369-5622) otherwise, with find_pareto_frontier / gap_penalty / mismatch_penalty / flank_penalty (:5263-5311),
// add_to_path (:5318-5367), process_until_threshold_e (src/minimizer_mapper.hpp:1580-1659), the Paths get_best_alignment_against_any_tree returns
// (:5626-5743) and GaplessExtension::to_path (src/gbwt_extender.cpp:119-156).  Host logic, the checker of the engine's vgk_read_alignments
// (include/vgk_engine.h): same rule, the reference's loop shape, over the stand-in's Path / Mapping / Edit.  The tails arrive aligned (their scores and
// ops), as the tail stage leaves them: this file aligns nothing.
// [PARITY-UNPINNED] the reference shuffles the extensions that tie for the top score with the read's generator (sort_shuffling_ties); here they stay in
// extension order.  Node ids are (oriented node >> 1) + 1.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>
#include "extension_anchors.hpp"
#include "vg_standin/alignment.hpp"

namespace vgamd {

struct OrientedGraph {                     // what the rule reads of the GBWTGraph: every oriented node's length and bases
    const uint32_t* length; const uint64_t* seq_off; const char* seq;
    size_t get_length(uint32_t o) const { return length[o]; }
    char base(uint32_t o, size_t at) const { return seq[seq_off[o] + at]; }
};
struct TailOp { uint32_t node; uint32_t length; int op; };        // vgk_op: 0 M, 1 I, 2 D, 3 S
struct TailResult { int32_t score = 0; size_t first_offset = 0; std::vector<TailOp> ops; };      // no ops: the soft clip
struct SetExtension : Extension { int32_t score = 0; TailResult left_tail, right_tail; };
struct TailScores { int32_t match, mismatch, gap_open, gap_extension, full_length_bonus; };
struct ReadAlignment { int kind = 0; size_t extension = SIZE_MAX; Alignment alignment; uint32_t identity_num = 0, identity_den = 0; };

Path extension_to_path(const SetExtension& extension, const OrientedGraph& graph, const std::string& sequence);
// -> DIRECT alignments in set order, or BEST and SECOND
std::vector<ReadAlignment> read_alignments(const std::string& sequence, const std::vector<SetExtension>& extensions, bool full_length_extensions, const OrientedGraph& graph,
                                           const TailScores& scorer, int extension_score_threshold, size_t max_local_extensions, size_t window_length);

}  // namespace vgamd
