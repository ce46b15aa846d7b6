// pair_mapq.hpp — the step MinimizerMapper::map_paired closes with (reference src/minimizer_mapper.cpp:2476-2765; score_alignment_pair :6017-6028),
// in the reference's loop shape: the candidate pairs' scores, process_until_threshold with ties in index order, the multiplicities of rescued
// pairs, the quality of the ordered scores (MappingQualityCalculator, vg_standin/mapping_quality.hpp), the fragment-cluster cap, the score groups,
// and per mate the caps both share — the two explored caps (faster_cap through read_mapq.hpp, or given) summed —, the unpaired cap, the halving for
// unreachable mates and max(min(capped, 120) / 2, 0).  The checker and the CPU baseline of the engine's vgk_pair_mapq (include/vgk_engine.h).
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace vgamd {

enum PairType { paired, unpaired, rescued_from_first, rescued_from_second };      // src/minimizer_mapper.hpp:626

struct PairCandidate {                          // one entry of paired_alignments with what the parallel vectors hold of it
    std::array<int32_t, 2> score{{0, 0}};       // the two alignments' scores
    int64_t fragment_distance = 0;              // distance_between; numeric_limits<int64_t>::max(): unreachable
    std::array<uint32_t, 2> alignment{{0, 0}};  // which of the pair's alignments of each read
    size_t better_cluster_count = 0;
    int type = paired;
    std::array<bool, 2> aligned{{true, true}};  // path().mapping_size() > 0
};

struct PairMapqScheme {
    double log_base = 1.0, fragment_mean = 0.0, fragment_sd = 1.0;
    size_t max_multimaps = 1, max_rescue_attempts = 15;
};

struct PairMapq {
    std::array<int32_t, 2> mapq{{0, 0}};
    bool stopped = false; std::string why;
    size_t n_chosen = 0;
    double uncapped = 0.0, fragment_cluster_cap = 0.0;
    std::array<double, 2> explored_cap{{0.0, 0.0}}, score_group{{0.0, 0.0}}, applied_cap{{0.0, 0.0}};
    std::vector<double> paired_scores;          // per candidate
    std::vector<size_t> order;                  // the candidates in score order
};

double score_alignment_pair(const PairMapqScheme& scheme, int32_t score1, int32_t score2, int64_t fragment_distance);
// A candidate's pair score (:2376 | :2388)
double pair_candidate_score(const PairMapqScheme& scheme, const PairCandidate& c);

// unpaired_scores: the scores of each read's unpaired alignments; explored_caps: faster_cap of each read.
// stopped: a pair this rule has no answer for (why) — everything else 0, the order the candidates'.
PairMapq pair_mapq(const PairMapqScheme& scheme, const std::vector<PairCandidate>& candidates, const std::array<size_t, 2>& unpaired_count,
                   const std::array<size_t, 2>& rescued_count, const std::array<std::vector<double>, 2>& unpaired_scores, const std::array<double, 2>& explored_caps);

}  // namespace vgamd
