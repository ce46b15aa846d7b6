// read_mapq.hpp — the step both mapping routes close with (MinimizerMapper::map, reference src/minimizer_mapper.cpp:1143-1188; map_from_chains,
// src/minimizer_mapper_from_chains.cpp:957-1057), in the reference's loop shape: the mapping quality of the alignments' scores
// (MappingQualityCalculator, vg_standin/mapping_quality.hpp), capped by faster_cap over the explored minimizers (mapq_cap.hpp), the escape bonus,
// round, clamp to 0 .. 60 — and the minimizers' agglomerations (src/minimizer_mapper.hpp:565-600, :3927-3957) by a plain scan of every window.
// The checker and the CPU baseline of the engine's vgk_read_mapq / vgk_minimizer_regions (include/vgk_engine.h).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>
#include "mapq_cap.hpp"

namespace vgamd {

// Thomas Wang's 64-bit mix of a k-mer's 2-bit key: gbwtgraph's minimizer hash
uint64_t minimizer_hash(uint64_t key);

struct MinimizerInstance { uint64_t key = 0; size_t offset = 0; };       // a list entry: canonical key, first base of the k-mer
struct Agglomeration { size_t start = 0, length = 0; };

// Per list entry (offset order) the stretch of windows it wins: window s is k-mers [s, s + w), its minimizer the leftmost smallest canonical hash among
// the k-mers of ACGT only.  Throws std::runtime_error when a window's minimizer is not in the list.
std::vector<Agglomeration> minimizer_regions(const std::string& sequence, size_t k, size_t w, const std::vector<MinimizerInstance>& minimizers);

struct ReadMapqScheme {
    double log_base = 1.0, score_scale = 1.0;        // mapq_score_scale
    size_t score_window = 0;                         // mapq_score_window
    bool first = false;                              // compute_first_mapping_quality (the chain route) instead of compute_max_mapping_quality
    bool use_explored_cap = true;
};
struct ReadMapq { int32_t mapq = 0; bool stopped = false; double uncapped = 0.0, explored_cap = 0.0; std::string why; };

// scores in the reference's order; multiplicities empty or as long; unmapped: the first alignment has no mappings; quality empty: no cap.
// stopped: the reference prints an error and exits on this read (why).
ReadMapq read_mapq(const ReadMapqScheme& scheme, const std::vector<double>& scores, const std::vector<double>& multiplicities, bool unmapped,
                   const std::vector<CapMinimizer>& minimizers, const std::vector<size_t>& explored, const std::string& sequence, const std::string& quality);

}  // namespace vgamd
