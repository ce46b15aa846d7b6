// read_mapq.cpp — see read_mapq.hpp.
#include "read_mapq.hpp"
#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>
#include "vg_standin/mapping_quality.hpp"

namespace vgamd {

uint64_t minimizer_hash(uint64_t key) {
    key = (~key) + (key << 21); key ^= key >> 24; key = (key + (key << 3)) + (key << 8); key ^= key >> 14;
    key = (key + (key << 2)) + (key << 4); key ^= key >> 28; key += key << 31;
    return key;
}

std::vector<Agglomeration> minimizer_regions(const std::string& sequence, size_t k, size_t w, const std::vector<MinimizerInstance>& minimizers) {
    std::vector<Agglomeration> out(minimizers.size());
    const size_t L = sequence.size();
    if (k == 0 || k > 31 || w == 0) throw std::runtime_error("minimizer_regions: k or w out of range");
    if (L + 1 < k + w) { if (!minimizers.empty()) throw std::runtime_error("minimizer_regions: a read with no complete window has minimizers"); return out; }
    // every k-mer's canonical hash, or none
    const size_t n_kmers = L - k + 1, n_windows = L - k - w + 2;
    std::vector<uint64_t> hash(n_kmers); std::vector<char> valid(n_kmers, 1);
    for (size_t j = 0; j < n_kmers; ++j) {
        uint64_t fwd = 0, rev = 0;
        for (size_t i = 0; i < k; ++i) {
            int x;
            switch (sequence[j + i]) { case 'A': x = 0; break; case 'C': x = 1; break; case 'G': x = 2; break; case 'T': x = 3; break; default: x = -1; }
            if (x < 0) { valid[j] = 0; break; }
            fwd = fwd << 2 | (uint64_t)x; rev = rev >> 2 | (uint64_t)(3 - x) << (2 * (k - 1));
        }
        if (valid[j]) hash[j] = std::min(minimizer_hash(fwd), minimizer_hash(rev));
    }
    std::vector<size_t> first(minimizers.size(), 0), last(minimizers.size(), 0); std::vector<char> won(minimizers.size(), 0);
    size_t at = 0;                                                // the winners' offsets never decrease: one cursor into the list
    for (size_t s = 0; s < n_windows; ++s) {
        size_t best = n_kmers;
        for (size_t j = s; j < s + w; ++j) if (valid[j] && (best == n_kmers || hash[j] < hash[best])) best = j;      // the leftmost smallest
        if (best == n_kmers) continue;                            // a window with no valid k-mer
        while (at < minimizers.size() && minimizers[at].offset < best) ++at;
        if (at == minimizers.size() || minimizers[at].offset != best) throw std::runtime_error("minimizer_regions: a window's minimizer is not in the list");
        if (!won[at]) { won[at] = 1; first[at] = s; }
        last[at] = s;
    }
    for (size_t i = 0; i < minimizers.size(); ++i) {
        if (!won[i]) throw std::runtime_error("minimizer_regions: a listed minimizer wins no window");
        out[i].start = first[i]; out[i].length = last[i] + w + k - 1 - first[i];
    }
    return out;
}

ReadMapq read_mapq(const ReadMapqScheme& scheme, const std::vector<double>& scores, const std::vector<double>& multiplicities, bool unmapped,
                   const std::vector<CapMinimizer>& minimizers, const std::vector<size_t>& explored_in, const std::string& sequence, const std::string& quality) {
    ReadMapq out;
    auto stop = [&](const std::string& why) { out = ReadMapq(); out.stopped = true; out.why = why; return out; };
    if (!unmapped && scores.empty()) return stop("no alignment");                        // crash_unless(!mappings.empty())
    // :957-968 (both factors are 1 on the short-read route)
    std::vector<double> scaled_scores; scaled_scores.reserve(scores.size());
    for (double score : scores) {
        double scaled_score = score;
        if (scheme.score_window > 0) scaled_score = scaled_score * scheme.score_window / sequence.size();
        scaled_score *= scheme.score_scale;
        scaled_scores.push_back(scaled_score);
    }
    const MappingQualityCalculator calc(1.0, 4.0, scheme.log_base);
    const std::vector<double>* mult = multiplicities.empty() ? nullptr : &multiplicities;
    // Compute MAPQ if not unmapped. Otherwise use 0 instead of the 50% this would give us.
    double mapq = unmapped ? 0 : scheme.first ? calc.compute_first_mapping_quality(scaled_scores, false, mult) : calc.compute_max_mapping_quality(scaled_scores, false, mult);
    out.uncapped = mapq;
    out.explored_cap = std::numeric_limits<double>::infinity();
    if (scheme.use_explored_cap) {
        std::vector<size_t> explored = explored_in;
        if (!quality.empty()) for (size_t i : explored) {
            if (minimizers[i].length > 32) return stop("a minimizer longer than prob_for_at_least_one's table");
            if (minimizers[i].length > 0 && minimizers[i].agglomeration_start > sequence.size()) return stop("an agglomeration behind the read");
        }
        // (ties of end and start in list order: std::sort inside faster_cap leaves them where it likes, and finds them sorted)
        std::stable_sort(explored.begin(), explored.end(), [&](size_t a, size_t b) {
            const size_t ae = minimizers[a].agglomeration_start + minimizers[a].agglomeration_length, be = minimizers[b].agglomeration_start + minimizers[b].agglomeration_length;
            return ae < be || (ae == be && minimizers[a].agglomeration_start < minimizers[b].agglomeration_start);
        });
        const double escape_bonus = mapq < std::numeric_limits<int32_t>::max() ? 1.0 : 2.0;
        try { out.explored_cap = faster_cap(minimizers, explored, sequence, quality); }
        catch (std::runtime_error& e) { return stop(e.what()); }
        const double mapq_explored_cap = escape_bonus * out.explored_cap;
        // Apply the caps and transformations (:1177 takes min(mapq, 60) first, :1042 does not: the clamp below makes them one)
        mapq = std::round(std::min(mapq_explored_cap, mapq));
    }
    // Make sure to clamp 0-60.
    mapq = std::max(mapq, 0.0);
    mapq = std::min(mapq, 60.0);
    out.mapq = (int32_t)mapq;
    return out;
}

}  // namespace vgamd
