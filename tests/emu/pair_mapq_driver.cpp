// pair_mapq_driver.cpp — test infrastructure only: the serial statement of the device's rule for a pair's mapping qualities (pair_mapq_device.hpp:
// pm_candidate_score, pm_pair_one — what the kernels call — and, without given caps, read_mapq_device.hpp's mq_cap_one for both mates) behind one C
// call with vgk_pair_mapq's arguments less the context, so that it can be held to the host shim and to a plain statement without a GPU
// (tests/test_pair_mapq.py).  The checks are the engine's own (pm_validate_pair, mq_validate_sweep).  With -DPM_DRIVER_MAIN the same call as a program
// of its own, for a run under the host sanitizers: it reads one call from a file of 64-bit words and raw arrays (the test writes it) and writes the
// answer likewise.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../vg_amd/csrc/pair_mapq_device.hpp"

using namespace vgk;

extern "C" int vgt_pair_mapq_serial(const vgk_pair_mapq_scheme* scheme, uint32_t n, const uint64_t* cand_off, const vgk_pair_candidate* candidates, const vgk_pair_counts* counts,
                                    const uint64_t* unpaired_off, const int32_t* unpaired_scores, const double* given_cap, const uint64_t* minimizer_off,
                                    const vgk_read_minimizer* minimizers, const vgk_minimizer_region* regions, const uint8_t* explored, const uint64_t* read_off,
                                    const uint8_t* quality, vgk_pair_mapq_result* out, double* pair_score, uint32_t* order) {
    if (!scheme || (scheme->flags & ~(uint32_t)VGK_PAIR_MAPQ_NO_EXPLORED_CAP)) return VGK_EINVAL;
    if (!(scheme->log_base > 0.0) || !(scheme->fragment_sd > 0.0) || std::isinf(scheme->log_base) || std::isinf(scheme->fragment_sd) || !std::isfinite(scheme->fragment_mean)) return VGK_EINVAL;
    if (!n) return VGK_OK;
    const bool capped = !(scheme->flags & VGK_PAIR_MAPQ_NO_EXPLORED_CAP), sweep = capped && !given_cap && quality;
    if (cand_off[0] != 0 || (unpaired_off && unpaired_off[0] != 0) || (sweep && (minimizer_off[0] != 0 || read_off[0] != 0))) return VGK_EINVAL;
    for (uint32_t p = 0; p < n; ++p) if (cand_off[p + 1] < cand_off[p]) return VGK_EINVAL;
    for (uint64_t r = 0; r < 2 * (uint64_t)n; ++r) {
        if (unpaired_off && unpaired_off[r + 1] < unpaired_off[r]) return VGK_EINVAL;
        if (sweep && (minimizer_off[r + 1] < minimizer_off[r] || read_off[r + 1] < read_off[r])) return VGK_EINVAL;
        if (sweep && minimizer_off[r + 1] - minimizer_off[r] >= MQ_MAX_READ_MINIMIZERS) return VGK_ETOOBIG;
    }
    // ---- the mates' caps
    std::vector<double> caps; std::vector<int32_t> cap_status;
    if (sweep) {
        std::vector<double> phred(MQ_PHRED_ENTRIES), events(MQ_EVENT_ENTRIES);
        read_mapq_tables(phred.data(), events.data());
        caps.assign(2 * (size_t)n, 0.0); cap_status.assign(2 * (size_t)n, 0);
        std::vector<int32_t> verdict(2 * (size_t)n);
        MqParams Q{};
        Q.k = scheme->k; Q.n_reads = 2 * n; Q.min_off = minimizer_off; Q.mins = minimizers; Q.regions = regions; Q.explored = explored; Q.read_off = read_off; Q.qual = quality;
        Q.phred = phred.data(); Q.events = events.data(); Q.status = verdict.data(); Q.cap_out = caps.data(); Q.cap_status = cap_status.data();
        for (uint32_t r = 0; r < 2 * n; ++r) {
            verdict[r] = mq_validate_sweep(Q, r);
            std::vector<uint32_t> work(mq_work_words(verdict[r] == VGK_OK ? mq_count_explored(Q, r) : 0));      // exactly its words: the sanitizer sees one too many
            mq_cap_one(Q, r, work.data());
        }
    }
    // ---- the pairs
    PmParams P{};
    P.log_base = scheme->log_base; P.mean = scheme->fragment_mean; P.sd = scheme->fragment_sd; P.quality_scale = 10.0 / std::log(10.0);
    P.max_multimaps = scheme->max_multimaps; P.max_rescue_attempts = scheme->max_rescue_attempts; P.n_pairs = n; P.n_candidates = cand_off[n];
    P.cand_off = cand_off; P.cands = candidates; P.counts = counts; P.unp_off = unpaired_off; P.unp_scores = unpaired_scores;
    P.caps = capped && given_cap ? given_cap : sweep ? caps.data() : nullptr; P.cap_status = sweep ? cap_status.data() : nullptr;
    P.pair_score = pair_score; P.order = order; P.out = out;
    std::vector<int32_t> status(n);
    P.status = status.data();
    for (uint64_t j = 0; j < P.n_candidates; ++j) pair_score[j] = pm_candidate_score(P, candidates[j]);
    for (uint32_t p = 0; p < n; ++p) {
        status[p] = pm_validate_pair(P, p);
        std::vector<uint32_t> work(pm_work_words(status[p] == VGK_OK ? cand_off[p + 1] - cand_off[p] : 0));
        pm_pair_one(P, p, work.data());
    }
    return VGK_OK;
}

#ifdef PM_DRIVER_MAIN
// in:  12 words (pairs, candidates, unpaired scores, minimizers, bases, max_multimaps, max_rescue_attempts, k, flags, has unpaired scores, has given caps, has
//      qualities), 3 doubles (log base, fragment mean, fragment sd), then cand_off, candidates, counts, unpaired_off, unpaired scores, given caps, minimizer_off,
//      minimizers, regions, explored, read_off, qualities — an absent array is empty
// out: 1 word (rc), then the 80-byte results, the pair scores and the order
template <class T> static bool get(FILE* f, std::vector<T>& v, uint64_t n) { v.assign(n + 1, T{}); return !n || fread(v.data(), sizeof(T), n, f) == n; }
int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s call.bin answer.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    uint64_t h[12]; double d[3];
    if (!f || fread(h, 8, 12, f) != 12 || fread(d, 8, 3, f) != 3) return 2;
    const uint32_t n = (uint32_t)h[0];
    std::vector<uint64_t> coff, uoff, moff, roff; std::vector<vgk_pair_candidate> cands; std::vector<vgk_pair_counts> counts; std::vector<int32_t> alone; std::vector<double> given;
    std::vector<vgk_read_minimizer> mins; std::vector<vgk_minimizer_region> regions; std::vector<uint8_t> explored, qual;
    if (!get(f, coff, (uint64_t)n + 1) || !get(f, cands, h[1]) || !get(f, counts, n) || !get(f, uoff, h[9] ? 2 * (uint64_t)n + 1 : 0) || !get(f, alone, h[9] ? h[2] : 0)
        || !get(f, given, h[10] ? 2 * (uint64_t)n : 0) || !get(f, moff, 2 * (uint64_t)n + 1) || !get(f, mins, h[3]) || !get(f, regions, h[3]) || !get(f, explored, h[3])
        || !get(f, roff, 2 * (uint64_t)n + 1) || !get(f, qual, h[11] ? h[4] : 0)) return 2;
    fclose(f);
    std::vector<vgk_pair_mapq_result> out((size_t)n + 1); std::vector<double> pair_score(h[1] + 1); std::vector<uint32_t> order(h[1] + 1);
    vgk_pair_mapq_scheme scheme = {d[0], d[1], d[2], (uint32_t)h[5], (uint32_t)h[6], (uint32_t)h[7], (uint32_t)h[8]};
    const int rc = vgt_pair_mapq_serial(&scheme, n, coff.data(), cands.data(), counts.data(), h[9] ? uoff.data() : nullptr, h[9] ? alone.data() : nullptr, h[10] ? given.data() : nullptr,
                                        moff.data(), mins.data(), regions.data(), explored.data(), roff.data(), h[11] ? qual.data() : nullptr, out.data(), pair_score.data(), order.data());
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    const uint64_t o[1] = {(uint64_t)(int64_t)rc};
    fwrite(o, 8, 1, g); fwrite(out.data(), sizeof(vgk_pair_mapq_result), n, g); fwrite(pair_score.data(), sizeof(double), h[1], g); fwrite(order.data(), sizeof(uint32_t), h[1], g);
    fclose(g);
    return rc ? 1 : 0;
}
#endif
