// read_mapq_driver.cpp — test infrastructure only: the serial statements of the device's rules for a read's mapping quality
// (read_mapq_device.hpp: mq_region_one, mq_read_one — what the kernels call) behind one C call each, with vgk_minimizer_regions' / vgk_read_mapq's
// arguments less the context, so that they can be held to the host shim and to a brute-force statement without a GPU (tests/test_read_mapq.py).  The
// checks are the engine's own (mq_validate_read).  With -DMQ_DRIVER_MAIN the same calls as a program of its own, for a run under the host sanitizers:
// it reads one call of each from a file of 64-bit words and raw arrays (the test writes it) and writes the answers likewise.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../vg_amd/csrc/read_mapq_device.hpp"

using namespace vgk;

extern "C" int vgt_minimizer_regions_serial(uint32_t k, uint32_t w, const uint64_t* read_off, uint32_t n, const uint64_t* minimizer_off,
                                            const vgk_read_minimizer* minimizers, vgk_minimizer_region* regions) {
    if (!k || k > MZ_MAX_K || !w || w > MZ_MAX_W) return VGK_EINVAL;
    if (!n) return VGK_OK;
    if (read_off[0] != 0 || minimizer_off[0] != 0) return VGK_EINVAL;
    for (uint32_t r = 0; r < n; ++r) {
        if (read_off[r + 1] < read_off[r] || minimizer_off[r + 1] < minimizer_off[r]) return VGK_EINVAL;
        const uint64_t L = read_off[r + 1] - read_off[r];
        if (minimizer_off[r + 1] > minimizer_off[r] && L + 1 < (uint64_t)k + w) return VGK_EINVAL;
        for (uint64_t j = minimizer_off[r]; j < minimizer_off[r + 1]; ++j) {
            if ((uint64_t)minimizers[j].offset + k > L) return VGK_EINVAL;
            if (j > minimizer_off[r] && minimizers[j].offset < minimizers[j - 1].offset) return VGK_EINVAL;
        }
    }
    MqRegionParams P{};
    P.k = k; P.w = w; P.n_reads = n; P.n_minimizers = minimizer_off[n]; P.read_off = read_off; P.min_off = minimizer_off; P.mins = minimizers; P.out = regions;
    for (uint64_t j = 0; j < P.n_minimizers; ++j) mq_region_one(P, j);
    return VGK_OK;
}

extern "C" int vgt_read_mapq_serial(const vgk_read_mapq_scheme* scheme, uint32_t n, const uint64_t* score_off, const int32_t* scores, const double* multiplicity,
                                    const uint8_t* unmapped, const uint64_t* minimizer_off, const vgk_read_minimizer* minimizers, const vgk_minimizer_region* regions,
                                    const uint8_t* explored, const uint64_t* read_off, const uint8_t* quality, vgk_read_mapq_result* out) {
    if (!scheme || (scheme->flags & ~7u) || !(scheme->log_base > 0.0) || !(scheme->score_scale > 0.0) || std::isinf(scheme->log_base) || std::isinf(scheme->score_scale)) return VGK_EINVAL;
    if (!n) return VGK_OK;
    if (score_off[0] != 0 || minimizer_off[0] != 0 || read_off[0] != 0) return VGK_EINVAL;
    for (uint32_t r = 0; r < n; ++r) {
        if (score_off[r + 1] < score_off[r] || minimizer_off[r + 1] < minimizer_off[r] || read_off[r + 1] < read_off[r]) return VGK_EINVAL;
        if (minimizer_off[r + 1] - minimizer_off[r] >= MQ_MAX_READ_MINIMIZERS) return VGK_ETOOBIG;
    }
    std::vector<double> phred(MQ_PHRED_ENTRIES), events(MQ_EVENT_ENTRIES);
    read_mapq_tables(phred.data(), events.data());
    MqParams P{};
    P.log_base = scheme->log_base; P.score_scale = scheme->score_scale; P.quality_scale = 10.0 / std::log(10.0);
    P.score_window = scheme->score_window; P.k = scheme->k; P.flags = scheme->flags; P.n_reads = n;
    P.score_off = score_off; P.scores = scores; P.mult = multiplicity; P.unmapped = unmapped; P.min_off = minimizer_off; P.mins = minimizers; P.regions = regions;
    P.explored = explored; P.read_off = read_off; P.qual = quality; P.phred = phred.data(); P.events = events.data(); P.out = out;
    std::vector<int32_t> status(n);
    P.status = status.data();
    const bool sweep = quality && !(scheme->flags & VGK_READ_MAPQ_NO_EXPLORED_CAP);
    for (uint32_t r = 0; r < n; ++r) {
        status[r] = mq_validate_read(P, r);
        std::vector<uint32_t> work(mq_work_words(status[r] == VGK_OK && sweep ? mq_count_explored(P, r) : 0));      // exactly its words: the sanitizer sees one too many
        mq_read_one(P, r, work.data());
    }
    return VGK_OK;
}

#ifdef MQ_DRIVER_MAIN
// in:  12 words (k, w, n reads, scores, minimizers, bases, flags, score window, scheme k, has multiplicities, has unmapped, has qualities), 2 doubles (log base,
//      score scale), then read_off, score_off, minimizer_off, scores, multiplicities, unmapped, minimizers, explored, the regions the mapping qualities take, qualities — an absent
//      array is empty
// out: 2 words (rc of the regions, rc of the mapping qualities), then the regions made here from the list and the 24-byte results
template <class T> static bool get(FILE* f, std::vector<T>& v, uint64_t n) { v.assign(n + 1, T{}); return !n || fread(v.data(), sizeof(T), n, f) == n; }
int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s call.bin answer.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    uint64_t h[12]; double d[2];
    if (!f || fread(h, 8, 12, f) != 12 || fread(d, 8, 2, f) != 2) return 2;
    const uint32_t n = (uint32_t)h[2];
    std::vector<uint64_t> roff, soff, moff; std::vector<int32_t> scores; std::vector<double> mult; std::vector<uint8_t> unmapped, explored, qual; std::vector<vgk_read_minimizer> mins; std::vector<vgk_minimizer_region> given;
    if (!get(f, roff, (uint64_t)n + 1) || !get(f, soff, (uint64_t)n + 1) || !get(f, moff, (uint64_t)n + 1) || !get(f, scores, h[3]) || !get(f, mult, h[9] ? h[3] : 0)
        || !get(f, unmapped, h[10] ? n : 0) || !get(f, mins, h[4]) || !get(f, explored, h[4]) || !get(f, given, h[4]) || !get(f, qual, h[11] ? h[5] : 0)) return 2;
    fclose(f);
    std::vector<vgk_minimizer_region> regions(h[4] + 1); std::vector<vgk_read_mapq_result> out((size_t)n + 1);
    const int rc_regions = vgt_minimizer_regions_serial((uint32_t)h[0], (uint32_t)h[1], roff.data(), n, moff.data(), mins.data(), regions.data());
    vgk_read_mapq_scheme scheme = {d[0], d[1], (uint32_t)h[7], (uint32_t)h[8], (uint32_t)h[6], 0u};
    const int rc_mapq = vgt_read_mapq_serial(&scheme, n, soff.data(), scores.data(), h[9] ? mult.data() : nullptr, h[10] ? unmapped.data() : nullptr,
                                           moff.data(), mins.data(), given.data(), explored.data(), roff.data(), h[11] ? qual.data() : nullptr, out.data());
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    const uint64_t o[2] = {(uint64_t)(int64_t)rc_regions, (uint64_t)(int64_t)rc_mapq};
    fwrite(o, 8, 2, g); fwrite(regions.data(), sizeof(vgk_minimizer_region), h[4], g); fwrite(out.data(), sizeof(vgk_read_mapq_result), n, g);
    fclose(g);
    return rc_mapq ? 1 : 0;                                        // (a list that is no read's list is the regions call's own answer)
}
#endif
