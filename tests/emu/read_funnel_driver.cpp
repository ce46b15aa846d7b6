// read_funnel_driver.cpp — test infrastructure only: the serial statements of the device's rules for a short read's funnel (read_funnel_device.hpp:
// rf_cluster_score_one, rf_clusters_one, rf_set_estimate_one, rf_sets_one, rf_winners_one, rf_gather_one — what the kernels call) behind one C call
// each, with vgk_funnel_*'s arguments less the context (the sets' call takes the gap penalties instead), so that they can be held to the host shim
// and to a statement in another shape without a GPU (tests/test_read_funnel.py).  The checks are the engine's own.  Every item gets exactly its
// working words.  With -DFN_DRIVER_MAIN the same calls as a program of its own, for a run under the host sanitizers: it reads one call from a file
// of framed arrays (the test writes it), sizes it with capacity 0, runs it again with exactly the capacity asked for, and writes the answers likewise.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../vg_amd/csrc/read_funnel_device.hpp"

using namespace vgk;

namespace {
// the walk of every read, then counts -> prefix sums -> the gather, as the engine lays a walk's accepted items out
template <class Words> void walk_all(FnParams& P, int what, uint32_t n, Words words) {
    P.what = what;
    for (uint32_t r = 0; r < n; ++r) { std::vector<uint32_t> order(words(r)); rf_item_one(P, r, order.data()); }
}
int lay_out(FnParams& P, uint32_t n, const uint64_t* src_off, const uint32_t* src, uint32_t words, uint64_t* off, uint32_t* dst, size_t cap, size_t* written, bool size_only) {
    std::vector<uint32_t> first((size_t)n + 1, 0);
    for (uint32_t r = 0; r < n; ++r) first[r + 1] = first[r] + P.count[r];
    for (uint32_t r = 0; r <= n; ++r) off[r] = first[r];
    if (written) written[0] = first[n];
    if (first[n] > cap) return VGK_EOPS;
    if (size_only) return VGK_OK;
    P.src_off = src_off; P.first = first.data(); P.src = src; P.dst = dst; P.gather_words = words;
    for (uint32_t r = 0; r < n; ++r) rf_gather_one(P, r);
    return VGK_OK;
}
}  // namespace

extern "C" int vgt_funnel_clusters_serial(const vgk_funnel_policy* policy, uint32_t n, const char* reads, const uint64_t* read_off, const uint64_t* minimizer_off,
                                          const vgk_read_minimizer* minimizers, const double* minimizer_score, const uint64_t* cluster_off, const uint64_t* cluster_seed_off,
                                          const uint32_t* sources, uint32_t* rng_state, vgk_funnel_cluster* clusters, int32_t* status, uint64_t* kept_off, uint32_t* kept,
                                          size_t kept_cap, size_t* written) {
    const int rc = rf_check_clusters_call(policy, n, reads, read_off, minimizer_off, cluster_off, cluster_seed_off, rng_state);
    if (kept_off) kept_off[0] = 0;
    if (written) written[0] = 0;
    if (rc || !n) return rc;
    const uint64_t n_clusters = cluster_off[n];
    FnParams P{};
    P.pol = *policy; P.n_reads = n; P.reads = reads; P.read_off = read_off; P.rng_state = rng_state; P.status = status; P.min_off = minimizer_off; P.mins = minimizers;
    P.min_score = minimizer_score; P.cluster_off = cluster_off; P.cluster_seed_off = cluster_seed_off; P.sources = sources; P.clusters = clusters;
    std::vector<uint32_t> tmp(n_clusters), count(n);
    P.tmp = tmp.data(); P.count = count.data();
    for (uint32_t r = 0; r < n; ++r) status[r] = rf_validate_clusters_read(P, r);
    P.what = FN_RUN_CLUSTER_SCORE;
    for (uint32_t r = 0; r < n; ++r) for (uint64_t c = cluster_off[r]; c < cluster_off[r + 1]; ++c) {
        std::vector<uint32_t> work(fn_cluster_words(minimizer_off[r + 1] - minimizer_off[r], read_off[r + 1] - read_off[r]));
        rf_item_one(P, (uint32_t)c, work.data());
    }
    walk_all(P, FN_RUN_CLUSTER_WALK, n, [&](uint32_t r) { return cluster_off[r + 1] - cluster_off[r]; });
    return lay_out(P, n, cluster_off, tmp.data(), 1, kept_off, kept, kept_cap, written, false);
}

extern "C" int vgt_funnel_extension_sets_serial(const vgk_funnel_policy* policy, int32_t gap_open, int32_t gap_extend, uint32_t n, const char* reads, const uint64_t* read_off,
                                                const uint64_t* set_off, const vgk_gapless_result* results, const vgk_extension* extensions, size_t n_extensions,
                                                const uint64_t* kept_off, const uint32_t* kept, const uint64_t* cluster_seed_off, size_t n_clusters, const uint32_t* sources,
                                                const uint64_t* minimizer_off, uint32_t* rng_state, vgk_funnel_set* sets, int32_t* status, uint64_t* aligned_off,
                                                uint32_t* aligned, size_t aligned_cap, uint8_t* explored, size_t* written) {
    const int rc = rf_check_sets_call(policy, n, reads, read_off, set_off, kept_off, cluster_seed_off, n_clusters, n_extensions, minimizer_off, rng_state);
    if (aligned_off) aligned_off[0] = 0;
    if (written) written[0] = 0;
    if (rc || !n) return rc;
    FnParams P{};
    P.pol = *policy; P.gap_open = gap_open; P.gap_extend = gap_extend; P.n_reads = n; P.reads = reads; P.read_off = read_off; P.rng_state = rng_state; P.status = status;
    P.min_off = minimizer_off; P.cluster_seed_off = cluster_seed_off; P.sources = sources; P.kept_off = kept_off; P.kept = kept; P.res = results; P.ext = extensions;
    P.sets = sets; P.explored = explored;
    std::vector<uint32_t> tmp(kept_off[n]), count(n);
    P.tmp = tmp.data(); P.count = count.data();
    for (uint32_t r = 0; r < n; ++r) status[r] = rf_validate_sets_read(P, r, n_extensions, n_clusters);
    P.what = FN_RUN_SET_ESTIMATE;
    for (uint32_t r = 0; r < n; ++r) for (uint64_t s = kept_off[r]; s < kept_off[r + 1]; ++s) {
        std::vector<uint32_t> work(status[r] == VGK_OK && results[s].status == VGK_OK ? results[s].n_ext : 0);
        rf_item_one(P, (uint32_t)s, work.data());
    }
    walk_all(P, FN_RUN_SET_WALK, n, [&](uint32_t r) { return kept_off[r + 1] - kept_off[r]; });
    return lay_out(P, n, kept_off, tmp.data(), 1, aligned_off, aligned, aligned_cap, written, false);
}

extern "C" int vgt_funnel_winners_serial(const vgk_funnel_policy* policy, uint32_t n, const char* reads, const uint64_t* read_off, const uint64_t* aligned_off,
                                         const uint64_t* aln_off, const int32_t* aln_score, const uint32_t* aln_mappings, uint32_t* rng_state, uint64_t* score_off,
                                         int32_t* scores, vgk_funnel_pick* reported, size_t score_cap, uint32_t* n_reported, uint8_t* unmapped, size_t* written) {
    const int rc = rf_check_winners_call(policy, n, reads, read_off, aligned_off, aln_off, rng_state);
    if (score_off) score_off[0] = 0;
    if (written) written[0] = 0;
    if (rc || !n) return rc;
    std::vector<uint64_t> flat_off((size_t)n + 1, 0);
    for (uint32_t r = 0; r < n; ++r) flat_off[r + 1] = flat_off[r] + rf_winner_bound(aligned_off, aln_off, r);
    std::vector<int32_t> flat_score(flat_off[n]), sorted_score(flat_off[n]); std::vector<vgk_funnel_pick> flat_pick(flat_off[n]), sorted_pick(flat_off[n]);
    std::vector<uint32_t> count(n);
    FnParams P{};
    P.pol = *policy; P.n_reads = n; P.reads = reads; P.read_off = read_off; P.rng_state = rng_state; P.aligned_off = aligned_off; P.aln_off = aln_off; P.aln_score = aln_score;
    P.aln_mappings = aln_mappings; P.flat_off = flat_off.data(); P.flat_score = flat_score.data(); P.flat_pick = flat_pick.data(); P.sorted_score = sorted_score.data();
    P.sorted_pick = sorted_pick.data(); P.n_reported = n_reported; P.unmapped = unmapped; P.count = count.data();
    walk_all(P, FN_RUN_WINNER_WALK, n, [&](uint32_t r) { return flat_off[r + 1] - flat_off[r]; });
    int ro = lay_out(P, n, flat_off.data(), (const uint32_t*)sorted_score.data(), 1, score_off, (uint32_t*)scores, score_cap, written, false);
    if (!ro) ro = lay_out(P, n, flat_off.data(), (const uint32_t*)sorted_pick.data(), 2, score_off, (uint32_t*)reported, score_cap, written, false);
    return ro;
}

#ifdef FN_DRIVER_MAIN
// in:  two words (which call: 0 clusters, 1 sets, 2 winners; the number of arrays), then per array two words (present, bytes) and the bytes, padded to
//      8.  Array 0 is the policy, array 1 the call's scalars as 64-bit words, the others the call's input arrays in argument order (absent = NULL).
// out: the same framing: array 0 = {rc of the sizing call, rc, written[0]} as 64-bit words, then the outputs in argument order and the generator states
struct Arr { bool present = false; std::vector<char> bytes; template <class T> T* as() { return present ? (T*)bytes.data() : nullptr; } size_t size() const { return bytes.size(); } };
static void put(FILE* g, const void* p, size_t bytes) {
    const uint64_t h[2] = {1, bytes}; static const char zero[8] = {0};
    fwrite(h, 8, 2, g); if (bytes) fwrite(p, 1, bytes, g); if (bytes % 8) fwrite(zero, 1, 8 - bytes % 8, g);
}
template <class T> static std::vector<T> exactly(size_t n) { return std::vector<T>(n); }
int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s call.bin answer.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    uint64_t h[2];
    if (!f || fread(h, 8, 2, f) != 2 || h[1] > 64) return 2;
    std::vector<Arr> a(h[1]);
    for (Arr& x : a) {
        uint64_t q[2];
        if (fread(q, 8, 2, f) != 2) return 2;
        x.present = q[0] != 0; x.bytes.resize(q[1]);
        if (q[1] && fread(x.bytes.data(), 1, q[1], f) != q[1]) return 2;
        char pad[8]; if (q[1] % 8 && fread(pad, 1, 8 - q[1] % 8, f) != 8 - q[1] % 8) return 2;
    }
    fclose(f);
    FILE* g = fopen(argv[2], "wb");
    if (!g || a.size() < 2 || a[0].size() != sizeof(vgk_funnel_policy)) return 2;
    const vgk_funnel_policy* pol = a[0].as<vgk_funnel_policy>(); const uint64_t* sc = a[1].as<uint64_t>();
    const uint32_t n = (uint32_t)sc[0];
    size_t written[1] = {0}; int rc0 = 0, rc = 0;
    std::vector<uint32_t> state0, state;
    if (h[0] == 0 && a.size() == 11) {
        if (a[10].present) state0.assign(a[10].as<uint32_t>(), a[10].as<uint32_t>() + n);
        state = state0;
        const uint64_t n_clusters = a[7].present && a[7].size() >= 8 * ((size_t)n + 1) ? a[7].as<uint64_t>()[n] : 0;
        auto clusters = exactly<vgk_funnel_cluster>(n_clusters); auto status = exactly<int32_t>(n); auto kept_off = exactly<uint64_t>((size_t)n + 1);
        auto call = [&](uint32_t* kept, size_t cap) {
            return vgt_funnel_clusters_serial(pol, n, a[2].as<char>(), a[3].as<uint64_t>(), a[4].as<uint64_t>(), a[5].as<vgk_read_minimizer>(), a[6].as<double>(), a[7].as<uint64_t>(),
                                              a[8].as<uint64_t>(), a[9].as<uint32_t>(), a[10].present ? state.data() : nullptr, clusters.data(), status.data(), kept_off.data(), kept, cap, written);
        };
        rc0 = call(nullptr, 0);
        auto kept = exactly<uint32_t>(written[0]);
        state = state0; rc = call(kept.data(), kept.size());
        const uint64_t o[3] = {(uint64_t)(int64_t)rc0, (uint64_t)(int64_t)rc, written[0]};
        const uint64_t count[2] = {6, 6}; fwrite(count, 8, 2, g);
        put(g, o, sizeof o); put(g, clusters.data(), clusters.size() * sizeof(vgk_funnel_cluster)); put(g, status.data(), 4 * status.size()); put(g, kept_off.data(), 8 * kept_off.size());
        put(g, kept.data(), 4 * kept.size()); put(g, state.data(), 4 * state.size());
    } else if (h[0] == 1 && a.size() == 13) {
        // scalars: n, gap open, gap extend, extensions, clusters, minimizers
        if (a[12].present) state0.assign(a[12].as<uint32_t>(), a[12].as<uint32_t>() + n);
        state = state0;
        const uint64_t n_sets = a[4].present && a[4].size() >= 8 * ((size_t)n + 1) ? a[4].as<uint64_t>()[n] : 0;
        auto sets = exactly<vgk_funnel_set>(n_sets); auto status = exactly<int32_t>(n); auto aligned_off = exactly<uint64_t>((size_t)n + 1); auto explored = exactly<uint8_t>(sc[5]);
        auto call = [&](uint32_t* aligned, size_t cap) {
            return vgt_funnel_extension_sets_serial(pol, (int32_t)sc[1], (int32_t)sc[2], n, a[2].as<char>(), a[3].as<uint64_t>(), a[4].as<uint64_t>(), a[5].as<vgk_gapless_result>(),
                                                    a[6].as<vgk_extension>(), sc[3], a[7].as<uint64_t>(), a[8].as<uint32_t>(), a[9].as<uint64_t>(), sc[4], a[10].as<uint32_t>(),
                                                    a[11].as<uint64_t>(), a[12].present ? state.data() : nullptr, sets.data(), status.data(), aligned_off.data(), aligned, cap,
                                                    explored.data(), written);
        };
        rc0 = call(nullptr, 0);
        auto aligned = exactly<uint32_t>(written[0]);
        state = state0; rc = call(aligned.data(), aligned.size());
        const uint64_t o[3] = {(uint64_t)(int64_t)rc0, (uint64_t)(int64_t)rc, written[0]};
        const uint64_t count[2] = {7, 7}; fwrite(count, 8, 2, g);
        put(g, o, sizeof o); put(g, sets.data(), sets.size() * sizeof(vgk_funnel_set)); put(g, status.data(), 4 * status.size()); put(g, aligned_off.data(), 8 * aligned_off.size());
        put(g, aligned.data(), 4 * aligned.size()); put(g, explored.data(), explored.size()); put(g, state.data(), 4 * state.size());
    } else if (h[0] == 2 && a.size() == 9) {
        if (a[8].present) state0.assign(a[8].as<uint32_t>(), a[8].as<uint32_t>() + n);
        state = state0;
        auto score_off = exactly<uint64_t>((size_t)n + 1); auto n_reported = exactly<uint32_t>(n); auto unmapped = exactly<uint8_t>(n);
        auto call = [&](int32_t* scores, vgk_funnel_pick* reported, size_t cap) {
            return vgt_funnel_winners_serial(pol, n, a[2].as<char>(), a[3].as<uint64_t>(), a[4].as<uint64_t>(), a[5].as<uint64_t>(), a[6].as<int32_t>(), a[7].as<uint32_t>(),
                                             a[8].present ? state.data() : nullptr, score_off.data(), scores, reported, cap, n_reported.data(), unmapped.data(), written);
        };
        rc0 = call(nullptr, nullptr, 0);
        auto scores = exactly<int32_t>(written[0]); auto reported = exactly<vgk_funnel_pick>(written[0]);
        state = state0; rc = call(scores.data(), reported.data(), scores.size());
        const uint64_t o[3] = {(uint64_t)(int64_t)rc0, (uint64_t)(int64_t)rc, written[0]};
        const uint64_t count[2] = {7, 7}; fwrite(count, 8, 2, g);
        put(g, o, sizeof o); put(g, score_off.data(), 8 * score_off.size()); put(g, scores.data(), 4 * scores.size()); put(g, reported.data(), 8 * reported.size());
        put(g, n_reported.data(), 4 * n_reported.size()); put(g, unmapped.data(), unmapped.size()); put(g, state.data(), 4 * state.size());
    } else return 2;
    fclose(g);
    return 0;
}
#endif
