// pick_mappings_driver.cpp — test infrastructure only: the serial composition of the device's rule for a long read's mappings
// (pick_mappings_device.hpp: pick_check_one, pick_stat_one, pick_alignment_one, pick_read_one on one lane — what the kernels call) behind one C call
// with vgk_pick_mappings' arguments less the context, so that it can be held to the host shim and to the tests' own statement without a GPU
// (tests/test_pick_mappings.py).  The call's checks, the mapping slots and the table sizes are the engine's own (pick_check_call, pick_node_bound,
// pick_slots_for).  With -DPICK_DRIVER_MAIN the same call as a program of its own, for a run under the host sanitizers: it reads one call from a
// file of 64-bit words and raw arrays (the test writes it) and writes the answer likewise.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../vg_amd/csrc/pick_mappings_device.hpp"

using namespace vgk;

extern "C" int vgt_pick_mappings_serial(const vgk_pick_scheme* scheme, uint32_t n_reads, const char* reads, const uint64_t* read_off, uint32_t* rng_state,
                                        const uint64_t* chain_off, const vgk_pick_chain* chains, const uint64_t* aln_off, const vgk_pick_alignment* alns,
                                        const vgk_chain_mapping* mappings, size_t n_mappings, const uint32_t* edits, size_t n_edits,
                                        vgk_pick_result* results, vgk_pick_verdict* verdicts, uint32_t* picked, int32_t* scores, double* multiplicity, size_t cap,
                                        size_t* written) {
    if (written) *written = 0;
    const int rc = pick_check_call(scheme, n_reads, reads, read_off, rng_state, chain_off, aln_off, n_mappings, n_edits);
    if (rc || !n_reads) return rc;
    const uint64_t n_chains = chain_off[n_reads], n_alns = aln_off[n_reads], room = n_alns + n_reads;
    if (written) *written = (size_t)room;
    if (room > cap) return VGK_EOPS;
    std::vector<uint64_t> slot_off((size_t)n_alns + 1, 0), node_bound(n_reads, 0); std::vector<uint32_t> counts;
    for (uint32_t r = 0; r < n_reads; ++r) {
        counts.clear();
        for (uint64_t i = aln_off[r]; i < aln_off[r + 1]; ++i) {
            const uint32_t m = pick_range_ok(alns[i].result, n_mappings) ? alns[i].result.n_mappings : 0u;
            slot_off[i + 1] = slot_off[i] + m; counts.push_back(m);
        }
        node_bound[r] = pick_node_bound(counts.data(), (uint32_t)counts.size(), scheme->max_multimaps);
    }
    const uint64_t n_slots = slot_off[n_alns];
    std::vector<unsigned long long> from_len(n_slots), sums(2 * n_alns, 0);                   // exactly their sizes: the sanitizer sees one too many
    std::vector<double> aln_mult(n_alns), aln_sort(n_alns);
    std::vector<vgk_pick_result> res(n_reads, vgk_pick_result{}); std::vector<vgk_pick_verdict> vd(n_alns, vgk_pick_verdict{});
    std::vector<uint32_t> out_picked(room, 0); std::vector<int32_t> out_scores(room, 0); std::vector<double> out_mult(room, 0.0);
    PickParams P{};
    P.sch = *scheme; P.n_reads = n_reads; P.n_alns = (uint32_t)n_alns; P.n_chains = (uint32_t)n_chains; P.n_slots = (uint32_t)n_slots; P.n_mappings = n_mappings; P.n_edits = n_edits;
    P.reads = reads; P.read_off = read_off; P.rng_state = rng_state; P.chain_off = chain_off; P.chains = chains; P.aln_off = aln_off; P.alns = alns; P.mappings = mappings; P.edits = edits;
    P.slot_off = slot_off.data(); P.from_len = from_len.data(); P.sums = sums.data(); P.aln_mult = aln_mult.data(); P.aln_sort = aln_sort.data(); P.res = res.data();
    P.verdicts = vd.data(); P.picked = out_picked.data(); P.scores = out_scores.data(); P.out_mult = out_mult.data();
    for (uint64_t i = 0; i < n_alns + n_chains; ++i) pick_check_one(P, i);
    for (uint32_t s = 0; s < n_slots; ++s) { uint32_t aln; unsigned long long share[2]; pick_stat_one(P, s, &aln, share); sums[2 * (size_t)aln] += share[0]; sums[2 * (size_t)aln + 1] += share[1]; }
    for (uint32_t i = 0; i < n_alns; ++i) pick_alignment_one(P, i);
    for (uint32_t r = 0; r < n_reads; ++r) {
        const uint64_t A = aln_off[r + 1] - aln_off[r];
        const uint32_t slots = A > FN_LDS_ITEMS || node_bound[r] > PICK_LDS_NODES ? pick_slots_for(node_bound[r]) : PICK_LDS_SLOTS;
        std::vector<uint32_t> order(A), table(slots);
        pick_read_one(P, r, order.data(), table.data(), slots, PickOneLane());
    }
    for (uint32_t r = 0; r < n_reads; ++r) results[r] = res[r];
    for (uint64_t i = 0; i < n_alns; ++i) verdicts[i] = vd[i];
    for (uint64_t i = 0; i < room; ++i) { picked[i] = out_picked[i]; scores[i] = out_scores[i]; multiplicity[i] = out_mult[i]; }
    return VGK_OK;
}

#ifdef PICK_DRIVER_MAIN
// in:  8 words (n reads, chains, alignments, mappings, edit runs, read bytes — the arrays' own sizes: a malformed call's offsets say nothing —, 1 when the
//      reads have generators, cap), the 16-byte scheme, then read_off, reads, rng_state (when given), chain_off, chains, aln_off, alns, mappings, edits
// out: 2 words (rc, written), then — when rc is VGK_OK — results, verdicts, picked, scores, multiplicity (`written` each), rng_state (when given)
template <class T> static bool get(FILE* f, std::vector<T>& v, uint64_t n) { v.assign(n, T{}); return !n || fread(v.data(), sizeof(T), n, f) == n; }
int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s call.bin answer.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    uint64_t h[8]; vgk_pick_scheme scheme;
    if (!f || fread(h, 8, 8, f) != 8 || fread(&scheme, sizeof scheme, 1, f) != 1) return 2;
    const uint32_t n_reads = (uint32_t)h[0];
    std::vector<uint64_t> roff, coff, aoff; std::vector<char> reads; std::vector<uint32_t> rng, edits; std::vector<vgk_pick_chain> chains; std::vector<vgk_pick_alignment> alns;
    std::vector<vgk_chain_mapping> mappings;
    if (!get(f, roff, (uint64_t)n_reads + 1) || !get(f, reads, h[5]) || !get(f, rng, h[6] ? n_reads : 0) || !get(f, coff, (uint64_t)n_reads + 1) || !get(f, chains, h[1])
        || !get(f, aoff, (uint64_t)n_reads + 1) || !get(f, alns, h[2]) || !get(f, mappings, h[3]) || !get(f, edits, h[4])) return 2;
    fclose(f);
    std::vector<vgk_pick_result> results(n_reads); std::vector<vgk_pick_verdict> verdicts(h[2]); std::vector<uint32_t> picked(h[7]); std::vector<int32_t> scores(h[7]);
    std::vector<double> mult(h[7]);
    size_t written = 0;
    const int rc = vgt_pick_mappings_serial(&scheme, n_reads, h[6] ? reads.data() : nullptr, roff.data(), h[6] ? rng.data() : nullptr, coff.data(), chains.data(), aoff.data(),
                                            alns.data(), mappings.data(), mappings.size(), edits.data(), edits.size(), results.data(), verdicts.data(), picked.data(), scores.data(),
                                            mult.data(), h[7], &written);
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    const uint64_t o[2] = {(uint64_t)(int64_t)rc, written};
    fwrite(o, 8, 2, g);
    auto put = [&](const void* p, size_t size, size_t n) { if (n) fwrite(p, size, n, g); };
    if (rc == VGK_OK) {
        put(results.data(), sizeof(vgk_pick_result), n_reads); put(verdicts.data(), sizeof(vgk_pick_verdict), verdicts.size()); put(picked.data(), 4, written); put(scores.data(), 4, written);
        put(mult.data(), 8, written); put(rng.data(), 4, rng.size());
    }
    fclose(g);
    return rc ? 1 : 0;
}
#endif
