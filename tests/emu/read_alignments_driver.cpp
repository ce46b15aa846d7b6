// read_alignments_driver.cpp — test infrastructure only: the serial statement of the device's rule for a short read's alignments
// (read_alignments_device.hpp: ra_read_one, what the kernels are checked against) behind one C call with vgk_read_alignments' arguments — context and
// index replaced by the five scores and the oriented nodes' lengths and bases —, so that it can be held to an independent restatement without a GPU
// (tests/test_read_alignments.py).  The checks are the engine's own (ra_validate_read).  With -DRA_DRIVER_MAIN the same call as a program of its own,
// for a run under the host sanitizers: it reads one call from a file of 64-bit words and raw arrays (the test writes it) and writes the answer likewise.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../vg_amd/csrc/read_alignments_device.hpp"

using namespace vgk;

// scores: match, mismatch, gap open, gap extend, full-length bonus.  oriented_seq: the bases of oriented node 0, 1, ... behind each other
extern "C" int vgt_read_alignments_serial(const int32_t scores[5], const uint32_t* oriented_node_length, const char* oriented_seq, uint64_t n_oriented,
                                          const vgk_read_alignments_policy* policy, const char* reads, const uint64_t* read_off, uint32_t n, const vgk_gapless_result* results,
                                          const vgk_extension* extensions, size_t n_extensions, const uint32_t* nodes, size_t n_nodes, const uint32_t* mismatches, size_t n_mismatches,
                                          const vgk_tail_alignment* tails, size_t n_tails, const vgk_op* ops, size_t n_ops,
                                          uint64_t* aln_off, vgk_read_alignment* alignments, size_t cap_alignments,
                                          vgk_chain_mapping* mappings, size_t cap_mappings, uint32_t* edits, size_t cap_edits, size_t written[3]) {
    if (!policy || policy->flags || !policy->window_length) return VGK_EINVAL;
    aln_off[0] = 0;
    if (written) written[0] = written[1] = written[2] = 0;
    if (!n) return VGK_OK;
    if (read_off[0] != 0) return VGK_EINVAL;
    for (uint32_t r = 0; r < n; ++r) if (read_off[r + 1] < read_off[r]) return VGK_EINVAL;
    std::vector<uint64_t> node_tab(n_oriented + 1, 0);
    uint64_t at = 0;
    for (uint64_t o = 0; o < n_oriented; ++o) { node_tab[o] = (uint64_t)oriented_node_length[o] << 32 | at; at += oriented_node_length[o]; }
    std::vector<uint32_t> tail_of(2 * n_extensions + 2);
    if (!ra_tail_table(tails, n_tails, n_extensions, tail_of.data())) return VGK_EINVAL;
    RaParams P{};
    P.match = scores[0]; P.mismatch = scores[1]; P.gap_open = scores[2]; P.gap_extend = scores[3]; P.bonus = scores[4];
    P.threshold = policy->extension_score_threshold; P.max_local = policy->max_local_extensions; P.window_length = policy->window_length;
    P.n_reads = n; P.n_oriented = (uint32_t)n_oriented; P.node_tab = node_tab.data(); P.seq = oriented_seq; P.reads = reads; P.read_off = read_off;
    P.res = results; P.ext = extensions; P.nodes = nodes; P.mism = mismatches; P.tails = tails; P.ops = ops; P.tail_of = tail_of.data();
    std::vector<int32_t> status(n); std::vector<RaChoice> choice(n); std::vector<uint32_t> aln_count(n + 1, 0), aln_first(n + 1, 0);
    P.status = status.data(); P.choice = choice.data(); P.aln_count = aln_count.data(); P.aln_first = aln_first.data();
    for (uint32_t r = 0; r < n; ++r) {
        status[r] = ra_validate_read(P, r, n_extensions, n_nodes, n_mismatches, n_ops);
        std::vector<uint32_t> work(ra_work_words(status[r] == VGK_OK ? results[r].n_ext : 0));
        ra_read_one(P, RA_RUN_SELECT, r, work.data());
        aln_first[r + 1] = aln_first[r] + aln_count[r];
    }
    const uint32_t n_aln = aln_first[n];
    std::vector<uint32_t> map_count(n_aln + 1, 0), edit_count(n_aln + 1, 0), map_first(n_aln + 1, 0), edit_first(n_aln + 1, 0);
    P.map_count = map_count.data(); P.edit_count = edit_count.data(); P.map_first = map_first.data(); P.edit_first = edit_first.data();
    for (uint32_t r = 0; r < n; ++r) ra_read_one(P, RA_RUN_COUNT, r, nullptr);
    for (uint32_t a = 0; a < n_aln; ++a) { map_first[a + 1] = map_first[a] + map_count[a]; edit_first[a + 1] = edit_first[a] + edit_count[a]; }
    if (written) { written[0] = n_aln; written[1] = map_first[n_aln]; written[2] = edit_first[n_aln]; }
    if (n_aln > cap_alignments || map_first[n_aln] > cap_mappings || edit_first[n_aln] > cap_edits) return VGK_EOPS;
    P.out = alignments; P.mappings = mappings; P.edits = edits;
    for (uint32_t r = 0; r < n; ++r) ra_read_one(P, RA_RUN_EMIT, r, nullptr);
    for (uint32_t r = 0; r <= n; ++r) aln_off[r] = aln_first[r];
    return VGK_OK;
}

#ifdef RA_DRIVER_MAIN
// in:  16 words (match, mismatch, gap open, gap extend, bonus, n_oriented, bases, threshold, max extensions, window length, n reads, extensions, path
//      nodes, mismatches, tails, ops), then oriented lengths, bases, read_off, reads, results, extensions, nodes, mismatches, tails, ops
// out: 4 words (rc, alignments, mappings, edit runs), then aln_off, the headers, mappings and edit runs
template <class T> static bool get(FILE* f, std::vector<T>& v, uint64_t n) { v.assign(n + 1, T{}); return !n || fread(v.data(), sizeof(T), n, f) == n; }
int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s call.bin answer.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    uint64_t h[16];
    if (!f || fread(h, 8, 16, f) != 16) return 2;
    const uint32_t n = (uint32_t)h[10];
    std::vector<uint32_t> len, nodes, mism; std::vector<char> seq, reads; std::vector<uint64_t> roff; std::vector<vgk_gapless_result> res; std::vector<vgk_extension> ext;
    std::vector<vgk_tail_alignment> tails; std::vector<vgk_op> ops;
    if (!get(f, len, h[5]) || !get(f, seq, h[6]) || !get(f, roff, (uint64_t)n + 1)) return 2;
    if (!get(f, reads, roff[n]) || !get(f, res, n) || !get(f, ext, h[11]) || !get(f, nodes, h[12]) || !get(f, mism, h[13]) || !get(f, tails, h[14]) || !get(f, ops, h[15])) return 2;
    fclose(f);
    const int32_t scores[5] = {(int32_t)h[0], (int32_t)h[1], (int32_t)h[2], (int32_t)h[3], (int32_t)h[4]};
    const vgk_read_alignments_policy policy = {(uint32_t)h[7], (uint32_t)h[8], (uint32_t)h[9], 0u};
    std::vector<uint64_t> aoff((size_t)n + 1); std::vector<vgk_read_alignment> aln; std::vector<vgk_chain_mapping> maps; std::vector<uint32_t> edits;
    size_t written[3] = {0, 0, 0};
    int rc = VGK_EOPS;
    for (int pass = 0; pass < 2 && rc == VGK_EOPS; ++pass) {       // sized by the first pass, as a caller would
        aln.assign(written[0] + 1, vgk_read_alignment{}); maps.assign(written[1] + 1, vgk_chain_mapping{}); edits.assign(written[2] + 1, 0u);
        rc = vgt_read_alignments_serial(scores, len.data(), seq.data(), h[5], &policy, reads.data(), roff.data(), n, res.data(), ext.data(), h[11], nodes.data(), h[12],
                                        mism.data(), h[13], tails.data(), h[14], ops.data(), h[15], aoff.data(), aln.data(), written[0], maps.data(), written[1],
                                        edits.data(), written[2], written);
    }
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    const uint64_t o[4] = {(uint64_t)(int64_t)rc, written[0], written[1], written[2]};
    fwrite(o, 8, 4, g); fwrite(aoff.data(), 8, (size_t)n + 1, g);
    if (!rc) { fwrite(aln.data(), sizeof(vgk_read_alignment), written[0], g); fwrite(maps.data(), sizeof(vgk_chain_mapping), written[1], g); fwrite(edits.data(), 4, written[2], g); }
    fclose(g);
    return rc ? 1 : 0;
}
#endif
