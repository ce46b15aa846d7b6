// chain_links_driver.cpp — test infrastructure only: the serial composition of the device's rule for a chain's links (chain_links_device.hpp:
// cl_check_one, cl_walk_one, cl_count_one, cl_write_one — what the kernels call) behind one C call with vgk_chain_links' arguments less the context,
// so that it can be held to the host shim and to the tests' own statement without a GPU (tests/test_chain_links.py).  The call's checks and bounds
// are the engine's own (cl_plan_call).  With -DCL_DRIVER_MAIN the same call as a program of its own, for a run under the host sanitizers: it reads
// one call from a file of 64-bit words and raw arrays (the test writes it) and writes the answer likewise.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../vg_amd/csrc/chain_links_device.hpp"

using namespace vgk;

extern "C" int vgt_chain_links_serial(const vgk_chain_links_scheme* scheme, uint32_t n_reads, const char* reads, const uint64_t* read_off,
                                      uint32_t n_sets, const uint64_t* anchor_off, const vgk_chain_anchor* anchors, const vgk_chain_site* sites,
                                      const uint32_t* items, size_t n_items, const uint64_t* dist_off, const vgk_chain_candidate* dist,
                                      uint32_t n_chains, const vgk_chain_problem* chains,
                                      vgk_chain_links_result* results, vgk_chain_link* links, size_t link_cap, uint32_t* kept, size_t kept_cap,
                                      char* seqs, uint64_t* seq_off, size_t seq_cap, size_t written[3]) {
    if (written) written[0] = written[1] = written[2] = 0;
    if (!scheme) return VGK_EINVAL;
    if (!n_chains) return VGK_OK;
    std::vector<uint32_t> slot_off((size_t)n_chains + 1);
    std::vector<int32_t> status(n_chains);
    uint64_t bound[3];
    const int rc = cl_plan_call(n_reads, read_off, n_sets, anchor_off, n_items, dist_off, n_chains, chains, 0xfffffff0ull, slot_off.data(), status.data(), bound);
    if (rc) return rc;
    ClParams P{};
    P.sch = *scheme; P.n_reads = n_reads; P.n_sets = n_sets; P.n_chains = n_chains; P.n_slots = slot_off[n_chains]; P.n_dist = dist_off[n_sets];
    P.reads = reads; P.read_off = read_off; P.anchor_off = anchor_off; P.anchors = anchors; P.sites = sites; P.items = items; P.dist_off = dist_off; P.dist = dist;
    P.chains = chains; P.slot_off = slot_off.data();
    const uint32_t LS = cl_link_slots(P); const size_t LS1 = (size_t)LS + 1;
    std::vector<uint8_t> set_bad(n_sets, 0), keep(P.n_slots, 0), route(LS, 0);                // exactly their sizes: the sanitizer sees one too many
    std::vector<uint32_t> cnt(3 * LS1, 0), first(3 * LS1, 0);
    std::vector<vgk_chain_links_result> res(n_chains, vgk_chain_links_result{});
    for (uint32_t c = 0; c < n_chains; ++c) res[c].status = status[c];
    unsigned long long totals[3] = {0, 0, 0};
    P.set_bad = set_bad.data(); P.keep = keep.data(); P.route = route.data(); P.cnt = cnt.data(); P.first = first.data(); P.totals = totals; P.res = res.data();
    for (uint64_t i = 0; i < P.n_slots + P.n_dist; ++i) cl_check_one(P, i);
    for (uint32_t c = 0; c < n_chains; ++c) cl_walk_one(P, c);
    for (uint32_t ls = 0; ls < LS; ++ls) { uint32_t out[3]; cl_count_one(P, ls, out); for (int k = 0; k < 3; ++k) totals[k] += out[k]; }
    if (written) for (int k = 0; k < 3; ++k) written[k] = (size_t)totals[k];
    if (totals[0] > link_cap || totals[1] > kept_cap || (seqs && totals[2] > seq_cap)) return VGK_EOPS;
    for (int k = 0; k < 3; ++k) { uint32_t s = 0; for (size_t i = 0; i < LS1; ++i) { first[k * LS1 + i] = s; s += cnt[k * LS1 + i]; } }
    std::vector<vgk_chain_link> out_links(totals[0]); std::vector<uint32_t> out_kept(totals[1]); std::vector<uint64_t> out_seq_off(totals[0] + 1);
    P.links = out_links.data(); P.kept = out_kept.data(); P.seq_off = seqs ? out_seq_off.data() : nullptr; P.n_links = (uint32_t)totals[0];
    for (uint32_t ls = 0; ls < LS; ++ls) { uint32_t c = 0; const int64_t share = cl_write_one(P, ls, &c); res[c].anchor_score += share; }
    for (uint32_t c = 0; c < n_chains; ++c) results[c] = res[c];
    for (size_t i = 0; i < out_links.size(); ++i) links[i] = out_links[i];
    for (size_t i = 0; i < out_kept.size(); ++i) kept[i] = out_kept[i];
    if (seqs) {
        for (size_t i = 0; i <= out_links.size(); ++i) seq_off[i] = out_seq_off[i];
        for (size_t i = 0; i < out_links.size(); ++i) {
            const vgk_chain_link& L = out_links[i];
            std::memcpy(seqs + seq_off[i], reads + read_off[chains[L.chain].read] + L.read_begin, L.length);
        }
    }
    return VGK_OK;
}

#ifdef CL_DRIVER_MAIN
// in:  10 words (n reads, n sets, n items, n chains, link cap, kept cap, seq cap, read bytes, anchors, distances — the arrays' own sizes: a malformed
//      call's offsets say nothing), the 64-byte scheme, then read_off, reads, anchor_off, anchors, sites,
//      items, dist_off, dist, chains — an absent array is empty
// out: 4 words (rc, written[0..2]), then results, links, kept, seq_off (links + 1), seqs — each as long as the call wrote it
template <class T> static bool get(FILE* f, std::vector<T>& v, uint64_t n) { v.assign(n, T{}); return !n || fread(v.data(), sizeof(T), n, f) == n; }
int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s call.bin answer.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    uint64_t h[10]; vgk_chain_links_scheme scheme;
    if (!f || fread(h, 8, 10, f) != 10 || fread(&scheme, sizeof scheme, 1, f) != 1) return 2;
    const uint32_t n_reads = (uint32_t)h[0], n_sets = (uint32_t)h[1], n_chains = (uint32_t)h[3];
    std::vector<uint64_t> roff, aoff, doff; std::vector<char> reads; std::vector<vgk_chain_anchor> anchors; std::vector<vgk_chain_site> sites; std::vector<uint32_t> items;
    std::vector<vgk_chain_candidate> dist; std::vector<vgk_chain_problem> chains;
    if (!get(f, roff, (uint64_t)n_reads + 1) || !get(f, reads, h[7]) || !get(f, aoff, (uint64_t)n_sets + 1) || !get(f, anchors, h[8]) || !get(f, sites, h[8])
        || !get(f, items, h[2]) || !get(f, doff, (uint64_t)n_sets + 1) || !get(f, dist, h[9]) || !get(f, chains, n_chains)) return 2;
    fclose(f);
    std::vector<vgk_chain_links_result> results(n_chains); std::vector<vgk_chain_link> links(h[4]); std::vector<uint32_t> kept(h[5]); std::vector<uint64_t> seq_off(h[4] + 1);
    std::vector<char> seqs(h[6] + 1);                                  // (never a null pointer: NULL means "no sequences wanted")
    size_t written[3];
    const int rc = vgt_chain_links_serial(&scheme, n_reads, reads.data(), roff.data(), n_sets, aoff.data(), anchors.data(), sites.data(), items.data(), items.size(), doff.data(),
                                          dist.data(), n_chains, chains.data(), results.data(), links.data(), links.size(), kept.data(), kept.size(), seqs.data(), seq_off.data(),
                                          h[6], written);
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    const uint64_t o[4] = {(uint64_t)(int64_t)rc, written[0], written[1], written[2]};
    fwrite(o, 8, 4, g);
    auto put = [&](const void* p, size_t size, size_t n) { if (n) fwrite(p, size, n, g); };
    if (rc == VGK_OK) {
        put(results.data(), sizeof(vgk_chain_links_result), n_chains); put(links.data(), sizeof(vgk_chain_link), written[0]); put(kept.data(), 4, written[1]);
        put(seq_off.data(), 8, written[0] + 1); put(seqs.data(), 1, written[2]);
    }
    fclose(g);
    return rc ? 1 : 0;
}
#endif
