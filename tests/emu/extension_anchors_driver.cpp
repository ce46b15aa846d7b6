// extension_anchors_driver.cpp — test infrastructure only: the serial statement of the device's rule for anchors from extensions
// (extension_anchors_device.hpp: ea_problem_one, what the kernels are checked against) behind one C call with vgk_extension_anchors' arguments — the
// index replaced by its oriented node lengths —, so that it can be held to the host shim's vgh_extension_anchors without a GPU
// (tests/test_extension_anchors.py).  Nothing is validated here beyond the seeds.  With -DEA_DRIVER_MAIN the same call as a program of its own, for a
// run under the host sanitizers: it reads one call from a file of 64-bit words and raw arrays (the test writes it) and writes the answer likewise.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../vg_amd/csrc/extension_anchors_device.hpp"

using namespace vgk;

extern "C" int vgt_extension_anchors_serial(const uint32_t* oriented_node_length, uint64_t n_oriented, int32_t match, int32_t mismatch, uint32_t flags, uint32_t default_max_extension_mismatches,
                                            uint32_t n_problems, const uint64_t* seed_off, const vgk_anchor_seed* seeds, const uint64_t* ext_off, const vgk_extension* extensions,
                                            const uint32_t* full_length, const uint32_t* nodes, size_t n_nodes, const uint32_t* mismatches, size_t n_mismatches,
                                            uint64_t* anchor_off, vgk_chain_anchor* anchors, vgk_anchor_origin* origins, size_t cap_anchors,
                                            uint64_t* rep_off, uint32_t* represented, size_t cap_rep, uint32_t* status, size_t written[2]) {
    (void)n_nodes; (void)n_mismatches;
    const bool from_seeds = (flags & VGK_ANCHORS_FROM_SEEDS) != 0;
    std::vector<uint64_t> node_tab(n_oriented + 1, 0);
    for (uint64_t o = 0; o < n_oriented; ++o) node_tab[o] = (uint64_t)oriented_node_length[o] << 32;
    std::vector<EaProb> probs(n_problems);
    for (uint32_t p = 0; p < n_problems; ++p)
        probs[p] = EaProb{seed_off[p], from_seeds ? 0 : ext_off[p], (uint32_t)(seed_off[p + 1] - seed_off[p]), from_seeds ? 0u : (uint32_t)(ext_off[p + 1] - ext_off[p]),
                          !from_seeds && full_length ? full_length[p] : 0u, 0u};
    const uint64_t ns = seed_off[n_problems], ne = from_seeds ? 0 : ext_off[n_problems];
    std::vector<vgk_chain_anchor> seed_anchor(ns + 1), made(ns + 1), sorted_anchor(ns + 1); std::vector<vgk_anchor_origin> made_origin(ns + 1), sorted_origin(ns + 1);
    std::vector<uint32_t> rep(ns + ne + 1), n_anchors(n_problems + 1), n_rep(n_problems + 1), flag(1, 0);
    EaParams P{};
    P.match = match; P.mismatch = mismatch; P.from_seeds = from_seeds; P.max_mismatches = default_max_extension_mismatches; P.n_problems = n_problems; P.n_oriented = (uint32_t)n_oriented;
    P.n_seeds = ns; P.n_ext = ne; P.node_tab = node_tab.data(); P.probs = probs.data(); P.seeds = seeds; P.ext = extensions; P.nodes = nodes; P.mism = mismatches;
    P.seed_anchor = seed_anchor.data(); P.flags = flag.data(); P.made = made.data(); P.made_origin = made_origin.data(); P.anchors = sorted_anchor.data(); P.origins = sorted_origin.data();
    P.rep = rep.data(); P.n_anchors = n_anchors.data(); P.n_rep = n_rep.data(); P.status = status;
    uint64_t total = 0, total_rep = 0;
    for (uint32_t p = 0; p < n_problems; ++p) { ea_problem_one(P, p); total += n_anchors[p]; total_rep += n_rep[p]; }
    if (flag[0]) return VGK_EINVAL;
    if (written) { written[0] = total; written[1] = total_rep; }
    if (total > cap_anchors || total_rep > cap_rep) return VGK_EOPS;
    uint64_t at = 0, rep_at = 0;
    for (uint32_t p = 0; p < n_problems; ++p) {
        anchor_off[p] = at; rep_off[p] = rep_at;
        const uint32_t* r = rep.data() + probs[p].s_off + probs[p].e_off;
        for (uint32_t k = 0; k < n_rep[p]; ++k) represented[rep_at + k] = r[k];
        for (uint32_t k = 0; k < n_anchors[p]; ++k) {
            anchors[at] = sorted_anchor[probs[p].s_off + k]; origins[at] = sorted_origin[probs[p].s_off + k];
            origins[at].rep_begin += (uint32_t)rep_at;
            ++at;
        }
        rep_at += n_rep[p];
    }
    anchor_off[n_problems] = at; rep_off[n_problems] = rep_at;
    return VGK_OK;
}

#ifdef EA_DRIVER_MAIN
// in:  10 words (n_oriented, match, mismatch, flags, max mismatches, n_problems, seeds, extensions, nodes, mismatches), then the arrays in the call's order
// out: 3 words (rc, anchors, represented), then anchor_off, rep_off, status, anchors, origins, represented
template <class T> static bool get(FILE* f, std::vector<T>& v, uint64_t n) { v.assign(n + 1, T{}); return !n || fread(v.data(), sizeof(T), n, f) == n; }
int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s call.bin answer.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    uint64_t h[10];
    if (!f || fread(h, 8, 10, f) != 10) return 2;
    const uint32_t n = (uint32_t)h[5];
    std::vector<uint32_t> len, full, nodes, mism; std::vector<uint64_t> soff, eoff; std::vector<vgk_anchor_seed> seeds; std::vector<vgk_extension> ext;
    if (!get(f, len, h[0]) || !get(f, soff, n + 1) || !get(f, seeds, h[6]) || !get(f, eoff, n + 1) || !get(f, ext, h[7]) || !get(f, full, n) || !get(f, nodes, h[8]) || !get(f, mism, h[9])) return 2;
    fclose(f);
    std::vector<uint64_t> aoff(n + 1), roff(n + 1); std::vector<uint32_t> status(n + 1), rep(h[6] + h[7] + 1);
    std::vector<vgk_chain_anchor> anchors(h[6] + 1); std::vector<vgk_anchor_origin> origins(h[6] + 1);
    size_t written[2] = {0, 0};
    const int rc = vgt_extension_anchors_serial(len.data(), h[0], (int32_t)h[1], (int32_t)h[2], (uint32_t)h[3], (uint32_t)h[4], n, soff.data(), seeds.data(), eoff.data(), ext.data(), full.data(),
                                                nodes.data(), h[8], mism.data(), h[9], aoff.data(), anchors.data(), origins.data(), h[6], roff.data(), rep.data(), h[6] + h[7], status.data(), written);
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    const uint64_t o[3] = {(uint64_t)(int64_t)rc, written[0], written[1]};
    fwrite(o, 8, 3, g); fwrite(aoff.data(), 8, n + 1, g); fwrite(roff.data(), 8, n + 1, g); fwrite(status.data(), 4, n, g);
    fwrite(anchors.data(), sizeof(vgk_chain_anchor), written[0], g); fwrite(origins.data(), sizeof(vgk_anchor_origin), written[0], g); fwrite(rep.data(), 4, written[1], g);
    fclose(g);
    return rc ? 1 : 0;
}
#endif
