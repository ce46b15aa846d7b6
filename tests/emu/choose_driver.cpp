// choose_driver.cpp — test infrastructure only: the serial lane code of find_seeds' choice (minimizer_device.hpp: mz_choose_one, the statement of
// the rule the kernel is checked against) behind one C call, so that it can be held to the host shim's select_minimizers without a GPU
// (tests/test_seed_choice_device.py).  The score table is made as vgk_minimizer_choose makes it.
#include <cmath>
#include <vector>
#include "../../vg_amd/csrc/minimizer_device.hpp"
#include "../../include/vgk_engine.h"

using namespace vgk;

extern "C" int vgt_choose_serial(const vgk_find_seeds_policy* p, uint32_t k, const char* reads, const uint64_t* read_off, uint32_t n,
                                 const uint64_t* minimizer_off, const vgk_read_minimizer* minimizers, uint8_t* verdict, uint32_t* over_rank_out) {
    if (!p || !p->hard_hit_cap || p->hard_hit_cap > 65535u) return VGK_EINVAL;
    std::vector<double> tab((size_t)p->hard_hit_cap + 1, 0.0);
    const double base = 1.0 + std::log((double)p->hard_hit_cap);
    for (uint32_t h = 1; h <= p->hard_hit_cap; ++h) tab[h] = base - std::log((double)h);
    MzChooseParams P{};
    MzChoosePolicy& Q = P.policy;
    Q.hit_cap = p->hit_cap; Q.hard_hit_cap = p->hard_hit_cap; Q.fraction = p->minimizer_score_fraction; Q.tab = tab.data();
    Q.max_unique_min = p->max_unique_min; Q.num_bp_per_min = p->num_bp_per_min; Q.flank = p->minimizer_coverage_flank; Q.exclude_overlapping = p->exclude_overlapping_min;
    Q.window_count = p->minimizer_downsampling_window_count; Q.max_window = p->minimizer_downsampling_max_window_length;
    Q.over_rank = mz_over_rank(tab.data(), p->hard_hit_cap);
    if (over_rank_out) *over_rank_out = Q.over_rank;
    P.k = k; P.reads = reads; P.read_off = read_off; P.min_off = minimizer_off; P.mins = minimizers; P.verdict = verdict; P.as_take = 0;
    for (uint32_t r = 0; r < n; ++r) {
        const size_t m = (size_t)(minimizer_off[r + 1] - minimizer_off[r]), L = (size_t)(read_off[r + 1] - read_off[r]);
        const uint64_t window = mz_choose_window(Q, L, k);
        if (m && window && k > window) return VGK_EINVAL;
        std::vector<uint32_t> order(m), tmp(m), start(m + 1), perm(m), dq(m); std::vector<uint8_t> kept(m), covered(L + 1), covered_by_minimizer(L + 1);
        const MzChooseScratch S{order.data(), tmp.data(), start.data(), perm.data(), dq.data(), kept.data(), covered.data(), covered_by_minimizer.data()};
        mz_choose_one(P, r, S);
    }
    return VGK_OK;
}
