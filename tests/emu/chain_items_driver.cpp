// chain_items_driver.cpp — test infrastructure only: the serial statement of the device's chaining rule (chain_items_device.hpp: ci_problem_one, what
// the kernels are checked against) behind one C call with vgk_chain_items' arguments, so that it can be held to the host shim's find_best_chains
// without a GPU (tests/test_chain_items.py).  The jump tables are made as vgk_chain_items makes them; nothing is validated here.
#include <cmath>
#include <map>
#include <vector>
#include "../../vg_amd/csrc/chain_items_device.hpp"

using namespace vgk;

extern "C" int vgt_chain_items_serial(const vgk_chain_scheme* scheme, uint32_t n_problems, const uint64_t* anchor_off, const vgk_chain_anchor* anchors,
                                      const uint64_t* cand_off, const vgk_chain_candidate* candidates, const uint32_t* read_lookback, const uint32_t* indel_limit,
                                      uint64_t* chain_off, vgk_chain_found* chains, uint32_t* items, uint32_t* rec_right, uint32_t* rec_left,
                                      int32_t* table_score, uint32_t* table_source) {
    std::vector<CiProb> probs(n_problems); std::vector<uint64_t> bsl(n_problems, 0);
    uint32_t max_limit = 0; uint64_t slot = 0;
    std::map<uint64_t, uint32_t> table_of;
    for (uint32_t p = 0; p < n_problems; ++p) {
        CiProb& q = probs[p];
        q.a_off = anchor_off[p]; q.n = (uint32_t)(anchor_off[p + 1] - anchor_off[p]); q.slot = slot;
        q.lookback = read_lookback ? read_lookback[p] : scheme->max_read_lookback_bases; q.limit = indel_limit ? indel_limit[p] : scheme->max_indel_bases;
        if (q.limit > CI_MAX_INDEL) return VGK_EUNSUPPORTED;
        slot += q.n < scheme->max_chains ? (q.n ? q.n : 1u) : (scheme->max_chains ? scheme->max_chains : 1u);
        if (!q.n) continue;
        max_limit = q.limit > max_limit ? q.limit : max_limit;
        for (uint32_t i = 0; i < q.n; ++i) bsl[p] += anchors[q.a_off + i].base_seed_length;
        bsl[p] /= q.n;
        table_of.emplace(bsl[p], (uint32_t)table_of.size());
    }
    const uint64_t table_len = (uint64_t)max_limit + 1;
    std::vector<int32_t> jump(table_of.size() * table_len + 1, 0);
    for (const auto& t : table_of)
        for (uint64_t d = 1; d < table_len; ++d) {
            const int gap = 0.01 * t.first * d + 0.5 * log2(d);
            jump[t.second * table_len + d] = (int32_t)(-gap * scheme->gap_scale);
        }
    for (uint32_t p = 0; p < n_problems; ++p) if (probs[p].n) probs[p].jump_off = (uint32_t)(table_of[bsl[p]] * table_len);
    const uint64_t n_cands = cand_off[n_problems], n_anchors = anchor_off[n_problems];
    std::vector<uint32_t> indel(n_cands + 1), n_chains(n_problems, 0), flags(1, 0); std::vector<vgk_chain_found> slots(slot);
    std::vector<int32_t> own_score(n_anchors + 1); std::vector<uint32_t> own_source(n_anchors + 1);
    CiParams P{};
    P.item_bonus = scheme->item_bonus; P.recombination_penalty = scheme->recombination_penalty; P.consistency_bonus = scheme->consistency_bonus; P.max_chains = scheme->max_chains;
    P.n_problems = n_problems; P.n_cands = n_cands; P.n_anchors = n_anchors;
    P.probs = probs.data(); P.cand_off = cand_off; P.anchors = anchors; P.cands = candidates; P.jump = jump.data(); P.indel = indel.data(); P.flags = flags.data();
    P.t_score = table_score ? table_score : own_score.data(); P.t_source = table_source ? table_source : own_source.data();
    P.chains = slots.data(); P.n_chains = n_chains.data(); P.items = items; P.rec_right = rec_right; P.rec_left = rec_left;
    uint64_t at = 0;
    for (uint32_t p = 0; p < n_problems; ++p) {
        ci_problem_one(P, p);
        chain_off[p] = at;
        for (uint32_t k = 0; k < n_chains[p]; ++k) chains[at++] = slots[probs[p].slot + k];
    }
    chain_off[n_problems] = at;
    return flags[0] ? VGK_EINVAL : VGK_OK;
}
