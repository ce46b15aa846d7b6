// pick_mappings_api.cpp — vgk_pick_mappings (include/vgk_engine.h): the host half of a long read's mappings chosen on the device
// (pick_mappings_device.hpp).
//
// Per call: the call's own checks and every size in 64 bits on the host (one pass over the alignments lays their mapping slots out), VGK_ETOOBIG and
// VGK_EOPS before anything is allocated; inputs go up in one copy each.  Then the checks (a lane per alignment and per chain) and the statistics (a
// lane per mapping slot); the reads' verdicts come down and the pick's plan is made from them — a read whose used set or walk order does not fit LDS
// goes into the second launch over a slab (launch_split.hpp); then multiplicities and sort scores (a lane per alignment) and the pick (a wavefront per
// read).  Everything comes back in one copy per array.
#include <algorithm>
#include <vector>
#include "ctx.hpp"
#include "pick_mappings_device.hpp"

using namespace vgk;

extern "C" {

int vgk_pick_mappings_limits(uint32_t out[4]) {
    if (!out) return VGK_EINVAL;
    out[0] = PICK_LDS_NODES; out[1] = PICK_LDS_SLOTS; out[2] = FN_LDS_ITEMS; out[3] = 64;
    return VGK_OK;
}
int vgk_pick_mappings_last_ms(vgk_ctx* ctx, double ms[4]) {
    if (!ctx || !ms) return VGK_EINVAL;
    for (int k = 0; k < 4; ++k) ms[k] = ctx->pick_mappings_ms[k];
    return VGK_OK;
}
int vgk_pick_mappings_last_launches(vgk_ctx* ctx, uint64_t reads[3]) {
    if (!ctx || !reads) return VGK_EINVAL;
    for (int k = 0; k < 3; ++k) reads[k] = ctx->pick_mappings_reads[k];
    return VGK_OK;
}

int vgk_pick_mappings(vgk_ctx* ctx, const vgk_pick_scheme* scheme, uint32_t n_reads, const char* reads, const uint64_t* read_off, uint32_t* rng_state,
                      const uint64_t* chain_off, const vgk_pick_chain* chains, const uint64_t* aln_off, const vgk_pick_alignment* alns,
                      const vgk_chain_mapping* mappings, size_t n_mappings, const uint32_t* edits, size_t n_edits,
                      vgk_pick_result* results, vgk_pick_verdict* verdicts, uint32_t* picked, int32_t* scores, double* multiplicity, size_t cap, size_t* written) try {
    if (written) *written = 0;
    if (!ctx || (n_reads && (!chain_off || !aln_off || !results || (rng_state && !read_off))) || (n_mappings && !mappings) || (n_edits && !edits)) return VGK_EINVAL;
    for (int k = 0; k < 4; ++k) ctx->pick_mappings_ms[k] = 0;
    for (int k = 0; k < 3; ++k) ctx->pick_mappings_reads[k] = 0;
    int rc = pick_check_call(scheme, n_reads, reads, read_off, rng_state, chain_off, aln_off, n_mappings, n_edits);
    if (rc || !n_reads) return rc;
    const uint64_t n_chains = chain_off[n_reads], n_alns = aln_off[n_reads], room = n_alns + n_reads;
    if ((n_chains && !chains) || (n_alns && (!alns || !verdicts))) return VGK_EINVAL;
    if (written) *written = (size_t)room;
    if (room > cap) return VGK_EOPS;
    if (!picked || !scores || !multiplicity) return VGK_EINVAL;
    // an alignment's mapping slots, and the most nodes a read's accepted alignments can hold
    std::vector<uint64_t> slot_off((size_t)n_alns + 1, 0); std::vector<uint64_t> node_bound(n_reads, 0); std::vector<uint32_t> counts;
    for (uint32_t r = 0; r < n_reads; ++r) {
        counts.clear();
        for (uint64_t i = aln_off[r]; i < aln_off[r + 1]; ++i) {
            const uint32_t m = pick_range_ok(alns[i].result, n_mappings) ? alns[i].result.n_mappings : 0u;
            slot_off[i + 1] = slot_off[i] + m; counts.push_back(m);
        }
        node_bound[r] = pick_node_bound(counts.data(), (uint32_t)counts.size(), scheme->max_multimaps);
        if (node_bound[r] > (1ull << 30)) return VGK_ETOOBIG;      // (its table of twice as many slots would leave 32 bits)
    }
    const uint64_t n_slots = slot_off[n_alns];
    if (n_slots > INDEX_MOST) return VGK_ETOOBIG;
    std::vector<vgk_pick_result> res0(n_reads, vgk_pick_result{});

    Backend* be = ctx->be.get();
    std::lock_guard<std::mutex> lock(ctx->mu);
    PickParams P{};
    P.sch = *scheme; P.n_reads = n_reads; P.n_alns = (uint32_t)n_alns; P.n_chains = (uint32_t)n_chains; P.n_slots = (uint32_t)n_slots; P.n_mappings = n_mappings; P.n_edits = n_edits;
    if (rng_state) {
        P.reads = ctx->scratch_dev<char>(PICK_READS, reads, read_off[n_reads]);
        P.read_off = ctx->scratch_dev<uint64_t>(PICK_READ_OFF, read_off, sizeof(uint64_t) * ((uint64_t)n_reads + 1));
        P.rng_state = ctx->scratch_dev<uint32_t>(PICK_RNG, rng_state, sizeof(uint32_t) * (uint64_t)n_reads);
        if (!P.reads || !P.read_off || !P.rng_state) return VGK_ENOMEM;
    }
    P.chain_off = ctx->scratch_dev<uint64_t>(PICK_CHAIN_OFF, chain_off, sizeof(uint64_t) * ((uint64_t)n_reads + 1));
    P.chains = ctx->scratch_dev<vgk_pick_chain>(PICK_CHAINS, chains, sizeof(vgk_pick_chain) * n_chains);
    P.aln_off = ctx->scratch_dev<uint64_t>(PICK_ALN_OFF, aln_off, sizeof(uint64_t) * ((uint64_t)n_reads + 1));
    P.alns = ctx->scratch_dev<vgk_pick_alignment>(PICK_ALNS, alns, sizeof(vgk_pick_alignment) * n_alns);
    P.mappings = ctx->scratch_dev<vgk_chain_mapping>(PICK_MAPPINGS, mappings, sizeof(vgk_chain_mapping) * (uint64_t)n_mappings);
    P.edits = ctx->scratch_dev<uint32_t>(PICK_EDITS, edits, sizeof(uint32_t) * (uint64_t)n_edits);
    P.slot_off = ctx->scratch_dev<uint64_t>(PICK_SLOT_OFF, slot_off.data(), sizeof(uint64_t) * (n_alns + 1));
    P.res = ctx->scratch_dev<vgk_pick_result>(PICK_RES, res0.data(), sizeof(vgk_pick_result) * (uint64_t)n_reads);
    P.from_len = (unsigned long long*)ctx->ensure_scratch(PICK_FROM_LEN, sizeof(unsigned long long) * (n_slots + 1));
    P.sums = (unsigned long long*)ctx->ensure_scratch(PICK_SUMS, sizeof(unsigned long long) * 2 * (n_alns + 1));
    P.aln_mult = (double*)ctx->ensure_scratch(PICK_ALN_MULT, sizeof(double) * (n_alns + 1));
    P.aln_sort = (double*)ctx->ensure_scratch(PICK_ALN_SORT, sizeof(double) * (n_alns + 1));
    P.verdicts = (vgk_pick_verdict*)ctx->ensure_scratch(PICK_VERDICTS, sizeof(vgk_pick_verdict) * (n_alns + 1));
    P.picked = (uint32_t*)ctx->ensure_scratch(PICK_PICKED, sizeof(uint32_t) * room);
    P.scores = (int32_t*)ctx->ensure_scratch(PICK_SCORES, sizeof(int32_t) * room);
    P.out_mult = (double*)ctx->ensure_scratch(PICK_OUT_MULT, sizeof(double) * room);
    if (!P.chain_off || !P.chains || !P.aln_off || !P.alns || !P.mappings || !P.edits || !P.slot_off || !P.res || !P.from_len || !P.sums || !P.aln_mult || !P.aln_sort
        || !P.verdicts || !P.picked || !P.scores || !P.out_mult) return VGK_ENOMEM;
    {
        Timed t(be, &ctx->pick_mappings_ms[0]);
        rc = be->zero(P.sums, sizeof(unsigned long long) * 2 * (n_alns + 1));
        if (!rc) rc = be->zero(P.verdicts, sizeof(vgk_pick_verdict) * (n_alns + 1));
        if (!rc) rc = be->zero(P.picked, sizeof(uint32_t) * room);
        if (!rc) rc = be->zero(P.scores, sizeof(int32_t) * room);
        if (!rc) rc = be->zero(P.out_mult, sizeof(double) * room);
        if (!rc) rc = be->run_pick_mappings(P, PICK_RUN_CHECK, 0);
        const int rs = t.done();                                    // (the staged host arrays may go)
        if (rc || rs) return rc ? rc : rs;
    }
    {
        Timed t(be, &ctx->pick_mappings_ms[1]);
        rc = be->run_pick_mappings(P, PICK_RUN_STATS, 0);
        const int rs = t.done();
        if (rc || rs) return rc ? rc : rs;
    }
    // the verdicts, and from them the plan of the pick: a refused read is in neither launch
    if ((rc = be->download(res0.data(), P.res, sizeof(vgk_pick_result) * (uint64_t)n_reads))) return rc;
    auto large = [&](uint32_t r) { return aln_off[r + 1] - aln_off[r] > FN_LDS_ITEMS || node_bound[r] > PICK_LDS_NODES; };
    const SlabPlan plan = slab_plan(n_reads, [&](uint32_t r) { return res0[r].status != VGK_OK ? ROUTE_SKIP : large(r) ? ROUTE_SLAB : ROUTE_LDS; },
                                    [&](uint32_t r) { return node_bound[r]; });
    ctx->pick_mappings_reads[0] = plan.n_lds; ctx->pick_mappings_reads[1] = plan.n_large; ctx->pick_mappings_reads[2] = (uint64_t)n_reads - plan.n_lds - plan.n_large;
    const uint32_t* d_ids = ctx->scratch_dev<uint32_t>(PICK_IDS, plan.ids.data(), sizeof(uint32_t) * plan.ids.size());
    if (!d_ids) return VGK_ENOMEM;
    uint32_t blocks = 0; char* slab = nullptr;
    if (plan.n_large) {
        uint64_t most_items = 1;
        for (uint32_t j = 0; j < plan.n_large; ++j) most_items = std::max<uint64_t>(most_items, aln_off[plan.large()[j] + 1] - aln_off[plan.large()[j]]);
        P.slab_items = (uint32_t)most_items; P.slab_slots = pick_slots_for(plan.slab_largest); P.slab_stride = sizeof(uint32_t) * ((uint64_t)P.slab_items + P.slab_slots);
        blocks = slab_blocks(plan.n_large, P.slab_stride);
        slab = (char*)ctx->ensure_scratch(PICK_SLAB, P.slab_stride * blocks);
        if (!slab) return VGK_ENOMEM;
    }
    if (n_alns) {
        Timed t(be, &ctx->pick_mappings_ms[2]);
        rc = be->run_pick_mappings(P, PICK_RUN_ALIGNMENTS, 0);
        const int rs = t.done();
        if (rc || rs) return rc ? rc : rs;
    }
    {
        Timed t(be, &ctx->pick_mappings_ms[3]);
        rc = launch_split(P, d_ids, plan, slab, blocks, [&](const PickParams& L, uint32_t grid) { return be->run_pick_mappings(L, PICK_RUN_PICK, grid); });
        const int rs = t.done();
        if (rc || rs) return rc ? rc : rs;
    }
    if ((rc = be->download(results, P.res, sizeof(vgk_pick_result) * (uint64_t)n_reads))) return rc;
    if (n_alns && (rc = be->download(verdicts, P.verdicts, sizeof(vgk_pick_verdict) * n_alns))) return rc;
    if ((rc = be->download(picked, P.picked, sizeof(uint32_t) * room)) || (rc = be->download(scores, P.scores, sizeof(int32_t) * room))
        || (rc = be->download(multiplicity, P.out_mult, sizeof(double) * room))) return rc;
    if (rng_state && (rc = be->download(rng_state, P.rng_state, sizeof(uint32_t) * (uint64_t)n_reads))) return rc;
    return VGK_OK;
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }      // (no exception leaves the C ABI)

}  // extern "C"
