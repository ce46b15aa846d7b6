// chain_items_api.cpp — vgk_chain_items (include/vgk_engine.h): the host half of choosing chains on the device (chain_items_device.hpp).
//
// Per call: every size is taken from the caller's offsets in 64 bits and checked before anything is allocated or scanned; the anchors are
// checked (order, lengths) and summed (the mean base seed length, the bound on the score sums) on a few host threads; one jump table per distinct
// mean base seed length is made in double, exactly as the reference evaluates it, up to the call's largest indel limit; anchors, candidates and
// tables go up in one copy each.  Three groups of kernels, timed apart: legality + grouping (two lanes-per-candidate kernels around a prefix
// sum) | the DP | the tracebacks.  The chains come back at their problems' slots and are packed behind each other here.
#include <algorithm>
#include <cmath>
#include <map>
#include <vector>
#include "ctx.hpp"
#include "host_parallel.hpp"
#include "chain_items_device.hpp"

using namespace vgk;

namespace {
// (int)(-score_chain_gap(d, bsl) * gap_scale), the reference's expression in its types (src/algorithms/chain_items.cpp:365-373, :511); false when
// either conversion to int would leave int
bool jump_of(uint64_t d, uint64_t bsl, double gap_scale, int32_t* out) {
    double gap = 0.0;
    if (d) gap = 0.01 * bsl * d + 0.5 * std::log2((double)d);
    if (!(gap < 2147483647.0)) return false;
    const int g = (int)gap;
    const double v = -g * gap_scale;
    if (!(v > -2147483647.0 && v < 2147483647.0)) return false;
    *out = (int32_t)v;
    return true;
}
}  // namespace

extern "C" {

int vgk_chain_items_limits(uint32_t out[4]) {
    if (!out) return VGK_EINVAL;
    out[0] = CI_LDS_MAX; out[1] = CI_MAX_INDEL; out[2] = 64; out[3] = 0;
    return VGK_OK;
}

int vgk_chain_items_last_ms(vgk_ctx* ctx, double ms[3]) {
    if (!ctx || !ms) return VGK_EINVAL;
    for (int k = 0; k < 3; ++k) ms[k] = ctx->chain_items_ms[k];
    return VGK_OK;
}

int vgk_chain_items(vgk_ctx* ctx, const vgk_chain_scheme* scheme, uint32_t n_problems, const uint64_t* anchor_off, const vgk_chain_anchor* anchors,
                    const uint64_t* cand_off, const vgk_chain_candidate* candidates, const uint32_t* read_lookback, const uint32_t* indel_limit,
                    uint64_t* chain_off, vgk_chain_found* chains, uint32_t* items, uint32_t* rec_right, uint32_t* rec_left,
                    int32_t* table_score, uint32_t* table_source) try {
    if (!ctx || !scheme || !chain_off || (n_problems && (!anchor_off || !cand_off || !chains || !items || !rec_right || !rec_left))) return VGK_EINVAL;
    if (scheme->recombination_penalty < 0 || scheme->consistency_bonus < 0 || !std::isfinite(scheme->gap_scale) || scheme->gap_scale < 0.0) return VGK_EINVAL;
    chain_off[0] = 0;
    if (!n_problems) return VGK_OK;
    // ---- sizes first, in 64 bits, from the offsets alone
    if (anchor_off[0] != 0 || cand_off[0] != 0) return VGK_EINVAL;
    uint64_t n_slots = 0;
    for (uint32_t p = 0; p < n_problems; ++p) {
        if (anchor_off[p + 1] < anchor_off[p] || cand_off[p + 1] < cand_off[p]) return VGK_EINVAL;
        const uint64_t n = anchor_off[p + 1] - anchor_off[p];
        n_slots += std::max<uint64_t>(1, std::min<uint64_t>(n, scheme->max_chains));
    }
    const uint64_t n_anchors = anchor_off[n_problems], n_cands = cand_off[n_problems];
    if (n_anchors > INDEX_MOST || n_cands > INDEX_MOST) return VGK_ETOOBIG;
    if ((n_anchors && !anchors) || (n_cands && !candidates)) return VGK_EINVAL;
    // ---- the problems: limits, anchors in order, the mean base seed length, the bound on what a score can sum to
    std::vector<CiProb> probs(n_problems); std::vector<uint64_t> bsl(n_problems, 0), own_sum(n_problems, 0); std::vector<uint8_t> bad(n_problems, 0);
    uint32_t max_limit = 0;
    for (uint32_t p = 0; p < n_problems; ++p) {
        CiProb& q = probs[p];
        q.a_off = anchor_off[p]; q.n = (uint32_t)(anchor_off[p + 1] - anchor_off[p]);
        q.lookback = read_lookback ? read_lookback[p] : scheme->max_read_lookback_bases; q.limit = indel_limit ? indel_limit[p] : scheme->max_indel_bases; q.jump_off = 0; q.slot = 0;
        if (q.limit > CI_MAX_INDEL) return VGK_EUNSUPPORTED;
        if (q.n) max_limit = std::max(max_limit, q.limit);
    }
    parallel_for(n_problems, [&](uint32_t p, unsigned) {
        const vgk_chain_anchor* a = anchors + probs[p].a_off; const uint32_t n = probs[p].n;
        uint64_t seed = 0, sum = 0; bool ok = true;
        for (uint32_t i = 0; i < n; ++i) {
            if (!a[i].length) ok = false;
            if (i && (a[i].read_start < a[i - 1].read_start || (a[i].read_start == a[i - 1].read_start && (uint64_t)a[i].read_start + a[i].length > (uint64_t)a[i - 1].read_start + a[i - 1].length))) ok = false;
            seed += a[i].base_seed_length;
            const int64_t points = (int64_t)a[i].score + scheme->item_bonus;
            sum += (uint64_t)(points < 0 ? -points : points);
        }
        bad[p] = ok ? 0 : 1; bsl[p] = n ? seed / n : 0; own_sum[p] = sum;
    });
    for (uint32_t p = 0; p < n_problems; ++p) if (bad[p]) return VGK_EINVAL;
    // ---- one jump table per distinct mean base seed length, up to the call's largest indel limit
    std::map<uint64_t, uint32_t> table_of;
    for (uint32_t p = 0; p < n_problems; ++p) if (probs[p].n) table_of.emplace(bsl[p], 0u);
    const uint64_t table_len = (uint64_t)max_limit + 1;
    if (table_of.size() * table_len > (1ull << 28)) return VGK_ENOMEM;
    std::vector<int32_t> jump(std::max<size_t>(1, table_of.size() * table_len), 0);
    {
        uint32_t k = 0;
        for (auto& t : table_of) t.second = k++;
        std::vector<const std::pair<const uint64_t, uint32_t>*> flat;
        for (auto& t : table_of) flat.push_back(&t);
        std::vector<uint8_t> over(flat.size(), 0);
        parallel_tasks((uint32_t)flat.size(), [&](uint32_t t) {
            int32_t* tab = jump.data() + (size_t)flat[t]->second * table_len;
            for (uint64_t d = 0; d < table_len; ++d) if (!jump_of(d, flat[t]->first, scheme->gap_scale, &tab[d])) { tab[d] = (int32_t)0x80000000; over[t] = 1; }
        });
    }
    // a problem whose sums could leave int32: every anchor's own points, and per step the largest jump of its limit, the recombination penalty; a
    // traceback's penalty is a difference of two such sums plus one more (the correction), the evaluation adds the bonus (times up to 64 paths)
    for (uint32_t p = 0; p < n_problems; ++p) {
        CiProb& q = probs[p];
        if (!q.n) continue;
        q.jump_off = (uint32_t)(table_of[bsl[p]] * table_len);
        const int32_t worst = jump[q.jump_off + q.limit];                  // (the gap grows with the distance: the last entry is the most negative)
        if (worst == (int32_t)0x80000000) return VGK_EUNSUPPORTED;
        const long double bound = 4.0L * ((long double)own_sum[p] + (long double)q.n * ((long double)(-(int64_t)worst) + scheme->recombination_penalty)) + 64.0L * scheme->consistency_bonus;
        if (bound > 2147483647.0L) return VGK_EUNSUPPORTED;
    }
    {
        uint64_t slot = 0;
        for (uint32_t p = 0; p < n_problems; ++p) { probs[p].slot = slot; slot += std::max<uint64_t>(1, std::min<uint64_t>(probs[p].n, scheme->max_chains)); }
    }
    // ---- the launches' problems: those whose tables fit LDS first, the others over slabs
    const SlabPlan plan = slab_plan(n_problems, [&](uint32_t p) { return probs[p].n <= CI_LDS_MAX ? ROUTE_LDS : ROUTE_SLAB; }, [&](uint32_t p) { return probs[p].n; });

    std::lock_guard<std::mutex> lock(ctx->mu);
    Backend* be = ctx->be.get();
    CiParams P{};
    P.item_bonus = scheme->item_bonus; P.recombination_penalty = scheme->recombination_penalty; P.consistency_bonus = scheme->consistency_bonus; P.max_chains = scheme->max_chains;
    P.n_problems = n_problems; P.n_cands = n_cands; P.n_anchors = n_anchors;
    P.probs = ctx->scratch_dev<CiProb>(CITEMS_PROBS, probs.data(), sizeof(CiProb) * n_problems);
    P.cand_off = ctx->scratch_dev<uint64_t>(CITEMS_CAND_OFF, cand_off, sizeof(uint64_t) * ((size_t)n_problems + 1));
    P.anchors = ctx->scratch_dev<vgk_chain_anchor>(CITEMS_ANCHORS, anchors, sizeof(vgk_chain_anchor) * n_anchors);
    P.cands = ctx->scratch_dev<vgk_chain_candidate>(CITEMS_CANDS, candidates, sizeof(vgk_chain_candidate) * n_cands);
    P.jump = ctx->scratch_dev<int32_t>(CITEMS_JUMP, jump.data(), sizeof(int32_t) * jump.size());
    const uint32_t* d_ids = ctx->scratch_dev<uint32_t>(CITEMS_IDS, plan.ids.data(), sizeof(uint32_t) * plan.ids.size());
    P.indel = (uint32_t*)ctx->ensure_scratch(CITEMS_INDEL, sizeof(uint32_t) * std::max<uint64_t>(n_cands, 4));
    P.count = (uint32_t*)ctx->ensure_scratch(CITEMS_COUNT, sizeof(uint32_t) * (n_anchors + 1));
    uint32_t* d_first = (uint32_t*)ctx->ensure_scratch(CITEMS_FIRST, sizeof(uint32_t) * (n_anchors + 1));
    P.first = d_first;
    P.cursor = (uint32_t*)ctx->ensure_scratch(CITEMS_CURSOR, sizeof(uint32_t) * (n_anchors + 1));
    P.grouped = (CiEdge*)ctx->ensure_scratch(CITEMS_GROUPED, sizeof(CiEdge) * std::max<uint64_t>(n_cands, 2));
    P.flags = (uint32_t*)ctx->ensure_scratch(CITEMS_FLAGS, 16);
    P.t_score = (int32_t*)ctx->ensure_scratch(CITEMS_TSCORE, sizeof(int32_t) * (n_anchors + 1));
    P.t_source = (uint32_t*)ctx->ensure_scratch(CITEMS_TSOURCE, sizeof(uint32_t) * (n_anchors + 1));
    P.chains = (vgk_chain_found*)ctx->ensure_scratch(CITEMS_CHAINS, sizeof(vgk_chain_found) * n_slots);
    P.n_chains = (uint32_t*)ctx->ensure_scratch(CITEMS_NCHAINS, sizeof(uint32_t) * n_problems);
    P.items = (uint32_t*)ctx->ensure_scratch(CITEMS_ITEMS, sizeof(uint32_t) * (n_anchors + 1));
    P.rec_right = (uint32_t*)ctx->ensure_scratch(CITEMS_REC_RIGHT, sizeof(uint32_t) * (n_anchors + 1));
    P.rec_left = (uint32_t*)ctx->ensure_scratch(CITEMS_REC_LEFT, sizeof(uint32_t) * (n_anchors + 1));
    if (!P.probs || !P.cand_off || !P.anchors || !P.cands || !P.jump || !d_ids || !P.indel || !P.count || !d_first || !P.cursor || !P.grouped || !P.flags || !P.t_score || !P.t_source
        || !P.chains || !P.n_chains || !P.items || !P.rec_right || !P.rec_left) return VGK_ENOMEM;
    uint32_t blocks = 0; char* slab = nullptr;
    if (plan.n_large) {
        const uint64_t np = pow2_at_least(plan.slab_largest);
        P.slab_n = (uint32_t)plan.slab_largest; P.slab_np = (uint32_t)np; P.slab_stride = ci_slab_bytes(plan.slab_largest, np);
        blocks = slab_blocks(plan.n_large, P.slab_stride);
        slab = (char*)ctx->ensure_scratch(CITEMS_SLAB, P.slab_stride * blocks);
        if (!slab) return VGK_ENOMEM;
    }
    P.lds_np = (uint32_t)pow2_at_least(plan.lds_largest);
    int rc = be->zero(P.count, sizeof(uint32_t) * (n_anchors + 1));
    if (!rc) rc = be->zero(P.cursor, sizeof(uint32_t) * (n_anchors + 1));
    if (!rc) rc = be->zero(P.flags, 16);
    // (what no chain uses of the lists stays 0: the call answers the same bytes whatever the buffers held)
    if (!rc) rc = be->zero(P.items, sizeof(uint32_t) * (n_anchors + 1));
    if (!rc) rc = be->zero(P.rec_right, sizeof(uint32_t) * (n_anchors + 1));
    if (!rc) rc = be->zero(P.rec_left, sizeof(uint32_t) * (n_anchors + 1));
    if (rc) return rc;
    for (int k = 0; k < 3; ++k) ctx->chain_items_ms[k] = 0;
    // ---- legality and grouping
    {
        Timed t(be, &ctx->chain_items_ms[0]);
        rc = be->run_chain_items(P, CI_RUN_LEGAL, 0);
        if (!rc) rc = be->scan_u32(P.count, d_first, (uint32_t)(n_anchors + 1));
        if (!rc) rc = be->run_chain_items(P, CI_RUN_SCATTER, 0);
        const int rs = t.done();                                           // (the staged host arrays may go)
        if (rc || rs) return rc ? rc : rs;
    }
    uint32_t flags = 0;
    if ((rc = be->download(&flags, P.flags, sizeof flags))) return rc;
    if (flags) return VGK_EINVAL;                                          // a candidate outside its problem
    // ---- the DP, then the tracebacks: a wavefront per problem
    for (int stage = 0; stage < 2; ++stage) {
        Timed t(be, &ctx->chain_items_ms[1 + stage]);
        const int what = stage ? CI_RUN_TRACE : CI_RUN_DP;
        rc = launch_split(P, d_ids, plan, slab, blocks, [&](const CiParams& L, uint32_t grid) { return be->run_chain_items(L, what, grid); });
        const int rs = t.done();
        if (rc || rs) return rc ? rc : rs;
    }
    // ---- down: the chains from their slots, packed; the lists and the table as they are
    std::vector<uint32_t> n_chains(n_problems);
    if ((rc = be->download(n_chains.data(), P.n_chains, sizeof(uint32_t) * n_problems))) return rc;
    if ((rc = be->download(chains, P.chains, sizeof(vgk_chain_found) * n_slots))) return rc;
    uint64_t at = 0;
    for (uint32_t p = 0; p < n_problems; ++p) {
        chain_off[p] = at;
        if (n_chains[p] < 1 || n_chains[p] > std::max<uint64_t>(1, std::min<uint64_t>(probs[p].n, scheme->max_chains))) return VGK_ENODEV;      // (what no kernel of this file writes)
        if (at != probs[p].slot) std::copy(chains + probs[p].slot, chains + probs[p].slot + n_chains[p], chains + at);
        at += n_chains[p];
    }
    chain_off[n_problems] = at;
    if (n_anchors) {
        if ((rc = be->download(items, P.items, sizeof(uint32_t) * n_anchors))) return rc;
        if ((rc = be->download(rec_right, P.rec_right, sizeof(uint32_t) * n_anchors))) return rc;
        if ((rc = be->download(rec_left, P.rec_left, sizeof(uint32_t) * n_anchors))) return rc;
        if (table_score && (rc = be->download(table_score, P.t_score, sizeof(int32_t) * n_anchors))) return rc;
        if (table_source && (rc = be->download(table_source, P.t_source, sizeof(uint32_t) * n_anchors))) return rc;
    }
    return VGK_OK;
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }

}  // extern "C"
