// pair_mapq_api.cpp — vgk_pair_mapq (include/vgk_engine.h): the host half of a pair's mapping qualities on the device (pair_mapq_device.hpp).
//
// Per call: every size is taken from the caller's offsets in 64 bits and checked before anything is allocated; every pair is checked on a few host
// threads (pm_validate_pair) and a pair that fails keeps its verdict as its status; inputs go up in one copy each.  Without given caps the mates'
// sweep runs first, as vgk_read_mapq launches it (reads whose explored minimizers fit a lane's LDS slice, then the others over a slab) but without
// the scores' half: each read's cap and verdict stay in HBM, where the pair kernels read them.  Then one launch scores every candidate, and the
// pairs follow in two: those whose candidates fit a lane's LDS slice, then the others over a slab.
#include <algorithm>
#include <cmath>
#include <vector>
#include "ctx.hpp"
#include "host_parallel.hpp"
#include "pair_mapq_device.hpp"

using namespace vgk;

namespace {
// The explored cap of each of the n reads into PAIRMAPQ_CAPS, its verdict into PAIRMAPQ_CAP_STATUS (`lock` holds the context; sizes are checked)
int sweep_caps(vgk_ctx* ctx, std::unique_lock<std::mutex>& lock, uint32_t k, uint32_t n, const uint64_t* minimizer_off, const vgk_read_minimizer* minimizers,
               const vgk_minimizer_region* regions, const uint8_t* explored, const uint64_t* read_off, const uint8_t* quality, const double** caps, const int32_t** cap_status) {
    MqParams H{};                                                   // the host's view, for the checks
    H.k = k; H.n_reads = n; H.min_off = minimizer_off; H.mins = minimizers; H.regions = regions; H.explored = explored; H.read_off = read_off; H.qual = quality;
    vgk_ctx::MapqSweep S;
    const int rt = ctx->stage_mapq_sweep(H, true, mq_validate_sweep, lock, &S);
    if (rt) return rt;
    MqParams& P = S.P;
    P.cap_out = (double*)ctx->ensure_scratch(PAIRMAPQ_CAPS, sizeof(double) * ((uint64_t)n + 2));
    P.cap_status = (int32_t*)ctx->ensure_scratch(PAIRMAPQ_CAP_STATUS, sizeof(int32_t) * ((uint64_t)n + 4));
    if (!P.cap_out || !P.cap_status) return VGK_ENOMEM;
    Backend* be = ctx->be.get();
    Timed t(be, &ctx->pair_mapq_ms[0]);
    const int rc = launch_split(P, S.d_ids, S.plan, S.d_work, S.d_work_off, [&](const MqParams& L) { return be->run_explored_caps(L); }, &ctx->pair_mapq_launches[0]);
    const int rs = t.done();                                        // (the staged host arrays may go)
    *caps = P.cap_out; *cap_status = P.cap_status;
    return rc ? rc : rs;
}
}  // namespace

extern "C" {

int vgk_pair_mapq_limits(uint32_t out[4]) {
    if (!out) return VGK_EINVAL;
    out[0] = PM_LDS_CANDIDATES; out[1] = 1; out[2] = 1; out[3] = 0;
    return VGK_OK;
}

int vgk_pair_mapq_last_ms(vgk_ctx* ctx, double ms[2]) {
    if (!ctx || !ms) return VGK_EINVAL;
    ms[0] = ctx->pair_mapq_ms[0]; ms[1] = ctx->pair_mapq_ms[1];
    return VGK_OK;
}

int vgk_pair_mapq_last_launches(vgk_ctx* ctx, uint64_t pairs[3]) {
    if (!ctx || !pairs) return VGK_EINVAL;
    for (int k = 0; k < 3; ++k) pairs[k] = ctx->pair_mapq_pairs[k];
    return VGK_OK;
}

int vgk_pair_mapq_last_kernel_launches(vgk_ctx* ctx, uint32_t launches[2]) {
    if (!ctx || !launches) return VGK_EINVAL;
    launches[0] = ctx->pair_mapq_launches[0]; launches[1] = ctx->pair_mapq_launches[1];
    return VGK_OK;
}

int vgk_pair_mapq(vgk_ctx* ctx, const vgk_pair_mapq_scheme* scheme, uint32_t n, const uint64_t* cand_off, const vgk_pair_candidate* candidates, const vgk_pair_counts* counts,
                  const uint64_t* unpaired_off, const int32_t* unpaired_scores, const double* given_cap, const uint64_t* minimizer_off, const vgk_read_minimizer* minimizers,
                  const vgk_minimizer_region* regions, const uint8_t* explored, const uint64_t* read_off, const uint8_t* quality, vgk_pair_mapq_result* out, double* pair_score,
                  uint32_t* order) try {
    if (!ctx || !scheme || (scheme->flags & ~(uint32_t)VGK_PAIR_MAPQ_NO_EXPLORED_CAP)) return VGK_EINVAL;
    if (!(scheme->log_base > 0.0) || !(scheme->fragment_sd > 0.0) || std::isinf(scheme->log_base) || std::isinf(scheme->fragment_sd) || !std::isfinite(scheme->fragment_mean)) return VGK_EINVAL;
    if (n && (!cand_off || !counts || !out)) return VGK_EINVAL;
    std::unique_lock<std::mutex> lock(ctx->mu);                     // from here on: the records of the last call belong to one call at a time
    ctx->pair_mapq_ms[0] = 0; ctx->pair_mapq_ms[1] = 0; ctx->pair_mapq_launches[0] = 0; ctx->pair_mapq_launches[1] = 0;
    for (int k = 0; k < 3; ++k) ctx->pair_mapq_pairs[k] = 0;
    if (!n) return VGK_OK;
    // ---- sizes first, in 64 bits, from the offsets alone
    const uint64_t n_reads = 2 * (uint64_t)n;
    if (n_reads > INDEX_MOST) return VGK_ETOOBIG;
    const bool alone = unpaired_off && unpaired_scores;
    const bool capped = !(scheme->flags & VGK_PAIR_MAPQ_NO_EXPLORED_CAP), sweep = capped && !given_cap && quality;
    if (sweep && (!minimizer_off || !read_off)) return VGK_EINVAL;
    if (cand_off[0] != 0 || (alone && unpaired_off[0] != 0) || (sweep && (minimizer_off[0] != 0 || read_off[0] != 0))) return VGK_EINVAL;
    for (uint32_t p = 0; p < n; ++p) if (cand_off[p + 1] < cand_off[p]) return VGK_EINVAL;
    for (uint64_t r = 0; r < n_reads; ++r) {
        if (alone && unpaired_off[r + 1] < unpaired_off[r]) return VGK_EINVAL;
        if (!sweep) continue;
        if (minimizer_off[r + 1] < minimizer_off[r] || read_off[r + 1] < read_off[r]) return VGK_EINVAL;
        if (read_off[r + 1] - read_off[r] > 0x3fffffffull || minimizer_off[r + 1] - minimizer_off[r] >= MQ_MAX_READ_MINIMIZERS) return VGK_ETOOBIG;
    }
    const uint64_t n_cands = cand_off[n], n_alone = alone ? unpaired_off[n_reads] : 0;
    if (n_cands > INDEX_MOST || n_alone > INDEX_MOST || (sweep && (minimizer_off[n_reads] > INDEX_MOST || read_off[n_reads] > INDEX_MOST))) return VGK_ETOOBIG;
    if (n_cands && (!candidates || !pair_score || !order)) return VGK_EINVAL;
    if (sweep && minimizer_off[n_reads] && (!minimizers || !regions || !explored)) return VGK_EINVAL;
    // ---- every pair checked; the pairs of the two launches (a refused pair rides in the first: its lane writes the verdict and touches no slice)
    PmParams H{};
    H.max_rescue_attempts = scheme->max_rescue_attempts; H.n_pairs = n; H.cand_off = cand_off; H.cands = candidates; H.counts = counts;
    std::vector<int32_t> status(n);
    parallel_for(n, [&](uint32_t p, unsigned) { status[p] = pm_validate_pair(H, p); });
    const uint64_t refused = (uint64_t)std::count_if(status.begin(), status.end(), [](int32_t v) { return v != VGK_OK; });
    const SlicePlan plan = slice_plan(n, [&](uint32_t p) { return status[p] == VGK_OK && cand_off[p + 1] - cand_off[p] > PM_LDS_CANDIDATES; },
                                      [&](uint32_t p) { return pm_work_words(cand_off[p + 1] - cand_off[p]); });
    if (plan.rc) return plan.rc;

    Backend* be = ctx->be.get();
    PmParams P{};
    P.log_base = scheme->log_base; P.mean = scheme->fragment_mean; P.sd = scheme->fragment_sd; P.quality_scale = 10.0 / std::log(10.0);
    P.max_multimaps = scheme->max_multimaps; P.max_rescue_attempts = scheme->max_rescue_attempts; P.n_pairs = n; P.n_candidates = n_cands;
    if (sweep) {
        const int rc = sweep_caps(ctx, lock, scheme->k, (uint32_t)n_reads, minimizer_off, minimizers, regions, explored, read_off, quality, &P.caps, &P.cap_status);
        if (rc) return rc;
    } else if (capped && given_cap && !(P.caps = ctx->scratch_dev<double>(PAIRMAPQ_CAPS, given_cap, sizeof(double) * n_reads))) return VGK_ENOMEM;
    P.cand_off = ctx->scratch_dev<uint64_t>(PAIRMAPQ_CAND_OFF, cand_off, sizeof(uint64_t) * ((uint64_t)n + 1));
    P.cands = ctx->scratch_dev<vgk_pair_candidate>(PAIRMAPQ_CANDS, candidates, sizeof(vgk_pair_candidate) * n_cands);
    P.counts = ctx->scratch_dev<vgk_pair_counts>(PAIRMAPQ_COUNTS, counts, sizeof(vgk_pair_counts) * (uint64_t)n);
    P.status = ctx->scratch_dev<int32_t>(PAIRMAPQ_STATUS, status.data(), sizeof(int32_t) * (uint64_t)n);
    const uint32_t* d_ids = ctx->scratch_dev<uint32_t>(PAIRMAPQ_IDS, plan.ids.data(), sizeof(uint32_t) * plan.ids.size());
    const uint64_t* d_work_off = ctx->scratch_dev<uint64_t>(PAIRMAPQ_WORK_OFF, plan.work_off.data(), sizeof(uint64_t) * plan.work_off.size());
    uint32_t* d_work = (uint32_t*)ctx->ensure_scratch(PAIRMAPQ_WORK, sizeof(uint32_t) * (plan.work_words + 4));
    P.pair_score = (double*)ctx->ensure_scratch(PAIRMAPQ_SCORE, sizeof(double) * (n_cands + 2));
    P.order = (uint32_t*)ctx->ensure_scratch(PAIRMAPQ_ORDER, sizeof(uint32_t) * (n_cands + 4));
    P.out = (vgk_pair_mapq_result*)ctx->ensure_scratch(PAIRMAPQ_OUT, sizeof(vgk_pair_mapq_result) * (uint64_t)n);
    if (!P.cand_off || !P.cands || !P.counts || !P.status || !d_ids || !d_work_off || !d_work || !P.pair_score || !P.order || !P.out) return VGK_ENOMEM;
    if (alone) {
        P.unp_off = ctx->scratch_dev<uint64_t>(PAIRMAPQ_UNP_OFF, unpaired_off, sizeof(uint64_t) * (n_reads + 1));
        P.unp_scores = ctx->scratch_dev<int32_t>(PAIRMAPQ_UNP_SCORES, unpaired_scores, sizeof(int32_t) * n_alone);
        if (!P.unp_off || !P.unp_scores) return VGK_ENOMEM;
    }
    {
        Timed t(be, &ctx->pair_mapq_ms[1]);
        int rc = be->run_pair_scores(P);
        ctx->pair_mapq_launches[1] += n_cands ? 1 : 0;              // (a run_* call with nothing to do launches nothing)
        if (!rc) rc = launch_split(P, d_ids, plan, d_work, d_work_off, [&](const PmParams& L) { return be->run_pair_mapq(L); }, &ctx->pair_mapq_launches[1]);
        const int rs = t.done();                                    // (the staged host arrays may go)
        if (rc || rs) return rc ? rc : rs;
    }
    ctx->pair_mapq_pairs[0] = plan.n_lds - refused; ctx->pair_mapq_pairs[1] = plan.n_large; ctx->pair_mapq_pairs[2] = refused;
    int rc = be->download(out, P.out, sizeof(vgk_pair_mapq_result) * (uint64_t)n);
    if (!rc && n_cands) rc = be->download(pair_score, P.pair_score, sizeof(double) * n_cands);
    if (!rc && n_cands) rc = be->download(order, P.order, sizeof(uint32_t) * n_cands);
    return rc;
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }

}  // extern "C"
