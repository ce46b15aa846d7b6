// read_mapq_api.cpp — vgk_minimizer_regions and vgk_read_mapq (include/vgk_engine.h): the host half of a read's mapping quality on the device
// (read_mapq_device.hpp).
//
// Per call: every size is taken from the caller's offsets in 64 bits and checked before anything is allocated; every read is checked on a few host
// threads (mq_validate_read) and a read that fails keeps its verdict as its status — no lane sweeps it; inputs go up in one copy each.  The two
// probability tables are made once per context with the host shim's expressions and stay in HBM.  vgk_read_mapq launches twice: the reads whose
// explored minimizers fit a lane's LDS slice, then the others over a slab, so that no wavefront of the first launch waits on a long read.
#include <algorithm>
#include <cmath>
#include <vector>
#include "ctx.hpp"
#include "host_parallel.hpp"
#include "read_mapq_device.hpp"

using namespace vgk;

// once per context: the shim's own expressions, evaluated here (no pow on the device)
int vgk_ctx::ensure_mapq_tables() {
    if (mapq_tables) return VGK_OK;
    std::vector<double> tab(MQ_PHRED_ENTRIES + MQ_EVENT_ENTRIES);
    read_mapq_tables(tab.data(), tab.data() + MQ_PHRED_ENTRIES);
    if (!scratch_dev(READMAPQ_TABLES, tab.data(), sizeof(double) * tab.size())) return VGK_ENOMEM;
    const int rt = be->sync();                                      // (tab may go)
    if (rt) return rt;
    mapq_tables = true;
    return VGK_OK;
}

// the sweep of vgk_read_mapq and of vgk_pair_mapq's mates up to its launches (ctx.hpp)
int vgk_ctx::stage_mapq_sweep(const MqParams& H, bool sweep, int32_t (*validate)(const MqParams&, uint32_t), std::unique_lock<std::mutex>& lock, MapqSweep* s) {
    const uint32_t n = H.n_reads;
    const uint64_t n_min = H.min_off[n], n_bases = H.read_off[n];
    s->status.resize(n); std::vector<uint32_t> n_explored(n, 0);
    parallel_for(n, [&](uint32_t r, unsigned) {
        s->status[r] = validate(H, r);
        if (s->status[r] == VGK_OK && sweep) n_explored[r] = mq_count_explored(H, r);
    });
    s->plan = slice_plan(n, [&](uint32_t r) { return n_explored[r] > MQ_LDS_EXPLORED; }, [&](uint32_t r) { return mq_work_words(n_explored[r]); });
    if (s->plan.rc) return s->plan.rc;
    if (!lock.owns_lock()) lock.lock();
    const int rt = ensure_mapq_tables();
    if (rt) return rt;
    MqParams& P = s->P;
    P.k = H.k; P.flags = H.flags; P.n_reads = n;
    P.phred = (const double*)scratch[READMAPQ_TABLES].p; P.events = P.phred + MQ_PHRED_ENTRIES;
    P.min_off = scratch_dev<uint64_t>(READMAPQ_MIN_OFF, H.min_off, sizeof(uint64_t) * ((uint64_t)n + 1));
    P.read_off = scratch_dev<uint64_t>(READMAPQ_READ_OFF, H.read_off, sizeof(uint64_t) * ((uint64_t)n + 1));
    P.status = scratch_dev<int32_t>(READMAPQ_STATUS, s->status.data(), sizeof(int32_t) * (uint64_t)n);
    s->d_ids = scratch_dev<uint32_t>(READMAPQ_IDS, s->plan.ids.data(), sizeof(uint32_t) * s->plan.ids.size());
    s->d_work_off = scratch_dev<uint64_t>(READMAPQ_WORK_OFF, s->plan.work_off.data(), sizeof(uint64_t) * s->plan.work_off.size());
    s->d_work = (uint32_t*)ensure_scratch(READMAPQ_WORK, sizeof(uint32_t) * (s->plan.work_words + 4));
    if (!P.min_off || !P.read_off || !P.status || !s->d_ids || !s->d_work_off || !s->d_work) return VGK_ENOMEM;
    if (sweep) {
        P.mins = scratch_dev<vgk_read_minimizer>(READMAPQ_MINS, H.mins, sizeof(vgk_read_minimizer) * n_min);
        P.regions = scratch_dev<vgk_minimizer_region>(READMAPQ_REGIONS, H.regions, sizeof(vgk_minimizer_region) * n_min);
        P.explored = scratch_dev<uint8_t>(READMAPQ_EXPLORED, H.explored, n_min);
        P.qual = scratch_dev<uint8_t>(READMAPQ_QUAL, H.qual, n_bases);
        if (!P.mins || !P.regions || !P.explored || !P.qual) return VGK_ENOMEM;
    }
    return VGK_OK;
}

extern "C" {

int vgk_read_mapq_limits(uint32_t out[4]) {
    if (!out) return VGK_EINVAL;
    out[0] = MQ_LDS_EXPLORED; out[1] = 1; out[2] = 1; out[3] = 0;
    return VGK_OK;
}

int vgk_read_mapq_last_ms(vgk_ctx* ctx, double ms[2]) {
    if (!ctx || !ms) return VGK_EINVAL;
    ms[0] = ctx->read_mapq_ms[0]; ms[1] = ctx->read_mapq_ms[1];
    return VGK_OK;
}

int vgk_read_mapq_last_launches(vgk_ctx* ctx, uint64_t reads[3]) {
    if (!ctx || !reads) return VGK_EINVAL;
    for (int k = 0; k < 3; ++k) reads[k] = ctx->read_mapq_reads[k];
    return VGK_OK;
}

int vgk_minimizer_regions(vgk_ctx* ctx, uint32_t k, uint32_t w, const uint64_t* read_off, uint32_t n, const uint64_t* minimizer_off,
                          const vgk_read_minimizer* minimizers, vgk_minimizer_region* regions) try {
    if (!ctx || !k || k > MZ_MAX_K || !w || w > MZ_MAX_W || (n && (!read_off || !minimizer_off))) return VGK_EINVAL;
    ctx->read_mapq_ms[0] = 0;
    if (!n) return VGK_OK;
    // ---- sizes first, in 64 bits, from the offsets alone; then what vgk_minimizer_choose checks of a list
    if (read_off[0] != 0 || minimizer_off[0] != 0) return VGK_EINVAL;
    if (n > INDEX_MOST) return VGK_ETOOBIG;
    for (uint32_t r = 0; r < n; ++r) {
        if (read_off[r + 1] < read_off[r] || minimizer_off[r + 1] < minimizer_off[r]) return VGK_EINVAL;
        if (read_off[r + 1] - read_off[r] > 0x3fffffffull) return VGK_ETOOBIG;
    }
    const uint64_t total = minimizer_off[n];
    if (total > INDEX_MOST) return VGK_ETOOBIG;
    if (!total) return VGK_OK;
    if (!minimizers || !regions) return VGK_EINVAL;
    std::vector<uint8_t> bad(n, 0);
    parallel_for(n, [&](uint32_t r, unsigned) {
        const uint64_t L = read_off[r + 1] - read_off[r];
        if (minimizer_off[r + 1] > minimizer_off[r] && L + 1 < (uint64_t)k + w) { bad[r] = 1; return; }      // no complete window: no minimizers
        for (uint64_t j = minimizer_off[r]; j < minimizer_off[r + 1]; ++j)
            if ((uint64_t)minimizers[j].offset + k > L || (j > minimizer_off[r] && minimizers[j].offset < minimizers[j - 1].offset)) { bad[r] = 1; return; }
    });
    for (uint32_t r = 0; r < n; ++r) if (bad[r]) return VGK_EINVAL;

    Backend* be = ctx->be.get();
    std::lock_guard<std::mutex> lock(ctx->mu);
    MqRegionParams P{};
    P.k = k; P.w = w; P.n_reads = n; P.n_minimizers = total;
    P.read_off = ctx->scratch_dev<uint64_t>(READMAPQ_READ_OFF, read_off, sizeof(uint64_t) * ((uint64_t)n + 1));
    P.min_off = ctx->scratch_dev<uint64_t>(READMAPQ_MIN_OFF, minimizer_off, sizeof(uint64_t) * ((uint64_t)n + 1));
    P.mins = ctx->scratch_dev<vgk_read_minimizer>(READMAPQ_MINS, minimizers, sizeof(vgk_read_minimizer) * total);
    P.out = (vgk_minimizer_region*)ctx->ensure_scratch(READMAPQ_REGIONS, sizeof(vgk_minimizer_region) * total);
    if (!P.read_off || !P.min_off || !P.mins || !P.out) return VGK_ENOMEM;
    Timed t(be, &ctx->read_mapq_ms[0]);
    int rc = be->run_minimizer_regions(P);
    const int rs = t.done();
    if (rc || rs) return rc ? rc : rs;
    return be->download(regions, P.out, sizeof(vgk_minimizer_region) * total);
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }

int vgk_read_mapq(vgk_ctx* ctx, const vgk_read_mapq_scheme* scheme, uint32_t n, const uint64_t* score_off, const int32_t* scores, const double* multiplicity,
                  const uint8_t* unmapped, const uint64_t* minimizer_off, const vgk_read_minimizer* minimizers, const vgk_minimizer_region* regions,
                  const uint8_t* explored, const uint64_t* read_off, const uint8_t* quality, vgk_read_mapq_result* out) try {
    if (!ctx || !scheme || (scheme->flags & ~(uint32_t)(VGK_READ_MAPQ_FIRST | VGK_READ_MAPQ_NO_EXPLORED_CAP | VGK_READ_MAPQ_OWN_LENGTH))) return VGK_EINVAL;
    if (!(scheme->log_base > 0.0) || !(scheme->score_scale > 0.0) || std::isinf(scheme->log_base) || std::isinf(scheme->score_scale)) return VGK_EINVAL;
    if (n && (!score_off || !minimizer_off || !read_off || !out)) return VGK_EINVAL;
    ctx->read_mapq_ms[1] = 0;
    for (int k = 0; k < 3; ++k) ctx->read_mapq_reads[k] = 0;
    if (!n) return VGK_OK;
    // ---- sizes first, in 64 bits, from the offsets alone
    if (score_off[0] != 0 || minimizer_off[0] != 0 || read_off[0] != 0) return VGK_EINVAL;
    if (n > INDEX_MOST) return VGK_ETOOBIG;
    for (uint32_t r = 0; r < n; ++r) {
        if (score_off[r + 1] < score_off[r] || minimizer_off[r + 1] < minimizer_off[r] || read_off[r + 1] < read_off[r]) return VGK_EINVAL;
        if (read_off[r + 1] - read_off[r] > 0x3fffffffull || minimizer_off[r + 1] - minimizer_off[r] >= MQ_MAX_READ_MINIMIZERS) return VGK_ETOOBIG;
    }
    const uint64_t n_scores = score_off[n], n_min = minimizer_off[n], n_bases = read_off[n];
    if (n_scores > INDEX_MOST || n_min > INDEX_MOST || n_bases > INDEX_MOST) return VGK_ETOOBIG;
    const bool sweep = quality && !(scheme->flags & VGK_READ_MAPQ_NO_EXPLORED_CAP);
    if ((n_scores && !scores) || (sweep && n_min && (!minimizers || !regions || !explored))) return VGK_EINVAL;
    // ---- every read checked, the sweep staged; then what the scores' half reads besides
    MqParams H{};                                                   // the host's view, for the checks
    H.k = scheme->k; H.flags = scheme->flags; H.n_reads = n; H.score_off = score_off; H.unmapped = unmapped; H.min_off = minimizer_off; H.mins = minimizers;
    H.regions = regions; H.explored = explored; H.read_off = read_off; H.qual = quality;
    Backend* be = ctx->be.get();
    std::unique_lock<std::mutex> lock(ctx->mu, std::defer_lock);
    vgk_ctx::MapqSweep S;
    const int rt = ctx->stage_mapq_sweep(H, sweep, mq_validate_read, lock, &S);
    if (rt) return rt;
    MqParams& P = S.P;
    P.log_base = scheme->log_base; P.score_scale = scheme->score_scale; P.quality_scale = 10.0 / std::log(10.0); P.score_window = scheme->score_window;
    P.score_off = ctx->scratch_dev<uint64_t>(READMAPQ_SCORE_OFF, score_off, sizeof(uint64_t) * ((uint64_t)n + 1));
    P.scores = ctx->scratch_dev<int32_t>(READMAPQ_SCORES, scores, sizeof(int32_t) * n_scores);
    P.out = (vgk_read_mapq_result*)ctx->ensure_scratch(READMAPQ_OUT, sizeof(vgk_read_mapq_result) * (uint64_t)n);
    if (!P.score_off || !P.scores || !P.out) return VGK_ENOMEM;
    if (multiplicity && !(P.mult = ctx->scratch_dev<double>(READMAPQ_MULT, multiplicity, sizeof(double) * n_scores))) return VGK_ENOMEM;
    if (unmapped && !(P.unmapped = ctx->scratch_dev<uint8_t>(READMAPQ_UNMAPPED, unmapped, n))) return VGK_ENOMEM;
    {
        Timed t(be, &ctx->read_mapq_ms[1]);
        const int rc = launch_split(P, S.d_ids, S.plan, S.d_work, S.d_work_off, [&](const MqParams& L) { return be->run_read_mapq(L); });
        const int rs = t.done();                                    // (the staged host arrays may go)
        if (rc || rs) return rc ? rc : rs;
    }
    const uint64_t refused = (uint64_t)std::count_if(S.status.begin(), S.status.end(), [](int32_t v) { return v != VGK_OK; });
    ctx->read_mapq_reads[0] = S.plan.n_lds - refused; ctx->read_mapq_reads[1] = S.plan.n_large; ctx->read_mapq_reads[2] = refused;
    return be->download(out, P.out, sizeof(vgk_read_mapq_result) * (uint64_t)n);
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }

}  // extern "C"
