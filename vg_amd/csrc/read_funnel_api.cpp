// read_funnel_api.cpp — vgk_funnel_clusters, vgk_funnel_extension_sets and vgk_funnel_winners (include/vgk_engine.h): the host half of a short read's
// funnel on the device (read_funnel_device.hpp).
//
// Per call: every size is taken from the caller's offsets in 64 bits and checked before anything is allocated; every read is checked on a few host
// threads and a read that fails keeps its verdict as its status — its lanes write zeroes and touch no slice; inputs go up in one copy each.  The
// scoring launches a lane per cluster or set, the walk a lane per read, each as a launch_split pair: the items whose working words fit a lane's LDS
// slice, then the others over a slab.  A walk leaves its accepted items at the read's first item and their number; prefix sums and a gather lay
// them out, as vgk_read_alignments lays its alignments out.
#include <algorithm>
#include <vector>
#include "ctx.hpp"
#include "host_parallel.hpp"
#include "read_funnel_device.hpp"

using namespace vgk;

namespace {

// one launch pair over a plan's items, P.what set by the caller
int funnel_launch(vgk_ctx* ctx, FnParams P, const SlicePlan& plan, Slot ids_slot, Slot off_slot, Slot work_slot) {
    const uint32_t* d_ids = ctx->scratch_dev<uint32_t>(ids_slot, plan.ids.data(), sizeof(uint32_t) * plan.ids.size());
    const uint64_t* d_work_off = ctx->scratch_dev<uint64_t>(off_slot, plan.work_off.data(), sizeof(uint64_t) * plan.work_off.size());
    uint32_t* d_work = (uint32_t*)ctx->ensure_scratch(work_slot, sizeof(uint32_t) * (plan.work_words + 4));
    if (!d_ids || !d_work_off || !d_work) return VGK_ENOMEM;
    Backend* be = ctx->be.get();
    return launch_split(P, d_ids, plan, d_work, d_work_off, [&](const FnParams& L) { return be->run_funnel(L); });
}

// what a walk accepted, laid out: off[] from the counts' prefix sums, then — when `cap` holds them — `arrays` gathers of `words[a]` words per element
// from src[a] (at src_off[r] per read) into dst[a]
int funnel_lay_out(vgk_ctx* ctx, FnParams P, double* ms, uint32_t n, const uint64_t* d_src_off, uint64_t* off, size_t cap, size_t* written, int arrays,
                   const uint32_t* const* src, void* const* dst, const uint32_t* words) {
    Backend* be = ctx->be.get();
    uint32_t* d_first = (uint32_t*)ctx->ensure_scratch(FUNNEL_FIRST, sizeof(uint32_t) * ((uint64_t)n + 2));
    if (!d_first) return VGK_ENOMEM;
    int rc;
    {
        Timed t(be, ms);
        rc = be->scan_u32(P.count, d_first, n + 1);
        const int rs = t.done();
        if (rc || rs) return rc ? rc : rs;
    }
    std::vector<uint32_t> first((size_t)n + 1);
    if ((rc = be->download(first.data(), d_first, sizeof(uint32_t) * ((uint64_t)n + 1)))) return rc;
    for (uint32_t r = 0; r <= n; ++r) off[r] = first[r];
    const uint32_t total = first[n];
    if (written) written[0] = total;
    if (total > cap) return VGK_EOPS;
    if (!total) return VGK_OK;
    const Slot out_slot[2] = {FUNNEL_OUT0, FUNNEL_OUT1};
    for (int a = 0; a < arrays; ++a) {
        if (!dst[a]) return VGK_EINVAL;
        uint32_t* d_out = (uint32_t*)ctx->ensure_scratch(out_slot[a], sizeof(uint32_t) * words[a] * ((uint64_t)total + 1));
        if (!d_out) return VGK_ENOMEM;
        P.what = FN_RUN_GATHER; P.src_off = d_src_off; P.first = d_first; P.src = src[a]; P.dst = d_out; P.gather_words = words[a];
        Timed t(be, ms);
        rc = be->run_funnel(P);
        const int rs = t.done();
        if (rc || rs) return rc ? rc : rs;
        if ((rc = be->download(dst[a], d_out, sizeof(uint32_t) * words[a] * (uint64_t)total))) return rc;
    }
    return VGK_OK;
}

// the reads, their offsets and generators, the verdicts: what all three calls put up first
int funnel_stage_reads(vgk_ctx* ctx, FnParams& P, uint32_t n, const char* reads, const uint64_t* read_off, const uint32_t* rng_state, const int32_t* status) {
    P.n_reads = n;
    P.read_off = ctx->scratch_dev<uint64_t>(FUNNEL_READ_OFF, read_off, sizeof(uint64_t) * ((uint64_t)n + 1));
    if (!P.read_off) return VGK_ENOMEM;
    if (rng_state) {
        P.reads = ctx->scratch_dev<char>(FUNNEL_READS, reads, read_off[n]);
        P.rng_state = ctx->scratch_dev<uint32_t>(FUNNEL_RNG, rng_state, sizeof(uint32_t) * (uint64_t)n);
        if (!P.reads || !P.rng_state) return VGK_ENOMEM;
    }
    if (status && !(P.status = ctx->scratch_dev<int32_t>(FUNNEL_STATUS, status, sizeof(int32_t) * (uint64_t)n))) return VGK_ENOMEM;
    P.count = (uint32_t*)ctx->ensure_scratch(FUNNEL_COUNT, sizeof(uint32_t) * ((uint64_t)n + 2));
    if (!P.count) return VGK_ENOMEM;
    return ctx->be->zero(P.count, sizeof(uint32_t) * ((uint64_t)n + 2));
}

void funnel_count_reads(vgk_ctx* ctx, uint32_t n, const int32_t* status, const std::vector<uint8_t>& over_slab) {
    uint64_t refused = 0, slab = 0;
    for (uint32_t r = 0; r < n; ++r) { if (status && status[r] != VGK_OK) ++refused; else if (over_slab[r]) ++slab; }
    ctx->funnel_reads[0] = n - refused - slab; ctx->funnel_reads[1] = slab; ctx->funnel_reads[2] = refused;
}

}  // namespace

extern "C" {

int vgk_funnel_limits(uint32_t out[4]) {
    if (!out) return VGK_EINVAL;
    out[0] = FN_LDS_MINIMIZERS; out[1] = FN_LDS_BASES; out[2] = FN_LDS_ITEMS; out[3] = FN_LDS_EXT;
    return VGK_OK;
}

int vgk_funnel_last_ms(vgk_ctx* ctx, double ms[3]) {
    if (!ctx || !ms) return VGK_EINVAL;
    for (int k = 0; k < 3; ++k) ms[k] = ctx->funnel_ms[k];
    return VGK_OK;
}

int vgk_funnel_last_launches(vgk_ctx* ctx, uint64_t reads[3]) {
    if (!ctx || !reads) return VGK_EINVAL;
    for (int k = 0; k < 3; ++k) reads[k] = ctx->funnel_reads[k];
    return VGK_OK;
}

int vgk_funnel_clusters(vgk_ctx* ctx, const vgk_funnel_policy* policy, uint32_t n, const char* reads, const uint64_t* read_off,
                        const uint64_t* minimizer_off, const vgk_read_minimizer* minimizers, const double* minimizer_score,
                        const uint64_t* cluster_off, const uint64_t* cluster_seed_off, const uint32_t* sources, uint32_t* rng_state,
                        vgk_funnel_cluster* clusters, int32_t* status, uint64_t* kept_off, uint32_t* kept, size_t kept_cap, size_t written[1]) try {
    if (!ctx || !kept_off || (n && (!read_off || !minimizer_off || !cluster_off || !cluster_seed_off || !status))) return VGK_EINVAL;
    ctx->funnel_ms[0] = 0;
    for (int k = 0; k < 3; ++k) ctx->funnel_reads[k] = 0;
    kept_off[0] = 0;
    if (written) written[0] = 0;
    int rc = rf_check_clusters_call(policy, n, reads, read_off, minimizer_off, cluster_off, cluster_seed_off, rng_state);
    if (rc || !n) return rc;
    const uint64_t n_min = minimizer_off[n], n_clusters = cluster_off[n], n_seeds = cluster_seed_off[n_clusters];
    if ((n_min && (!minimizers || !minimizer_score)) || (n_seeds && !sources) || (n_clusters && !clusters)) return VGK_EINVAL;
    // ---- every read checked, the two plans
    FnParams H{};                                                   // the host's view, for the checks
    H.pol = *policy; H.n_reads = n; H.read_off = read_off; H.min_off = minimizer_off; H.mins = minimizers; H.min_score = minimizer_score; H.cluster_off = cluster_off;
    H.cluster_seed_off = cluster_seed_off; H.sources = sources;
    std::vector<uint32_t> read_of(n_clusters); std::vector<uint8_t> over_slab(n, 0);
    parallel_for(n, [&](uint32_t r, unsigned) {
        status[r] = rf_validate_clusters_read(H, r);
        for (uint64_t c = cluster_off[r]; c < cluster_off[r + 1]; ++c) read_of[c] = r;
        const uint64_t C = cluster_off[r + 1] - cluster_off[r];
        over_slab[r] = C > FN_LDS_ITEMS || (C && fn_cluster_large(minimizer_off[r + 1] - minimizer_off[r], read_off[r + 1] - read_off[r]));
    });
    auto M = [&](uint32_t r) { return minimizer_off[r + 1] - minimizer_off[r]; };
    auto L = [&](uint32_t r) { return read_off[r + 1] - read_off[r]; };
    const SlicePlan score_plan = slice_plan((uint32_t)n_clusters, [&](uint32_t c) { const uint32_t r = read_of[c]; return status[r] == VGK_OK && fn_cluster_large(M(r), L(r)); },
                                            [&](uint32_t c) { const uint32_t r = read_of[c]; return fn_cluster_words(M(r), L(r)); });
    const SlicePlan walk_plan = slice_plan(n, [&](uint32_t r) { return status[r] == VGK_OK && cluster_off[r + 1] - cluster_off[r] > FN_LDS_ITEMS; },
                                           [&](uint32_t r) { return cluster_off[r + 1] - cluster_off[r]; });
    if (score_plan.rc || walk_plan.rc) return VGK_ETOOBIG;

    Backend* be = ctx->be.get();
    std::lock_guard<std::mutex> lock(ctx->mu);
    FnParams P{};
    P.pol = *policy;
    if ((rc = funnel_stage_reads(ctx, P, n, reads, read_off, rng_state, status))) return rc;
    P.min_off = ctx->scratch_dev<uint64_t>(FUNNEL_MIN_OFF, minimizer_off, sizeof(uint64_t) * ((uint64_t)n + 1));
    P.mins = ctx->scratch_dev<vgk_read_minimizer>(FUNNEL_MINS, minimizers, sizeof(vgk_read_minimizer) * n_min);
    P.min_score = ctx->scratch_dev<double>(FUNNEL_MIN_SCORE, minimizer_score, sizeof(double) * n_min);
    P.cluster_off = ctx->scratch_dev<uint64_t>(FUNNEL_CLUSTER_OFF, cluster_off, sizeof(uint64_t) * ((uint64_t)n + 1));
    P.cluster_seed_off = ctx->scratch_dev<uint64_t>(FUNNEL_SEED_OFF, cluster_seed_off, sizeof(uint64_t) * (n_clusters + 1));
    P.sources = ctx->scratch_dev<uint32_t>(FUNNEL_SOURCES, sources, sizeof(uint32_t) * n_seeds);
    P.clusters = (vgk_funnel_cluster*)ctx->ensure_scratch(FUNNEL_CLUSTERS, sizeof(vgk_funnel_cluster) * (n_clusters + 1));
    P.tmp = (uint32_t*)ctx->ensure_scratch(FUNNEL_TMP, sizeof(uint32_t) * (n_clusters + 1));
    if (!P.min_off || !P.mins || !P.min_score || !P.cluster_off || !P.cluster_seed_off || !P.sources || !P.clusters || !P.tmp) return VGK_ENOMEM;
    {
        Timed t(be, &ctx->funnel_ms[0]);
        P.what = FN_RUN_CLUSTER_SCORE;
        rc = funnel_launch(ctx, P, score_plan, FUNNEL_IDS, FUNNEL_WORK_OFF, FUNNEL_WORK);
        P.what = FN_RUN_CLUSTER_WALK;
        if (!rc) rc = funnel_launch(ctx, P, walk_plan, FUNNEL_WALK_IDS, FUNNEL_WALK_WORK_OFF, FUNNEL_WALK_WORK);
        const int rs = t.done();                                    // (the staged host arrays may go)
        if (rc || rs) return rc ? rc : rs;
    }
    funnel_count_reads(ctx, n, status, over_slab);
    if (n_clusters && (rc = be->download(clusters, P.clusters, sizeof(vgk_funnel_cluster) * n_clusters))) return rc;
    if (rng_state && (rc = be->download(rng_state, P.rng_state, sizeof(uint32_t) * (uint64_t)n))) return rc;
    const uint32_t* src[1] = {P.tmp}; void* dst[1] = {kept}; const uint32_t words[1] = {1};
    return funnel_lay_out(ctx, P, &ctx->funnel_ms[0], n, P.cluster_off, kept_off, kept_cap, written, 1, src, dst, words);
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }

int vgk_funnel_extension_sets(vgk_ctx* ctx, const vgk_funnel_policy* policy, uint32_t n, const char* reads, const uint64_t* read_off,
                              const uint64_t* set_off, const vgk_gapless_result* results, const vgk_extension* extensions, size_t n_extensions,
                              const uint64_t* kept_off, const uint32_t* kept, const uint64_t* cluster_seed_off, size_t n_clusters, const uint32_t* sources,
                              const uint64_t* minimizer_off, uint32_t* rng_state,
                              vgk_funnel_set* sets, int32_t* status, uint64_t* aligned_off, uint32_t* aligned, size_t aligned_cap, uint8_t* explored, size_t written[1]) try {
    if (!ctx || !aligned_off || (n && (!read_off || !set_off || !kept_off || !cluster_seed_off || !minimizer_off || !status))) return VGK_EINVAL;
    if (ctx->has_qa) return VGK_EUNSUPPORTED;
    ctx->funnel_ms[1] = 0;
    for (int k = 0; k < 3; ++k) ctx->funnel_reads[k] = 0;
    aligned_off[0] = 0;
    if (written) written[0] = 0;
    int rc = rf_check_sets_call(policy, n, reads, read_off, set_off, kept_off, cluster_seed_off, n_clusters, n_extensions, minimizer_off, rng_state);
    if (rc || !n) return rc;
    const uint64_t n_min = minimizer_off[n], n_sets = kept_off[n], n_seeds = cluster_seed_off[n_clusters];
    if ((n_sets && (!results || !kept || !sets)) || (n_extensions && !extensions) || (n_seeds && !sources) || (n_min && !explored)) return VGK_EINVAL;
    FnParams H{};
    H.pol = *policy; H.n_reads = n; H.read_off = read_off; H.min_off = minimizer_off; H.cluster_seed_off = cluster_seed_off; H.sources = sources; H.kept_off = kept_off;
    H.kept = kept; H.res = results; H.ext = extensions;
    std::vector<uint32_t> read_of(n_sets); std::vector<uint8_t> over_slab(n, 0);
    auto set_large = [&](uint64_t s) { return results[s].status == VGK_OK && results[s].n_ext > FN_LDS_EXT; };
    parallel_for(n, [&](uint32_t r, unsigned) {
        status[r] = rf_validate_sets_read(H, r, n_extensions, n_clusters);
        over_slab[r] = kept_off[r + 1] - kept_off[r] > FN_LDS_ITEMS;
        for (uint64_t s = kept_off[r]; s < kept_off[r + 1]; ++s) { read_of[s] = r; if (set_large(s)) over_slab[r] = 1; }
    });
    const SlicePlan score_plan = slice_plan((uint32_t)n_sets, [&](uint32_t s) { return status[read_of[s]] == VGK_OK && set_large(s); }, [&](uint32_t s) { return results[s].n_ext; });
    const SlicePlan walk_plan = slice_plan(n, [&](uint32_t r) { return status[r] == VGK_OK && kept_off[r + 1] - kept_off[r] > FN_LDS_ITEMS; },
                                           [&](uint32_t r) { return kept_off[r + 1] - kept_off[r]; });
    if (score_plan.rc || walk_plan.rc) return VGK_ETOOBIG;

    Backend* be = ctx->be.get();
    std::lock_guard<std::mutex> lock(ctx->mu);
    FnParams P{};
    P.pol = *policy; P.gap_open = ctx->sc.gap_open; P.gap_extend = ctx->sc.gap_extend;
    if ((rc = funnel_stage_reads(ctx, P, n, reads, read_off, rng_state, status))) return rc;
    P.min_off = ctx->scratch_dev<uint64_t>(FUNNEL_MIN_OFF, minimizer_off, sizeof(uint64_t) * ((uint64_t)n + 1));
    P.cluster_seed_off = ctx->scratch_dev<uint64_t>(FUNNEL_SEED_OFF, cluster_seed_off, sizeof(uint64_t) * ((uint64_t)n_clusters + 1));
    P.sources = ctx->scratch_dev<uint32_t>(FUNNEL_SOURCES, sources, sizeof(uint32_t) * n_seeds);
    P.kept_off = ctx->scratch_dev<uint64_t>(FUNNEL_KEPT_OFF, kept_off, sizeof(uint64_t) * ((uint64_t)n + 1));
    P.kept = ctx->scratch_dev<uint32_t>(FUNNEL_KEPT, kept, sizeof(uint32_t) * n_sets);
    P.res = ctx->scratch_dev<vgk_gapless_result>(FUNNEL_RES, results, sizeof(vgk_gapless_result) * n_sets);
    P.ext = ctx->scratch_dev<vgk_extension>(FUNNEL_EXT, extensions, sizeof(vgk_extension) * n_extensions);
    P.sets = (vgk_funnel_set*)ctx->ensure_scratch(FUNNEL_SETS, sizeof(vgk_funnel_set) * (n_sets + 1));
    P.explored = (uint8_t*)ctx->ensure_scratch(FUNNEL_EXPLORED, n_min + 16);
    P.tmp = (uint32_t*)ctx->ensure_scratch(FUNNEL_TMP, sizeof(uint32_t) * (n_sets + 1));
    if (!P.min_off || !P.cluster_seed_off || !P.sources || !P.kept_off || !P.kept || !P.res || !P.ext || !P.sets || !P.explored || !P.tmp) return VGK_ENOMEM;
    {
        Timed t(be, &ctx->funnel_ms[1]);
        P.what = FN_RUN_SET_ESTIMATE;
        rc = funnel_launch(ctx, P, score_plan, FUNNEL_IDS, FUNNEL_WORK_OFF, FUNNEL_WORK);
        P.what = FN_RUN_SET_WALK;
        if (!rc) rc = funnel_launch(ctx, P, walk_plan, FUNNEL_WALK_IDS, FUNNEL_WALK_WORK_OFF, FUNNEL_WALK_WORK);
        const int rs = t.done();
        if (rc || rs) return rc ? rc : rs;
    }
    funnel_count_reads(ctx, n, status, over_slab);
    if (n_sets && (rc = be->download(sets, P.sets, sizeof(vgk_funnel_set) * n_sets))) return rc;
    if (n_min && (rc = be->download(explored, P.explored, n_min))) return rc;
    if (rng_state && (rc = be->download(rng_state, P.rng_state, sizeof(uint32_t) * (uint64_t)n))) return rc;
    const uint32_t* src[1] = {P.tmp}; void* dst[1] = {aligned}; const uint32_t words[1] = {1};
    return funnel_lay_out(ctx, P, &ctx->funnel_ms[1], n, P.kept_off, aligned_off, aligned_cap, written, 1, src, dst, words);
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }

int vgk_funnel_winners(vgk_ctx* ctx, const vgk_funnel_policy* policy, uint32_t n, const char* reads, const uint64_t* read_off,
                       const uint64_t* aligned_off, const uint64_t* aln_off, const int32_t* aln_score, const uint32_t* aln_mappings, uint32_t* rng_state,
                       uint64_t* score_off, int32_t* scores, vgk_funnel_pick* reported, size_t score_cap, uint32_t* n_reported, uint8_t* unmapped, size_t written[1]) try {
    if (!ctx || !score_off || (n && (!read_off || !aligned_off || !aln_off || !n_reported || !unmapped))) return VGK_EINVAL;
    ctx->funnel_ms[2] = 0;
    for (int k = 0; k < 3; ++k) ctx->funnel_reads[k] = 0;
    score_off[0] = 0;
    if (written) written[0] = 0;
    int rc = rf_check_winners_call(policy, n, reads, read_off, aligned_off, aln_off, rng_state);
    if (rc || !n) return rc;
    const uint64_t n_aligned = aligned_off[n], n_aln = aln_off[n_aligned];
    if (n_aln && (!aln_score || !aln_mappings)) return VGK_EINVAL;
    std::vector<uint64_t> flat_off((size_t)n + 1, 0); std::vector<uint8_t> over_slab(n, 0);
    for (uint32_t r = 0; r < n; ++r) { const uint64_t most = rf_winner_bound(aligned_off, aln_off, r); flat_off[r + 1] = flat_off[r] + most; over_slab[r] = most > FN_LDS_ITEMS; }
    const uint64_t n_flat = flat_off[n];                           // (<= n_aln + n: the call's checks)
    const SlicePlan walk_plan = slice_plan(n, [&](uint32_t r) { return over_slab[r] != 0; }, [&](uint32_t r) { return flat_off[r + 1] - flat_off[r]; });
    if (walk_plan.rc) return VGK_ETOOBIG;

    Backend* be = ctx->be.get();
    std::lock_guard<std::mutex> lock(ctx->mu);
    FnParams P{};
    P.pol = *policy;
    if ((rc = funnel_stage_reads(ctx, P, n, reads, read_off, rng_state, nullptr))) return rc;
    P.aligned_off = ctx->scratch_dev<uint64_t>(FUNNEL_ALIGNED_OFF, aligned_off, sizeof(uint64_t) * ((uint64_t)n + 1));
    P.aln_off = ctx->scratch_dev<uint64_t>(FUNNEL_ALN_OFF, aln_off, sizeof(uint64_t) * (n_aligned + 1));
    P.aln_score = ctx->scratch_dev<int32_t>(FUNNEL_ALN_SCORE, aln_score, sizeof(int32_t) * n_aln);
    P.aln_mappings = ctx->scratch_dev<uint32_t>(FUNNEL_ALN_MAPPINGS, aln_mappings, sizeof(uint32_t) * n_aln);
    P.flat_off = ctx->scratch_dev<uint64_t>(FUNNEL_FLAT_OFF, flat_off.data(), sizeof(uint64_t) * ((uint64_t)n + 1));
    P.flat_score = (int32_t*)ctx->ensure_scratch(FUNNEL_FLAT_SCORE, sizeof(int32_t) * (n_flat + 1));
    P.flat_pick = (vgk_funnel_pick*)ctx->ensure_scratch(FUNNEL_FLAT_PICK, sizeof(vgk_funnel_pick) * (n_flat + 1));
    P.sorted_score = (int32_t*)ctx->ensure_scratch(FUNNEL_SORTED_SCORE, sizeof(int32_t) * (n_flat + 1));
    P.sorted_pick = (vgk_funnel_pick*)ctx->ensure_scratch(FUNNEL_SORTED_PICK, sizeof(vgk_funnel_pick) * (n_flat + 1));
    P.n_reported = (uint32_t*)ctx->ensure_scratch(FUNNEL_N_REPORTED, sizeof(uint32_t) * ((uint64_t)n + 1));
    P.unmapped = (uint8_t*)ctx->ensure_scratch(FUNNEL_UNMAPPED, (uint64_t)n + 16);
    if (!P.aligned_off || !P.aln_off || !P.aln_score || !P.aln_mappings || !P.flat_off || !P.flat_score || !P.flat_pick || !P.sorted_score || !P.sorted_pick || !P.n_reported
        || !P.unmapped) return VGK_ENOMEM;
    {
        Timed t(be, &ctx->funnel_ms[2]);
        P.what = FN_RUN_WINNER_WALK;
        rc = funnel_launch(ctx, P, walk_plan, FUNNEL_WALK_IDS, FUNNEL_WALK_WORK_OFF, FUNNEL_WALK_WORK);
        const int rs = t.done();
        if (rc || rs) return rc ? rc : rs;
    }
    funnel_count_reads(ctx, n, nullptr, over_slab);
    if ((rc = be->download(n_reported, P.n_reported, sizeof(uint32_t) * (uint64_t)n)) || (rc = be->download(unmapped, P.unmapped, n))) return rc;
    if (rng_state && (rc = be->download(rng_state, P.rng_state, sizeof(uint32_t) * (uint64_t)n))) return rc;
    const uint32_t* src[2] = {(const uint32_t*)P.sorted_score, (const uint32_t*)P.sorted_pick}; void* dst[2] = {scores, reported}; const uint32_t words[2] = {1, 2};
    return funnel_lay_out(ctx, P, &ctx->funnel_ms[2], n, P.flat_off, score_off, score_cap, written, 2, src, dst, words);
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }

}  // extern "C"
