// extension_anchors_api.cpp — vgk_extension_anchors (include/vgk_engine.h): the host half of making chaining anchors from seeds and gapless extensions
// on the device (extension_anchors_device.hpp).
//
// Per call: every size is taken from the caller's offsets in 64 bits and checked before anything is allocated; the extensions are checked on a few host
// threads (paths and mismatches inside their arrays, nodes inside the index, mismatches ascending inside the read interval) — the seeds are checked by
// the lanes that make their anchors; inputs go up in one copy each.  Three groups of kernels, timed apart: seed anchors + the diagonal sort | the
// extensions' seed lists (count, prefix sums, emit) | the order-dependent part with its sorts.  The anchors come back at their problems' slots (a
// problem has no more anchors than seeds) and are packed behind each other here.
#include <algorithm>
#include <vector>
#include "ctx.hpp"
#include "haplo.hpp"
#include "host_parallel.hpp"
#include "extension_anchors_device.hpp"

using namespace vgk;

extern "C" {

int vgk_extension_anchors_limits(uint32_t out[4]) {
    if (!out) return VGK_EINVAL;
    out[0] = EA_LDS_SEEDS; out[1] = 64; out[2] = EA_LDS_EXT; out[3] = 0;
    return VGK_OK;
}

int vgk_extension_anchors_last_ms(vgk_ctx* ctx, double ms[3]) {
    if (!ctx || !ms) return VGK_EINVAL;
    for (int k = 0; k < 3; ++k) ms[k] = ctx->extension_anchors_ms[k];
    return VGK_OK;
}

int vgk_extension_anchors(vgk_ctx* ctx, const vgk_haplo* index, int32_t match, int32_t mismatch, uint32_t flags, uint32_t default_max_extension_mismatches,
                          uint32_t n_problems, const uint64_t* seed_off, const vgk_anchor_seed* seeds,
                          const uint64_t* ext_off, const vgk_extension* extensions, const uint32_t* full_length,
                          const uint32_t* nodes, size_t n_nodes, const uint32_t* mismatches, size_t n_mismatches,
                          uint64_t* anchor_off, vgk_chain_anchor* anchors, vgk_anchor_origin* origins, size_t cap_anchors,
                          uint64_t* rep_off, uint32_t* represented, size_t cap_rep, uint32_t* status, size_t written[2]) try {
    const bool from_seeds = (flags & VGK_ANCHORS_FROM_SEEDS) != 0;
    if (!ctx || !index || !anchor_off || !rep_off || (flags & ~VGK_ANCHORS_FROM_SEEDS) || (n_problems && (!seed_off || !status || (!from_seeds && (!ext_off || !full_length))))) return VGK_EINVAL;
    if (ctx->has_qa) return VGK_EUNSUPPORTED;
    if (!vgk_tables_usable(index->ctx, ctx)) return VGK_EINVAL;
    if (match < 0 || mismatch < 0 || match > 1024 || mismatch > 1024) return VGK_EINVAL;
    anchor_off[0] = 0; rep_off[0] = 0;
    if (written) written[0] = written[1] = 0;
    if (!n_problems) return VGK_OK;
    // ---- sizes first, in 64 bits, from the offsets alone
    if (seed_off[0] != 0 || (!from_seeds && ext_off[0] != 0)) return VGK_EINVAL;
    uint64_t list_bound = 0;
    for (uint32_t p = 0; p < n_problems; ++p) {
        if (seed_off[p + 1] < seed_off[p] || (!from_seeds && ext_off[p + 1] < ext_off[p])) return VGK_EINVAL;
        const uint64_t ns = seed_off[p + 1] - seed_off[p], ne = from_seeds ? 0 : ext_off[p + 1] - ext_off[p];
        if (ns > INDEX_MOST || ne > INDEX_MOST) return VGK_ETOOBIG;
        list_bound += ns * ne;                                      // (an extension contains a seed once at most)
        if (list_bound > INDEX_MOST) return VGK_ETOOBIG;
    }
    const uint64_t n_seeds = seed_off[n_problems], n_ext = from_seeds ? 0 : ext_off[n_problems];
    if (n_seeds > INDEX_MOST || n_ext > INDEX_MOST || n_nodes > INDEX_MOST || n_mismatches > INDEX_MOST || n_seeds + n_ext > INDEX_MOST) return VGK_ETOOBIG;
    if ((n_seeds && !seeds) || (n_ext && (!extensions || !nodes)) || (n_mismatches && !mismatches)) return VGK_EINVAL;
    // ---- the problems; the extensions checked
    std::vector<EaProb> probs(n_problems); std::vector<uint32_t> prob_of_ext(std::max<uint64_t>(n_ext, 1)); std::vector<uint8_t> bad(n_problems, 0);
    const uint32_t n_oriented = index->n_oriented; const std::vector<uint32_t>& len = index->len;
    parallel_for(n_problems, [&](uint32_t p, unsigned) {
        EaProb& q = probs[p];
        q.s_off = seed_off[p]; q.n_seeds = (uint32_t)(seed_off[p + 1] - seed_off[p]); q.e_off = from_seeds ? 0 : ext_off[p]; q.n_ext = from_seeds ? 0u : (uint32_t)(ext_off[p + 1] - ext_off[p]);
        q.full_length = from_seeds ? 0u : full_length[p]; q.pad = 0;
        bool ok = true;
        for (uint32_t x = 0; x < q.n_ext && ok; ++x) {
            const vgk_extension& e = extensions[q.e_off + x];
            prob_of_ext[q.e_off + x] = p;
            if (!e.path_len || (uint64_t)e.path_begin + e.path_len > n_nodes || (uint64_t)e.mism_begin + e.n_mismatches > n_mismatches || e.read_begin >= e.read_end || e.read_end > 0x40000000u) { ok = false; break; }
            for (uint32_t i = 0; i < e.path_len; ++i) if (nodes[e.path_begin + i] >= n_oriented) ok = false;
            if (!ok || e.offset >= len[nodes[e.path_begin]]) { ok = false; break; }
            for (uint32_t i = 0; i < e.n_mismatches; ++i) {
                const uint32_t m = mismatches[e.mism_begin + i];
                if (m < e.read_begin || m >= e.read_end || (i && m <= mismatches[e.mism_begin + i - 1])) ok = false;
            }
        }
        bad[p] = ok ? 0 : 1;
    });
    for (uint32_t p = 0; p < n_problems; ++p) if (bad[p]) return VGK_EINVAL;
    // ---- the launches' problems: those whose working arrays fit LDS first, the others over slabs
    const SlabPlan plan = slab_plan(n_problems, [&](uint32_t p) { return probs[p].n_seeds <= EA_LDS_SEEDS && probs[p].n_ext <= EA_LDS_EXT ? ROUTE_LDS : ROUTE_SLAB; },
                                    [&](uint32_t p) { return std::max(probs[p].n_seeds, probs[p].n_ext); });
    if (plan.slab_largest > 0x80000000ull) return VGK_ETOOBIG;      // (the sorts' power of two would leave 32 bits)
    uint64_t slab_seeds = 0;                                       // the slab's second size: the most seeds of a large problem
    for (uint32_t j = 0; j < plan.n_large; ++j) slab_seeds = std::max<uint64_t>(slab_seeds, probs[plan.large()[j]].n_seeds);

    std::lock_guard<std::mutex> lock(ctx->mu);
    Backend* be = ctx->be.get();
    EaParams P{};
    P.match = match; P.mismatch = mismatch; P.from_seeds = from_seeds ? 1u : 0u; P.max_mismatches = default_max_extension_mismatches;
    P.n_problems = n_problems; P.n_oriented = n_oriented; P.n_seeds = n_seeds; P.n_ext = n_ext; P.node_tab = index->dev.node_tab;
    P.probs = ctx->scratch_dev<EaProb>(EANCH_PROBS, probs.data(), sizeof(EaProb) * n_problems);
    P.seeds = ctx->scratch_dev<vgk_anchor_seed>(EANCH_SEEDS, seeds, sizeof(vgk_anchor_seed) * n_seeds);
    P.ext = ctx->scratch_dev<vgk_extension>(EANCH_EXT, extensions, sizeof(vgk_extension) * n_ext);
    P.nodes = ctx->scratch_dev<uint32_t>(EANCH_NODES, nodes, n_ext ? sizeof(uint32_t) * n_nodes : 0);
    P.mism = ctx->scratch_dev<uint32_t>(EANCH_MISM, mismatches, n_ext ? sizeof(uint32_t) * n_mismatches : 0);
    P.prob_of_ext = ctx->scratch_dev<uint32_t>(EANCH_PROB_OF_EXT, prob_of_ext.data(), sizeof(uint32_t) * n_ext);
    const uint32_t* d_ids = ctx->scratch_dev<uint32_t>(EANCH_IDS, plan.ids.data(), sizeof(uint32_t) * plan.ids.size());
    P.seed_anchor = (vgk_chain_anchor*)ctx->ensure_scratch(EANCH_SEED_ANCHOR, sizeof(vgk_chain_anchor) * (n_seeds + 1));
    P.sorted = (uint32_t*)ctx->ensure_scratch(EANCH_SORTED, sizeof(uint32_t) * (n_seeds + 1));
    P.ext_count = (uint32_t*)ctx->ensure_scratch(EANCH_EXT_COUNT, sizeof(uint32_t) * (n_ext + 1));
    uint32_t* d_first = (uint32_t*)ctx->ensure_scratch(EANCH_EXT_FIRST, sizeof(uint32_t) * (n_ext + 1));
    P.ext_first = d_first;
    P.flags = (uint32_t*)ctx->ensure_scratch(EANCH_FLAGS, 16);
    P.made = (vgk_chain_anchor*)ctx->ensure_scratch(EANCH_MADE, sizeof(vgk_chain_anchor) * (n_seeds + 1));
    P.made_origin = (vgk_anchor_origin*)ctx->ensure_scratch(EANCH_MADE_ORIGIN, sizeof(vgk_anchor_origin) * (n_seeds + 1));
    P.anchors = (vgk_chain_anchor*)ctx->ensure_scratch(EANCH_ANCHORS, sizeof(vgk_chain_anchor) * (n_seeds + 1));
    P.origins = (vgk_anchor_origin*)ctx->ensure_scratch(EANCH_ORIGINS, sizeof(vgk_anchor_origin) * (n_seeds + 1));
    P.rep = (uint32_t*)ctx->ensure_scratch(EANCH_REP, sizeof(uint32_t) * (n_seeds + n_ext + 1));
    P.n_anchors = (uint32_t*)ctx->ensure_scratch(EANCH_N_ANCHORS, sizeof(uint32_t) * n_problems);
    P.n_rep = (uint32_t*)ctx->ensure_scratch(EANCH_N_REP, sizeof(uint32_t) * n_problems);
    P.status = (uint32_t*)ctx->ensure_scratch(EANCH_STATUS, sizeof(uint32_t) * n_problems);
    if (!P.probs || !P.seeds || !P.ext || !P.nodes || !P.mism || !P.prob_of_ext || !d_ids || !P.seed_anchor || !P.sorted || !P.ext_count || !d_first || !P.flags || !P.made || !P.made_origin
        || !P.anchors || !P.origins || !P.rep || !P.n_anchors || !P.n_rep || !P.status) return VGK_ENOMEM;
    uint32_t blocks = 0; char* slab = nullptr;
    if (plan.n_large) {
        P.slab_np = (uint32_t)pow2_at_least(plan.slab_largest); P.slab_seeds = (uint32_t)slab_seeds; P.slab_stride = ea_work_bytes(P.slab_np, slab_seeds);
        blocks = slab_blocks(plan.n_large, P.slab_stride);
        slab = (char*)ctx->ensure_scratch(EANCH_SLAB, P.slab_stride * blocks);
        if (!slab) return VGK_ENOMEM;
    }
    P.lds_np = (uint32_t)pow2_at_least(plan.lds_largest);
    int rc = be->zero(P.flags, 16);
    if (!rc) rc = be->zero(P.ext_count, sizeof(uint32_t) * (n_ext + 1));
    if (rc) return rc;
    auto per_problem = [&](int what) { return launch_split(P, d_ids, plan, slab, blocks, [&](const EaParams& L, uint32_t grid) { return be->run_extension_anchors(L, what, grid); }); };
    for (int k = 0; k < 3; ++k) ctx->extension_anchors_ms[k] = 0;
    // ---- every seed's anchor, every problem's seeds in diagonal order
    {
        Timed t(be, &ctx->extension_anchors_ms[0]);
        rc = n_seeds ? be->run_extension_anchors(P, EA_RUN_SEEDS, 0) : VGK_OK;
        if (!rc && n_ext && n_seeds) rc = per_problem(EA_RUN_SORT);
        const int rs = t.done();                                    // (the staged host arrays may go)
        if (rc || rs) return rc ? rc : rs;
    }
    uint32_t dev_flags = 0;
    if ((rc = be->download(&dev_flags, P.flags, sizeof dev_flags))) return rc;
    if (dev_flags) return VGK_EINVAL;                               // a malformed seed
    // ---- the seeds every extension contains
    if (n_ext) {
        Timed t(be, &ctx->extension_anchors_ms[1]);
        rc = be->run_extension_anchors(P, EA_RUN_COUNT, 0);
        if (!rc) rc = be->scan_u32(P.ext_count, d_first, (uint32_t)(n_ext + 1));
        int rs = t.done();
        if (rc || rs) return rc ? rc : rs;
        uint32_t total = 0;
        if ((rc = be->download(&total, d_first + n_ext, sizeof total))) return rc;
        P.ext_seeds = (uint32_t*)ctx->ensure_scratch(EANCH_EXT_SEEDS, sizeof(uint32_t) * ((uint64_t)total + 1));
        if (!P.ext_seeds) return VGK_ENOMEM;
        double emit_ms = 0;
        Timed u(be, &emit_ms);
        rc = be->run_extension_anchors(P, EA_RUN_EMIT, 0);
        rs = u.done();
        if (rc || rs) return rc ? rc : rs;
        ctx->extension_anchors_ms[1] += emit_ms;
    }
    // ---- the order-dependent part: a wavefront per problem
    {
        Timed t(be, &ctx->extension_anchors_ms[2]);
        rc = per_problem(EA_RUN_ANCHORS);
        const int rs = t.done();
        if (rc || rs) return rc ? rc : rs;
    }
    // ---- down: the counts, then the anchors from their slots, packed
    std::vector<uint32_t> n_anchors(n_problems), n_rep(n_problems);
    if ((rc = be->download(n_anchors.data(), P.n_anchors, sizeof(uint32_t) * n_problems))) return rc;
    if ((rc = be->download(n_rep.data(), P.n_rep, sizeof(uint32_t) * n_problems))) return rc;
    uint64_t total_anchors = 0, total_rep = 0;
    for (uint32_t p = 0; p < n_problems; ++p) {
        if (n_anchors[p] > probs[p].n_seeds || n_rep[p] > (uint64_t)probs[p].n_seeds + probs[p].n_ext) return VGK_ENODEV;      // (what no kernel of this file writes)
        total_anchors += n_anchors[p]; total_rep += n_rep[p];
    }
    if (written) { written[0] = total_anchors; written[1] = total_rep; }
    if (total_anchors > cap_anchors || total_rep > cap_rep) return VGK_EOPS;
    if ((total_anchors && (!anchors || !origins)) || (total_rep && !represented)) return VGK_EINVAL;
    if ((rc = be->download(status, P.status, sizeof(uint32_t) * n_problems))) return rc;
    std::vector<vgk_chain_anchor> slot_anchors(n_seeds + 1); std::vector<vgk_anchor_origin> slot_origins(n_seeds + 1); std::vector<uint32_t> slot_rep(n_seeds + n_ext + 1);
    if (total_anchors) {
        if ((rc = be->download(slot_anchors.data(), P.anchors, sizeof(vgk_chain_anchor) * n_seeds))) return rc;
        if ((rc = be->download(slot_origins.data(), P.origins, sizeof(vgk_anchor_origin) * n_seeds))) return rc;
    }
    if (total_rep && (rc = be->download(slot_rep.data(), P.rep, sizeof(uint32_t) * (n_seeds + n_ext)))) return rc;
    uint64_t at = 0, rep_at = 0;
    for (uint32_t p = 0; p < n_problems; ++p) {
        anchor_off[p] = at; rep_off[p] = rep_at;
        const EaProb& q = probs[p];
        std::copy(slot_rep.begin() + (q.s_off + q.e_off), slot_rep.begin() + (q.s_off + q.e_off + n_rep[p]), represented + rep_at);
        for (uint32_t k = 0; k < n_anchors[p]; ++k) {
            anchors[at] = slot_anchors[q.s_off + k]; origins[at] = slot_origins[q.s_off + k];
            origins[at].rep_begin += (uint32_t)rep_at;
            ++at;
        }
        rep_at += n_rep[p];
    }
    anchor_off[n_problems] = at; rep_off[n_problems] = rep_at;
    return VGK_OK;
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }

}  // extern "C"
