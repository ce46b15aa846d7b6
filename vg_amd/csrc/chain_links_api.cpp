// chain_links_api.cpp — vgk_chain_links (include/vgk_engine.h): the host half of a chain's links on the device (chain_links_device.hpp).
//
// Per call: the call's own checks and every bound in 64 bits on the host (cl_plan_call: one pass over the chains, which also lays their item slots
// out), VGK_ETOOBIG before anything is allocated; inputs go up in one copy each.  Then the checks that need no walk (a lane per item slot and per
// distance entry), the walk (a lane per chain), the three counts of every link slot with their 64-bit totals — which come down and are held against
// the caller's room — three prefix sums, the write-out (a lane per link slot) and the sequences (a wavefront per link).  Everything comes back in
// one copy per array.
#include <vector>
#include "ctx.hpp"
#include "chain_links_device.hpp"

using namespace vgk;

extern "C" {

int vgk_chain_links_last_ms(vgk_ctx* ctx, double ms[3]) {
    if (!ctx || !ms) return VGK_EINVAL;
    for (int k = 0; k < 3; ++k) ms[k] = ctx->chain_links_ms[k];
    return VGK_OK;
}

int vgk_chain_links(vgk_ctx* ctx, const vgk_chain_links_scheme* scheme, uint32_t n_reads, const char* reads, const uint64_t* read_off,
                    uint32_t n_sets, const uint64_t* anchor_off, const vgk_chain_anchor* anchors, const vgk_chain_site* sites,
                    const uint32_t* items, size_t n_items, const uint64_t* dist_off, const vgk_chain_candidate* dist,
                    uint32_t n_chains, const vgk_chain_problem* chains,
                    vgk_chain_links_result* results, vgk_chain_link* links, size_t link_cap, uint32_t* kept, size_t kept_cap,
                    char* seqs, uint64_t* seq_off, size_t seq_cap, size_t written[3]) try {
    if (written) written[0] = written[1] = written[2] = 0;
    if (!ctx || !scheme || (n_reads && !read_off) || (n_sets && (!anchor_off || !dist_off)) || (n_chains && (!chains || !results)) || (n_items && !items)
        || (link_cap && !links) || (kept_cap && !kept) || (seqs && !seq_off)) return VGK_EINVAL;
    if (ctx->has_qa) return VGK_EUNSUPPORTED;
    for (int k = 0; k < 3; ++k) ctx->chain_links_ms[k] = 0;
    if (!n_chains) return VGK_OK;
    std::vector<uint32_t> slot_off((size_t)n_chains + 1);
    std::vector<vgk_chain_links_result> res0(n_chains, vgk_chain_links_result{});
    std::vector<int32_t> status(n_chains);
    uint64_t bound[3];
    int rc = cl_plan_call(n_reads, read_off, n_sets, anchor_off, n_items, dist_off, n_chains, chains, INDEX_MOST, slot_off.data(), status.data(), bound);
    if (rc) return rc;
    for (uint32_t c = 0; c < n_chains; ++c) res0[c].status = status[c];
    const uint64_t n_anchors = anchor_off[n_sets], n_dist = dist_off[n_sets], read_bytes = read_off[n_reads];
    if ((n_anchors && (!anchors || !sites)) || (n_dist && !dist) || (read_bytes && seqs && !reads)) return VGK_EINVAL;

    Backend* be = ctx->be.get();
    std::lock_guard<std::mutex> lock(ctx->mu);
    ClParams P{};
    P.sch = *scheme; P.n_reads = n_reads; P.n_sets = n_sets; P.n_chains = n_chains; P.n_slots = slot_off[n_chains]; P.n_dist = n_dist;
    const uint64_t LS = bound[0], LS1 = LS + 1;
    P.read_off = ctx->scratch_dev<uint64_t>(CHAINLINKS_READ_OFF, read_off, sizeof(uint64_t) * ((uint64_t)n_reads + 1));
    P.reads = seqs ? ctx->scratch_dev<char>(CHAINLINKS_READS, reads, read_bytes) : nullptr;
    P.anchor_off = ctx->scratch_dev<uint64_t>(CHAINLINKS_ANCHOR_OFF, anchor_off, sizeof(uint64_t) * ((uint64_t)n_sets + 1));
    P.anchors = ctx->scratch_dev<vgk_chain_anchor>(CHAINLINKS_ANCHORS, anchors, sizeof(vgk_chain_anchor) * n_anchors);
    P.sites = ctx->scratch_dev<vgk_chain_site>(CHAINLINKS_SITES, sites, sizeof(vgk_chain_site) * n_anchors);
    P.items = ctx->scratch_dev<uint32_t>(CHAINLINKS_ITEMS, items, sizeof(uint32_t) * (uint64_t)n_items);
    P.dist_off = ctx->scratch_dev<uint64_t>(CHAINLINKS_DIST_OFF, dist_off, sizeof(uint64_t) * ((uint64_t)n_sets + 1));
    P.dist = ctx->scratch_dev<vgk_chain_candidate>(CHAINLINKS_DIST, dist, sizeof(vgk_chain_candidate) * n_dist);
    P.chains = ctx->scratch_dev<vgk_chain_problem>(CHAINLINKS_CHAINS, chains, sizeof(vgk_chain_problem) * (uint64_t)n_chains);
    P.slot_off = ctx->scratch_dev<uint32_t>(CHAINLINKS_SLOT_OFF, slot_off.data(), sizeof(uint32_t) * ((uint64_t)n_chains + 1));
    P.res = ctx->scratch_dev<vgk_chain_links_result>(CHAINLINKS_RES, res0.data(), sizeof(vgk_chain_links_result) * (uint64_t)n_chains);
    const uint64_t n_bytes = (uint64_t)n_sets + P.n_slots + LS;                     // set verdicts | kept bytes | route bytes
    uint8_t* d_bytes = (uint8_t*)ctx->ensure_scratch(CHAINLINKS_BYTES, n_bytes + 16);
    P.cnt = (uint32_t*)ctx->ensure_scratch(CHAINLINKS_COUNT, sizeof(uint32_t) * 3 * LS1);
    P.first = (uint32_t*)ctx->ensure_scratch(CHAINLINKS_FIRST, sizeof(uint32_t) * 3 * LS1);
    P.totals = (unsigned long long*)ctx->ensure_scratch(CHAINLINKS_TOTALS, 32);
    if (!P.read_off || (seqs && !P.reads) || !P.anchor_off || !P.anchors || !P.sites || !P.items || !P.dist_off || !P.dist || !P.chains || !P.slot_off || !P.res || !d_bytes
        || !P.cnt || !P.first || !P.totals) return VGK_ENOMEM;
    P.set_bad = d_bytes; P.keep = d_bytes + n_sets; P.route = P.keep + P.n_slots;
    {
        Timed t(be, &ctx->chain_links_ms[0]);
        rc = be->zero(d_bytes, n_bytes);
        if (!rc) rc = be->zero(P.totals, 32);
        if (!rc) rc = be->run_chain_links(P, CL_RUN_CHECK);
        if (!rc) rc = be->run_chain_links(P, CL_RUN_WALK);
        const int rs = t.done();                                    // (the staged host arrays may go)
        if (rc || rs) return rc ? rc : rs;
    }
    unsigned long long totals[3] = {0, 0, 0};
    {
        Timed t(be, &ctx->chain_links_ms[1]);
        for (int k = 0; k < 3 && !rc; ++k) rc = be->zero(P.cnt + (k + 1) * LS1 - 1, sizeof(uint32_t));      // (the entry behind the last link slot)
        if (!rc) rc = be->run_chain_links(P, CL_RUN_COUNT);
        const int rs = t.done();
        if (rc || rs) return rc ? rc : rs;
    }
    if ((rc = be->download(totals, P.totals, sizeof totals))) return rc;
    // (the totals are sums over slots inside the bounds above: they fit 32 bits, and so do the prefix sums below)
    if (totals[0] > bound[0] || totals[1] > bound[1] || totals[2] > bound[2]) return VGK_EINVAL;
    if (written) { written[0] = totals[0]; written[1] = totals[1]; written[2] = totals[2]; }
    if (totals[0] > link_cap || totals[1] > kept_cap || (seqs && totals[2] > seq_cap)) return VGK_EOPS;
    P.links = (vgk_chain_link*)ctx->ensure_scratch(CHAINLINKS_LINKS, sizeof(vgk_chain_link) * (totals[0] + 1));
    P.kept = (uint32_t*)ctx->ensure_scratch(CHAINLINKS_KEPT, sizeof(uint32_t) * (totals[1] + 1));
    P.seq_off = seqs ? (uint64_t*)ctx->ensure_scratch(CHAINLINKS_SEQ_OFF, sizeof(uint64_t) * (totals[0] + 2)) : nullptr;
    P.seqs = seqs ? (char*)ctx->ensure_scratch(CHAINLINKS_SEQS, totals[2] + 16) : nullptr;
    if (!P.links || !P.kept || (seqs && (!P.seq_off || !P.seqs))) return VGK_ENOMEM;
    P.n_links = (uint32_t)totals[0];
    {
        Timed t(be, &ctx->chain_links_ms[1]);
        for (int k = 0; k < 3 && !rc; ++k) rc = be->scan_u32(P.cnt + k * LS1, P.first + k * LS1, (uint32_t)LS1);
        if (!rc) rc = be->run_chain_links(P, CL_RUN_WRITE);
        const int rs = t.done();
        if (rc || rs) return rc ? rc : rs;
    }
    if (seqs) {
        Timed t(be, &ctx->chain_links_ms[2]);
        rc = be->run_chain_links(P, CL_RUN_SEQS);
        const int rs = t.done();
        if (rc || rs) return rc ? rc : rs;
    }
    if ((rc = be->download(results, P.res, sizeof(vgk_chain_links_result) * (uint64_t)n_chains))) return rc;
    if (totals[0] && (rc = be->download(links, P.links, sizeof(vgk_chain_link) * totals[0]))) return rc;
    if (totals[1] && (rc = be->download(kept, P.kept, sizeof(uint32_t) * totals[1]))) return rc;
    if (seqs) {
        if ((rc = be->download(seq_off, P.seq_off, sizeof(uint64_t) * (totals[0] + 1)))) return rc;
        if (totals[2] && (rc = be->download(seqs, P.seqs, totals[2]))) return rc;
    }
    return VGK_OK;
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }      // (no exception leaves the C ABI)

}  // extern "C"
