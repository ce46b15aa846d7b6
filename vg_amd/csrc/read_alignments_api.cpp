// read_alignments_api.cpp — vgk_read_alignments (include/vgk_engine.h): the host half of composing a short read's alignments from its extension set and
// its tails' alignments on the device (read_alignments_device.hpp).
//
// Per call: every size is taken from the caller's offsets in 64 bits and checked before anything is allocated; every read is checked on a few host
// threads (ra_validate_read: nothing a lane indexes with lies outside its array) and a read that fails keeps its verdict as the status of its one
// header — no lane walks its extensions; inputs go up in one copy each.  Three groups of kernels, timed apart: the selection (sets within
// RA_LDS_EXT in LDS, the others over a slab) | count with its prefix sums | emit.  The sizes are exact after the count, so the outputs are
// allocated once and come down in one copy each.
#include <algorithm>
#include <vector>
#include "ctx.hpp"
#include "haplo.hpp"
#include "host_parallel.hpp"
#include "read_alignments_device.hpp"

using namespace vgk;

// The kernels and the way back, for inputs that lie in HBM already (the caller holds ctx->mu): the explicit call's after its uploads, and the resident
// form's inside the tail stage (tail_api.cpp), whose sets, tails and ops never left the device.  d_ids: the reads of `split` (launch_split.hpp), the
// large sets' slices at d_work_off; nullptr: every read in one launch, a large set's slice by the extensions before it.
int vgk_read_alignments_run(vgk_ctx* ctx, RaParams& P, const uint32_t* d_ids, const LaunchSplit& split, uint32_t* d_work, const uint64_t* d_work_off, uint64_t out_bound,
                            uint64_t* aln_off, vgk_read_alignment* alignments, size_t cap_alignments, vgk_chain_mapping* mappings, size_t cap_mappings,
                            uint32_t* edits, size_t cap_edits, size_t written[3]) {
    Backend* be = ctx->be.get();
    const uint32_t n = P.n_reads;
    P.choice = (RaChoice*)ctx->ensure_scratch(READALN_CHOICE, sizeof(RaChoice) * (uint64_t)n);
    P.aln_count = (uint32_t*)ctx->ensure_scratch(READALN_ALN_COUNT, sizeof(uint32_t) * ((uint64_t)n + 1));
    uint32_t* d_aln_first = (uint32_t*)ctx->ensure_scratch(READALN_ALN_FIRST, sizeof(uint32_t) * ((uint64_t)n + 1));
    P.totals = (unsigned long long*)ctx->ensure_scratch(READALN_TOTALS, 16);
    P.aln_first = d_aln_first;
    if (!P.choice || !P.aln_count || !d_aln_first || !P.totals) return VGK_ENOMEM;
    for (int k = 0; k < 3; ++k) ctx->read_alignments_ms[k] = 0;
    int rc = be->zero(P.aln_count, sizeof(uint32_t) * ((uint64_t)n + 1));
    if (!rc) rc = be->zero(P.totals, 16);
    if (rc) return rc;
    // ---- which extensions: the small sets in LDS, the large ones over the slab
    {
        Timed t(be, &ctx->read_alignments_ms[0]);
        if (d_ids) rc = launch_split(P, d_ids, split, d_work, d_work_off, [&](const RaParams& L) { return be->run_read_alignments(L, RA_RUN_SELECT); });
        else { RaParams L = P; L.ids = nullptr; L.n = n; L.work = d_work; L.work_off = nullptr; rc = be->run_read_alignments(L, RA_RUN_SELECT); }
        const int rs = t.done();                                    // (the staged host arrays may go)
        if (rc || rs) return rc ? rc : rs;
    }
    // ---- the sizes: alignments per read, mappings and edit runs per alignment
    uint32_t n_aln = 0, totals[2] = {0, 0};
    {
        Timed t(be, &ctx->read_alignments_ms[1]);
        rc = be->scan_u32(P.aln_count, d_aln_first, n + 1);
        const int rs = t.done();
        if (rc || rs) return rc ? rc : rs;
        if ((rc = be->download(&n_aln, d_aln_first + n, sizeof n_aln))) return rc;
        if (n_aln > out_bound) return VGK_ENODEV;                   // (what no kernel of this file writes)
        P.map_count = (uint32_t*)ctx->ensure_scratch(READALN_MAP_COUNT, sizeof(uint32_t) * ((uint64_t)n_aln + 1));
        P.edit_count = (uint32_t*)ctx->ensure_scratch(READALN_EDIT_COUNT, sizeof(uint32_t) * ((uint64_t)n_aln + 1));
        uint32_t* d_map_first = (uint32_t*)ctx->ensure_scratch(READALN_MAP_FIRST, sizeof(uint32_t) * ((uint64_t)n_aln + 1));
        uint32_t* d_edit_first = (uint32_t*)ctx->ensure_scratch(READALN_EDIT_FIRST, sizeof(uint32_t) * ((uint64_t)n_aln + 1));
        P.map_first = d_map_first; P.edit_first = d_edit_first;
        if (!P.map_count || !P.edit_count || !d_map_first || !d_edit_first) return VGK_ENOMEM;
        if ((rc = be->zero(P.map_count + n_aln, sizeof(uint32_t))) || (rc = be->zero(P.edit_count + n_aln, sizeof(uint32_t)))) return rc;
        Timed u(be, &ctx->read_alignments_ms[1]);
        rc = be->run_read_alignments(P, RA_RUN_COUNT);
        if (!rc) rc = be->scan_u32(P.map_count, d_map_first, n_aln + 1);
        if (!rc) rc = be->scan_u32(P.edit_count, d_edit_first, n_aln + 1);
        const int ru = u.done();
        if (rc || ru) return rc ? rc : ru;
        if ((rc = be->download(&totals[0], d_map_first + n_aln, sizeof(uint32_t))) || (rc = be->download(&totals[1], d_edit_first + n_aln, sizeof(uint32_t)))) return rc;
        unsigned long long wide[2] = {0, 0};                        // the same sums in 64 bits: the prefix sums are 32-bit
        if ((rc = be->download(wide, P.totals, sizeof wide))) return rc;
        if (wide[0] > INDEX_MOST || wide[1] > INDEX_MOST) return VGK_ETOOBIG;
        if (wide[0] != totals[0] || wide[1] != totals[1] || totals[0] > out_bound || totals[1] > out_bound) return VGK_ENODEV;
    }
    if (written) { written[0] = n_aln; written[1] = totals[0]; written[2] = totals[1]; }
    if (n_aln > cap_alignments || totals[0] > cap_mappings || totals[1] > cap_edits) return VGK_EOPS;
    if ((n_aln && !alignments) || (totals[0] && !mappings) || (totals[1] && !edits)) return VGK_EINVAL;
    // ---- the alignments themselves, at their prefix sums
    P.out = (vgk_read_alignment*)ctx->ensure_scratch(READALN_OUT, sizeof(vgk_read_alignment) * ((uint64_t)n_aln + 1));
    P.mappings = (vgk_chain_mapping*)ctx->ensure_scratch(READALN_MAPPINGS, sizeof(vgk_chain_mapping) * ((uint64_t)totals[0] + 1));
    P.edits = (uint32_t*)ctx->ensure_scratch(READALN_EDITS, sizeof(uint32_t) * ((uint64_t)totals[1] + 1));
    if (!P.out || !P.mappings || !P.edits) return VGK_ENOMEM;
    {
        Timed t(be, &ctx->read_alignments_ms[2]);
        rc = be->run_read_alignments(P, RA_RUN_EMIT);
        const int rs = t.done();
        if (rc || rs) return rc ? rc : rs;
    }
    std::vector<uint32_t> first((size_t)n + 1);
    if ((rc = be->download(first.data(), d_aln_first, sizeof(uint32_t) * ((uint64_t)n + 1)))) return rc;
    for (uint32_t r = 0; r <= n; ++r) aln_off[r] = first[r];
    if (n_aln && (rc = be->download(alignments, P.out, sizeof(vgk_read_alignment) * (uint64_t)n_aln))) return rc;
    if (totals[0] && (rc = be->download(mappings, P.mappings, sizeof(vgk_chain_mapping) * (uint64_t)totals[0]))) return rc;
    if (totals[1] && (rc = be->download(edits, P.edits, sizeof(uint32_t) * (uint64_t)totals[1]))) return rc;
    return VGK_OK;
}

extern "C" {

int vgk_read_alignments_limits(uint32_t out[4]) {
    if (!out) return VGK_EINVAL;
    out[0] = RA_LDS_EXT; out[1] = 1; out[2] = 1; out[3] = 0;
    return VGK_OK;
}

int vgk_read_alignments_last_ms(vgk_ctx* ctx, double ms[3]) {
    if (!ctx || !ms) return VGK_EINVAL;
    for (int k = 0; k < 3; ++k) ms[k] = ctx->read_alignments_ms[k];
    return VGK_OK;
}

int vgk_read_alignments(vgk_ctx* ctx, const vgk_haplo* index, const vgk_read_alignments_policy* policy,
                        const char* reads, const uint64_t* read_off, uint32_t n, const vgk_gapless_result* results,
                        const vgk_extension* extensions, size_t n_extensions, const uint32_t* nodes, size_t n_nodes, const uint32_t* mismatches, size_t n_mismatches,
                        const vgk_tail_alignment* tails, size_t n_tails, const vgk_op* ops, size_t n_ops,
                        uint64_t* aln_off, vgk_read_alignment* alignments, size_t cap_alignments,
                        vgk_chain_mapping* mappings, size_t cap_mappings, uint32_t* edits, size_t cap_edits, size_t written[3]) try {
    if (!ctx || !index || !policy || !aln_off || policy->flags || !policy->window_length || (n && (!read_off || !results))) return VGK_EINVAL;
    if (ctx->has_qa) return VGK_EUNSUPPORTED;
    if (!vgk_tables_usable(index->ctx, ctx)) return VGK_EINVAL;
    aln_off[0] = 0;
    if (written) written[0] = written[1] = written[2] = 0;
    if (!n) return VGK_OK;
    // ---- sizes first, in 64 bits, from the offsets alone
    if (read_off[0] != 0) return VGK_EINVAL;
    if (n > INDEX_MOST) return VGK_ETOOBIG;
    for (uint32_t r = 0; r < n; ++r) {
        if (read_off[r + 1] < read_off[r]) return VGK_EINVAL;
        if (read_off[r + 1] - read_off[r] > 0x3fffffffull) return VGK_ETOOBIG;
    }
    const uint64_t read_bytes = read_off[n];
    if (read_bytes > INDEX_MOST || n_extensions > INDEX_MOST / 2 || n_nodes > INDEX_MOST || n_mismatches > INDEX_MOST || n_tails > INDEX_MOST - 2 || n_ops > INDEX_MOST) return VGK_ETOOBIG;
    if ((read_bytes && !reads) || (n_extensions && (!extensions || !nodes)) || (n_mismatches && !mismatches) || (n_tails && !tails) || (n_ops && !ops)) return VGK_EINVAL;
    std::vector<uint32_t> tail_of(2 * n_extensions + 2);
    if (!ra_tail_table(tails, n_tails, n_extensions, tail_of.data())) return VGK_EINVAL;
    // ---- every read checked; a bound on what the call can put out
    RaParams H{};                                                   // the host's view, for the checks
    H.n_reads = n; H.n_oriented = index->n_oriented; H.read_off = read_off; H.res = results; H.ext = extensions; H.nodes = nodes; H.mism = mismatches;
    H.tails = tails; H.ops = ops; H.tail_of = tail_of.data();
    std::vector<uint64_t> host_tab(index->len.size());              // (lengths only: the checks read no base)
    for (size_t o = 0; o < host_tab.size(); ++o) host_tab[o] = (uint64_t)index->len[o] << 32;
    H.node_tab = host_tab.data();
    std::vector<int32_t> status(n); std::vector<uint64_t> bound(n, 0);
    parallel_for(n, [&](uint32_t r, unsigned) {
        status[r] = ra_validate_read(H, r, n_extensions, n_nodes, n_mismatches, n_ops);
        if (status[r] != VGK_OK) { bound[r] = 1; return; }
        const vgk_gapless_result g = results[r]; const uint64_t L = read_off[r + 1] - read_off[r];
        uint64_t most = 0;
        for (uint32_t x = 0; x < g.n_ext; ++x) {
            uint64_t one = 2 * L + extensions[g.ext_begin + x].path_len + 4;
            for (uint32_t left = 0; left < 2; ++left) { const uint32_t t = tail_of[2 * ((uint64_t)g.ext_begin + x) + left]; if (t != RA_NONE) one += tails[t].n_ops; }
            most = g.full_length ? most + one : std::max(most, one);
        }
        bound[r] = g.full_length ? most : 2 * most + 2;
    });
    uint64_t out_bound = 0;
    for (uint32_t r = 0; r < n; ++r) {
        out_bound += bound[r];
        if (out_bound > INDEX_MOST) return VGK_ETOOBIG;
    }
    // (plan.rc is not asked: the select kernel finds a slice by a 64-bit offset, and a slab too large to allocate answers VGK_ENOMEM below)
    const SlicePlan plan = slice_plan(n, [&](uint32_t r) { return status[r] == VGK_OK && results[r].n_ext > RA_LDS_EXT; }, [&](uint32_t r) { return ra_work_words(results[r].n_ext); });

    std::lock_guard<std::mutex> lock(ctx->mu);
    RaParams P{};
    const vgk_scoring& sc = ctx->sc;
    P.match = sc.matrix[0]; P.mismatch = -sc.matrix[1]; P.gap_open = sc.gap_open; P.gap_extend = sc.gap_extend; P.bonus = sc.full_length_bonus;
    P.threshold = policy->extension_score_threshold; P.max_local = policy->max_local_extensions; P.window_length = policy->window_length;
    P.n_reads = n; P.n_oriented = index->n_oriented; P.node_tab = index->dev.node_tab; P.seq = index->dev.seq;
    P.reads = ctx->scratch_dev<char>(READALN_READS, reads, read_bytes);
    P.read_off = ctx->scratch_dev<uint64_t>(READALN_READ_OFF, read_off, sizeof(uint64_t) * ((uint64_t)n + 1));
    P.res = ctx->scratch_dev<vgk_gapless_result>(READALN_RES, results, sizeof(vgk_gapless_result) * (uint64_t)n);
    P.ext = ctx->scratch_dev<vgk_extension>(READALN_EXT, extensions, sizeof(vgk_extension) * n_extensions);
    P.nodes = ctx->scratch_dev<uint32_t>(READALN_NODES, nodes, sizeof(uint32_t) * n_nodes);
    P.mism = ctx->scratch_dev<uint32_t>(READALN_MISM, mismatches, sizeof(uint32_t) * n_mismatches);
    P.tails = ctx->scratch_dev<vgk_tail_alignment>(READALN_TAILS, tails, sizeof(vgk_tail_alignment) * n_tails);
    P.ops = ctx->scratch_dev<vgk_op>(READALN_OPS, ops, sizeof(vgk_op) * n_ops);
    P.tail_of = ctx->scratch_dev<uint32_t>(READALN_TAIL_OF, tail_of.data(), sizeof(uint32_t) * 2 * n_extensions);
    P.status = ctx->scratch_dev<int32_t>(READALN_STATUS, status.data(), sizeof(int32_t) * (uint64_t)n);
    const uint32_t* d_ids = ctx->scratch_dev<uint32_t>(READALN_IDS, plan.ids.data(), sizeof(uint32_t) * plan.ids.size());
    const uint64_t* d_work_off = ctx->scratch_dev<uint64_t>(READALN_WORK_OFF, plan.work_off.data(), sizeof(uint64_t) * plan.work_off.size());
    uint32_t* d_work = (uint32_t*)ctx->ensure_scratch(READALN_WORK, sizeof(uint32_t) * (plan.work_words + 4));
    if (!P.reads || !P.read_off || !P.res || !P.ext || !P.nodes || !P.mism || !P.tails || !P.ops || !P.tail_of || !P.status || !d_ids || !d_work_off || !d_work) return VGK_ENOMEM;
    return vgk_read_alignments_run(ctx, P, d_ids, plan, d_work, d_work_off, out_bound, aln_off, alignments, cap_alignments, mappings, cap_mappings, edits, cap_edits, written);
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }

}  // extern "C"
