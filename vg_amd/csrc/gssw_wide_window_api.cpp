// gssw_wide_window_api.cpp — vgk_gssw_align_windows (include/vgk_engine.h): windows of the resident graph of ANY read length and scoring in one call,
// each answered in its own status.  Windows the packed kernels take go through the window packer (window_api.cpp) as one batch; the others go to
// the wide kernels (gssw_wide_device.hpp), packed on the device (gssw_wide_pack_device.hpp) in sub-batches that fit wide_align's budget.
//
// The host's share: the two flat buffers go up through page-locked staging; per problem it reads 16 bytes back (status, route, byte need), cuts
// the call by them, and sums n_nodes to place the per-node temporaries; per sub-batch it reads eight totals that size the arenas.  It never
// looks at a node, a base or a row.  Results and the ops actually written come back packed (Backend::ops_offsets / ops_gather).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>
#include "batch.hpp"
#include "dgraph.hpp"
#include "host_parallel.hpp"
#include "staged_upload.hpp"

extern "C" int vgk_pack_windows_impl(vgk_ctx* ctx, const vgk_dgraph* dg, const char* reads, size_t reads_bytes,
                                     const vgk_window_problem* problems, uint32_t n, uint32_t ops_per_problem, vgk_batch** out, bool on_device, uint32_t forced_k,
                                     const vgk::WinExt* extensions);

namespace {

struct StagingLease {
    vgk_ctx* ctx; std::unique_ptr<vgk_ctx::Staging> s;
    ~StagingLease() { if (s) ctx->staging_release(std::move(s)); }
};

// the wide windows wides[0 .. nw) of the call, in sub-batches; results[i] with ops_begin = the position of the window's ops in `pool`.  The caller
// holds the context lock and has W.problems, W.meta (and `meta`, their copy) in place.
int wide_windows(vgk_ctx* ctx, WideWinParams W, const char* reads, size_t reads_bytes, const vgk_window_problem* problems, const std::vector<WwMeta>& meta,
                 const std::vector<uint32_t>& wides, StagingLease& lease, vgk_result* results, std::vector<uint64_t>& src, std::vector<vgk_op>& pool) {
    Backend* be = ctx->be.get();
    const uint32_t nw = (uint32_t)wides.size();
    uint64_t budget = be->memory_bytes() ? be->memory_bytes() / 4 : (2ull << 30);
    if (const char* e = std::getenv("VGAMD_MAX_BATCH_BYTES")) budget = std::strtoull(e, nullptr, 10);
    int rc;
    // the reads: behind 8 bytes of slack, up through page-locked staging on the side stream; the main stream's kernels start after them
    uint8_t* d_reads = ctx->scratch_dev<uint8_t>(WIDEWIN_READS, nullptr, reads_bytes + 8);
    if (!d_reads) return VGK_ENOMEM;
    if ((rc = staged_upload(be, *lease.s, 0, d_reads, reads, reads_bytes))) return rc;
    if ((rc = be->main_after_side())) return rc;
    W.raw_reads = d_reads;
    std::vector<WwSub> subs;
    uint32_t begin = 0;
    while (begin < nw) {
        subs.clear();
        uint32_t end = begin, n8 = 0; uint64_t bytes = 0, n_nodes = 0;
        for (; end < nw; ++end) {
            const uint32_t i = wides[end];
            if (end > begin && bytes + meta[i].need > budget) break;
            bytes += meta[i].need;
            subs.push_back(WwSub{i, 0u, n_nodes});
            n_nodes += problems[i].n_nodes;
            const uint32_t L = problems[i].read_len + ((problems[i].flags & 15u) == VGK_XDROP_PINNED ? 1u : 0u);
            if (L <= WIDE_LANES * 8u) ++n8;
        }
        const uint32_t m = end - begin; const uint64_t m1 = (uint64_t)m + 1;
        W.m = m;
        W.sub = ctx->scratch_dev<const WwSub>(WIDEWIN_SUB, subs.data(), sizeof(WwSub) * m);
        W.store = ctx->scratch_dev<uint8_t>(WIDEWIN_STORE, nullptr, n_nodes + 8);
        W.node_flags = ctx->scratch_dev<uint32_t>(WIDEWIN_NODE_FLAGS, nullptr, 4 * n_nodes);
        W.slot_at = ctx->scratch_dev<uint32_t>(WIDEWIN_SLOT_AT, nullptr, 4 * n_nodes);
        W.pred_at = ctx->scratch_dev<uint32_t>(WIDEWIN_PRED_AT, nullptr, 4 * n_nodes);
        W.win_slots = ctx->scratch_dev<uint32_t>(WIDEWIN_WIN_SLOTS, nullptr, 4ull * m);
        W.sizes = ctx->scratch_dev<unsigned long long>(WIDEWIN_SIZES, nullptr, 8 * WW_NCOL * m1);
        W.offs = ctx->scratch_dev<unsigned long long>(WIDEWIN_OFFS, nullptr, 8 * WW_NCOL * (m1 + 1));
        uint32_t* key = ctx->scratch_dev<uint32_t>(WIDEWIN_KEY, nullptr, 4ull * m); uint32_t* idx = ctx->scratch_dev<uint32_t>(WIDEWIN_IDX, nullptr, 4ull * m);
        uint32_t* key_sorted = ctx->scratch_dev<uint32_t>(WIDEWIN_KEY_SORTED, nullptr, 4ull * m); uint32_t* idx_sorted = ctx->scratch_dev<uint32_t>(WIDEWIN_IDX_SORTED, nullptr, 4ull * m);
        uint32_t* key2 = ctx->scratch_dev<uint32_t>(WIDEWIN_KEY2, nullptr, 4ull * m);
        if (!W.sub || !W.store || !W.node_flags || !W.slot_at || !W.pred_at || !W.win_slots || !W.sizes || !W.offs || !key || !idx || !key_sorted || !idx_sorted || !key2) return VGK_ENOMEM;
        W.totals = W.offs + WW_NCOL * m1;
        W.key = key; W.idx = idx; W.idx_sorted = idx_sorted; W.key2 = key2;
        // ---- nodes, sizes, offsets; the eight totals come down
        if ((rc = be->zero(W.store, n_nodes + 8))) return rc;
        be->watch(0);
        rc = be->run_wide_windows(W, WW_RUN_NODES);
        if (!rc) rc = be->run_wide_windows(W, WW_RUN_OFFSETS);
        be->watch(1);
        unsigned long long T[WW_NCOL];
        if (!rc) rc = be->download(T, W.totals, sizeof T);                  // (synchronises: the staged windows may go)
        if (rc) return rc;
        ctx->widewin_ms[0] += be->watch_ms();
        if (T[WW_COLS] >= (1ull << 32) || T[WW_PROF] >= (1ull << 32) || T[WW_OPS] >= (1ull << 32)) return VGK_ETOOBIG;
        // ---- the arenas, the order, the kernels
        WideParams P{};
        W.probs = ctx->scratch_dev<WideProb>(WIDEWIN_PROBS, nullptr, sizeof(WideProb) * m);
        uint32_t* order = ctx->scratch_dev<uint32_t>(WIDEWIN_ORDER, nullptr, 4ull * m);
        W.colinfo = ctx->scratch_dev<uint8_t>(WIDEWIN_COLINFO, nullptr, T[WW_COLS] + 8);
        W.prof = ctx->scratch_dev<uint32_t>(WIDEWIN_PROF, nullptr, 4 * T[WW_PROF]);
        W.nodes = ctx->scratch_dev<NodeRec>(WIDEWIN_NODES, nullptr, sizeof(NodeRec) * T[WW_NODES]);
        W.preds = ctx->scratch_dev<uint32_t>(WIDEWIN_PREDS, nullptr, 4 * T[WW_PREDS]);
        P.scratch = ctx->scratch_dev<WPair>(WIDEWIN_SCRATCH, nullptr, sizeof(WPair) * (T[WW_SCRATCH] + 1));
        P.carry = ctx->scratch_dev<WPair>(WIDEWIN_CARRY, nullptr, sizeof(WPair) * (T[WW_CARRY] + 1));
        P.tb = ctx->scratch_dev<uint32_t>(WIDEWIN_TB, nullptr, 4 * (T[WW_TB] + 1));
        P.best = ctx->scratch_dev<unsigned long long>(WIDEWIN_BEST, nullptr, 8 * m1);
        P.results = ctx->scratch_dev<vgk_result>(WIDEWIN_RESULTS, nullptr, sizeof(vgk_result) * m1);
        P.ops = ctx->scratch_dev<vgk_op>(WIDEWIN_OPS, nullptr, sizeof(vgk_op) * (T[WW_OPS] + 1));
        if (!W.probs || !order || !W.colinfo || !W.prof || !W.nodes || !W.preds || !P.scratch || !P.carry || !P.tb || !P.best || !P.results || !P.ops) return VGK_ENOMEM;
        P.probs = W.probs; P.n = m; P.order = order; P.colinfo = W.colinfo; P.prof = W.prof; P.nodes = W.nodes; P.preds = W.preds;
        P.bias = (int32_t)ctx->bias; P.go = ctx->sc.gap_open; P.ge = ctx->sc.gap_extend;
        be->watch(0);
        rc = be->fill(W.colinfo + T[WW_COLS], (int)CI_INVALID, 8);
        if (!rc) rc = be->run_wide_windows(W, WW_RUN_EMIT);
        if (!rc) rc = be->run_wide_windows(W, WW_RUN_KEYS);
        if (!rc) rc = be->sort_pairs_u32(key, key_sorted, idx, idx_sorted, m, 32);
        if (!rc) rc = be->run_wide_windows(W, WW_RUN_KEYS2);
        if (!rc) rc = be->sort_pairs_u32(key2, key_sorted, idx_sorted, order, m, 5);
        be->watch(1);
        if (!rc) rc = be->zero(P.best, 8 * m1);
        if (!rc) rc = be->run_gssw_wide(P, n8, m - n8);
        if (!rc) rc = be->sync();
        if (rc) return rc;
        ctx->widewin_ms[0] += be->watch_ms(); ctx->widewin_ms[1] += be->last_ms(13); ctx->widewin_ms[2] += be->last_ms(14);
        ctx->widewin_windows += m; ctx->widewin_batches += 1;
        // ---- home: results, and the ops behind each other
        const uint32_t blocks = (m + Backend::OPS_SCAN_BLOCK - 1) / Backend::OPS_SCAN_BLOCK;
        uint32_t* o_offs = ctx->scratch_dev<uint32_t>(WIDEWIN_OPS_OFFS, nullptr, 4ull * m);
        uint32_t* o_sums = ctx->scratch_dev<uint32_t>(WIDEWIN_OPS_SUMS, nullptr, 4ull * (blocks + 8));
        if (!o_offs || !o_sums) return VGK_ENOMEM;
        uint64_t total = 0;
        if ((rc = be->ops_offsets(P.results, m, o_offs, o_sums, &total))) return rc;
        vgk_result* out_res = ctx->scratch_dev<vgk_result>(WIDEWIN_RES_OUT, nullptr, sizeof(vgk_result) * m);
        vgk_op* out_ops = ctx->scratch_dev<vgk_op>(WIDEWIN_OPS_OUT, nullptr, sizeof(vgk_op) * (total + 1));
        if (!out_res || !out_ops) return VGK_ENOMEM;
        if ((rc = be->ops_gather(P.results, P.ops, m, o_offs, o_sums, out_res, out_ops))) return rc;
        const uint64_t res_bytes = sizeof(vgk_result) * m, ops_bytes = sizeof(vgk_op) * total;
        uint8_t* stage = (uint8_t*)lease.s->get(5, res_bytes + ops_bytes);
        if (!stage) return VGK_ENOMEM;
        if ((rc = be->download_fetch(stage, out_res, res_bytes))) return rc;
        if (ops_bytes && (rc = be->download_fetch(stage + res_bytes, out_ops, ops_bytes))) return rc;
        ctx->widewin_op_bytes += ops_bytes;
        const vgk_result* res = (const vgk_result*)stage;
        const uint64_t base = pool.size();
        pool.resize(base + total);
        if (total) std::memcpy(pool.data() + base, stage + res_bytes, ops_bytes);
        for (uint32_t k = 0; k < m; ++k) { const uint32_t i = subs[k].prob; results[i] = res[k]; src[i] = base + res[k].ops_begin; }
        begin = end;
    }
    return VGK_OK;
}

}  // namespace

extern "C" {

int vgk_gssw_align_windows(vgk_ctx* ctx, const vgk_dgraph* dg, const char* reads, size_t reads_bytes, const vgk_window_problem* problems, uint32_t n,
                           vgk_result* results, vgk_op* ops, size_t ops_cap, size_t* ops_written) try {
    if (!ctx || !dg || dg->ctx != ctx || (!problems && n) || (!reads && reads_bytes) || (!results && n)) return VGK_EINVAL;
    if (ops_written) *ops_written = 0;
    if (ctx->has_qa) return VGK_EUNSUPPORTED;
    Backend* be = ctx->be.get();
    std::vector<WwMeta> meta(n);
    std::vector<uint32_t> shorts, wides;
    std::vector<uint64_t> src(n, 0);               // where a window's ops lie in `pool`
    std::vector<vgk_op> pool;
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        ctx->widewin_ms[0] = ctx->widewin_ms[1] = ctx->widewin_ms[2] = 0; ctx->widewin_windows = ctx->widewin_batches = ctx->widewin_op_bytes = 0;
        if (!n) return VGK_OK;
        StagingLease lease{ctx, ctx->staging_acquire()};
        WideWinParams W{};
        W.g = dg->g; W.n = n; W.raw_bytes = reads_bytes;
        W.max_score = ctx->max_score; W.max_bonus = ctx->max_bonus; W.bonus = ctx->sc.full_length_bonus; W.bias = ctx->bias;
        std::memcpy(W.matrix, ctx->sc.matrix, 25);
        // ---- classify: the windows go up, 16 bytes per window come back
        vgk_window_problem* d_problems = ctx->scratch_dev<vgk_window_problem>(WIDEWIN_PROBLEMS, nullptr, sizeof(vgk_window_problem) * n);
        W.meta = ctx->scratch_dev<WwMeta>(WIDEWIN_META, nullptr, sizeof(WwMeta) * n);
        if (!d_problems || !W.meta) return VGK_ENOMEM;
        W.problems = d_problems;
        int rc = staged_upload(be, *lease.s, 1, d_problems, problems, sizeof(vgk_window_problem) * n);
        if (!rc) rc = be->main_after_side();
        if (rc) return rc;
        be->watch(0);
        rc = be->run_wide_windows(W, WW_RUN_CLASSIFY);                       // (a backend without the stages: VGK_EUNSUPPORTED for the call)
        be->watch(1);
        if (!rc) rc = be->download(meta.data(), W.meta, sizeof(WwMeta) * n);
        if (rc) return rc;
        ctx->widewin_ms[0] += be->watch_ms();
        for (uint32_t i = 0; i < n; ++i) {
            std::memset(&results[i], 0, sizeof(vgk_result));
            results[i].status = meta[i].status;
            if (meta[i].status != VGK_OK) continue;
            if (meta[i].route == WW_ROUTE_WIDE) wides.push_back(i); else shorts.push_back(i);
        }
        if (!wides.empty() && (rc = wide_windows(ctx, W, reads, reads_bytes, problems, meta, wides, lease, results, src, pool))) return rc;
    }
    // ---- the windows the packed kernels take: one batch through the window packer, in their original relative order
    if (!shorts.empty()) {
        const uint32_t ns = (uint32_t)shorts.size();
        std::vector<vgk_window_problem> sp(ns);
        for (uint32_t k = 0; k < ns; ++k) sp[k] = problems[shorts[k]];
        vgk_batch* b = nullptr;
        int rc = vgk_pack_windows_impl(ctx, dg, reads, reads_bytes, sp.data(), ns, 0, &b, false, 0, nullptr);
        if (rc) return rc;
        std::vector<vgk_result> sr(ns);
        const uint64_t base = pool.size(), cap = b->ops_total;
        pool.resize(base + cap);
        size_t w = 0;
        rc = vgk_gssw_run(b);
        if (!rc) rc = vgk_gssw_fetch(b, sr.data(), pool.data() + base, cap, &w);
        vgk_batch_free(b);
        if (rc) return rc;
        for (uint32_t k = 0; k < ns; ++k) { results[shorts[k]] = sr[k]; src[shorts[k]] = base + sr[k].ops_begin; }
    }
    // ---- the ops in problem order in the caller's array; what does not fit what is left of it: VGK_EOPS, as vgk_gssw_align answers it
    size_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        vgk_result& r = results[i];
        if (r.status == VGK_OK && r.n_ops) {
            if (!ops || at + r.n_ops > ops_cap) { r.status = VGK_EOPS; r.n_ops = 0; }
        } else r.n_ops = 0;
        r.ops_begin = (uint32_t)at; at += r.n_ops;
    }
    parallel_for(n, [&](uint32_t i, unsigned) {
        const vgk_result& r = results[i];
        if (r.n_ops) std::memcpy(ops + r.ops_begin, pool.data() + src[i], sizeof(vgk_op) * r.n_ops);
    });
    if (ops_written) *ops_written = at;
    return VGK_OK;
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }      // (no exception leaves the C ABI)

double vgk_gssw_align_windows_last(vgk_ctx* ctx, int which) {
    if (!ctx) return 0.0;
    std::lock_guard<std::mutex> lock(ctx->mu);
    switch (which) {
        case 0: case 1: case 2: return ctx->widewin_ms[which];
        case 3: return (double)ctx->widewin_windows;
        case 4: return (double)ctx->widewin_batches;
        case 5: return (double)ctx->widewin_op_bytes;
        default: return 0.0;
    }
}

}  // extern "C"
