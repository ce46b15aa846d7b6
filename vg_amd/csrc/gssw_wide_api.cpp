// gssw_wide_api.cpp — vgk_gssw_align's route for problems outside the packed kernels' range (gssw_wide_device.hpp): reads of more
// than 1024 rows and scorings whose reachable scores do not fit the packed kernels' 11 bits.  Same modes, same results; the
// reference's own 4.4 kbp tail (src/unittest/minimizer_mapper.cpp:682-709) takes this route.
//
// Packing follows vgk_gssw_pack (vgk_api.cpp) — the same column-info stream, node table and predecessor CSR, what
// GSSWAligner::create_gssw_graph builds per call (src/aligner.cpp:30-85) as flat arenas — serially: these problems are rare and
// large, the host's share is a few microseconds per thousand cells.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>
#include "backend.hpp"
#include "batch.hpp"
#include "ctx.hpp"
#include "gssw_wide.hpp"
#include "gssw_wide_pack.hpp"

using namespace vgk;

namespace {

using Packed = WidePacked;

// what the packer (gssw_wide_pack.hpp) reads of a context
WideScoring scoring_view(const vgk_ctx* ctx) {
    return WideScoring{ctx->sc.matrix, ctx->bias, ctx->sc.full_length_bonus, ctx->has_qa ? ctx->qmat.data() : nullptr, ctx->has_qa ? ctx->qbon.data() : nullptr};
}

}  // namespace

int vgk::wide_problem_status(const vgk_ctx* ctx, const vgk_gssw_problem& p) {
    if (p.read_len == 0 || !p.read || p.graph.n_nodes == 0) return VGK_EINVAL;
    const uint32_t mode = p.flags & 15u;
    if (mode != VGK_GSSW_LOCAL && mode != VGK_GSSW_PINNED && mode != VGK_XDROP_PINNED) return VGK_EINVAL;
    const vgk_graph& g = p.graph;
    if ((ctx->has_qa && !p.qual) || (mode == VGK_GSSW_PINNED && !p.pinning) || !g.node_len || !g.pred_off || !g.seq) return VGK_EINVAL;
    if (p.read_len >= 65535u) return VGK_ETOOLONG;            // vgk_op.len is 16 bits: a whole-read insertion must fit
    uint64_t R = 0;
    for (uint32_t v = 0; v < g.n_nodes; ++v) {
        const uint32_t pb = g.pred_off[v], pe = g.pred_off[v + 1];
        if (pe < pb || g.node_len[v] == 0 || (pe > pb && !g.pred_idx)) return VGK_EINVAL;
        if (g.node_len[v] > 65535u) return VGK_ETOOBIG;
        for (uint32_t k = pb; k < pe; ++k) if (g.pred_idx[k] >= v) return VGK_EINVAL;
        R += g.node_len[v];
    }
    if (R >= (1u << 20)) return VGK_ETOOBIG;
    return VGK_OK;
}

int vgk::wide_align(vgk_ctx* ctx, const vgk_gssw_problem* problems, const uint32_t* idx, uint32_t m,
                    vgk_result* results, vgk_op* ops, size_t ops_cap, size_t* ops_at) {
    if (!m) return VGK_OK;
    Backend* be = ctx->be.get();
    ctx->wide_ms[0] = ctx->wide_ms[1] = 0; ctx->wide_cells = ctx->wide_tb_cells = 0; ctx->wide_launches = 0;
    uint64_t budget = be->memory_bytes() ? be->memory_bytes() / 4 : (2ull << 30);
    if (const char* e = std::getenv("VGAMD_MAX_BATCH_BYTES")) budget = std::strtoull(e, nullptr, 10);
    std::lock_guard<std::mutex> lock(ctx->mu);
    Packed A; const WideScoring view = scoring_view(ctx);
    // an upper bound of what a problem takes in HBM (every node saved; codes for every cell), to cut the call into sub-batches
    auto estimate = [&](const vgk_gssw_problem& p) -> uint64_t {
        uint64_t R = 0; for (uint32_t v = 0; v < p.graph.n_nodes; ++v) R += p.graph.node_len[v];
        return wide_estimate_bytes(p.read_len, p.graph.n_nodes, R);
    };
    uint32_t begin = 0;
    while (begin < m) {
        A.clear();
        uint32_t end = begin; uint64_t bytes = 0;
        std::vector<uint32_t> owner;                       // runnable problems of this sub-batch (positions in idx)
        for (; end < m; ++end) {
            const vgk_gssw_problem& p = problems[idx[end]];
            const int st = wide_problem_status(ctx, p);
            if (st != VGK_OK) { std::memset(&results[idx[end]], 0, sizeof(vgk_result)); results[idx[end]].status = st; continue; }
            const uint64_t pb = estimate(p);
            if (!owner.empty() && bytes + pb > budget) break;
            bytes += pb; owner.push_back(end);
        }
        for (uint32_t k : owner) wide_pack_one(view, problems[idx[k]], A);
        const uint32_t n = (uint32_t)owner.size();
        if (n) {
            if (A.colinfo.size() >= (1ull << 32) || A.prof.size() >= (1ull << 32) || A.ops >= (1ull << 32)) return VGK_ETOOBIG;
            WideParams P{};
            std::vector<uint32_t> order(n);
            uint32_t n8 = 0;
            for (uint32_t k = 0; k < n; ++k) if (A.probs[k].K == 8) order[n8++] = k;
            { uint32_t at = n8; for (uint32_t k = 0; k < n; ++k) if (A.probs[k].K != 8) order[at++] = k; }
            A.colinfo.resize(A.colinfo.size() + 8, (uint8_t)CI_INVALID);
            P.probs = ctx->scratch_dev<const WideProb>(WIDE_PROBS, A.probs.data(), sizeof(WideProb) * n); P.n = n;
            P.order = ctx->scratch_dev<const uint32_t>(WIDE_ORDER, order.data(), 4ull * n);
            P.colinfo = ctx->scratch_dev<const uint8_t>(WIDE_COLINFO, A.colinfo.data(), A.colinfo.size());
            P.prof = ctx->scratch_dev<const uint32_t>(WIDE_PROF, A.prof.data(), 4ull * A.prof.size());
            P.nodes = ctx->scratch_dev<const NodeRec>(WIDE_NODES, A.nodes.data(), sizeof(NodeRec) * A.nodes.size());
            P.preds = ctx->scratch_dev<const uint32_t>(WIDE_PREDS, A.preds.data(), 4ull * A.preds.size());
            P.scratch = ctx->scratch_dev<WPair>(WIDE_SCRATCH, nullptr, sizeof(WPair) * (A.scratch + 1));
            P.carry = ctx->scratch_dev<WPair>(WIDE_CARRY, nullptr, sizeof(WPair) * (A.carry + 1));
            P.tb = ctx->scratch_dev<uint32_t>(WIDE_TB, nullptr, 4ull * (A.tb + 1));
            P.best = ctx->scratch_dev<unsigned long long>(WIDE_BEST, nullptr, 8ull * (n + 1));
            P.results = ctx->scratch_dev<vgk_result>(WIDE_RESULTS, nullptr, sizeof(vgk_result) * (n + 1ull));
            P.ops = ctx->scratch_dev<vgk_op>(WIDE_OPS, nullptr, sizeof(vgk_op) * (A.ops + 1));
            if (!P.probs || !P.order || !P.colinfo || !P.prof || !P.nodes || !P.preds || !P.scratch || !P.carry || !P.tb || !P.best || !P.results || !P.ops) return VGK_ENOMEM;
            P.bias = (int32_t)ctx->bias; P.go = ctx->sc.gap_open; P.ge = ctx->sc.gap_extend;
            int rc = be->zero(P.best, 8ull * (n + 1));
            if (!rc) rc = be->run_gssw_wide(P, n8, n - n8);
            if (rc) return rc;
            { uint64_t cells = 0, tb = 0; for (uint32_t k = 0; k < n; ++k) { const WideProb& d = A.probs[k]; cells += (uint64_t)d.L * d.R; if (d.flags & VGK_GSSW_TRACEBACK) tb += (uint64_t)d.L * d.R; }
              ctx->wide_cells += cells; ctx->wide_tb_cells += tb; ctx->wide_launches += 1; }
            std::vector<vgk_result> res(n); std::vector<vgk_op> all(A.ops + 1);
            if ((rc = be->download(res.data(), P.results, sizeof(vgk_result) * n))) return rc;
            if (A.ops && (rc = be->download(all.data(), P.ops, sizeof(vgk_op) * A.ops))) return rc;
            for (uint32_t k = 0; k < n; ++k) {
                vgk_result r = res[k];
                const uint32_t src = r.ops_begin;
                if (r.status == VGK_OK && r.n_ops) {
                    if (!ops || *ops_at + r.n_ops > ops_cap) { r.status = VGK_EOPS; r.n_ops = 0; }
                    else { std::memcpy(ops + *ops_at, all.data() + src, sizeof(vgk_op) * r.n_ops); }
                } else r.n_ops = 0;
                r.ops_begin = (uint32_t)*ops_at; *ops_at += r.n_ops;
                results[idx[owner[k]]] = r;
            }
            ctx->wide_ms[0] += be->last_ms(13); ctx->wide_ms[1] += be->last_ms(14);
        }
        begin = end;
    }
    return VGK_OK;
}

extern "C" double vgk_gssw_wide_last(vgk_ctx* ctx, int which) {
    if (!ctx) return 0.0;
    switch (which) { case 0: return ctx->wide_ms[0]; case 1: return ctx->wide_ms[1]; case 2: return (double)ctx->wide_cells; case 3: return (double)ctx->wide_tb_cells; case 4: return (double)ctx->wide_launches; default: return 0.0; }
}
