// wide_windows_driver.cpp — test infrastructure only: the serial statement of the device rule that packs windows of a resident graph for the wide
// kernels (gssw_wide_pack_device.hpp: what the kernels of pack_hip.hip are checked against), beside the host packer of explicit graphs
// (gssw_wide_pack.hpp: wide_pack_one) on the induced subgraphs of the same windows — both behind one C call, so that tests/test_wide_windows.py can
// hold one to the other byte for byte without a GPU.  The resident tables are made as vgk_graph_create makes them.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "../../vg_amd/csrc/gssw_wide_pack.hpp"
#include "../../vg_amd/csrc/gssw_wide_pack_device.hpp"

using namespace vgk;

namespace {
struct Arenas { std::vector<uint8_t> probs, colinfo, prof, nodes, preds; std::vector<uint32_t> order; std::vector<WwMeta> meta; };
Arenas g_dev, g_host;

template <class T> std::vector<uint8_t> bytes_of(const std::vector<T>& v) { std::vector<uint8_t> o(v.size() * sizeof(T)); if (!o.empty()) std::memcpy(o.data(), v.data(), o.size()); return o; }
}  // namespace

extern "C" {

// Packs the windows both ways (every window of the call must classify as runnable; `all_wide`: as if the packed kernels took none).  `lanes`: the
// lanes the emit stage is stepped with.  Returns the number of windows packed, or a negative status; vgt_wide_windows_get hands the arenas back.
int vgt_wide_windows_pack(const vgk_scoring* sc, uint32_t bias, int32_t max_score, int32_t max_bonus, const vgk_graph* graph, const char* reads, size_t reads_bytes,
                          const vgk_window_problem* problems, uint32_t n, int all_wide, uint32_t lanes) {
    const vgk_graph& g = *graph;
    const uint32_t N = g.n_nodes;
    // ---- the resident tables (window_api.cpp: vgk_graph_create)
    std::vector<uint32_t> col(N + 1), slot(N + 1), po(N + 1);
    std::vector<uint8_t> slow(N, 0), store(N, 0);
    uint64_t cols = 0;
    for (uint32_t v = 0; v < N; ++v) {
        const uint32_t pb = g.pred_off[v], pe = g.pred_off[v + 1];
        const bool chain = (pe - pb == 1) && g.pred_idx[pb] + 1 == v;
        slow[v] = (v > 0 && !chain) ? 1 : 0;
        if (slow[v]) for (uint32_t k = pb; k < pe; ++k) store[g.pred_idx[k]] = 1;
        col[v] = (uint32_t)cols; cols += g.node_len[v];
    }
    col[N] = (uint32_t)cols;
    { uint32_t s = 0; for (uint32_t v = 0; v < N; ++v) { slot[v] = s; s += store[v]; } slot[N] = s; }
    for (uint32_t v = 0; v <= N; ++v) po[v] = g.pred_off[v] - g.pred_off[0];
    std::vector<uint8_t> info((size_t)cols + 8, (uint8_t)CI_INVALID);
    for (uint32_t v = 0; v < N; ++v) {
        const uint32_t len = g.node_len[v];
        for (uint32_t k = 0; k < len; ++k) info[col[v] + k] = (uint8_t)wide_nt_ref(g.seq[col[v] + k]);
        info[col[v]] |= CI_NODE_START | (slow[v] ? CI_SEED_SLOW : 0);
        if (store[v]) info[col[v] + len - 1] |= CI_STORE_END;
    }
    WideWinParams W{};
    W.g.col = col.data(); W.g.info = info.data(); W.g.pred_off = po.data(); W.g.pred_idx = g.pred_idx + g.pred_off[0]; W.g.slot = slot.data();
    W.g.n_nodes = N; W.g.n_cols = (uint32_t)cols;
    W.problems = problems; W.n = n; W.raw_reads = (const uint8_t*)reads; W.raw_bytes = reads_bytes;
    W.max_score = max_score; W.max_bonus = max_bonus; W.bonus = sc->full_length_bonus; W.bias = bias;
    std::memcpy(W.matrix, sc->matrix, 25);
    // ---- the device rule, serially
    g_dev = Arenas(); g_host = Arenas();
    g_dev.meta.resize(n);
    W.meta = g_dev.meta.data();
    for (uint32_t i = 0; i < n; ++i) wwin_classify_one(W, i);
    std::vector<WwSub> subs; uint64_t n_nodes = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (g_dev.meta[i].status != VGK_OK) return g_dev.meta[i].status;
        if (g_dev.meta[i].route != WW_ROUTE_WIDE && !all_wide) continue;
        subs.push_back(WwSub{i, 0u, n_nodes}); n_nodes += problems[i].n_nodes;
    }
    const uint32_t m = (uint32_t)subs.size(); const uint64_t m1 = (uint64_t)m + 1;
    std::vector<uint8_t> t_store(n_nodes + 8, 0); std::vector<uint32_t> t_flags(n_nodes + 1), t_slot(n_nodes + 1), t_pred(n_nodes + 1), win_slots(m + 1);
    std::vector<unsigned long long> sizes(WW_NCOL * m1), offs(WW_NCOL * (m1 + 1));
    std::vector<uint32_t> key(m + 1), idx(m + 1);
    W.sub = subs.data(); W.m = m; W.store = t_store.data(); W.node_flags = t_flags.data(); W.slot_at = t_slot.data(); W.pred_at = t_pred.data();
    W.win_slots = win_slots.data(); W.sizes = sizes.data(); W.offs = offs.data(); W.totals = offs.data() + WW_NCOL * m1; W.key = key.data(); W.idx = idx.data();
    wwin_serial_sizes(W);
    const unsigned long long* T = W.totals;
    std::vector<WideProb> probs(m); std::vector<uint8_t> colinfo(T[WW_COLS] + 8, (uint8_t)CI_INVALID); std::vector<uint32_t> prof(T[WW_PROF]), preds(T[WW_PREDS]);
    std::vector<NodeRec> nodes(T[WW_NODES]);
    W.probs = probs.data(); W.colinfo = colinfo.data(); W.prof = prof.data(); W.nodes = nodes.data(); W.preds = preds.data();
    wwin_serial_emit(W, lanes ? lanes : 1u);
    // the order: the two stable passes of 32-bit keys the glue runs on the device
    std::vector<uint32_t> pass1(m), order(m);
    for (uint32_t k = 0; k < m; ++k) pass1[k] = idx[k];
    std::stable_sort(pass1.begin(), pass1.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    std::vector<uint32_t> key2(m + 1);
    W.idx_sorted = pass1.data(); W.key2 = key2.data();
    for (uint32_t j = 0; j < m; ++j) wwin_key2_one(W, j);
    std::vector<uint32_t> pos(m);
    for (uint32_t j = 0; j < m; ++j) pos[j] = j;
    std::stable_sort(pos.begin(), pos.end(), [&](uint32_t a, uint32_t b) { return (key2[a] & 31u) < (key2[b] & 31u); });
    for (uint32_t j = 0; j < m; ++j) order[j] = pass1[pos[j]];
    g_dev.probs = bytes_of(probs); g_dev.colinfo = colinfo; g_dev.prof = bytes_of(prof); g_dev.nodes = bytes_of(nodes); g_dev.preds = bytes_of(preds); g_dev.order = order;
    // ---- the host packer on the induced subgraphs of the same windows, in index order
    WideScoring S{sc->matrix, bias, sc->full_length_bonus, nullptr, nullptr};
    WidePacked A;
    for (uint32_t k = 0; k < m; ++k) {
        const vgk_window_problem& w = problems[subs[k].prob];
        const uint32_t a = w.first_node, b = w.first_node + w.n_nodes;
        std::vector<uint32_t> ipo(w.n_nodes + 1, 0), ipi;
        for (uint32_t v = a; v < b; ++v) {
            for (uint32_t e = g.pred_off[v]; e < g.pred_off[v + 1]; ++e) if (g.pred_idx[e] >= a) ipi.push_back(g.pred_idx[e] - a);
            ipo[v - a + 1] = (uint32_t)ipi.size();
        }
        if (ipi.empty()) ipi.push_back(0);
        vgk_gssw_problem p{};
        p.read = reads + w.read_off; p.read_len = w.read_len; p.flags = w.flags; p.max_gap_length = w.max_gap_length;
        p.graph.n_nodes = w.n_nodes; p.graph.node_len = g.node_len + a; p.graph.seq = g.seq + col[a]; p.graph.pred_off = ipo.data(); p.graph.pred_idx = ipi.data();
        wide_pack_one(S, p, A);
    }
    A.colinfo.resize(A.colinfo.size() + 8, (uint8_t)CI_INVALID);
    g_host.probs = bytes_of(A.probs); g_host.colinfo = A.colinfo; g_host.prof = bytes_of(A.prof); g_host.nodes = bytes_of(A.nodes); g_host.preds = bytes_of(A.preds);
    return (int)m;
}

// which: 0 WideProb[], 1 colinfo, 2 prof, 3 NodeRec[], 4 preds, 5 order (device rule only), 6 the per-problem verdicts (device rule only).  side: 0 the device
// rule, 1 the host packer.  Returns the arena's bytes; copies min(bytes, cap) of them to out.
size_t vgt_wide_windows_get(int side, int which, void* out, size_t cap) {
    const Arenas& A = side ? g_host : g_dev;
    const void* p = nullptr; size_t bytes = 0;
    switch (which) {
        case 0: p = A.probs.data(); bytes = A.probs.size(); break;
        case 1: p = A.colinfo.data(); bytes = A.colinfo.size(); break;
        case 2: p = A.prof.data(); bytes = A.prof.size(); break;
        case 3: p = A.nodes.data(); bytes = A.nodes.size(); break;
        case 4: p = A.preds.data(); bytes = A.preds.size(); break;
        case 5: p = A.order.data(); bytes = A.order.size() * 4; break;
        case 6: p = A.meta.data(); bytes = A.meta.size() * sizeof(WwMeta); break;
        default: break;
    }
    if (out && bytes) std::memcpy(out, p, std::min(bytes, cap));
    return bytes;
}

// the verdicts alone (statuses and routes of malformed or short windows too): meta[n] = {status, route, need}
int vgt_wide_windows_classify(int32_t max_score, int32_t max_bonus, uint32_t graph_nodes, const uint32_t* col, size_t reads_bytes, const vgk_window_problem* problems, uint32_t n, void* meta) {
    WideWinParams W{};
    W.g.col = col; W.g.n_nodes = graph_nodes; W.problems = problems; W.n = n; W.raw_bytes = reads_bytes; W.max_score = max_score; W.max_bonus = max_bonus;
    W.meta = (WwMeta*)meta;
    for (uint32_t i = 0; i < n; ++i) wwin_classify_one(W, i);
    return VGK_OK;
}

}  // extern "C"
