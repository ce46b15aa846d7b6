// gssw_wide_pack_device.hpp — packing for the WIDE kernels (gssw_wide_device.hpp) on the device, for windows of a resident graph
// (vgk_gssw_align_windows, gssw_wide_window_api.cpp): reads of any length, scorings of any range, against runs of consecutive nodes of the graph
// vgk_graph_create left in HBM.
//
// THE RULE.  Within a sub-batch the arenas the wide kernels read — WideProb[], colinfo (with its 8 bytes of CI_INVALID behind), prof, NodeRec[],
// preds — come out BYTE FOR BYTE as wide_pack_one (gssw_wide_pack.hpp) writes them for the induced subgraphs of the same windows in index order;
// every offset too.  Unlike the packed window packer (gssw_pack_device.hpp), which inherits the resident graph's flags and so keeps two harmless
// supersets, the flags are derived for the window:
//   in-window predecessors of v = its resident predecessors >= first_node, in their resident order;
//   chain[v]  = exactly one in-window predecessor, and it is v - 1;
//   slow[v]   = (v > first_node || xdrop) && !chain[v];
//   store[u]  = some slow node inside the window has u among its in-window predecessors (a scatter over the predecessor CSR: no successor table);
//   slot[v]   = stored nodes before v;  CI_NODE_START / CI_SEED_SLOW / CI_STORE_END from those, over the base codes of the resident bytes.
//
// The serial statement per problem: wwin_classify_one for every window of the call; then per sub-batch wwin_serial_sizes (nodes: wwin_node_one
// for each node, then the running counts; sizes; the exclusive sums over the windows) and wwin_serial_emit (wwin_emit_copy, wwin_emit_patch,
// the order's keys).  The kernels (pack_hip.hip) call the same per-item functions; only the scans differ (a block scan there).
//
// Plain C++ over VGK_HD, like the other lane code.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/vgk.h"
#include "gssw_device.hpp"
#include "gssw_pack_device.hpp"
#include "gssw_wide_device.hpp"

namespace vgk {

// an upper bound of what a problem of read_len bases over n_nodes nodes and R columns takes in HBM (every node saved; codes for every cell):
// what a call is cut into sub-batches by
VGK_HD unsigned long long wide_estimate_bytes(unsigned long long read_len, unsigned long long n_nodes, unsigned long long R) {
    const unsigned long long L = read_len + 1ull, K = L <= WIDE_LANES * 8u ? 8 : 16, strips = (L + WIDE_LANES * K - 1) / (WIDE_LANES * K), Lpad = strips * WIDE_LANES * K;
    return sizeof(WPair) * (n_nodes * Lpad + R) + 4 * (R + WIDE_LANES) * WIDE_LANES * (K / 8) * strips + 16 * (L + R) + 64ull * n_nodes + 1024;
}

enum { WW_ROUTE_NONE = 0, WW_ROUTE_PACKED = 1, WW_ROUTE_WIDE = 2 };
struct WwMeta {                      // per problem of the call: everything the host reads back
    int32_t status;                  // VGK_OK, or what the problem is answered with
    uint32_t route;                  // WW_ROUTE_*
    unsigned long long need;         // wide: wide_estimate_bytes
};
struct WwSub {                       // a wide window of a sub-batch
    uint32_t prob, pad;              // its problem in the call
    unsigned long long tmp_off;      // its first entry in the per-node temporaries (a prefix sum of n_nodes)
};
enum { WW_COLS = 0, WW_PROF, WW_NODES, WW_PREDS, WW_SCRATCH, WW_CARRY, WW_TB, WW_OPS, WW_NCOL };      // the size columns of a window
enum { WW_RUN_CLASSIFY = 0, WW_RUN_NODES, WW_RUN_OFFSETS, WW_RUN_EMIT, WW_RUN_KEYS, WW_RUN_KEYS2 };   // Backend::run_wide_windows' stages

struct WideWinParams {
    WinGraph g;
    const vgk_window_problem* problems; uint32_t n;             // the whole call
    const uint8_t* raw_reads; unsigned long long raw_bytes;     // the caller's reads, ASCII
    int32_t max_score, max_bonus, bonus; uint32_t bias;
    int8_t matrix[25];
    WwMeta* meta;                    // [n]
    // one sub-batch: m wide windows
    const WwSub* sub; uint32_t m;
    uint8_t*  store;                 // per node: some slow node of the window seeds from it (zeroed before the nodes stage)
    uint32_t* node_flags;            // per node: in-window predecessors | slow << 31
    uint32_t* slot_at; uint32_t* pred_at;      // per node: stored nodes | in-window predecessors before it in the window
    uint32_t* win_slots;             // [m] stored nodes of the window
    unsigned long long* sizes;       // [WW_NCOL][m + 1]
    unsigned long long* offs;        // [WW_NCOL][m + 1] exclusive sums; offs[c][m] = the column's total
    unsigned long long* totals;      // [WW_NCOL] the totals again, side by side: what the host reads of a sub-batch
    uint32_t* key; uint32_t* idx;    // [m] the order's first pass: low 32 bits of the key, 0 .. m - 1
    const uint32_t* idx_sorted; uint32_t* key2;      // [m] its second pass: what the first left, the key's high bits in that order
    // the arenas of WideParams
    WideProb* probs; uint8_t* colinfo; uint32_t* prof; NodeRec* nodes; uint32_t* preds;
};

struct WwGeom { uint32_t L, K, n_strips, Lpad, R, xdrop, tb; };
VGK_HD WwGeom wwin_geometry(const WideWinParams& P, const vgk_window_problem& p) {
    WwGeom q;
    q.xdrop = (p.flags & 15u) == VGK_XDROP_PINNED ? 1u : 0u; q.tb = (p.flags & VGK_GSSW_TRACEBACK) ? 1u : 0u;
    q.L = p.read_len + q.xdrop;
    q.K = q.L <= WIDE_LANES * 8u ? 8u : 16u;
    q.n_strips = (q.L + WIDE_LANES * q.K - 1) / (WIDE_LANES * q.K);
    q.Lpad = q.n_strips * WIDE_LANES * q.K;
    q.R = P.g.col[p.first_node + p.n_nodes] - P.g.col[p.first_node];
    return q;
}

// classify, a lane per problem: its status and its route.  "The packed kernels take it" = the two tests of win_size_one.
VGK_HD void wwin_classify_one(const WideWinParams& P, uint32_t i) {
    const vgk_window_problem p = P.problems[i];
    WwMeta m; m.status = VGK_OK; m.route = WW_ROUTE_NONE; m.need = 0;
    const uint32_t mode = p.flags & 15u;
    const bool xdrop = mode == VGK_XDROP_PINNED;
    const uint32_t rows = p.read_len + (xdrop ? 1u : 0u);
    const long long ms = P.max_score > 0 ? P.max_score : 0;
    if (p.read_len == 0 || p.n_nodes == 0 || (unsigned long long)p.first_node + p.n_nodes > P.g.n_nodes ||
        p.read_off + p.read_len > P.raw_bytes || p.read_off + p.read_len < p.read_off) m.status = VGK_EINVAL;
    else if (mode != VGK_GSSW_LOCAL && mode != VGK_XDROP_PINNED) m.status = VGK_EINVAL;
    else if (p.read_len >= 65535u) m.status = VGK_ETOOLONG;                  // vgk_op.len is 16 bits: a whole-read insertion must fit
    else {
        const uint32_t R = P.g.col[p.first_node + p.n_nodes] - P.g.col[p.first_node];
        if (R >= (1u << 20)) m.status = VGK_ETOOBIG;
        else {
            const bool packed = rows <= 1024 && !((long long)rows * ms + 2ll * P.max_bonus > 2046) &&
                                !(xdrop && (long long)p.read_len * ms + P.max_bonus >= (long long)XOFF);
            m.route = packed ? WW_ROUTE_PACKED : WW_ROUTE_WIDE;
            if (!packed) m.need = wide_estimate_bytes(p.read_len, p.n_nodes, R);
        }
    }
    P.meta[i] = m;
}

// nodes, a lane per node j of a window: its in-window predecessors, chain / slow, and the store scatter
VGK_HD void wwin_node_one(const WideWinParams& P, const vgk_window_problem& p, unsigned long long tmp_off, uint32_t j) {
    const uint32_t a = p.first_node, v = a + j;
    const bool xdrop = (p.flags & 15u) == VGK_XDROP_PINNED;
    const uint32_t pb = P.g.pred_off[v], pe = P.g.pred_off[v + 1];
    uint32_t np = 0, only = 0xffffffffu;
    for (uint32_t k = pb; k < pe; ++k) { const uint32_t u = P.g.pred_idx[k]; if (u >= a && u < v) { ++np; only = u; } }
    const bool chain = np == 1 && only + 1 == v;
    const bool slow = (j > 0 || xdrop) && !chain;
    if (slow) for (uint32_t k = pb; k < pe; ++k) { const uint32_t u = P.g.pred_idx[k]; if (u >= a && u < v) P.store[tmp_off + (u - a)] = 1; }
    P.node_flags[tmp_off + j] = np | (slow ? 0x80000000u : 0u);
}

// lane 0 of a window, after the counts over its nodes: the window's sizes
VGK_HD void wwin_sizes_one(const WideWinParams& P, uint32_t k, uint32_t n_slots, uint32_t n_preds) {
    const vgk_window_problem p = P.problems[P.sub[k].prob];
    const WwGeom q = wwin_geometry(P, p);
    const unsigned long long m1 = (unsigned long long)P.m + 1;
    const unsigned long long strip_dwords = (unsigned long long)(q.R + WIDE_LANES - 1) * WIDE_LANES * (q.K / 8);
    P.sizes[WW_COLS * m1 + k] = q.R; P.sizes[WW_PROF * m1 + k] = q.L; P.sizes[WW_NODES * m1 + k] = p.n_nodes; P.sizes[WW_PREDS * m1 + k] = n_preds;
    P.sizes[WW_SCRATCH * m1 + k] = (unsigned long long)n_slots * q.Lpad;
    P.sizes[WW_CARRY * m1 + k] = q.n_strips > 1 ? q.R : 0u;
    P.sizes[WW_TB * m1 + k] = q.tb ? strip_dwords * q.n_strips : 0ull;
    P.sizes[WW_OPS * m1 + k] = q.tb ? (unsigned long long)p.read_len + q.R + 2u : 0ull;
    P.win_slots[k] = n_slots;
}

#if defined(__HIP_DEVICE_COMPILE__)
static __device__ __forceinline__ uint32_t ww_load32(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }      // p is 4-byte aligned
static __device__ __forceinline__ void ww_store32(uint8_t* p, uint32_t v) { *reinterpret_cast<uint32_t*>(p) = v; }
#else
static inline uint32_t ww_load32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
static inline void ww_store32(uint8_t* p, uint32_t v) { memcpy(p, &v, 4); }
#endif

// emit, `lanes` lanes per window, first half: the column bytes (base codes of the resident bytes, a dword per lane where the destination has a
// whole one; the window's first and last bytes one by one: they share their dwords with the neighbours), the profile words (a lane per row),
// NodeRec and preds (a lane per node), WideProb (lane 0)
VGK_HD void wwin_emit_copy(const WideWinParams& P, uint32_t k, uint32_t lane, uint32_t lanes) {
    const WwSub s = P.sub[k];
    const vgk_window_problem p = P.problems[s.prob];
    const WwGeom q = wwin_geometry(P, p);
    const unsigned long long m1 = (unsigned long long)P.m + 1;
    const uint32_t a = p.first_node;
    const unsigned long long col_off = P.offs[WW_COLS * m1 + k], prof_off = P.offs[WW_PROF * m1 + k], node_off = P.offs[WW_NODES * m1 + k], pred_off = P.offs[WW_PREDS * m1 + k];
    // ---- columns
    const uint32_t src0 = P.g.col[a];
    uint8_t* dst = P.colinfo + col_off;
    uint32_t head = (4u - (uint32_t)(col_off & 3u)) & 3u; if (head > q.R) head = q.R;
    const uint32_t n_dw = (q.R - head) / 4u, tail0 = head + 4u * n_dw;
    for (uint32_t w = lane; w < n_dw; w += lanes) {
        const uint32_t o = head + 4u * w, sp = src0 + o, sa = sp & ~3u, sh = (sp & 3u) * 8u;
        uint32_t v = ww_load32(P.g.info + sa);
        if (sh) v = (v >> sh) | (ww_load32(P.g.info + sa + 4u) << (32u - sh));      // (the resident bytes have 8 bytes of padding behind them)
        ww_store32(dst + o, v & 0x07070707u);
    }
    for (uint32_t t = lane; t < head + (q.R - tail0); t += lanes) {
        const uint32_t o = t < head ? t : tail0 + (t - head);
        dst[o] = P.g.info[src0 + o] & (uint8_t)CI_BASE_MASK;
    }
    // ---- profile words: byte b = score against reference base b + bias, both bonuses folded in; X-drop row 0 consumes nothing
    const int32_t bonus_start = q.xdrop ? 0 : P.bonus, bonus_end = P.bonus;
    for (uint32_t r = lane; r < q.L; r += lanes) {
        uint32_t w = 0;
        if (!(q.xdrop && r == 0)) {
            const uint32_t code = win_nt_read(P.raw_reads[p.read_off + (r - q.xdrop)]);
            for (int b4 = 0; b4 < 4; ++b4) w |= (uint32_t)((int)P.matrix[5 * b4 + (int)code] + (int)P.bias) << (8 * b4);
            w += 0x01010101u * row_bonus((uint32_t)bonus_start, (uint32_t)bonus_end, r, q.L);
        }
        P.prof[prof_off + r] = w;
    }
    // ---- nodes and their in-window predecessors, counted from the window's first node
    for (uint32_t j = lane; j < p.n_nodes; j += lanes) {
        const uint32_t v = a + j, nf = P.node_flags[s.tmp_off + j];
        NodeRec nr;
        nr.col_start = P.g.col[v] - src0; nr.col_end = P.g.col[v + 1] - src0;
        nr.pred_begin = (uint32_t)(pred_off + P.pred_at[s.tmp_off + j]); nr.n_pred = nf & 0x7fffffffu;
        nr.slot = P.store[s.tmp_off + j] ? (int32_t)P.slot_at[s.tmp_off + j] : -1;
        nr.pinning = 0u;
        P.nodes[node_off + j] = nr;
        uint32_t at = nr.pred_begin;
        for (uint32_t e = P.g.pred_off[v]; e < P.g.pred_off[v + 1]; ++e) { const uint32_t u = P.g.pred_idx[e]; if (u >= a && u < v) P.preds[at++] = u - a; }
    }
    if (lane == 0) {
        WideProb d;
        d.col_off = (uint32_t)col_off; d.R = q.R; d.L = q.L; d.prof_off = (uint32_t)prof_off; d.node_off = (uint32_t)node_off; d.n_nodes = p.n_nodes;
        d.flags = p.flags; d.ops_off = (uint32_t)P.offs[WW_OPS * m1 + k]; d.ops_cap = q.tb ? p.read_len + q.R + 2u : 0u;
        d.max_gap = q.xdrop ? (((p.max_gap_length > 1u ? p.max_gap_length : 1u) + 7u) & ~7u) : 0u;
        d.bonus_start = bonus_start; d.bonus_end = bonus_end;
        d.K = q.K; d.n_strips = q.n_strips; d.Lpad = q.Lpad; d.n_slots = P.win_slots[k];
        d.scratch_off = P.offs[WW_SCRATCH * m1 + k]; d.tb_off = P.offs[WW_TB * m1 + k]; d.carry_off = P.offs[WW_CARRY * m1 + k];
        d.strip_dwords = (unsigned long long)(q.R + WIDE_LANES - 1) * WIDE_LANES * (q.K / 8);
        P.probs[k] = d;
    }
}
// ... second half, once the window's column bytes are there: the flags at node starts and ends, a lane per node
VGK_HD void wwin_emit_patch(const WideWinParams& P, uint32_t k, uint32_t lane, uint32_t lanes) {
    const WwSub s = P.sub[k];
    const vgk_window_problem p = P.problems[s.prob];
    const unsigned long long m1 = (unsigned long long)P.m + 1;
    const uint32_t a = p.first_node, src0 = P.g.col[a];
    uint8_t* dst = P.colinfo + P.offs[WW_COLS * m1 + k];
    for (uint32_t j = lane; j < p.n_nodes; j += lanes) {
        const uint32_t cs = P.g.col[a + j] - src0, ce = P.g.col[a + j + 1] - src0;
        dst[cs] = (uint8_t)(dst[cs] | CI_NODE_START | ((P.node_flags[s.tmp_off + j] & 0x80000000u) ? CI_SEED_SLOW : 0));
        if (P.store[s.tmp_off + j]) dst[ce - 1] = (uint8_t)(dst[ce - 1] | CI_STORE_END);
    }
}

// The order the fill kernels take the windows in (blocks start in index order): 8 rows per lane first, then 16, each class by L * R descending,
// index ascending among equals — a 37-bit key, sorted in two stable passes of 32-bit keys (low word, then the rest)
VGK_HD unsigned long long wwin_order_key(const WideWinParams& P, uint32_t k) {
    const WwGeom q = wwin_geometry(P, P.problems[P.sub[k].prob]);
    return ((unsigned long long)(q.K == 8u ? 0u : 1u) << 36) | (((1ull << 36) - 1ull) - (unsigned long long)q.L * q.R);      // L < 2^16, R < 2^20
}
VGK_HD void wwin_key_one(const WideWinParams& P, uint32_t k) { P.key[k] = (uint32_t)wwin_order_key(P, k); P.idx[k] = k; }
VGK_HD void wwin_key2_one(const WideWinParams& P, uint32_t j) { P.key2[j] = (uint32_t)(wwin_order_key(P, P.idx_sorted[j]) >> 32); }

// ---- the serial statement of a sub-batch
inline void wwin_serial_sizes(const WideWinParams& P) {
    const unsigned long long m1 = (unsigned long long)P.m + 1;
    for (uint32_t k = 0; k < P.m; ++k) {
        const WwSub s = P.sub[k]; const vgk_window_problem p = P.problems[s.prob];
        for (uint32_t j = 0; j < p.n_nodes; ++j) wwin_node_one(P, p, s.tmp_off, j);
        uint32_t slots = 0, preds = 0;
        for (uint32_t j = 0; j < p.n_nodes; ++j) {
            P.slot_at[s.tmp_off + j] = slots; P.pred_at[s.tmp_off + j] = preds;
            slots += P.store[s.tmp_off + j]; preds += P.node_flags[s.tmp_off + j] & 0x7fffffffu;
        }
        wwin_sizes_one(P, k, slots, preds);
    }
    for (uint32_t c = 0; c < WW_NCOL; ++c) {
        unsigned long long run = 0;
        for (uint32_t k = 0; k < P.m; ++k) { P.offs[c * m1 + k] = run; run += P.sizes[c * m1 + k]; }
        P.offs[c * m1 + P.m] = run; P.totals[c] = run;
    }
}
inline void wwin_serial_emit(const WideWinParams& P, uint32_t lanes) {
    for (uint32_t k = 0; k < P.m; ++k) {
        for (uint32_t l = 0; l < lanes; ++l) wwin_emit_copy(P, k, l, lanes);
        for (uint32_t l = 0; l < lanes; ++l) wwin_emit_patch(P, k, l, lanes);
        wwin_key_one(P, k);
    }
}

}  // namespace vgk
