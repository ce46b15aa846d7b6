// gssw_wide_pack.hpp — the wide route's host packer (gssw_wide_api.cpp: vgk_gssw_align's problems with explicit graphs) as a function of a small
// scoring view instead of the engine context, so that a stand-alone driver can call it too: it is the statement the device packer of the window
// route (gssw_wide_pack_device.hpp) is held to, arena for arena (tests/emu/wide_windows_driver.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "gssw_wide_device.hpp"

namespace vgk {

// what pack_one reads of a context: the plain table and its bias, the full-length bonus, and a quality-adjusted context's tables (null: plain)
struct WideScoring {
    const int8_t* matrix;            // 5 x 5: [5 * reference base + read base]
    uint32_t bias;
    int32_t full_length_bonus;
    const int8_t* qmat;              // [25 * quality + 5 * reference base + read base], or null
    const int8_t* qbon;              // [quality], or null
};

struct WidePacked {
    std::vector<WideProb> probs;
    std::vector<uint8_t> colinfo; std::vector<uint32_t> prof; std::vector<NodeRec> nodes; std::vector<uint32_t> preds;
    uint64_t scratch = 0, tb = 0, carry = 0, ops = 0;
    void clear() { probs.clear(); colinfo.clear(); prof.clear(); nodes.clear(); preds.clear(); scratch = tb = carry = ops = 0; }
};

inline int wide_nt_read(char ch) {   // gssw_create_nt_table: case-insensitive ACGT, else N
    switch (ch) { case 'A': case 'a': return 0; case 'C': case 'c': return 1;
                  case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return 4; }
}
inline int wide_nt_ref(char ch) {    // after nonATGCNtoN (src/aligner.cpp:39): upper-case ACGT only
    switch (ch) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return 4; }
}

// Appends problem p to the arenas.  The caller has checked it with wide_problem_status.
inline void wide_pack_one(const WideScoring& S, const vgk_gssw_problem& p, WidePacked& A) {
    const vgk_graph& g = p.graph;
    const uint32_t mode = p.flags & 15u; const bool xdrop = mode == VGK_XDROP_PINNED;
    const bool has_qa = S.qmat != nullptr;
    WideProb d{};
    d.flags = p.flags; d.L = p.read_len + (xdrop ? 1u : 0u); d.n_nodes = g.n_nodes;
    d.max_gap = xdrop ? ((std::max<uint32_t>(p.max_gap_length, 1u) + 7u) & ~7u) : 0u;
    // which full-length bonuses this problem grants, and their values (src/aligner.cpp:401-402, 942-952, 1164-1167)
    const int first_b = has_qa ? S.qbon[p.qual[0]] : S.full_length_bonus;
    const int last_b = has_qa ? S.qbon[p.qual[p.read_len - 1]] : S.full_length_bonus;
    d.bonus_start = xdrop ? 0 : first_b;
    d.bonus_end = (mode == VGK_GSSW_PINNED) ? 0 : last_b;
    // rows per lane: 8 while one strip of 256 lanes holds the read, else 16
    d.K = d.L <= WIDE_LANES * 8u ? 8u : 16u;
    d.n_strips = (d.L + WIDE_LANES * d.K - 1) / (WIDE_LANES * d.K);
    d.Lpad = d.n_strips * WIDE_LANES * d.K;
    // per-row profile words: byte b = score against reference base b + bias, both bonuses folded in; X-drop row 0 consumes nothing
    d.prof_off = (uint32_t)A.prof.size();
    if (xdrop) A.prof.push_back(0u);
    for (uint32_t r = 0; r < p.read_len; ++r) {
        const int code = wide_nt_read(p.read[r]);
        uint32_t w = 0;
        for (int b4 = 0; b4 < 4; ++b4) {
            const int s = has_qa ? S.qmat[25 * p.qual[r] + 5 * b4 + code] : S.matrix[5 * b4 + code];
            w |= (uint32_t)(s + (int)S.bias) << (8 * b4);
        }
        const uint32_t row = r + (xdrop ? 1u : 0u);
        w += 0x01010101u * row_bonus((uint32_t)d.bonus_start, (uint32_t)d.bonus_end, row, d.L);
        A.prof.push_back(w);
    }
    // nodes whose last column is saved (a successor seeds from it / the pinned end) and nodes seeded from scratch
    std::vector<uint8_t> store(g.n_nodes, 0), slow(g.n_nodes, 0);
    for (uint32_t v = 0; v < g.n_nodes; ++v) {
        const uint32_t pb = g.pred_off[v], pe = g.pred_off[v + 1];
        const bool chain = (pe - pb == 1) && g.pred_idx[pb] + 1 == v;
        slow[v] = ((v > 0 || xdrop) && !chain) ? 1 : 0;
        if (slow[v]) for (uint32_t k = pb; k < pe; ++k) store[g.pred_idx[k]] = 1;
        if (mode == VGK_GSSW_PINNED && p.pinning[v]) store[v] = 1;
    }
    d.col_off = (uint32_t)A.colinfo.size(); d.node_off = (uint32_t)A.nodes.size();
    uint32_t col = 0, slots = 0, seq_pos = 0;
    for (uint32_t v = 0; v < g.n_nodes; ++v) {
        NodeRec nr;
        nr.col_start = col; nr.col_end = col + g.node_len[v];
        nr.pred_begin = (uint32_t)A.preds.size(); nr.n_pred = g.pred_off[v + 1] - g.pred_off[v];
        for (uint32_t k = g.pred_off[v]; k < g.pred_off[v + 1]; ++k) A.preds.push_back(g.pred_idx[k]);
        nr.slot = store[v] ? (int32_t)slots++ : -1;
        nr.pinning = (mode == VGK_GSSW_PINNED && p.pinning[v]) ? 1u : 0u;
        A.nodes.push_back(nr);
        for (uint32_t k = 0; k < g.node_len[v]; ++k, ++seq_pos) {
            uint8_t ci = (uint8_t)wide_nt_ref(g.seq[seq_pos]);
            if (k == 0) { ci |= CI_NODE_START; if (slow[v]) ci |= CI_SEED_SLOW; }
            if (k + 1 == g.node_len[v] && store[v]) ci |= CI_STORE_END;
            A.colinfo.push_back(ci);
        }
        col = nr.col_end;
    }
    d.R = col; d.n_slots = slots;
    d.scratch_off = A.scratch; A.scratch += (uint64_t)slots * d.Lpad;
    d.carry_off = A.carry; A.carry += d.n_strips > 1 ? d.R : 0;
    d.strip_dwords = (uint64_t)(d.R + WIDE_LANES - 1) * WIDE_LANES * (d.K / 8);
    d.tb_off = A.tb;
    if (p.flags & VGK_GSSW_TRACEBACK) A.tb += d.strip_dwords * d.n_strips;
    d.ops_off = (uint32_t)A.ops; d.ops_cap = (p.flags & VGK_GSSW_TRACEBACK) ? p.read_len + d.R + 2 : 0;
    A.ops += d.ops_cap;
    A.probs.push_back(d);
}

}  // namespace vgk
