// minimizer_api.cpp — vgk_minimizer_index_create / vgk_minimizer_seeds (minimizer_device.hpp): the minimizer index of the haplotype
// threads built on host threads and kept in HBM; the reads' minimizers, lookups and seeds on the device.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>
#include "ctx.hpp"
#include "haplo.hpp"
#include "host_parallel.hpp"
#include "minimizer_device.hpp"
#include "../../include/vgk_engine.h"

using namespace vgk;

struct vgk_minimizer_index {
    vgk_ctx* ctx = nullptr;
    MzIndex dev{};
    std::vector<void*> held;
    uint64_t n_keys = 0, n_pos = 0;
    std::vector<vgk_minimizer_hit> hits;      // what the index holds (vgk_minimizer_index_fetch)
    MzPolicy policy{};                        // vgk_minimizer_set_policy (on == 0: none); its score table in `policy_tab` (device)
    void* policy_tab = nullptr;
};

namespace {
char mz_comp(char c) { switch (c) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; default: return 'N'; } }
struct Entry { uint64_t key, hash; uint32_t node, offset; };
}

extern "C" {

int vgk_minimizer_index_create(vgk_ctx* ctx, const vgk_haplotypes* d, uint32_t k, uint32_t w, vgk_minimizer_index** out) try {
    if (!ctx || !d || !out || !d->n_nodes || !d->node_len || !d->seq || (d->n_threads && (!d->thread_off || !d->thread_nodes))) return VGK_EINVAL;
    if (k == 0 || k > MZ_MAX_K || w == 0 || w > MZ_MAX_W) return VGK_EINVAL;
    *out = nullptr;
    const uint32_t N = d->n_nodes;
    std::vector<uint64_t> node_at((size_t)N + 1, 0);
    for (uint32_t i = 0; i < N; ++i) node_at[i + 1] = node_at[i] + d->node_len[i];
    for (uint32_t t = 0; t < d->n_threads; ++t) for (uint32_t x = d->thread_off[t]; x < d->thread_off[t + 1]; ++x) if (d->thread_nodes[x] >= 2 * N) return VGK_EINVAL;
    for (uint32_t i = 0; i < N; ++i) if (d->node_len[i] > 65535u) return VGK_ETOOBIG;      // (a position's offset word holds the offset from either end in 16 bits each)
    // the minimizers of every thread, read along the thread; a reverse-canonical one is filed under the position its
    // reverse complement starts at: the k-mer's last base, seen from the other strand
    std::vector<std::vector<Entry>> per_thread(d->n_threads);
    parallel_tasks(d->n_threads, [&](uint32_t t) {
        const uint32_t* tn = d->thread_nodes + d->thread_off[t]; const uint32_t len = d->thread_off[t + 1] - d->thread_off[t];
        size_t bases = 0;
        for (uint32_t x = 0; x < len; ++x) bases += d->node_len[tn[x] >> 1];
        std::vector<char> seq(bases); std::vector<uint32_t> step(bases);          // step[b] = index in the thread of the node that holds base b
        std::vector<uint64_t> start((size_t)len + 1, 0);
        size_t at = 0;
        for (uint32_t x = 0; x < len; ++x) {
            const uint32_t o = tn[x], v = o >> 1, L = d->node_len[v]; const char* s = d->seq + node_at[v];
            start[x] = at;
            for (uint32_t b = 0; b < L; ++b) { seq[at] = (o & 1) ? mz_comp(s[L - 1 - b]) : s[b]; step[at] = x; ++at; }
        }
        start[len] = at;
        std::vector<Entry>& outv = per_thread[t];
        mz_minimizers(seq.data(), (uint32_t)std::min<size_t>(bases, 0xffffffffu), k, w, [&](uint32_t p, const MzKmer& m) {
            Entry e; e.key = m.key; e.hash = m.hash;
            if (!m.reverse) { const uint32_t x = step[p]; e.node = tn[x]; e.offset = (uint32_t)(p - start[x]); }
            else { const size_t q = (size_t)p + k - 1; const uint32_t x = step[q]; const uint32_t L = d->node_len[tn[x] >> 1]; e.node = tn[x] ^ 1u; e.offset = L - 1 - (uint32_t)(q - start[x]); }
            outv.push_back(e);
        });
    });
    std::vector<Entry> all;
    for (auto& v : per_thread) { all.insert(all.end(), v.begin(), v.end()); std::vector<Entry>().swap(v); }
    std::sort(all.begin(), all.end(), [](const Entry& a, const Entry& b) { return a.key != b.key ? a.key < b.key : a.node != b.node ? a.node < b.node : a.offset < b.offset; });
    all.erase(std::unique(all.begin(), all.end(), [](const Entry& a, const Entry& b) { return a.key == b.key && a.node == b.node && a.offset == b.offset; }), all.end());
    uint64_t n_keys = 0;
    for (size_t i = 0; i < all.size(); ++i) if (i == 0 || all[i].key != all[i - 1].key) ++n_keys;
    uint64_t cap = 16; while (cap < 2 * n_keys + 2) cap <<= 1;
    if (cap > (1ull << 31)) return VGK_ETOOBIG;
    std::vector<MzSlot> slots(cap, MzSlot{0, 0, 0});
    std::vector<MzPos> pos(all.size() + 1);
    for (size_t i = 0; i < all.size();) {
        size_t j = i; while (j < all.size() && all[j].key == all[i].key) { pos[j] = MzPos{all[j].node, mz_pack_offset(all[j].offset, d->node_len[all[j].node >> 1])}; ++j; }
        uint32_t s = (uint32_t)all[i].hash & (uint32_t)(cap - 1);
        while (slots[s].count) s = (s + 1) & (uint32_t)(cap - 1);
        // a key with one position keeps it in its slot (one request per lookup); its offset word must leave the flag bit free
        if (j - i == 1 && !(pos[i].offset & MZ_INLINE)) slots[s] = MzSlot{all[i].key, pos[i].node, pos[i].offset | MZ_INLINE};
        else slots[s] = MzSlot{all[i].key, (uint32_t)i, (uint32_t)(j - i)};
        i = j;
    }
    std::unique_ptr<vgk_minimizer_index> ix(new (std::nothrow) vgk_minimizer_index());
    if (!ix) return VGK_ENOMEM;
    ix->ctx = ctx; ix->n_keys = n_keys; ix->n_pos = all.size();
    ix->hits.resize(all.size());
    for (size_t i = 0; i < all.size(); ++i) ix->hits[i] = vgk_minimizer_hit{all[i].key, all[i].node, all[i].offset};
    Backend* be = ctx->be.get();
    std::lock_guard<std::mutex> lk(ctx->mu);
    void* ds = be->alloc(sizeof(MzSlot) * cap); void* dp = be->alloc(sizeof(MzPos) * pos.size());
    if (ds) ix->held.push_back(ds);
    if (dp) ix->held.push_back(dp);
    int rc = (ds && dp) ? VGK_OK : VGK_ENOMEM;
    if (!rc) rc = be->upload(ds, slots.data(), sizeof(MzSlot) * cap);
    if (!rc) rc = be->upload(dp, pos.data(), sizeof(MzPos) * pos.size());
    if (!rc) rc = be->sync();
    if (rc) { for (void* p : ix->held) be->release(p); return rc; }
    ix->dev.slots = (const MzSlot*)ds; ix->dev.mask = (uint32_t)(cap - 1); ix->dev.pos = (const MzPos*)dp; ix->dev.k = k; ix->dev.w = w;
    *out = ix.release();
    return VGK_OK;
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }      // (no exception leaves the C ABI)

void vgk_minimizer_index_destroy(vgk_minimizer_index* ix) {
    if (!ix) return;
    { std::lock_guard<std::mutex> lk(ix->ctx->mu); ix->ctx->be->sync(); for (void* p : ix->held) ix->ctx->be->release(p); if (ix->policy_tab) ix->ctx->be->release(ix->policy_tab); }
    delete ix;
}
int vgk_minimizer_set_policy(vgk_minimizer_index* ix, const vgk_seed_policy* policy) try {
    if (!ix) return VGK_EINVAL;
    std::lock_guard<std::mutex> lk(ix->ctx->mu);
    Backend* be = ix->ctx->be.get();
    if (!policy) { ix->policy = MzPolicy{}; return VGK_OK; }
    if (!policy->hard_hit_cap || policy->hard_hit_cap > 65535u || !(policy->minimizer_score_fraction >= 0.0 && policy->minimizer_score_fraction <= 1.0)) return VGK_EINVAL;
    // find_minimizers' scores by hit count, with the host's logarithm (src/minimizer_mapper.cpp:3927-3937)
    std::vector<double> tab((size_t)policy->hard_hit_cap + 1, 0.0);
    const double base = 1.0 + std::log((double)policy->hard_hit_cap);
    for (uint32_t h = 1; h <= policy->hard_hit_cap; ++h) tab[h] = base - std::log((double)h);
    int rc = be->sync();
    if (rc) return rc;
    if (ix->policy_tab) { be->release(ix->policy_tab); ix->policy_tab = nullptr; ix->policy = MzPolicy{}; }
    void* d = be->alloc(sizeof(double) * tab.size());
    if (!d) return VGK_ENOMEM;
    if ((rc = be->upload(d, tab.data(), sizeof(double) * tab.size())) || (rc = be->sync())) { be->release(d); return rc; }
    ix->policy_tab = d;
    ix->policy.on = 1; ix->policy.hit_cap = policy->hit_cap; ix->policy.hard_hit_cap = policy->hard_hit_cap; ix->policy.fraction = policy->minimizer_score_fraction; ix->policy.paired = policy->paired;
    ix->policy.tab = (const double*)d;
    return VGK_OK;
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }
uint64_t vgk_minimizer_index_keys(const vgk_minimizer_index* ix) { return ix ? ix->n_keys : 0; }
uint64_t vgk_minimizer_index_hits(const vgk_minimizer_index* ix) { return ix ? ix->hits.size() : 0; }
int vgk_minimizer_index_fetch(const vgk_minimizer_index* ix, vgk_minimizer_hit* hits, size_t cap) try {
    if (!ix || (!hits && cap)) return VGK_EINVAL;
    if (cap < ix->hits.size()) return VGK_EOPS;
    if (!ix->hits.empty()) std::memcpy(hits, ix->hits.data(), sizeof(vgk_minimizer_hit) * ix->hits.size());
    return VGK_OK;
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }      // (no exception leaves the C ABI)

int vgk_minimizer_seeds(vgk_ctx* ctx, const vgk_minimizer_index* ix, const vgk_haplo* graph, const char* reads, const uint64_t* read_off, uint32_t n,
                        uint32_t hit_cap, uint32_t* seed_off, uint32_t* minimizers, vgk_seed* seeds, size_t seeds_cap, size_t* written) try {
    if (!ctx || !ix || !graph || !vgk_tables_usable(ix->ctx, ctx) || !vgk_tables_usable(graph->ctx, ctx) || (n && (!reads || !read_off || !seed_off))) return VGK_EINVAL;
    if (written) *written = 0;
    if (!n) { if (seed_off) seed_off[0] = 0; return VGK_OK; }
    for (uint32_t i = 0; i < n; ++i) if (read_off[i + 1] < read_off[i]) return VGK_EINVAL;
    const uint64_t bytes = read_off[n] - read_off[0];
    if (bytes > INDEX_MOST) return VGK_ETOOBIG;
    Backend* be = ctx->be.get();
    std::lock_guard<std::mutex> stage(ctx->stage_mu);
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->seeded.valid = false;
    char* d_reads = (char*)ctx->ensure_scratch(SEEDED_READS, bytes + 32);              // 8 bytes of padding at either end, as the extension kernels want them
    uint64_t* d_off = (uint64_t*)ctx->ensure_scratch(SEEDED_READ_OFF, sizeof(uint64_t) * ((size_t)n + 1));
    uint32_t* d_tab = (uint32_t*)ctx->ensure_scratch(SEEDED_TAB, sizeof(uint32_t) * 3 * ((size_t)n + 1));
    if (!d_reads || !d_off || !d_tab) return VGK_ENOMEM;
    const size_t n1 = (size_t)n + 1;
    std::vector<uint64_t> rel(n1);
    for (size_t i = 0; i < n1; ++i) rel[i] = read_off[i] - read_off[0];
    MinimizerParams P{};
    P.index = ix->dev; P.graph = graph->dev; P.reads = d_reads + 8; P.read_off = d_off; P.n = n; P.hit_cap = hit_cap ? hit_cap : 0xffffffffu;
    P.policy = ix->policy;
    if (P.policy.on) P.hit_cap = P.policy.hard_hit_cap;                     // (what a read beyond the selection's 64 minimizers is held to)
    P.counts = d_tab; P.mins = d_tab + n1; P.first = d_tab + 2 * n1;
    int rc = be->upload(d_off, rel.data(), sizeof(uint64_t) * n1);
    if (!rc) rc = be->zero(d_tab, sizeof(uint32_t) * 3 * n1);
    if (!rc) rc = be->zero(d_reads, 8);
    if (!rc) rc = be->zero(d_reads + 8 + bytes, 8);
    be->watch(0);                                                          // (the stopwatch covers copies, kernels and scans from here on)
    // The reads go up in slices on the copy stream; a slice is masked (ReadMasker once, for the seeding — anything but ACGT is no k-mer —
    // and the extension) and its minimizers found on the main stream while the next slice travels.
    P.pass = 1;
    const uint32_t slices = n >= (1u << 16) ? 4u : 1u;
    for (uint32_t c = 0; c < slices && !rc; ++c) {
        const uint32_t lo = (uint32_t)((uint64_t)n * c / slices), hi = (uint32_t)((uint64_t)n * (c + 1) / slices);
        const uint64_t a = rel[lo], b = rel[hi];
        if (b > a) { rc = be->upload_side(d_reads + 8 + a, reads + read_off[0] + a, b - a); if (!rc) rc = be->sync_side(); if (!rc) { const uint64_t from = (8 + a) & ~15ull; rc = be->mask_reads(d_reads + from, 8 + b - from); } }      // (from a 16-byte boundary: the few bytes before `a` are the previous slice's, masked already — masking is idempotent)
        P.lo = lo; P.hi = hi;
        if (!rc) rc = be->run_minimizer(P);
    }
    if (!rc) rc = be->scan_u32(d_tab, d_tab + 2 * n1, (uint32_t)n1);
    if (!rc) rc = be->download(seed_off, d_tab + 2 * n1, sizeof(uint32_t) * n1);      // synchronises (rel[] may go)
    if (!rc && minimizers) rc = be->download(minimizers, d_tab + n1, sizeof(uint32_t) * n);
    if (rc) return rc;
    const size_t total = seed_off[n];
    if (written) *written = total;
    const bool keep_on_device = !seeds && !seeds_cap;                         // the caller goes on with vgk_gapless_extend_seeded: the seeds need not come down
    if (!keep_on_device && (total > seeds_cap || (total && !seeds))) return VGK_EOPS;
    // (the seed buffer exists even for a batch without a single seed: the seeded extension call tells "no seeds" from "no memory" by it)
    vgk_seed* d_seeds = (vgk_seed*)ctx->ensure_scratch(SEEDED_SEEDS, sizeof(vgk_seed) * std::max<size_t>(total, 1));
    if (!d_seeds) return VGK_ENOMEM;
    P.seeds = d_seeds;
    if (total) {
        P.pass = 2;
        rc = be->run_minimizer(P);
        be->watch(1);
        if (!rc) rc = keep_on_device ? be->sync() : be->download(seeds, d_seeds, sizeof(vgk_seed) * total);
        if (rc) return rc;
    } else { be->watch(1); be->sync(); }
    ctx->minimizer_ms = be->watch_ms();
    ctx->seeded.valid = true; ctx->seeded.n = n; ctx->seeded.reads = d_reads; ctx->seeded.bytes = bytes; ctx->seeded.read_off = d_off;
    ctx->seeded.seed_off = d_tab + 2 * n1; ctx->seeded.seeds = P.seeds; ctx->seeded.n_seeds = total; ctx->seeded.graph = graph;
    return VGK_OK;
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }      // (no exception leaves the C ABI)

double vgk_minimizer_last_ms(vgk_ctx* ctx) { return ctx ? ctx->minimizer_ms : 0.0; }

// ---- reads of any length: every minimizer listed; the seeds of those the caller takes (include/vgk.h) ----------------------------------------
// the list of n >= 1 reads made in HBM (callers hold ctx->mu): minimizer_off[n + 1] and *total on the host; the reads (behind 8 bytes of padding), their
// offsets and the records stay in MZLIST_READS / MZLIST_READ_OFF / MZLIST_MINIMIZERS.  The records are written only when total <= cap
static int list_on_device(vgk_ctx* ctx, const vgk_minimizer_index* ix, const char* reads, const uint64_t* read_off, uint32_t n, uint64_t* minimizer_off, size_t cap, size_t* total_out) {
    *total_out = 0;
    for (uint32_t i = 0; i < n; ++i) if (read_off[i + 1] < read_off[i]) return VGK_EINVAL;
    const uint64_t bytes = read_off[n] - read_off[0];
    if (bytes > INDEX_MOST) return VGK_ETOOBIG;
    Backend* be = ctx->be.get();
    // a read is cut into stretches of MZ_LIST_WINDOWS windows, a lane each (a 15 kbp read alone would keep one lane busy for 15 000 steps)
    std::vector<MzListItem> items; std::vector<uint64_t> item_first((size_t)n + 1, 0);
    const uint32_t k = ix->dev.k, w = ix->dev.w;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t L = read_off[i + 1] - read_off[i];
        if (L > INDEX_MOST) return VGK_ETOOBIG;
        const uint32_t windows = L >= (uint64_t)k + w - 1 ? (uint32_t)(L - k - w + 2) : 0u;
        for (uint32_t s = 0; s < windows; s += MZ_LIST_WINDOWS) items.push_back(MzListItem{i, s});
        item_first[i + 1] = items.size();
    }
    if (items.size() > INDEX_MOST) return VGK_ETOOBIG;
    const uint32_t n_items = (uint32_t)items.size();
    const size_t n1 = (size_t)n + 1, m1 = (size_t)n_items + 1;
    char* d_reads = (char*)ctx->ensure_scratch(MZLIST_READS, bytes + 32);
    uint64_t* d_off = (uint64_t*)ctx->ensure_scratch(MZLIST_READ_OFF, sizeof(uint64_t) * n1);
    uint32_t* d_tab = (uint32_t*)ctx->ensure_scratch(MZLIST_TAB, sizeof(uint32_t) * 2 * m1);
    MzListItem* d_items = (MzListItem*)ctx->ensure_scratch(MZLIST_ITEMS, sizeof(MzListItem) * std::max<size_t>(n_items, 1));
    if (!d_reads || !d_off || !d_tab || !d_items) return VGK_ENOMEM;
    std::vector<uint64_t> rel(n1);
    for (size_t i = 0; i < n1; ++i) rel[i] = read_off[i] - read_off[0];
    MzListParams P{};
    P.index = ix->dev; P.reads = d_reads + 8; P.read_off = d_off; P.n = n_items; P.items = d_items; P.counts = d_tab; P.first = d_tab + m1; P.pass = 1;
    int rc = be->upload(d_off, rel.data(), sizeof(uint64_t) * n1);
    if (!rc && n_items) rc = be->upload(d_items, items.data(), sizeof(MzListItem) * n_items);
    if (!rc) rc = be->zero(d_reads, 8);
    if (!rc) rc = be->zero(d_reads + 8 + bytes, 16);
    if (!rc && bytes) rc = be->upload(d_reads + 8, reads + read_off[0], bytes);
    if (!rc) rc = be->run_minimizer_list(P);
    if (!rc) rc = be->scan_u32(d_tab, d_tab + m1, (uint32_t)m1);
    std::vector<uint32_t> first(m1);
    if (!rc) rc = be->download(first.data(), d_tab + m1, sizeof(uint32_t) * m1);      // synchronises (rel[], items may go)
    if (rc) return rc;
    for (size_t i = 0; i < n1; ++i) minimizer_off[i] = first[item_first[i]];
    const size_t total = first[n_items];
    *total_out = total;
    if (total > cap) return VGK_EOPS;
    if (!total) return VGK_OK;
    vgk_read_minimizer* d_out = (vgk_read_minimizer*)ctx->ensure_scratch(MZLIST_MINIMIZERS, sizeof(vgk_read_minimizer) * total);
    if (!d_out) return VGK_ENOMEM;
    P.out = d_out; P.pass = 2;
    return be->run_minimizer_list(P);
}
int vgk_minimizer_list(vgk_ctx* ctx, const vgk_minimizer_index* ix, const char* reads, const uint64_t* read_off, uint32_t n,
                       uint64_t* minimizer_off, vgk_read_minimizer* minimizers, size_t cap, size_t* written) try {
    if (!ctx || !ix || !vgk_tables_usable(ix->ctx, ctx) || !minimizer_off || (n && (!reads || !read_off)) || (!minimizers && cap)) return VGK_EINVAL;
    if (written) *written = 0;
    minimizer_off[0] = 0;
    if (!n) return VGK_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    size_t total = 0;
    const int rc = list_on_device(ctx, ix, reads, read_off, n, minimizer_off, cap, &total);
    if (written) *written = total;
    if (rc || !total) return rc;
    return ctx->be->download(minimizers, ctx->scratch[MZLIST_MINIMIZERS].p, sizeof(vgk_read_minimizer) * total);
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }

// the seeds of the taken minimizers, list and choice in MZLIST_MINIMIZERS / MZLIST_TAKE already (callers hold ctx->mu; minimizers / take: the host's copies)
static int seeds_of_on_device(vgk_ctx* ctx, const vgk_minimizer_index* ix, const vgk_read_minimizer* minimizers, const uint8_t* take, size_t n_minimizers,
                              uint64_t* seed_off, vgk_seed* seeds, size_t cap, size_t* written) {
    Backend* be = ctx->be.get();
    const uint32_t n = (uint32_t)n_minimizers; const size_t n1 = (size_t)n + 1;
    uint32_t* d_tab = (uint32_t*)ctx->ensure_scratch(MZLIST_SEED_TAB, sizeof(uint32_t) * 2 * n1);
    if (!d_tab) return VGK_ENOMEM;
    MzSeedsOfParams P{};
    P.index = ix->dev; P.mins = (const vgk_read_minimizer*)ctx->scratch[MZLIST_MINIMIZERS].p; P.take = (const uint8_t*)ctx->scratch[MZLIST_TAKE].p; P.n = n; P.counts = d_tab; P.first = d_tab + n1; P.pass = 1;
    int rc = be->run_minimizer_seeds_of(P);
    // (a 32-bit prefix sum: the hits of the taken minimizers of one call stay below 2^32 — checked against the index's own size below)
    if (!rc) rc = be->scan_u32(d_tab, d_tab + n1, (uint32_t)n1);
    std::vector<uint32_t> first(n1);
    if (!rc) rc = be->download(first.data(), d_tab + n1, sizeof(uint32_t) * n1);
    if (rc) return rc;
    uint64_t check = 0;
    for (size_t j = 0; j < n_minimizers; ++j) if (take[j]) check += minimizers[j].hits;
    if (check > INDEX_MOST) return VGK_ETOOBIG;
    for (size_t j = 0; j < n1; ++j) seed_off[j] = first[j];
    const size_t total = first[n];
    if (written) *written = total;
    if (total > cap) return VGK_EOPS;
    if (!total) return VGK_OK;
    vgk_seed* d_out = (vgk_seed*)ctx->ensure_scratch(MZLIST_SEEDS, sizeof(vgk_seed) * total);
    if (!d_out) return VGK_ENOMEM;
    P.out = d_out; P.pass = 2;
    if ((rc = be->run_minimizer_seeds_of(P))) return rc;
    return be->download(seeds, d_out, sizeof(vgk_seed) * total);
}
int vgk_minimizer_seeds_of(vgk_ctx* ctx, const vgk_minimizer_index* ix, const vgk_read_minimizer* minimizers, const uint8_t* take, size_t n_minimizers,
                           uint64_t* seed_off, vgk_seed* seeds, size_t cap, size_t* written) try {
    if (!ctx || !ix || !vgk_tables_usable(ix->ctx, ctx) || !seed_off || (n_minimizers && (!minimizers || !take)) || (!seeds && cap)) return VGK_EINVAL;
    if (written) *written = 0;
    seed_off[0] = 0;
    if (!n_minimizers) return VGK_OK;
    if (n_minimizers > INDEX_MOST) return VGK_ETOOBIG;
    Backend* be = ctx->be.get();
    std::lock_guard<std::mutex> lk(ctx->mu);
    vgk_read_minimizer* d_min = (vgk_read_minimizer*)ctx->ensure_scratch(MZLIST_MINIMIZERS, sizeof(vgk_read_minimizer) * n_minimizers);
    uint8_t* d_take = (uint8_t*)ctx->ensure_scratch(MZLIST_TAKE, n_minimizers + 16);
    if (!d_min || !d_take) return VGK_ENOMEM;
    int rc = be->upload(d_min, minimizers, sizeof(vgk_read_minimizer) * n_minimizers);
    if (!rc) rc = be->upload(d_take, take, n_minimizers);
    if (rc) return rc;
    return seeds_of_on_device(ctx, ix, minimizers, take, n_minimizers, seed_off, seeds, cap, written);
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }

// ---- find_seeds' choice on the device (include/vgk_engine.h; minimizer_device.hpp: mz_choose_one is the rule) --------------------------------------
namespace {
// the policy as the kernels read it; its score table (the host's logarithm, as vgk_minimizer_set_policy makes it) goes to MZCHOOSE_TAB
int choose_policy(vgk_ctx* ctx, const vgk_find_seeds_policy* p, MzChoosePolicy* Q) {
    if (!p->hard_hit_cap || p->hard_hit_cap > 65535u || !(p->minimizer_score_fraction >= 0.0 && p->minimizer_score_fraction <= 1.0)) return VGK_EINVAL;
    std::vector<double> tab((size_t)p->hard_hit_cap + 1, 0.0);
    const double base = 1.0 + std::log((double)p->hard_hit_cap);
    for (uint32_t h = 1; h <= p->hard_hit_cap; ++h) tab[h] = base - std::log((double)h);
    for (uint32_t h = 2; h <= p->hard_hit_cap; ++h) if (!(tab[h] < tab[h - 1])) return VGK_EINVAL;      // (mz_choose_rank stands on it; consecutive logarithms are far more than an ulp apart)
    if (!(tab[p->hard_hit_cap] > 0.0)) return VGK_EINVAL;
    const double* d = ctx->scratch_dev<double>(MZCHOOSE_TAB, tab.data(), sizeof(double) * tab.size());
    if (!d) return VGK_ENOMEM;
    const int rc = ctx->be->sync();                                        // (tab may go)
    if (rc) return rc;
    Q->hit_cap = p->hit_cap; Q->hard_hit_cap = p->hard_hit_cap; Q->fraction = p->minimizer_score_fraction; Q->tab = d;
    Q->max_unique_min = p->max_unique_min; Q->num_bp_per_min = p->num_bp_per_min; Q->flank = p->minimizer_coverage_flank; Q->exclude_overlapping = p->exclude_overlapping_min;
    Q->window_count = p->minimizer_downsampling_window_count; Q->max_window = p->minimizer_downsampling_max_window_length;
    Q->over_rank = mz_over_rank(tab.data(), p->hard_hit_cap);
    return VGK_OK;
}
// the choice kernels over a list in HBM (P: everything but ids and the slab): the reads that fit LDS a workgroup each, the others over slabs
int choose_on_device(vgk_ctx* ctx, MzChooseParams P, const uint64_t* read_off, const uint64_t* minimizer_off, uint32_t n) {
    Backend* be = ctx->be.get();
    const auto minimizers_of = [&](uint32_t r) { return minimizer_off[r + 1] - minimizer_off[r]; };
    const auto bases_of = [&](uint32_t r) { return read_off[r + 1] - read_off[r]; };
    for (uint32_t r = 0; r < n; ++r) {
        const uint64_t m = minimizers_of(r), L = bases_of(r);
        if (!m) continue;
        if (m > 0x80000000ull || L > INDEX_MOST) return VGK_ETOOBIG;
        const uint64_t window = mz_choose_window(P.policy, L, P.k);
        if (window && P.k > window) return VGK_EINVAL;                     // (find_seeds' crash_unless(length <= window))
    }
    const SlabPlan plan = slab_plan(n, [&](uint32_t r) {
        if (!minimizers_of(r)) return ROUTE_SKIP;                              // nothing to choose from: in neither launch
        return minimizers_of(r) <= MZ_CHOOSE_LDS_MAX && bases_of(r) <= MZ_CHOOSE_LDS_BASES ? ROUTE_LDS : ROUTE_SLAB;
    }, minimizers_of);
    ctx->minimizer_choose_ms = 0.0;
    if (plan.ids.empty()) return VGK_OK;
    const uint32_t* d_ids = ctx->scratch_dev<uint32_t>(MZCHOOSE_IDS, plan.ids.data(), sizeof(uint32_t) * plan.ids.size());
    if (!d_ids) return VGK_ENOMEM;
    uint32_t blocks = 0; char* slab = nullptr;
    if (plan.n_large) {
        uint64_t max_L = 0;                                                // the slab's second size: the longest large read
        for (uint32_t j = 0; j < plan.n_large; ++j) max_L = std::max<uint64_t>(max_L, bases_of(plan.large()[j]));
        P.slab_np = (uint32_t)pow2_at_least(plan.slab_largest); P.slab_words = (uint32_t)((max_L + 64) / 64);
        P.slab_stride = mz_choose_slab_bytes(P.slab_np, P.slab_words);
        blocks = slab_blocks(plan.n_large, P.slab_stride);
        slab = (char*)ctx->ensure_scratch(MZCHOOSE_SLAB, P.slab_stride * blocks);
        if (!slab) return VGK_ENOMEM;
    }
    Timed t(be, &ctx->minimizer_choose_ms);
    const int rc = launch_split(P, d_ids, plan, slab, blocks, [&](const MzChooseParams& L, uint32_t grid) { return be->run_minimizer_choose(L, grid); });
    const int rs = t.done();                                               // (ids may go)
    return rc ? rc : rs;
}
}  // namespace

int vgk_minimizer_choose(vgk_ctx* ctx, const vgk_find_seeds_policy* policy, uint32_t k, const char* reads, const uint64_t* read_off, uint32_t n,
                         const uint64_t* minimizer_off, const vgk_read_minimizer* minimizers, uint8_t* verdict) try {
    if (!ctx || !policy || !k || k > MZ_MAX_K || (n && (!read_off || !minimizer_off))) return VGK_EINVAL;
    if (!n) return VGK_OK;
    if (minimizer_off[0] != 0) return VGK_EINVAL;
    for (uint32_t r = 0; r < n; ++r) {
        if (read_off[r + 1] < read_off[r] || minimizer_off[r + 1] < minimizer_off[r]) return VGK_EINVAL;
        if (minimizer_off[r + 1] > minimizer_off[r] && !minimizers) return VGK_EINVAL;
        const uint64_t L = read_off[r + 1] - read_off[r];
        for (uint64_t j = minimizer_off[r]; j < minimizer_off[r + 1]; ++j) {
            if ((uint64_t)minimizers[j].offset + k > L) return VGK_EINVAL;
            if (j > minimizer_off[r] && minimizers[j].offset < minimizers[j - 1].offset) return VGK_EINVAL;
        }
    }
    const uint64_t total = minimizer_off[n], bytes = read_off[n] - read_off[0];
    if (!total) return VGK_OK;
    if (!verdict || (bytes && !reads)) return VGK_EINVAL;
    if (total > INDEX_MOST || bytes > INDEX_MOST) return VGK_ETOOBIG;
    Backend* be = ctx->be.get();
    std::lock_guard<std::mutex> lk(ctx->mu);
    MzChooseParams P{};
    int rc = choose_policy(ctx, policy, &P.policy);
    if (rc) return rc;
    const size_t n1 = (size_t)n + 1;
    std::vector<uint64_t> rel(n1);
    for (size_t i = 0; i < n1; ++i) rel[i] = read_off[i] - read_off[0];
    char* d_reads = ctx->scratch_dev<char>(MZLIST_READS, bytes ? reads + read_off[0] : nullptr, bytes);
    const uint64_t* d_off = ctx->scratch_dev<uint64_t>(MZLIST_READ_OFF, rel.data(), sizeof(uint64_t) * n1);
    const uint64_t* d_moff = ctx->scratch_dev<uint64_t>(MZCHOOSE_MIN_OFF, minimizer_off, sizeof(uint64_t) * n1);
    const vgk_read_minimizer* d_min = ctx->scratch_dev<vgk_read_minimizer>(MZLIST_MINIMIZERS, minimizers, sizeof(vgk_read_minimizer) * total);
    uint8_t* d_verdict = (uint8_t*)ctx->ensure_scratch(MZLIST_TAKE, total + 16);
    if (!d_reads || !d_off || !d_moff || !d_min || !d_verdict) return VGK_ENOMEM;
    P.k = k; P.reads = d_reads; P.read_off = d_off; P.min_off = d_moff; P.mins = d_min; P.verdict = d_verdict; P.as_take = 0;
    if ((rc = choose_on_device(ctx, P, rel.data(), minimizer_off, n))) return rc;
    return be->download(verdict, d_verdict, total);
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }

int vgk_minimizer_find_seeds(vgk_ctx* ctx, const vgk_minimizer_index* ix, const vgk_find_seeds_policy* policy, const char* reads, const uint64_t* read_off, uint32_t n,
                             uint64_t* minimizer_off, vgk_read_minimizer* minimizers, uint8_t* take, size_t cap_m,
                             uint64_t* seed_off, vgk_seed* seeds, size_t cap_s, size_t written[2]) try {
    if (!ctx || !ix || !policy || !vgk_tables_usable(ix->ctx, ctx) || !minimizer_off || !written || (n && (!reads || !read_off)) || (cap_m && (!minimizers || !take || !seed_off)) || (!seeds && cap_s)) return VGK_EINVAL;
    written[0] = written[1] = 0;
    minimizer_off[0] = 0;
    if (seed_off) seed_off[0] = 0;
    if (!n) return VGK_OK;
    Backend* be = ctx->be.get();
    std::lock_guard<std::mutex> lk(ctx->mu);
    MzChooseParams P{};
    int rc = choose_policy(ctx, policy, &P.policy);
    if (rc) return rc;
    // the list is made in HBM whatever room the caller has: the needed sizes of BOTH outputs are then known from one call
    size_t total = 0;
    if ((rc = list_on_device(ctx, ix, reads, read_off, n, minimizer_off, (size_t)-1, &total))) return rc;
    written[0] = total;
    if (!total) return VGK_OK;
    const size_t n1 = (size_t)n + 1;
    std::vector<uint64_t> rel(n1);
    for (size_t i = 0; i < n1; ++i) rel[i] = read_off[i] - read_off[0];
    const uint64_t* d_moff = ctx->scratch_dev<uint64_t>(MZCHOOSE_MIN_OFF, minimizer_off, sizeof(uint64_t) * n1);
    uint8_t* d_take = (uint8_t*)ctx->ensure_scratch(MZLIST_TAKE, total + 16);
    if (!d_moff || !d_take) return VGK_ENOMEM;
    P.k = ix->dev.k; P.reads = (const char*)ctx->scratch[MZLIST_READS].p + 8; P.read_off = (const uint64_t*)ctx->scratch[MZLIST_READ_OFF].p; P.min_off = d_moff;
    P.mins = (const vgk_read_minimizer*)ctx->scratch[MZLIST_MINIMIZERS].p; P.verdict = d_take; P.as_take = 1;
    if ((rc = choose_on_device(ctx, P, rel.data(), minimizer_off, n))) return rc;
    // list and choice come down (into the caller's arrays when they are large enough), the seeds of the taken are counted and written
    std::vector<vgk_read_minimizer> own_m; std::vector<uint8_t> own_t; std::vector<uint64_t> own_s;
    const bool fits = total <= cap_m;
    if (!fits) { own_m.resize(total); own_t.resize(total); own_s.resize(total + 1); }
    vgk_read_minimizer* hm = fits ? minimizers : own_m.data(); uint8_t* ht = fits ? take : own_t.data();
    if ((rc = be->download(hm, P.mins, sizeof(vgk_read_minimizer) * total))) return rc;
    if ((rc = be->download(ht, d_take, total))) return rc;
    rc = seeds_of_on_device(ctx, ix, hm, ht, total, fits ? seed_off : own_s.data(), fits ? seeds : nullptr, fits ? cap_s : 0, &written[1]);
    if (rc) return rc;
    return fits ? VGK_OK : VGK_EOPS;
} catch (const std::bad_alloc&) { return VGK_ENOMEM; } catch (...) { return VGK_EINVAL; }

double vgk_minimizer_choose_last_ms(vgk_ctx* ctx) { return ctx ? ctx->minimizer_choose_ms : 0.0; }

}  // extern "C"
