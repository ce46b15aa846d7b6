// chain_stitch_san_main.cpp — one vgk_haplo_create + vgk_chain_stitch call on the emulated backend as a program of its own, built with the host
// sanitizers (make chainstitch_san): the lane code of chain_device.hpp — bounds, stretches, the in-place joins, the gather — and the host half's
// sizing of the work arrays run under AddressSanitizer and UBSan on the CPU.
// Test infrastructure only (tests/test_chain_stitch_definition.py writes the call and compares the output with the emulator library's).
//
//   chain_stitch_san <call file> <output file>
//
// call file (little endian): "VGKC" | u32 n_nodes | u32 node_len[n_nodes] | bases | u32 n_threads | u32 thread_off[n_threads + 1] | u32 thread_nodes[] |
//   u32 n_reads | u64 piece_off[n_reads + 1] | vgk_chain_piece pieces[] | u64 n | u32 nodes[n] | u64 n | vgk_chain_mapping mappings[n] | u64 n | u32 edits[n] |
//   u64 mapping_cap | u64 edit_cap
// output file: i32 status of vgk_haplo_create | i32 status of vgk_chain_stitch | u64 written[2] | results[n_reads] |
//   mappings[min(written[0], mapping_cap)] | edits[min(written[1], edit_cap)]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "vgk.h"

namespace {
struct Reader {
    std::vector<unsigned char> buf; size_t at = 0; bool ok = true;
    void get(void* out, size_t n) { if (n > buf.size() - at) { ok = false; std::memset(out, 0, n); return; } std::memcpy(out, buf.data() + at, n); at += n; }
    uint32_t u32() { uint32_t v; get(&v, 4); return v; }
    uint64_t u64() { uint64_t v; get(&v, 8); return v; }
    template <class T> std::vector<T> many(size_t n) { if (n > (buf.size() - at) / sizeof(T)) { ok = false; return {}; } std::vector<T> v(n); if (n) get(v.data(), n * sizeof(T)); return v; }
};
template <class T> void put(FILE* f, const T* p, size_t n) { if (n) std::fwrite(p, sizeof(T), n, f); }
}

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s <call file> <output file>\n", argv[0]); return 2; }
    Reader r;
    { FILE* f = std::fopen(argv[1], "rb"); if (!f) { std::perror(argv[1]); return 2; }
      unsigned char chunk[65536]; size_t n; while ((n = std::fread(chunk, 1, sizeof chunk, f)) > 0) r.buf.insert(r.buf.end(), chunk, chunk + n);
      std::fclose(f); }
    char magic[4]; r.get(magic, 4);
    if (std::memcmp(magic, "VGKC", 4) != 0) { std::fprintf(stderr, "not a call file\n"); return 2; }
    const uint32_t n_nodes = r.u32();
    std::vector<uint32_t> node_len = r.many<uint32_t>(n_nodes);
    size_t total = 0; for (uint32_t l : node_len) total += l;
    std::vector<char> bases = r.many<char>(total);
    const uint32_t n_threads = r.u32();
    std::vector<uint32_t> thread_off = r.many<uint32_t>((size_t)n_threads + 1);
    std::vector<uint32_t> thread_nodes = r.many<uint32_t>(n_threads && r.ok ? thread_off[n_threads] : 0);
    const uint32_t n_reads = r.u32();
    std::vector<uint64_t> piece_off = r.many<uint64_t>((size_t)n_reads + 1);
    std::vector<vgk_chain_piece> pieces = r.many<vgk_chain_piece>(r.ok ? (size_t)piece_off[n_reads] : 0);
    std::vector<uint32_t> nodes = r.many<uint32_t>((size_t)r.u64());
    std::vector<vgk_chain_mapping> mappings = r.many<vgk_chain_mapping>((size_t)r.u64());
    std::vector<uint32_t> edits = r.many<uint32_t>((size_t)r.u64());
    const uint64_t mapping_cap = r.u64(), edit_cap = r.u64();
    if (!r.ok) { std::fprintf(stderr, "call file truncated\n"); return 2; }
    if (bases.empty()) bases.push_back('A');
    if (thread_nodes.empty()) thread_nodes.push_back(0);

    vgk_scoring scoring{};                                  // (stitch scores nothing: the reference's defaults 1 / 4 / 6 / 1 / 5, as capi.Engine has them)
    for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) scoring.matrix[5 * a + b] = a == b ? 1 : -4;
    scoring.gap_open = 6; scoring.gap_extend = 1; scoring.full_length_bonus = 5;
    vgk_ctx* ctx = nullptr;
    if (int rc = vgk_create(0, &scoring, &ctx)) { std::fprintf(stderr, "vgk_create: %d\n", rc); return 3; }
    vgk_haplotypes hd; hd.n_nodes = n_nodes; hd.node_len = node_len.data(); hd.seq = bases.data(); hd.n_threads = n_threads; hd.thread_off = thread_off.data(); hd.thread_nodes = thread_nodes.data();
    vgk_haplo* index = nullptr;
    const int32_t create_rc = vgk_haplo_create(ctx, &hd, &index);
    // (the output arrays are exactly as long as the caps say: a write past either is the sanitizer's to find)
    std::vector<vgk_chain_result> results(n_reads);
    std::vector<vgk_chain_mapping> out_m((size_t)mapping_cap); std::vector<uint32_t> out_e((size_t)edit_cap);
    size_t written[2] = {0, 0};
    int32_t rc = 0;
    if (create_rc == VGK_OK)
        rc = vgk_chain_stitch(ctx, index, pieces.empty() ? nullptr : pieces.data(), piece_off.data(), n_reads, nodes.empty() ? nullptr : nodes.data(), nodes.size(),
                              mappings.empty() ? nullptr : mappings.data(), mappings.size(), edits.empty() ? nullptr : edits.data(), edits.size(),
                              results.data(), out_m.empty() ? nullptr : out_m.data(), out_m.size(), out_e.empty() ? nullptr : out_e.data(), out_e.size(), written);
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::perror(argv[2]); return 2; }
    const uint64_t w[2] = {written[0], written[1]};
    put(out, &create_rc, 1); put(out, &rc, 1); put(out, w, 2);
    put(out, results.data(), n_reads);
    put(out, out_m.data(), (size_t)std::min<uint64_t>(w[0], mapping_cap)); put(out, out_e.data(), (size_t)std::min<uint64_t>(w[1], edit_cap));
    std::fclose(out);
    if (index) vgk_haplo_destroy(index);
    vgk_destroy(ctx);
    return 0;
}
