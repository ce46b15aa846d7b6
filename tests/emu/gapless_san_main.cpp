// gapless_san_main.cpp — one vgk_haplo_create + vgk_gapless_extend call on the emulated backend as a program of its own, built with the host
// sanitizers (make gapless_san): the lane code of gapless_device.hpp and its per-thread slabs run under AddressSanitizer and UBSan on the CPU.
// Test infrastructure only (tests/test_gapless_definition.py writes the call and compares the output with the emulator library's).
//
//   gapless_san <call file> <output file>
//
// call file (little endian): "VGKG" | vgk_scoring (29 bytes) | u32 n_nodes | u32 node_len[n_nodes] | bases | u32 n_threads |
//   u32 thread_off[n_threads + 1] | u32 thread_nodes[] | u32 n_problems | per problem { u32 read_len, n_seeds, max_mismatches, flags; f64 overlap } |
//   reads, behind each other | seeds { u32 node; i32 diff }, behind each other
// output file: i32 status of vgk_haplo_create | i32 status of vgk_gapless_extend | u64 written[3] | results | extensions | nodes | mismatches
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "vgk.h"

namespace {
struct Reader {
    std::vector<unsigned char> buf; size_t at = 0; bool ok = true;
    void get(void* out, size_t n) { if (at + n > buf.size()) { ok = false; std::memset(out, 0, n); return; } std::memcpy(out, buf.data() + at, n); at += n; }
    uint32_t u32() { uint32_t v; get(&v, 4); return v; }
    template <class T> std::vector<T> many(size_t n) { std::vector<T> v(n); if (n) get(v.data(), n * sizeof(T)); return v; }
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
    if (std::memcmp(magic, "VGKG", 4) != 0) { std::fprintf(stderr, "not a call file\n"); return 2; }
    vgk_scoring scoring; r.get(&scoring, sizeof scoring);
    const uint32_t n_nodes = r.u32();
    std::vector<uint32_t> node_len = r.many<uint32_t>(n_nodes);
    size_t total = 0; for (uint32_t l : node_len) total += l;
    std::vector<char> bases = r.many<char>(total);
    const uint32_t n_threads = r.u32();
    std::vector<uint32_t> thread_off = r.many<uint32_t>((size_t)n_threads + 1);
    std::vector<uint32_t> thread_nodes = r.many<uint32_t>(n_threads ? thread_off[n_threads] : 0);
    const uint32_t n = r.u32();
    struct Head { uint32_t read_len, n_seeds, max_mismatches, flags; double overlap; };
    std::vector<Head> heads = r.many<Head>(n);
    size_t read_bytes = 0, n_seeds = 0; for (const Head& h : heads) { read_bytes += h.read_len; n_seeds += h.n_seeds; }
    std::vector<char> reads = r.many<char>(read_bytes);
    std::vector<vgk_seed> seeds = r.many<vgk_seed>(n_seeds);
    if (!r.ok) { std::fprintf(stderr, "call file truncated\n"); return 2; }
    if (bases.empty()) bases.push_back('A');
    if (thread_nodes.empty()) thread_nodes.push_back(0);
    if (reads.empty()) reads.push_back('A');
    if (seeds.empty()) seeds.push_back(vgk_seed{0, 0});

    vgk_ctx* ctx = nullptr;
    if (int rc = vgk_create(0, &scoring, &ctx)) { std::fprintf(stderr, "vgk_create: %d\n", rc); return 3; }
    vgk_haplotypes hd; hd.n_nodes = n_nodes; hd.node_len = node_len.data(); hd.seq = bases.data(); hd.n_threads = n_threads; hd.thread_off = thread_off.data(); hd.thread_nodes = thread_nodes.data();
    vgk_haplo* index = nullptr;
    const int32_t create_rc = vgk_haplo_create(ctx, &hd, &index);
    std::vector<vgk_gapless_problem> problems(n);
    size_t ext_cap = 1, node_cap = 1, mism_cap = 1;
    { size_t ra = 0, sa = 0;
      for (uint32_t i = 0; i < n; ++i) {
          vgk_gapless_problem& p = problems[i]; const Head& h = heads[i];
          p.read = reads.data() + ra; p.read_len = h.read_len; p.n_seeds = h.n_seeds; p.seeds = seeds.data() + sa;
          p.max_mismatches = h.max_mismatches; p.flags = h.flags; p.overlap_threshold = h.overlap;
          ra += h.read_len; sa += h.n_seeds;
          ext_cap += h.n_seeds; node_cap += (size_t)h.n_seeds * (h.read_len + 2); mism_cap += (size_t)h.n_seeds * h.read_len;
      } }
    std::vector<vgk_gapless_result> results(n);
    std::vector<vgk_extension> ext(ext_cap); std::vector<uint32_t> nodes(node_cap), mism(mism_cap);
    size_t written[3] = {0, 0, 0};
    int32_t extend_rc = 0;
    if (create_rc == VGK_OK) extend_rc = vgk_gapless_extend(ctx, index, problems.data(), n, results.data(), ext.data(), ext_cap, nodes.data(), node_cap, mism.data(), mism_cap, written);
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::perror(argv[2]); return 2; }
    const uint64_t w[3] = {written[0], written[1], written[2]};
    put(out, &create_rc, 1); put(out, &extend_rc, 1); put(out, w, 3);
    if (create_rc == VGK_OK && extend_rc == VGK_OK) { put(out, results.data(), n); put(out, ext.data(), written[0]); put(out, nodes.data(), written[1]); put(out, mism.data(), written[2]); }
    std::fclose(out);
    if (index) vgk_haplo_destroy(index);
    vgk_destroy(ctx);
    return 0;
}
