// launch_split_san_main.cpp — the launch plans of vg_amd/csrc/launch_split.hpp as a program of its own, built with the host sanitizers (make
// launch_split_san): the index arithmetic that decides which item runs in which launch and which slice of the slab a lane writes, held to a brute
// force written here.  It needs no GPU and no engine: the header is all it includes.
// Test infrastructure only (tests/test_launch_split.py builds and runs it).
//
//   launch_split_san          exits 0, or prints the first violated statement with its case and exits 1
#include <cstdio>
#include <string>
#include "launch_split.hpp"

using namespace vgk;

namespace {
std::string at;                                                   // the case under test, for the message
#define HOLDS(cond) do { if (!(cond)) { std::fprintf(stderr, "launch_split: violated: %s  [%s]\n", #cond, at.c_str()); return false; } } while (0)

const uint32_t SIZES[] = {0, 1, 63, 64, 65, 1000};
const char* const PATTERNS[] = {"none", "all", "first", "last", "alternating"};
bool in_pattern(int pattern, uint32_t i, uint32_t n) { return pattern == 1 || (pattern == 2 && i == 0) || (pattern == 3 && i + 1 == n) || (pattern == 4 && (i & 1)); }

// ids: a permutation of the expected items — `small` ascending, then `large` ascending
bool ids_are(const LaunchSplit& s, const std::vector<uint32_t>& small, const std::vector<uint32_t>& large) {
    HOLDS(s.n_lds == small.size());
    HOLDS(s.n_large == large.size());
    HOLDS(s.ids.size() == small.size() + large.size());
    for (size_t j = 0; j < small.size(); ++j) HOLDS(s.ids[j] == small[j]);
    for (size_t j = 0; j < large.size(); ++j) HOLDS(s.large()[j] == large[j]);
    return true;
}

// words: 0 = every slice empty, 1 = one word each, 2 = the slices' sum lands on INDEX_MOST, 3 = one past it
bool slice_case(uint32_t n, int pattern, int words) {
    at = "slice plan, n " + std::to_string(n) + ", large: " + PATTERNS[pattern] + ", words case " + std::to_string(words);
    std::vector<uint32_t> small, large;                           // the brute force
    for (uint32_t i = 0; i < n; ++i) (in_pattern(pattern, i, n) ? large : small).push_back(i);
    const auto words_of = [&](uint32_t i) -> uint64_t {
        if (words < 2) return (uint64_t)words;
        return i != large.back() ? 1 : INDEX_MOST - (large.size() - 1) + (words == 3 ? 1 : 0);
    };
    const SlicePlan s = slice_plan(n, [&](uint32_t i) { return in_pattern(pattern, i, n); }, words_of);
    if (!ids_are(s, small, large)) return false;
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t id : s.ids) { HOLDS(id < n); HOLDS(!seen[id]); seen[id] = 1; }
    HOLDS(s.ids.size() == n);
    for (uint32_t j = 0; j < s.n_lds; ++j) HOLDS(!in_pattern(pattern, s.ids[j], n) && (!j || s.ids[j - 1] < s.ids[j]));
    for (uint32_t j = 0; j < s.n_large; ++j) HOLDS(in_pattern(pattern, s.large()[j], n) && (!j || s.large()[j - 1] < s.large()[j]));
    HOLDS(s.work_off.size() == large.size());
    uint64_t before = 0;
    for (size_t j = 0; j < large.size(); ++j) { HOLDS(s.work_off[j] == before); before += words_of(large[j]); }
    HOLDS(s.work_words == before);
    HOLDS(s.rc == (before > INDEX_MOST ? VGK_ETOOBIG : VGK_OK));
    if (words == 2 && !large.empty()) HOLDS(before == INDEX_MOST && s.rc == VGK_OK);
    if (words == 3 && !large.empty()) HOLDS(before == INDEX_MOST + 1 && s.rc == VGK_ETOOBIG);
    return true;
}

// routes: 0 = skip | LDS | slab in turn, 1 = every item skipped, 2 = the slice plan's patterns without a skip
bool slab_case(uint32_t n, int routes, int pattern) {
    at = "slab plan, n " + std::to_string(n) + ", routes case " + std::to_string(routes) + ", large: " + PATTERNS[pattern];
    const auto route_of = [&](uint32_t i) { return routes == 1 ? ROUTE_SKIP : routes == 0 ? (Route)(i % 3) : in_pattern(pattern, i, n) ? ROUTE_SLAB : ROUTE_LDS; };
    const auto size_of = [](uint32_t i) { return (uint64_t)i * 7919u % 1000u + 1u; };
    std::vector<uint32_t> small, large; uint64_t lds_largest = 0, slab_largest = 0;      // the brute force
    for (uint32_t i = 0; i < n; ++i) {
        if (route_of(i) == ROUTE_LDS) { small.push_back(i); lds_largest = std::max(lds_largest, size_of(i)); }
        if (route_of(i) == ROUTE_SLAB) { large.push_back(i); slab_largest = std::max(slab_largest, size_of(i)); }
    }
    const SlabPlan s = slab_plan(n, route_of, size_of);
    if (!ids_are(s, small, large)) return false;
    for (uint32_t id : s.ids) HOLDS(id < n && route_of(id) != ROUTE_SKIP);
    HOLDS(s.lds_largest == lds_largest);
    HOLDS(s.slab_largest == slab_largest);
    return true;
}

bool grid_cases() {
    const uint64_t G = 1ull << 30;
    const uint64_t larges[] = {0, 1, 511, 512, 513}, strides[] = {1, G - 1, G, G + 1, 1ull << 40, G / 512, G / 256};
    for (uint64_t n_large : larges) for (uint64_t stride : strides) {
        at = "slab_blocks(" + std::to_string(n_large) + ", " + std::to_string(stride) + ")";
        const uint64_t slabs = stride > G ? 1 : G / stride;        // slabs in 1 GiB, and one at least
        uint64_t want = n_large;
        if (want > 512) want = 512;
        if (want > slabs) want = slabs;
        HOLDS(slab_blocks(n_large, stride) == want);
        if (n_large) HOLDS(slab_blocks(n_large, stride) >= 1);
    }
    at = "slab_blocks, the points by hand";
    HOLDS(slab_blocks(513, 1) == 512 && slab_blocks(511, 1) == 511 && slab_blocks(513, 1ull << 40) == 1 && slab_blocks(513, G + 1) == 1 && slab_blocks(513, G / 256) == 256 && slab_blocks(0, 1) == 0);
    at = "pow2_at_least";
    HOLDS(pow2_at_least(0) == 1 && pow2_at_least(1) == 1 && pow2_at_least(2) == 2 && pow2_at_least(3) == 4 && pow2_at_least(1024) == 1024 && pow2_at_least(1025) == 2048);
    HOLDS(pow2_at_least(0x80000000ull) == 0x80000000ull && pow2_at_least(0x80000001ull) == 0x100000000ull);
    return true;
}
}  // namespace

int main() {
    for (uint32_t n : SIZES) for (int pattern = 0; pattern < 5; ++pattern) {
        for (int words = 0; words < 4; ++words) if (!slice_case(n, pattern, words)) return 1;
        if (!slab_case(n, 2, pattern)) return 1;
    }
    for (uint32_t n : SIZES) for (int routes = 0; routes < 2; ++routes) if (!slab_case(n, routes, 0)) return 1;
    if (!grid_cases()) return 1;
    return 0;
}
