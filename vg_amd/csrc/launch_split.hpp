// launch_split.hpp — the plan of a call whose items run in two launches: those whose working set fits a fixed piece of LDS first,
// the few large ones behind them in the same `ids` array, over a slab in HBM.  Host only, and plain C++17: no HIP, no context — tests/emu/
// launch_split_san_main.cpp runs all of it without a GPU.  The launches themselves are ctx.hpp's launch_split().
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "vgk.h"

namespace vgk {

// the largest count or total that a 32-bit index of the kernels may carry
constexpr uint64_t INDEX_MOST = 0xfffffff0ull;

inline uint64_t pow2_at_least(uint64_t n) { uint64_t np = 1; while (np < n) np <<= 1; return np; }

// ids[0, n_lds): the items of the LDS launch in index order; ids[n_lds, n_lds + n_large): the slab's, in index order
struct LaunchSplit {
    std::vector<uint32_t> ids; uint32_t n_lds = 0, n_large = 0;
    const uint32_t* large() const { return ids.data() + n_lds; }
};

// ---- a wavefront (or workgroup) per item: every block of the second launch owns one slab of `stride` bytes and strides over the large items
enum Route { ROUTE_SKIP, ROUTE_LDS, ROUTE_SLAB };                 // ROUTE_SKIP: the item is in neither launch
struct SlabPlan : LaunchSplit { uint64_t lds_largest = 0, slab_largest = 0; };      // the largest size(i) of either launch (0: none)
template <class RouteOf, class SizeOf> SlabPlan slab_plan(uint32_t n, RouteOf route, SizeOf size) {
    SlabPlan s;
    s.ids.resize(n);
    uint32_t lo = 0, hi = n;                                      // the large ones from the back, turned round below
    for (uint32_t i = 0; i < n; ++i) {
        const Route r = route(i);
        if (r == ROUTE_SKIP) continue;
        uint64_t& largest = r == ROUTE_LDS ? s.lds_largest : s.slab_largest;
        largest = std::max<uint64_t>(largest, size(i));
        if (r == ROUTE_LDS) s.ids[lo++] = i; else s.ids[--hi] = i;
    }
    s.n_lds = lo; s.n_large = n - hi;
    std::reverse(s.ids.begin() + hi, s.ids.end());
    if (lo != hi) std::move(s.ids.begin() + hi, s.ids.end(), s.ids.begin() + lo);
    s.ids.resize((size_t)lo + s.n_large);
    return s;
}
// blocks of the second launch: no more than large items, than 512, than slabs of `stride` bytes in 1 GiB — and one at least
inline uint32_t slab_blocks(uint64_t n_large, uint64_t stride) {
    return (uint32_t)std::min<uint64_t>(std::min<uint64_t>(n_large, 512), std::max<uint64_t>(1, (1ull << 30) / stride));
}

// ---- a lane per item: every large item owns words(i) words of the slab, at work_off[j] for the j-th of them.  An item that the caller's checks
// refused is "not large": its lane writes the verdict in the first launch and touches no slice
struct SlicePlan : LaunchSplit {
    std::vector<uint64_t> work_off; uint64_t work_words = 0;
    int rc = VGK_OK;                                              // VGK_ETOOBIG: more words than a 32-bit index carries
};
template <class IsLarge, class WordsOf> SlicePlan slice_plan(uint32_t n, IsLarge is_large, WordsOf words) {
    SlicePlan s;
    static_cast<LaunchSplit&>(s) = slab_plan(n, [&](uint32_t i) { return is_large(i) ? ROUTE_SLAB : ROUTE_LDS; }, [](uint32_t) { return 0u; });
    s.work_off.reserve(s.n_large);
    for (uint32_t j = 0; j < s.n_large; ++j) { s.work_off.push_back(s.work_words); s.work_words += words(s.large()[j]); }
    if (s.work_words > INDEX_MOST) s.rc = VGK_ETOOBIG;
    return s;
}

}  // namespace vgk
