// staged_upload.hpp — a caller's flat buffer on its way to HBM: host threads copy it into page-locked staging, slice by slice, and each slice
// starts its way up on the side stream as soon as it is there (the caller's buffers are pageable: a direct copy would be staged by the runtime
// on one thread).  Shared by the window packers (window_api.cpp, gssw_wide_window_api.cpp).
#pragma once
#include <algorithm>
#include <cstring>
#include "ctx.hpp"
#include "host_parallel.hpp"

inline int staged_upload(vgk::Backend* be, vgk_ctx::Staging& staging, int slot, void* dst, const void* src, uint64_t bytes) {
    if (!bytes) return VGK_OK;
    uint8_t* st = (uint8_t*)staging.get(slot, bytes);
    if (!st) return VGK_ENOMEM;
    const uint64_t SLICE = 16ull << 20, PIECE = 256ull << 10;
    for (uint64_t at = 0; at < bytes; at += SLICE) {
        const uint64_t len = std::min(SLICE, bytes - at);
        parallel_tasks((uint32_t)((len + PIECE - 1) / PIECE), [&](uint32_t c) {
            const uint64_t o = at + (uint64_t)c * PIECE;
            std::memcpy(st + o, (const uint8_t*)src + o, (size_t)std::min(PIECE, at + len - o));
        });
        const int e = be->upload_side((uint8_t*)dst + at, st + at, len);
        if (e) return e;
    }
    return VGK_OK;
}
