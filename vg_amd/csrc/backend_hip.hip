// backend_hip.hip — HIP runtime plumbing + the gfx950 kernel entry points.
// There is deliberately no CPU fallback here: if no HIP device answers,
// make_backend() fails and vgk_create() returns VGK_ENODEV.
#include <chrono>
#include <thread>
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <string>
#include "backend.hpp"
#include "pack_hip.hpp"

namespace vgk {

// one DPP wave_shr:1 — lane l receives lane l-1's value (lane 0 receives 0: bound_ctrl, so no old value has to be set up)
static __device__ __forceinline__ uint32_t from_lane_above(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x138 /* wave_shr:1 */, 0xf, 0xf, true);
}

// Fill: 4 independent wavefronts per workgroup; each wavefront owns
// floor(64/G) read pairs for the whole skewed sweep.  No barriers; LDS only as the staging buffer of the traceback records (below).
// Occupancy: K = 16 fits 128 VGPRs (4 waves/SIMD); K = 20/24 keep 4K+ state registers per
// lane and run 3 waves/SIMD (<= 168 VGPRs) rather than spill in the hot loop.
// Traceback records on their way out (tiled layout, gssw_device.hpp): a wavefront keeps the records of TB_TILE = 8 steps in LDS — written
// step-major, one 16-byte slot per lane and step (slot index XOR step: the flush below then reads conflict-free too) plus the part-B
// dwords — and every eighth step copies the tile to HBM in the layout the walker reads: 8 + 2 (K = 19 / 20) whole-wave 1-KB bursts per
// tile instead of two partial stores per step.  10 KB of LDS per wavefront (K = 19 / 20; 8 for K = 16, 12 for K = 24): 3 (4) wavefronts per
// SIMD still fit a CU's 160 KB.  One wavefront owns its buffer and LDS executes a wavefront's instructions in order: no barrier.
template <int K>
struct TbStage {
    static constexpr uint32_t REC = (K + 3) / 4, RB = REC - 4;                // dwords per record; of them in part B
    static constexpr uint32_t DWORDS = TB_TILE * 64u * REC;
    uint32_t* lds;                                                            // this wavefront's buffer: [8][64] x 16 B, then [8][64] x RB dwords
    __device__ __forceinline__ uint32_t* slot_a(uint32_t t, uint32_t lane) const { const uint32_t s = t % TB_TILE; return lds + (s * 64u + (lane ^ s)) * 4u; }
    __device__ __forceinline__ uint32_t* slot_b(uint32_t t, uint32_t lane) const { return lds + TB_TILE * 64u * 4u + ((t % TB_TILE) * 64u + lane) * RB; }
    __device__ __forceinline__ void flush(uint32_t* tile, uint32_t lane) const {      // tile = where this tile starts in HBM
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (uint32_t j = 0; j < TB_TILE; ++j) {                              // part A: 16-byte slot g of the tile = (lane g / 8, step g % 8)
            const uint32_t g = j * 64u + lane, L = g / TB_TILE, s = g % TB_TILE;
            const uint4 v = *reinterpret_cast<const uint4*>(lds + (s * 64u + (L ^ s)) * 4u);
            reinterpret_cast<uint4*>(tile)[g] = v;
        }
        if constexpr (RB > 0) {
            uint32_t* part_b = tile + TB_TILE * 64u * 4u;
            const uint32_t* lb = lds + TB_TILE * 64u * 4u;
#pragma unroll
            for (uint32_t j = 0; j < 2u * RB; ++j) {                          // part B: dword d of it = (record d / RB, component d % RB), record r = (lane r / 8, step r % 8)
                const uint32_t q = j * 64u + lane;
                uint4 v; uint32_t* w = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
                for (uint32_t c = 0; c < 4u; ++c) { const uint32_t d = 4u * q + c, r = d / RB, L = r / TB_TILE, st = r % TB_TILE; w[c] = lb[(st * 64u + L) * RB + d % RB]; }
                reinterpret_cast<uint4*>(part_b)[q] = v;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
};

// The walks at the end of a speculative batch's second fill (GsswParams::refill_walk; the NOKEY kernels below): lane s < 2 * (64 / G) takes the s-th read of its
// wavefront's pairs, the end cell the first fill's.  Everything the walks need — the parameter block, the wavefront, the lane — is read afresh here, through a
// copy of the kernel-argument pointer the optimiser cannot see through: nothing of it is live across the step loop, whose registers and instructions stay what
// they are without the walks.  (GsswParams is the kernel's only argument: the block starts at the segment's first byte.)
static __device__ __forceinline__ void refill_walk_own_reads(uint32_t wave) {
    typedef __attribute__((address_space(4))) const GsswParams KernArgs;
    KernArgs* kp = (KernArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));
    GsswParams P;
    __builtin_memcpy(&P, kp, sizeof P);
    if (!P.refill_walk) return;
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));      // (threadIdx.x & 63, without the register that holds threadIdx.x)
    const WaveDesc wd = P.waves[wave];
    // This wave's traceback codes / scratch columns -> visible to its walker lanes, which are lanes of the SAME wavefront: its stores have left for the L2
    // its loads go to (the CU's vector cache writes through) once they are waited for — a fence at workgroup scope.  __threadfence(), the agent-scope fence
    // of the whole-batch fused path below, also writes the L2's dirty lines back for the other dies' sake: with every wavefront of a fill that streams
    // codes out doing so, the second fill went from 1.37 to 2.91 ms per million reads (profiles/r10_refill_walk).
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    const uint32_t n_slots = 2u * (64u / wd.G);
    for (uint32_t slot = lane; slot < n_slots; slot += 64u) {
        const uint32_t pair = wd.first_pair + (slot >> 1);
        if (pair >= wd.pair_end) continue;
        const uint32_t prob = P.order[2u * pair + (slot & 1u)];
        if (prob != 0xffffffffu) walk_one(P, prob, P.best[prob]);
    }
}

// CODES = false: the recurrence alone and nothing of a traceback (GsswParams::spec_fill's first fill)
// NOKEY: the second fill of a speculative batch (spec_fill == 2) — codes only; the end cells are the first fill's, nothing is tracked or published.
//        With GsswParams::refill_walk each wavefront then walks the reads it filled (refill_walk_own_reads) and no gssw_walk_missed_kernel follows: a
//        wavefront's sixteen walks wait for their codes while the other wavefronts of its SIMD issue rows.  Built, exact, and OFF by default: on the MI355X
//        the fill with its walks takes 2.43 ms per million reads against 1.11 + 0.87 ms for the two kernels (profiles/r10_refill_walk) — 16 of 64 lanes hold a
//        168-register wavefront slot for the length of a walk, and the separate kernel's 2 000 wavefronts overlap their fetches better than that.
// OFFS: a KEY3 first fill whose rows run in the offset form (gssw_device.hpp: gssw_row_offset; GsswParams::row_off != 0)
template <int K, bool S8, bool REWALK, bool CODES = true, bool KEY3 = false, bool NOKEY = false, bool OFFS = false>
__global__ __launch_bounds__(256, (K <= 16 ? 4 : 3)) void gssw_fill_kernel(const GsswParams P) {
    constexpr uint32_t REC = (K + 3) / 4;   // dwords per (step, lane) traceback record
    __shared__ __attribute__((aligned(16))) uint32_t stage_lds[4][REWALK ? 64u * TB_BND_CHUNK * 2u : (TB_TILE > 1 ? TbStage<K>::DWORDS : 256u)];      // (also the fused walk's best keys, below)
    const uint32_t wave = P.wave_begin + blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (wave >= P.wave_begin + P.wave_count) return;
    if (P.wave_limit && wave - P.wave_begin >= *P.wave_limit) return;
    const WaveDesc wd = P.waves[wave];
    uint32_t wave_s = 0;             // (NOKEY: for the walks behind the step loop, in a scalar register)
    if constexpr (NOKEY) wave_s = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave);
    Lane<K> s;
#if VGK_PB_LDS
    __shared__ uint32_t pb_lds[4][64 * K];      // read B's profile words, [row][lane] per wavefront (gssw_device.hpp: VGK_PB_LDS)
    s.PBL = (typename Lane<K>::lds_u32*)(pb_lds[threadIdx.x >> 6] + lane);
#endif
    lane_init<K, NOKEY ? 1 : 0, OFFS ? 1 : 0>(s, P, wd, lane);
    asm volatile("" : "+v"(s.one));   // keep min(x,1) a packed min instead of cmp+cndmask
    uint32_t* tb = P.want_tb ? P.tb : nullptr;
    TbStage<K> stage{stage_lds[threadIdx.x >> 6]};
    // the first fill of a speculative batch runs its steady middle — every lane with a column of both reads — through a copy of the step that tests nothing for
    // being there (gssw_device.hpp, AV)
    uint32_t steady_from = 0, steady_to = 0;
    if constexpr (!CODES) {
        uint32_t shortest = s.RA < s.RB ? s.RA : s.RB;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)shortest, d, 64); shortest = o < shortest ? o : shortest; }
        steady_steps(wd.G, shortest, wd.n_steps, steady_from, steady_to);
        steady_from = (uint32_t)__builtin_amdgcn_readfirstlane((int)steady_from); steady_to = (uint32_t)__builtin_amdgcn_readfirstlane((int)steady_to);
    }
    if constexpr (!CODES) {
        // three loops, not a branch in one: the step's two copies share no block, and each loop keeps the registers of one
        uint32_t t = 0;
        for (; t < steady_from; ++t) {
            if ((t & 3u) == 0) lane_prefetch(s, P, t);
            const uint32_t rh = from_lane_above(s.out_h), rf = from_lane_above(s.out_f), ri = from_lane_above(s.info);
            lane_step<K, S8, false, KEY3, false, false, OFFS ? 1 : 0>(s, P, t, rh, rf, ri, nullptr, nullptr);
        }
        for (; t < steady_to; ++t) {
            if ((t & 3u) == 0) lane_prefetch(s, P, t);
            const uint32_t rh = from_lane_above(s.out_h), rf = from_lane_above(s.out_f), ri = from_lane_above(s.info);
            lane_step<K, S8, false, KEY3, false, true, OFFS ? 1 : 0>(s, P, t, rh, rf, ri, nullptr, nullptr);
        }
        for (; t < wd.n_steps; ++t) {
            if ((t & 3u) == 0) lane_prefetch(s, P, t);
            const uint32_t rh = from_lane_above(s.out_h), rf = from_lane_above(s.out_f), ri = from_lane_above(s.info);
            lane_step<K, S8, false, KEY3, false, false, OFFS ? 1 : 0>(s, P, t, rh, rf, ri, nullptr, nullptr);
        }
    }
    for (uint32_t t = 0; CODES && t < wd.n_steps; ++t) {
        if ((t & 3u) == 0) lane_prefetch(s, P, t);
        const uint32_t rh = from_lane_above(s.out_h);
        const uint32_t rf = from_lane_above(s.out_f);
        const uint32_t ri = from_lane_above(s.info);
        if constexpr (!CODES) {
        } else if constexpr (REWALK) {
            // the recurrence alone; what the traceback needs to run a window of it again (gssw_device.hpp, TB_REWALK)
            lane_step<K, S8, false, false, false, false, 0>(s, P, t, rh, rf, ri, nullptr, nullptr);
            if (tb) {
                // boundary rows: TB_BND_CHUNK steps gathered per lane in LDS (slot index XOR lane: the per-step writes and the flush's reads
                // both spread over the banks), then each lane's chunk leaves as one 128-byte line of the lane-major layout
                uint32_t* st = stage_lds[threadIdx.x >> 6] + lane * (TB_BND_CHUNK * 2u);
                const uint32_t slot = (t ^ lane) & (TB_BND_CHUNK - 1u);
                *reinterpret_cast<uint2*>(st + slot * 2u) = make_uint2(s.out_h, s.out_f);
                if ((t & (TB_BND_CHUNK - 1u)) == TB_BND_CHUNK - 1u || t + 1u == wd.n_steps) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
                    uint4* out = reinterpret_cast<uint4*>(tb + tb_bnd(wd.tb_off, wd.n_steps, t & ~(TB_BND_CHUNK - 1u), lane));
#pragma unroll
                    for (uint32_t j = 0; j < TB_BND_CHUNK; j += 2) {
                        const uint2 a = *reinterpret_cast<const uint2*>(st + ((j ^ lane) & (TB_BND_CHUNK - 1u)) * 2u), b = *reinterpret_cast<const uint2*>(st + (((j + 1u) ^ lane) & (TB_BND_CHUNK - 1u)) * 2u);
                        out[j >> 1] = make_uint4(a.x, a.y, b.x, b.y);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
                }
                lane_store_checkpoint<K>(s, P, wd, t, lane);
            }
        } else if constexpr (TB_TILE > 1) {
            lane_step<K, S8, true, false, NOKEY, false, 0>(s, P, t, rh, rf, ri, tb ? stage.slot_a(t, lane) : nullptr, stage.slot_b(t, lane));
            if (tb && ((t % TB_TILE) == TB_TILE - 1u || t + 1u == wd.n_steps)) stage.flush(tb + tb_tile_base(wd.tb_off, t, REC), lane);
        } else
            lane_step<K, S8, true, false, NOKEY, false, 0>(s, P, t, rh, rf, ri, tb ? tb + tb_dword(wd.tb_off, t, lane, REC, 0) : nullptr, tb ? tb + tb_dword(wd.tb_off, t, lane, REC, 4) : nullptr);
    }
    if constexpr (NOKEY) { refill_walk_own_reads(wave_s); return; }
    if (REWALK || !CODES || !P.fused) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            uint32_t prob; unsigned long long key;
            if (lane_best(s, half, prob, key)) atomicMax(&P.best[prob], key);
        }
        return;
    }
    // Fused traceback: the wavefront that filled a read pair also walks it back while its
    // traceback codes are still in L2 / Infinity Cache.  The walk is a latency-bound pointer
    // chase (one lane per read); the other wavefronts resident on the SIMD keep the VALU busy.
    unsigned long long* mine = reinterpret_cast<unsigned long long*>(stage_lds[threadIdx.x >> 6]);      // 128 keys: 1 KB of the wavefront's staging buffer
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        uint32_t prob; unsigned long long key = 0;
        if (!lane_best(s, half, prob, key)) key = 0;
        mine[lane * 2 + half] = key;
    }
    __threadfence();      // this wave's traceback codes / scratch columns -> visible to its walker lanes
    const uint32_t n_slots = 2u * (64u / wd.G);
    for (uint32_t slot = lane; slot < n_slots; slot += 64u) {
        const uint32_t q = slot >> 1, half = slot & 1u;
        if (wd.first_pair + q >= wd.pair_end) continue;
        const uint32_t prob = P.order[2u * (wd.first_pair + q) + half];
        if (prob == 0xffffffffu) continue;
        unsigned long long key = 0;
        for (uint32_t g = 0; g < wd.G; ++g) { const unsigned long long k = mine[(q * wd.G + g) * 2 + half]; key = k > key ? k : key; }
        walk_one(P, prob, key);
    }
}

// One thread per read, in the order the fill placed the reads (order[] = the reads of wavefront 0, pair by pair, then wavefront 1 ...):
// the threads of a walker wavefront then read traceback records that one or two fill wavefronts wrote next to each other, and the two
// reads of a pair — whose codes share every dword — sit in neighbouring lanes.
#ifndef VGK_WALK_WAVES
#define VGK_WALK_WAVES 0
#endif
#if VGK_WALK_WAVES
__global__ __launch_bounds__(256, VGK_WALK_WAVES) void gssw_walk_kernel(const GsswParams P, const int in_fill_order) {
#else
__global__ __launch_bounds__(256) void gssw_walk_kernel(const GsswParams P, const int in_fill_order) {
#endif
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (!in_fill_order) { if (k < P.n_problems) walk_one(P, k, P.best[k]); return; }
    if (k >= 2u * P.n_pairs) return;
    const uint32_t i = P.order[k];
    if (i != 0xffffffffu) walk_one(P, i, P.best[i]);
}
// the band geometry of a batch of banded problems (banded_geom_device.hpp): a lane per problem
__global__ __launch_bounds__(64) void banded_geometry_kernel(const BGeomParams P) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P.n) banded_geometry_one(P, i);
}

// The tracebacks as two kernels (GsswParams::walk_passes == 2): every read by diagonal runs alone; then the reads that needed a code — one in
// eight on the headline batch — side by side, so that the wavefronts of the first kernel are never held by a lane that walks cell by cell
__global__ __launch_bounds__(64) void gssw_walk_first_kernel(const GsswParams P, const int in_fill_order) {
    __shared__ uint32_t blk[2 * WD_DWORDS * 64];                   // a lane's 160 read bytes and 160 column bytes, dwords interleaved across the lanes
    __shared__ int16_t tab[WD_TAB];
    if (threadIdx.x < WD_TAB) tab[threadIdx.x] = wd_table_entry(P, threadIdx.x);
    __syncthreads();
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (!in_fill_order) { if (k < P.n_problems) walk_first_one(P, k, P.best[k], blk + threadIdx.x, 64, tab); return; }
    if (k >= 2u * P.n_pairs) return;
    const uint32_t i = P.order[k];
    if (i != 0xffffffffu) walk_first_one(P, i, P.best[i], blk + threadIdx.x, 64, tab);
}
// a lane per read slot of the miss list (gssw_device.hpp: refill_layout_read): the 2 * 64 / G slots of one second-fill wavefront in neighbouring lanes — a
// group of min(slots, 64) lanes, a lane of it taking every 64th slot where there are more —, the widest column range by shuffles inside the group, the
// wavefront's descriptor from the group's first lane.  A wavefront of this kernel lays out 64 / group second-fill wavefronts.
__host__ __device__ static inline uint32_t refill_layout_group(uint32_t G) { const uint32_t slots = 2u * (64u / G); return slots < 64u ? slots : 64u; }
__global__ __launch_bounds__(256) void gssw_refill_layout_kernel(const GsswParams P) {
    const uint32_t lane = threadIdx.x & 63u, slots = 2u * (64u / P.refill_G), group = refill_layout_group(P.refill_G), per_wave = 64u / group;
    const uint32_t q = lane / group, at = lane - q * group;
    const uint32_t w2 = (blockIdx.x * 4u + (threadIdx.x >> 6)) * per_wave + q;
    const uint32_t M = *tb_miss_count(P);
    uint32_t rmax = 0;
    if (q < per_wave)
        for (uint32_t s = at; s < slots; s += group) { const uint32_t cols = refill_layout_read(P, M, w2 * slots + s); rmax = cols > rmax ? cols : rmax; }
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) { const uint32_t o = (uint32_t)__shfl_down((int)rmax, d, 64); if (at + d < group && o > rmax) rmax = o; }
    if (q < per_wave && at == 0) refill_layout_wave(P, M, w2, rmax);
}
__global__ __launch_bounds__(256) void gssw_refill_restore_kernel(const GsswParams P) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P.n_problems) refill_restore_one(P, i);
}
__global__ __launch_bounds__(256) void gssw_walk_missed_kernel(const GsswParams P) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= *tb_miss_count(P)) return;
    const uint32_t i = tb_miss_list(P)[k];
    walk_one(P, i, P.best[i]);
}

// TB_REWALK (gssw_device.hpp), first the band: the fill's wavefronts again — same grid, same lane <-> (pair, lane block) map — each lane over
// the band columns of its lane block with the code-building lane code; no lane talks to another (the rows above come from HBM).
template <int K, bool S8>
__global__ __launch_bounds__(256, 2) void gssw_band_kernel(const GsswParams P) {
    const uint32_t wave = P.wave_begin + blockIdx.x * 4u + (threadIdx.x >> 6);
    if (wave >= P.wave_begin + P.wave_count) return;
    band_fill_lane<K, S8>(P, P.waves[wave], threadIdx.x & 63u);
}
// ... then the walks over the band's records, one lane per read in fill order (the stored-codes walk kernel's shape)
__global__ __launch_bounds__(256) void gssw_bandwalk_kernel(const GsswParams P) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= 2u * P.n_pairs) return;
    const uint32_t i = P.order[k];
    if (i != 0xffffffffu) bandwalk_one(P, i, P.best[i]);
}
// ... then, for the reads whose walk left its band (status W_MISSED), the on-demand form: one lane per read over the reads of ONE fill launch (the lane code is
// instantiated per rows-per-lane K), in the order the fill placed them.  A wavefront's windows live in LDS, lane-interleaved.
template <int K, bool S8>
__global__ __launch_bounds__(64, 2) void gssw_rewalk_kernel(const GsswParams P) {
    __shared__ uint32_t win[(TB_CKPT / 2) * ((K + 3) / 4) * 64];
    const uint32_t count = *tb_miss_count(P);
    const uint32_t* list = tb_miss_list(P);
    for (uint32_t k = blockIdx.x * 64u + threadIdx.x; k < count; k += gridDim.x * 64u) {
        const uint32_t i = list[k];
        rewalk_one<K, S8>(P, i, P.best[i], win + threadIdx.x, 64u);
    }
}

// ---- CIGAR ops on their way back: exclusive prefix sums of the per-problem op counts, then a gather ------------------
// One block scans OPS_SCAN_BLOCK = 1024 problems (4 per thread): wave-level inclusive scans on DPP-backed shuffles, the four
// wave totals through LDS.
static __device__ __forceinline__ uint32_t ops_of(const vgk_result* res, uint32_t i, uint32_t n) {
    return (i < n && res[i].status == VGK_OK) ? res[i].n_ops : 0u;
}
__global__ __launch_bounds__(256) void ops_scan_kernel(const vgk_result* res, uint32_t n, uint32_t* offs, uint32_t* sums) {
    __shared__ uint32_t wave_total[4];
    const uint32_t i0 = (blockIdx.x * 256u + threadIdx.x) * 4u, lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t c0 = ops_of(res, i0, n), c1 = ops_of(res, i0 + 1, n), c2 = ops_of(res, i0 + 2, n), c3 = ops_of(res, i0 + 3, n);
    uint32_t incl = c0 + c1 + c2 + c3;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t up = __shfl_up(incl, d, 64); if (lane >= d) incl += up; }
    if (lane == 63) wave_total[w] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t k = 0; k < w; ++k) before += wave_total[k];
    uint32_t at = before + incl - (c0 + c1 + c2 + c3);
    if (i0 < n) offs[i0] = at;
    at += c0; if (i0 + 1 < n) offs[i0 + 1] = at;
    at += c1; if (i0 + 2 < n) offs[i0 + 2] = at;
    at += c2; if (i0 + 3 < n) offs[i0 + 3] = at;
    if (threadIdx.x == 255) sums[blockIdx.x] = before + incl;
}
// one block turns the block totals into block starts (exclusive) and the grand total
__global__ __launch_bounds__(256) void ops_sums_kernel(uint32_t* sums, uint32_t n_blocks, unsigned long long* total) {
    __shared__ uint32_t wave_total[4];
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    for (uint32_t base = 0; base < n_blocks; base += 256u) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t c = i < n_blocks ? sums[i] : 0u;
        uint32_t incl = c;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t up = __shfl_up(incl, d, 64); if (lane >= d) incl += up; }
        if (lane == 63) wave_total[w] = incl;
        __syncthreads();
        uint32_t before = 0;
        for (uint32_t k = 0; k < w; ++k) before += wave_total[k];
        const unsigned long long start = carry + before + incl - c;
        if (i < n_blocks) sums[i] = (uint32_t)start;         // the caller has checked that all ops fit 32 bits
        __syncthreads();
        if (threadIdx.x == 255) carry += before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}
__global__ __launch_bounds__(256) void ops_gather_kernel(const vgk_result* res, const vgk_op* ops, uint32_t n, const uint32_t* offs,
                                                         const uint32_t* sums, vgk_result* out_res, vgk_op* out_ops) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    vgk_result r = res[i];
    const uint32_t at = sums[i / Backend::OPS_SCAN_BLOCK] + offs[i];
    if (r.status == VGK_OK && r.n_ops) {
        const vgk_op* from = ops + r.ops_begin;
        for (uint32_t k = 0; k < r.n_ops; ++k) out_ops[at + k] = from[k];
    } else r.n_ops = 0;
    r.ops_begin = at;
    out_res[i] = r;
}

// ---- banded global alignment (banded_device.hpp): cross-lane primitives on DPP ------------------------------------
struct XlDpp {
    static __device__ __forceinline__ int32_t dpp_up(int32_t v)   { return __builtin_amdgcn_update_dpp(BNEG, v, 0x130 /* wave_shl:1 */, 0xf, 0xf, false); }
    static __device__ __forceinline__ int32_t dpp_down(int32_t v) { return __builtin_amdgcn_update_dpp(BNEG, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }
    __device__ __forceinline__ int32_t up(int32_t v) const { return dpp_up(v); }
    __device__ __forceinline__ int32_t down(int32_t v) const { return dpp_down(v); }
    // lane +- 1's value minus s in ONE instruction; the lane without that neighbour has no DPP source, is skipped and keeps `old`
    // (s_nop: 2 wait states between a VALU write and a DPP read of the same VGPR)
    __device__ __forceinline__ int32_t up_sub(int32_t old, int32_t v, int32_t s) const {
        asm volatile("s_nop 1\n\tv_sub_u32_dpp %0, %1, %2 wave_shl:1 row_mask:0xf bank_mask:0xf" : "+v"(old) : "v"(v), "v"(s));
        return old;
    }
    __device__ __forceinline__ int32_t down_sub(int32_t old, int32_t v, int32_t s) const {
        asm volatile("s_nop 1\n\tv_sub_u32_dpp %0, %1, %2 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(old) : "v"(v), "v"(s));
        return old;
    }
    __device__ __forceinline__ int32_t scalar(int32_t s) const { int32_t o; const int32_t u = __builtin_amdgcn_readfirstlane(s); asm volatile("s_mov_b32 %0, %1" : "=s"(o) : "s"(u)); return o; }
    __device__ __forceinline__ int32_t add3(int32_t a, int32_t b, int32_t s) const { int32_t o; asm("v_add3_u32 %0, %1, %2, %3" : "=v"(o) : "v"(a), "v"(b), "s"(s)); return o; }
    __device__ __forceinline__ int32_t in_lanes(int32_t s) const { int32_t v; asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(s)); return v; }
    // exclusive max-scan over the 64 lanes: row_shr 1/2/4/8 inside each row of 16, then row_bcast:15 and row_bcast:31
    __device__ __forceinline__ int32_t scan_excl(int32_t v) const {
        // v_max_i32_dpp with the destination tied to both sources: a lane whose DPP source does not exist is disabled and
        // keeps its value, which is the identity we want — one instruction per step instead of mov_dpp + max + constant.
        // (s_nop: 2 wait states between a VALU write and a DPP read of the same VGPR; 5 after an EXEC write.)
        asm volatile("s_nop 4\n\tv_max_i32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                     "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
                     "s_nop 1" : "+v"(v));
        return dpp_down(v);
    }
    // the same with the last step's destination kept by the caller: lane 0 has no source and keeps `old`
    __device__ __forceinline__ int32_t scan_excl_keep(int32_t old, int32_t v) const {
        asm volatile("s_nop 4\n\tv_max_i32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                     "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
                     "s_nop 1\n\tv_mov_b32_dpp %1, %0 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(v), "+v"(old));
        return old;
    }
    __device__ __forceinline__ uint32_t width() const { return 64u; }
    __device__ __forceinline__ int32_t first_lane(int32_t v) const { return __builtin_amdgcn_readlane(v, 0); }
    __device__ __forceinline__ int32_t last_lane(int32_t v) const { return __builtin_amdgcn_readlane(v, 63); }
    __device__ __forceinline__ void fence() const { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }
    __device__ __forceinline__ bool any(int32_t flag) const { return __ballot(flag != 0) != 0ull; }
    __device__ __forceinline__ unsigned long long ballot(bool flag) const { return __ballot(flag); }
    __device__ __forceinline__ int32_t reduce_max(int32_t v) const {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { const int32_t o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
        return v;
    }
    __device__ __forceinline__ unsigned long long reduce_add(unsigned long long v) const {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
        return v;
    }
};

template <int R, bool QA, bool LDS>
__global__ void __launch_bounds__(64) banded_fill_kernel(const BandedParams P, const uint32_t begin) {
    extern __shared__ uint8_t smem[];
    const BProb pb = P.probs[P.order[begin + blockIdx.x]];
    BSrc src;
    constexpr bool FAST = LDS && !QA && R <= 4;
    if (FAST) {      // the FAST score path (banded_device.hpp): padded copies of the read and graph codes, the table rows in scalar registers
        uint8_t* srd = smem + 48;                                            // 8 B of padding in front (windows start up to 8 rows early) ...
        uint8_t* sg = smem + ((48u + pb.L + 16u + 3u) & ~3u);                // ... and behind (a window is three dwords); graph codes dword-aligned
        for (uint32_t i = threadIdx.x; i < 48; i += 64) smem[i] = i < 40 ? (uint8_t)P.mat[BMAT_ROWS_AT + i] : (uint8_t)0;      // the table rows as 64-bit words, then the padding
        for (uint32_t i = threadIdx.x; i < pb.L + 16u; i += 64) srd[i] = i < pb.L ? P.reads[pb.read_off + i] : (uint8_t)0;
        for (uint32_t i = threadIdx.x; i < pb.graph_len + 8u; i += 64) sg[i] = i < pb.graph_len ? P.graph[pb.graph_off + i] : (uint8_t)0;
        __syncthreads();
        src.rd = srd; src.q = nullptr; src.graph = sg; src.mat = P.mat; src.rows = reinterpret_cast<const uint64_t*>(smem);
    } else if (LDS) {       // stage what every column reads — score table, read, qualities, graph bases — into LDS once
        constexpr uint32_t MAT = QA ? 6400u : 32u;
        int8_t* smat = reinterpret_cast<int8_t*>(smem);
        uint8_t* srd = smem + MAT; uint8_t* sq = srd + pb.L; uint8_t* sg = QA ? sq + pb.L : sq;
        for (uint32_t i = threadIdx.x; i < (QA ? 6400u : 25u); i += 64) smat[i] = P.mat[i];
        for (uint32_t i = threadIdx.x; i < pb.L; i += 64) { srd[i] = P.reads[pb.read_off + i]; if (QA) sq[i] = P.quals[pb.read_off + i]; }
        for (uint32_t i = threadIdx.x; i < pb.graph_len; i += 64) sg[i] = P.graph[pb.graph_off + i];
        __syncthreads();
        src.rd = srd; src.q = sq; src.graph = sg; src.mat = smat;
    } else {
        src.rd = P.reads + pb.read_off; src.q = QA ? P.quals + pb.read_off : nullptr; src.graph = P.graph + pb.graph_off; src.mat = P.mat;
    }
    XlDpp xl;
    banded_fill_lane<R, QA, FAST>(P, pb, src, threadIdx.x, xl);
}

// Wide bands (more than 512 diagonals): B blocks of 64 lanes x 8 rows per column, a lane's rows of the other blocks in LDS (banded_fill_lane_blocks)
// — instead of 16 / 32 rows per lane in registers, which needed 399-512 VGPRs and up to 1.6 KB of scratch per lane.
template <int B, bool QA, bool LDS>
__global__ void __launch_bounds__(64) banded_fill_blocks_kernel(const BandedParams P, const uint32_t begin) {
    extern __shared__ uint8_t smem[];
    __shared__ int32_t bstate[B * 3 * 8 * 64];          // element e of lane l at bstate[e * 64 + l]: no bank conflicts
    const BProb pb = P.probs[P.order[begin + blockIdx.x]];
    BSrc src;
    if (LDS) {       // stage what every column reads — score table, read, qualities, graph bases — into LDS once (as banded_fill_kernel)
        constexpr uint32_t MAT = QA ? 6400u : 32u;
        int8_t* smat = reinterpret_cast<int8_t*>(smem);
        uint8_t* srd = smem + MAT; uint8_t* sq = srd + pb.L; uint8_t* sg = QA ? sq + pb.L : sq;
        for (uint32_t i = threadIdx.x; i < (QA ? 6400u : 25u); i += 64) smat[i] = P.mat[i];
        for (uint32_t i = threadIdx.x; i < pb.L; i += 64) { srd[i] = P.reads[pb.read_off + i]; if (QA) sq[i] = P.quals[pb.read_off + i]; }
        for (uint32_t i = threadIdx.x; i < pb.graph_len; i += 64) sg[i] = P.graph[pb.graph_off + i];
        __syncthreads();
        src.rd = srd; src.q = sq; src.graph = sg; src.mat = smat;
    } else {
        src.rd = P.reads + pb.read_off; src.q = QA ? P.quals + pb.read_off : nullptr; src.graph = P.graph + pb.graph_off; src.mat = P.mat;
    }
    src.rows = nullptr;
    XlDpp xl;
    banded_fill_lane_blocks<B, QA>(P, pb, src, threadIdx.x, xl, bstate + threadIdx.x, 64u);
}
// Bands of more than 2048 diagonals: any number of blocks, their state in an HBM slab per wavefront (banded_fill_lane_blocks<0>); the inputs are read
// where they lie (such a problem's read and graph are long: no LDS staging)
template <bool QA>
__global__ void __launch_bounds__(64) banded_fill_blocks_any_kernel(const BandedParams P, const uint32_t begin, const uint32_t nb, int32_t* slabs) {
    const BProb pb = P.probs[P.order[begin + blockIdx.x]];
    BSrc src;
    src.rd = P.reads + pb.read_off; src.q = QA ? P.quals + pb.read_off : nullptr; src.graph = P.graph + pb.graph_off; src.mat = P.mat; src.rows = nullptr;
    XlDpp xl;
    int32_t* mine = slabs + (size_t)blockIdx.x * ((size_t)nb * 3u * 8u + 3u * ((size_t)nb + 1u)) * 64u;
    banded_fill_lane_blocks<0, QA>(P, pb, src, threadIdx.x, xl, mine + threadIdx.x, 64u, nb, mine + (size_t)nb * 3u * 8u * 64u + threadIdx.x);
}
template <int B>
static void launch_banded_fill_blocks(const BandedParams& p, const BandedLaunch& L, hipStream_t stream) {
    const dim3 grid(L.count), block(64);
    const bool qa = p.quals != nullptr;
    const uint32_t dyn = (L.lds_bytes && L.lds_bytes + (uint32_t)sizeof(int32_t) * B * 3 * 8 * 64 <= 64u * 1024u) ? L.lds_bytes : 0u;      // (the blocks' state and the staged inputs share a workgroup's 64 KB)
    if (dyn) {
        if (qa) hipLaunchKernelGGL((banded_fill_blocks_kernel<B, true, true>), grid, block, dyn, stream, p, L.begin);
        else    hipLaunchKernelGGL((banded_fill_blocks_kernel<B, false, true>), grid, block, dyn, stream, p, L.begin);
    } else {
        if (qa) hipLaunchKernelGGL((banded_fill_blocks_kernel<B, true, false>), grid, block, 0, stream, p, L.begin);
        else    hipLaunchKernelGGL((banded_fill_blocks_kernel<B, false, false>), grid, block, 0, stream, p, L.begin);
    }
}

template <int R>
static void launch_banded_fill(const BandedParams& p, const BandedLaunch& L, hipStream_t stream) {
    const dim3 grid(L.count), block(64);
    const bool qa = p.quals != nullptr;
    if (L.lds_bytes) {
        if (qa) hipLaunchKernelGGL((banded_fill_kernel<R, true, true>), grid, block, L.lds_bytes, stream, p, L.begin);
        else    hipLaunchKernelGGL((banded_fill_kernel<R, false, true>), grid, block, L.lds_bytes, stream, p, L.begin);
    } else {
        if (qa) hipLaunchKernelGGL((banded_fill_kernel<R, true, false>), grid, block, 0, stream, p, L.begin);
        else    hipLaunchKernelGGL((banded_fill_kernel<R, false, false>), grid, block, 0, stream, p, L.begin);
    }
}

__global__ void __launch_bounds__(64) banded_walk_kernel(const BandedParams P) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < P.n) banded_walk_one(P, i);
}

// ---- gapless extension (gapless_device.hpp): resident threads, one scratch slab per thread
// Three kernels.  gapless_search_kernel runs every read's searches as one flat loop per lane, the queue of a search in LDS
// (lane-interleaved dwords: no bank conflicts, no HBM traffic; 35 dwords per thread) and only the write-once path links in the
// thread's slab; gapless_rules_kernel applies the set rules to the winners, one read per lane; a search whose queue outgrows the LDS
// slots marks its read G_RETRY and the slab kernel below (nested loops, the whole search in the thread's 11 KB HBM slab, round 1's
// kernel) runs exactly those reads again.
template <bool MG> __global__ void __launch_bounds__(64, 4) gapless_kernel(const GaplessParams P, const uint32_t threads, const int retry_only) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= threads) return;
    GStoreSlab Q{P.scratch[t]};
    for (uint32_t k = t; k < P.n; k += threads) {
        const uint32_t i = P.order[k];
        if (retry_only && !(P.retry ? P.retry[i] != 0 : P.results[i].status == G_RETRY)) continue;
        gapless_extend_one<MG>(P, i, Q, P.scratch[t], P.cold[t]);
    }
}
// The flat form (gapless_device.hpp, "the flat form"): lanes take reads from a counter and never wait for another lane's search; the
// rules over the winners run in their own kernel.  Reads whose queue outgrew the LDS slots go to the slab kernel as before.
struct GWaveDev {
    GProf* p; uint32_t min_idle;
    __device__ GProf* prof() const { return p; }
    __device__ int vote(bool idle, bool searching) const {
        const unsigned long long bi = __ballot(idle), bs = __ballot(searching);
        if (!(bi | bs)) return 0;
        return ((uint32_t)__popcll(bi) >= min_idle || !bs) ? 1 : 2;
    }
    __device__ uint32_t next_read(const GaplessParams& P) const {
        const unsigned long long k = atomicAdd(P.counters + 4, 1ull);
        return k < (unsigned long long)P.n ? (uint32_t)k : 0xffffffffu;
    }
};
#ifndef VGK_GAPLESS_OCC
#define VGK_GAPLESS_OCC 4          // wavefronts per SIMD the search kernel is built for (tools/build_variant.sh: 5 and 6 measured in round 6, profiles/r06/NOTES.md §5)
#endif
template <bool MG> __global__ void __launch_bounds__(64, VGK_GAPLESS_OCC) gapless_search_kernel(const GaplessParams P, const uint32_t threads) {
    __shared__ uint32_t lds[64 * G_FAST_DW];
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= threads) return;
    GStoreLds Q{lds + threadIdx.x, 64u, P.scratch[t], 0u};
#if defined(VGAMD_GAPLESS_PROF)
    GProf prof; prof.start();
    GWaveDev wave{&prof, P.flat_min_idle};
    gapless_search_lane<MG>(P, Q, P.scratch[t], wave);
    if ((threadIdx.x & 63) == 0) for (int i = 0; i < 12; ++i) atomicAdd(P.counters + 8 + i, prof.acc[i]);
#else
    GWaveDev wave{nullptr, P.flat_min_idle};
    gapless_search_lane<MG>(P, Q, P.scratch[t], wave);
#endif
}
template <bool MG> __global__ void __launch_bounds__(64, 6) gapless_rules_kernel(const GaplessParams P) {
    __shared__ uint8_t order[64 * G_SEEDS];           // the permutation the rules sort, per lane
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k >= P.n) return;
    gapless_rules_one<MG>(P, P.order[k], order + threadIdx.x * G_SEEDS);
}

__global__ void __launch_bounds__(256) gapless_order_kernel(const GOrderParams P, const int stage) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.n) return;
    if (stage == 1) g_order_sizes_one(P, i); else g_order_gather_one(P, i);
}
__global__ void __launch_bounds__(256) gapless_seeded_kernel(const GSeededParams P) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < P.n) g_seeded_one(P, i);
}
// hipMemsetAsync's fill kernel was measured at ~30 GB/s for the stage's 22 MB table (0.7 ms per step): large clears go through this one
__global__ void __launch_bounds__(256) zero_kernel(uint4* dst, const size_t vecs, unsigned char* tail, const uint32_t tail_bytes) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < vecs; i += stride) dst[i] = make_uint4(0u, 0u, 0u, 0u);
    if (blockIdx.x == 0 && threadIdx.x < tail_bytes) tail[threadIdx.x] = 0;
}
__global__ void __launch_bounds__(256) mask_reads_kernel(char* reads, const size_t bytes) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (i >= bytes) return;
    if (i + 16 <= bytes) {
        uint4 w = *reinterpret_cast<const uint4*>(reads + i);
        char* c = reinterpret_cast<char*>(&w);
#pragma unroll
        for (int k = 0; k < 16; ++k) c[k] = g_mask_base(c[k]);
        *reinterpret_cast<uint4*>(reads + i) = w;
    } else for (size_t k = i; k < bytes; ++k) reads[k] = g_mask_base(reads[k]);
}

// ---- minimizer seeding (minimizer_device.hpp): one wavefront per read, one lane per k-mer position
// Rounds of 64 k-mer positions, 65 - w of them new (a round's first w - 1 lanes only complete the windows that end behind them).
// Per round every lane builds the forward and reverse keys of ITS k-mer from unaligned 8-byte loads, hashes both and keeps the
// canonical one; whether a k-mer is a candidate is k consecutive set bits in the ballots of "this base is ACGT"; the minimum of the w
// candidates ending at a lane — (hash, position) lexicographic = the leftmost smallest — comes from doubling steps over lane
// shuffles plus one combining step; a window reports its minimum when that lies behind everything reported before (window minima
// move right only): a prefix maximum.  The round's reported minimizers (at most 65 - w) are compacted into LDS by ballot + popcount,
// one lane each probes the table, and their hits become seeds in order, a (node, diagonal) pair the read already has being dropped by
// one ballot over the seeds kept so far.  Results are those of minimizer_one, which the emulator and the index builder run.
struct MzMin { uint64_t key; uint32_t hash_lo; uint32_t pos_rev; };        // pos_rev = read offset << 1 | reverse
// Four reads per workgroup, one wavefront each (no workgroup barrier anywhere: a wavefront's LDS operations complete in order, the
// fence only keeps the compiler from moving them).  The seeds go to slots of MZ_MAX_SEEDS per read; minimizer_gather_kernel packs
// them behind each other once the prefix sums of the counts are known — one pass over the reads instead of a counting and a writing one.
#define MZ_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
__global__ void __launch_bounds__(256) minimizer_kernel(const MinimizerParams P, vgk_seed* slots) {
    __shared__ MzMin mins_all[4][64];
    __shared__ unsigned long long seen_all[4][MZ_MAX_SEEDS];
    __shared__ unsigned long long cand_all[4][64];                           // a round's candidate seeds, in hit order
    __shared__ uint8_t own_all[4][64];                                       // the minimizer (lane) each of them belongs to
    // find_seeds' choice (MinimizerParams::policy): the read's minimizers in read order — key, hits, the hits of the key's run, score — and
    // the order the filters take them in
    __shared__ unsigned long long pkey_all[4][MZ_POLICY_MAX];
    __shared__ double psc_all[4][MZ_POLICY_MAX];
    __shared__ uint32_t phit_all[4][MZ_POLICY_MAX], prun_all[4][MZ_POLICY_MAX];
    __shared__ uint8_t pord_all[4][MZ_POLICY_MAX];
    __shared__ uint8_t ptie_all[4][3 * (MZ_POLICY_MAX + 1)];                  // the top tie's runs, their permutation and the new order (mz_shuffle_top_ties)
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t i = P.lo + blockIdx.x * 4u + wv;
    if (i >= P.hi) return;
    MzMin* mins = mins_all[wv]; unsigned long long* seen = seen_all[wv]; unsigned long long* cand = cand_all[wv]; uint8_t* own = own_all[wv];
    const uint64_t a = P.read_off[i]; const uint32_t L = (uint32_t)(P.read_off[i + 1] - a);
    const uint32_t k = P.index.k, w = P.index.w;
    const char* rd = P.reads + a;
    vgk_seed* dst = slots + (size_t)i * MZ_MAX_SEEDS;
    uint32_t n_min = 0, n_seeds = 0; bool truncated = false;
    unsigned long long* pkey = pkey_all[wv]; double* psc = psc_all[wv]; uint32_t* phit = phit_all[wv]; uint32_t* prun = prun_all[wv]; uint8_t* pord = pord_all[wv];
    unsigned long long chosen = ~0ull; bool skipped = false;
    // With a policy the rounds run twice: first only to list the read's minimizers and their hit counts (the choice needs all of them
    // before the first seed is written), then — the choice made, across the lanes, between the two — as without one, the minimizers that were
    // not chosen giving no seeds.
    if (L >= k + w - 1) for (int phase = P.policy.on ? 0 : 1; phase < 2; ++phase) {
        if (phase == 1 && P.policy.on) {
            const uint32_t np = n_min;
            if (np > MZ_POLICY_MAX) skipped = true;
            else {
                const MzPolicy& Q = P.policy;
                const unsigned long long my_key = lane < np ? pkey[lane] : 0ull; const uint32_t my_hits = lane < np ? phit[lane] : 0u;
                uint32_t run = 0;
                for (uint32_t j = 0; j < np; ++j) run += pkey[j] == my_key ? phit[j] : 0u;
                const double my_sc = mz_score(Q, my_hits);
                if (lane < np) { psc[lane] = my_sc; prun[lane] = run; }
                MZ_WAVE_SYNC();
                uint32_t rank = 0;
                for (uint32_t j = 0; j < np; ++j) rank += mz_better(psc[j], pkey[j], j, my_sc, my_key, lane) ? 1u : 0u;
                if (lane < np) pord[rank] = (uint8_t)lane;
                MZ_WAVE_SYNC();
                // the runs tied at the top, shuffled as the reference shuffles them (minimizer_device.hpp) — when their order can change the choice at
                // all: tied runs with at most hit_cap hits are all taken whatever their order (nearly every read: its unique minimizers tie at the
                // top), so the generator is only made for a read whose BEST minimizers are repetitive.  The seed is folded across the lanes
                // (seed = sum of byte_i x 13^(L - 1 - i) in 32 bits: a lane's bytes times their powers, summed over the wavefront).
                { // (the tie itself across the lanes: lane r looks at the r-th minimizer of the order — tied with the first one? the first of its run?)
                  const uint32_t xr = lane < np ? pord[lane] : 0u, x0 = np ? pord[0] : 0u;
                  const bool tied = lane < np && psc[xr] == psc[x0];
                  const bool opens = tied && (lane == 0 || pkey[pord[lane - 1]] != pkey[xr]);
                  const uint32_t t_elems = (uint32_t)__popcll(__ballot(tied)), t_runs = (uint32_t)__popcll(__ballot(opens)), t_hits = np ? phit[x0] : 0u;
                  if (mz_tie_matters(Q, t_runs, t_hits)) {
                      uint32_t part = 0; bool other = false;
                      for (uint32_t b = lane; b < L; b += 64u) {
                          const char c = rd[b]; other = other || !(c == 'A' || c == 'C' || c == 'G' || c == 'T');
                          uint32_t pw = 1u, base = 13u;
                          for (uint32_t e = L - 1u - b; e; e >>= 1) { if (e & 1u) pw *= base; base *= base; }
                          part += (uint32_t)(uint8_t)c * pw;
                      }
#pragma unroll
                      for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d, 64);
                      if (__ballot(other) != 0ull || Q.paired) skipped = true;          // a masked base — or a mate of a pair, whose generator is the pair's (include/vgk.h): the reference's seed cannot be made here — not chosen for
                      else if (lane == 0) { uint8_t* t = ptie_all[wv]; mz_shuffle_top_ties(pord, pkey, t_elems, t_runs, part, t, t + (MZ_POLICY_MAX + 1), t + 2 * (MZ_POLICY_MAX + 1)); }
                  }
                  MZ_WAVE_SYNC(); }
                // the filters, in that order: every lane the same few dozen steps (the sums must be made in this order)
                const bool use_score = Q.hit_cap != 0 || Q.fraction != 1.0;
                double target = 0.0, selected = 0.0;
                if (use_score) { double base = 0.0; for (uint32_t r = 0; r < np; ++r) base = mz_add(base, psc[pord[r]]); target = mz_add(mz_mul(base, Q.fraction), 0.000001); }
                unsigned long long mask = 0ull; bool taking = false; unsigned long long prev = 0ull;
                for (uint32_t r = 0; r < np; ++r) {
                    const uint32_t x = pord[r]; const unsigned long long kx = pkey[x]; const uint32_t hx = phit[x]; const double sx = psc[x];
                    if (r == 0 || kx != prev) taking = false;
                    prev = kx;
                    bool pass = hx != 0u && prun[x] <= Q.hard_hit_cap;
                    if (pass && use_score) {
                        if (hx <= Q.hit_cap || mz_add(selected, sx) <= target || taking) selected = mz_add(selected, sx);
                        else { pass = false; target = selected; }
                    }
                    if (pass) { mask |= 1ull << x; taking = true; }
                }
                chosen = skipped ? ~0ull : mask;                             // (a read that is not chosen for is seeded as without a policy)
            }
            n_min = 0;
        }
        const uint32_t cap_now = P.policy.on && !skipped ? 0xffffffffu : P.hit_cap;      // (the choice held the run's hits against the hard cap)
        const uint32_t n_kmers = L - k + 1, step = 65 - w;
        const uint64_t kmask = (1ull << (2 * k)) - 1ull;                   // k <= 31
        const unsigned long long need = (1ull << k) - 1ull;
        const unsigned long long below = (1ull << lane) - 1ull;
        uint32_t last_plus1 = 0;                                            // 1 + the last reported position (0: none yet)
        for (uint32_t base = 0; base + w - 1 < n_kmers; base += step) {
            const uint32_t q = base + lane;                                 // this lane's k-mer position = the end of its window
            // The 2-bit codes of bases base .. base + 127 as two bit planes held in four ballots; a lane's k-mer is k consecutive positions
            // from bit `lane` on: funnel-shifted out of the planes, interleaved once into the reverse-complement key's layout (base t at
            // bits 2t), from which the forward key is the same pairs in reverse order.  No per-base loop, no byte loads beyond two per lane.
            const char c0 = q < L ? rd[q] : 'N', c1 = q + 64 < L ? rd[q + 64] : 'N';
            const int x0 = mz_code(c0), x1 = mz_code(c1);
            const unsigned long long v0 = __ballot(x0 >= 0), v1 = __ballot(x1 >= 0);
            const unsigned long long lo0 = __ballot(x0 & 1), lo1 = __ballot(x1 & 1), hi0 = __ballot((x0 >> 1) & 1), hi1 = __ballot((x1 >> 1) & 1);      // (x < 0: both bits set, and the k-mer is no candidate)
            auto from_lane = [&](unsigned long long a0, unsigned long long a1) { return lane ? ((a0 >> lane) | (a1 << (64 - lane))) : a0; };
            const unsigned long long vbits = from_lane(v0, v1);
            const bool valid = q < n_kmers && (vbits & need) == need;
            const uint32_t b_lo = (uint32_t)(from_lane(lo0, lo1) & need), b_hi = (uint32_t)(from_lane(hi0, hi1) & need);
            auto spread = [](uint32_t v) {                                  // bit t -> bit 2t
                uint64_t z = v;
                z = (z | (z << 16)) & 0x0000ffff0000ffffull; z = (z | (z << 8)) & 0x00ff00ff00ff00ffull; z = (z | (z << 4)) & 0x0f0f0f0f0f0f0f0full;
                z = (z | (z << 2)) & 0x3333333333333333ull; z = (z | (z << 1)) & 0x5555555555555555ull;
                return z;
            };
            const uint64_t pairs = spread(b_lo) | (spread(b_hi) << 1);       // base t's code at bits 2t, 2t + 1
            uint64_t rev = ~pairs & kmask;                                   // complement of every base, the k-mer's last base in the highest pair
            uint64_t br = __builtin_bitreverse64(pairs);                     // pairs in reverse order, the two bits of a pair swapped
            br = ((br >> 1) & 0x5555555555555555ull) | ((br & 0x5555555555555555ull) << 1);
            uint64_t fwd = (br >> (64 - 2 * k)) & kmask;                      // base 0 in the highest pair
            if (!valid) { fwd = 0; rev = 0; }
            const uint64_t hf = mz_hash(fwd), hr = mz_hash(rev);
            const bool reverse = hr < hf;
            const uint64_t my_hash = reverse ? hr : hf, my_key = reverse ? rev : fwd;
            uint64_t h = valid ? my_hash : ~0ull;                           // ~0: no candidate
            uint32_t hp = q;
            uint32_t span = 1;
            while (2 * span <= w) {
                const uint64_t oh = __shfl_up(h, span, 64); const uint32_t op = __shfl_up(hp, span, 64);
                if (lane >= span && (oh < h || (oh == h && op < hp))) { h = oh; hp = op; }
                span *= 2;
            }
            if (span < w) {
                const uint32_t d = w - span;
                const uint64_t oh = __shfl_up(h, d, 64); const uint32_t op = __shfl_up(hp, d, 64);
                if (lane >= d && (oh < h || (oh == h && op < hp))) { h = oh; hp = op; }
            }
            const bool ends = lane >= w - 1 && q < n_kmers && h != ~0ull;   // a complete window with a candidate
            uint32_t run = ends ? hp + 1 : 0u;                              // prefix maximum of the minima so far in this round
            for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(run, d, 64); if (lane >= d && o > run) run = o; }
            uint32_t before = __shfl_up(run, 1, 64); if (lane == 0) before = 0;
            if (last_plus1 > before) before = last_plus1;
            const bool report = ends && hp + 1 > before;
            const uint32_t owner = hp - base;                               // the lane that built the minimum's k-mer (inside this round for every complete window)
            const uint64_t okey = __shfl(my_key, owner & 63u, 64), ohash = __shfl(my_hash, owner & 63u, 64);
            const uint32_t orev = __shfl((uint32_t)reverse, owner & 63u, 64);
            const unsigned long long rb = __ballot(report);
            const uint32_t n_round = (uint32_t)__popcll(rb);
            if (report) { MzMin& mm = mins[__popcll(rb & below)]; mm.key = okey; mm.hash_lo = (uint32_t)ohash; mm.pos_rev = (hp << 1) | orev; }
            const uint32_t round_max = __shfl(run, 63, 64);
            if (round_max > last_plus1) last_plus1 = round_max;
            const uint32_t n_before = n_min;
            n_min += n_round;
            MZ_WAVE_SYNC();
            if (phase == 0) {                                                // list them; nothing else
                if (lane < n_round && n_before + lane < MZ_POLICY_MAX) {
                    const MzMin mm = mins[lane];
                    MzKmer km; km.key = mm.key; km.hash = mm.hash_lo; km.reverse = (mm.pos_rev & 1u) != 0;
                    uint32_t f0 = 0, c0 = 0; MzPos o0{0u, 0u};
                    pkey[n_before + lane] = mm.key; phit[n_before + lane] = mz_find(P.index, km, f0, c0, o0) ? c0 : 0u;
                }
                MZ_WAVE_SYNC();
                continue;
            }
            // this round's minimizers: one lane each probes the table (a key's single position comes with its slot); then ALL their hits at
            // once — hit c of the round in lane c: an exclusive prefix sum of the counts, the owners spread through LDS, one load for the
            // positions that are not in their slots, every candidate held against the seeds kept so far and the candidates before it
            // (uniform LDS reads), the survivors ranked by ballot.  The result is the serial order's (minimizer_one): a candidate is looked
            // at iff the read is not full when its turn comes, the first of equal (node, diagonal) pairs is kept.  A round with more than
            // 64 hits takes the serial form below.
            uint32_t first = 0, count = 0, p = 0, rv = 0; MzPos one{0u, 0u};
            if (lane < n_round) {                                            // (also for a read that is full already: whether hits are left decides its truncated flag)
                const MzMin mm = mins[lane];
                MzKmer km; km.key = mm.key; km.hash = mm.hash_lo; km.reverse = (mm.pos_rev & 1u) != 0;
                p = mm.pos_rev >> 1; rv = mm.pos_rev & 1u;
                if (!mz_find(P.index, km, first, count, one) || count > cap_now) count = 0;
                if (n_before + lane < 64u && !((chosen >> (n_before + lane)) & 1ull)) count = 0;
            }
            const unsigned long long hb = __ballot(count != 0);
            const uint32_t cc = count > 65u ? 65u : count;                   // (clamped: the sum must not wrap; a round within 64 hits has no clamped count)
            uint32_t incl = cc;
            for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
            const uint32_t total = __shfl(incl, 63, 64), excl = incl - cc;
            if (hb && total <= 64u) {
                for (uint32_t h0 = 0; h0 < count; ++h0) own[excl + h0] = (uint8_t)lane;
                MZ_WAVE_SYNC();
                const uint32_t j = lane < total ? own[lane] : 0u;
                const uint32_t fj = __shfl(first, j, 64), ej = __shfl(excl, j, 64), pj = __shfl(p, j, 64), rj = __shfl(rv, j, 64);
                MzPos qp; qp.node = __shfl(one.node, j, 64); qp.offset = __shfl(one.offset, j, 64);
                if (lane < total && fj != MZ_ONE) qp = P.index.pos[fj + (lane - ej)];
                const vgk_seed sd = mz_seed(qp, pj, rj != 0u, k);
                const unsigned long long key = ((unsigned long long)sd.node << 32) | (uint32_t)sd.diff;
                cand[lane] = key;
                MZ_WAVE_SYNC();
                bool dup = false;
                for (uint32_t x = 0; x < n_seeds; ++x) dup |= seen[x] == key;
                for (uint32_t x = 0; x + 1u < total; ++x) dup |= x < lane && cand[x] == key;
                const bool keep = lane < total && !dup;
                const unsigned long long kb = __ballot(keep);
                const uint32_t rank = n_seeds + (uint32_t)__popcll(kb & below);      // seeds kept when this candidate's turn comes
                if (keep && rank < MZ_MAX_SEEDS) { seen[rank] = key; dst[rank] = sd; }
                if (__ballot(lane < total && rank >= MZ_MAX_SEEDS) != 0ull) truncated = true;      // the cap: that hit and the rest are never looked at
                n_seeds += (uint32_t)__popcll(kb); if (n_seeds > MZ_MAX_SEEDS) n_seeds = MZ_MAX_SEEDS;
            } else
            for (unsigned long long todo = hb; todo; todo &= todo - 1) {
                if (n_seeds >= MZ_MAX_SEEDS) { truncated = true; break; }    // the cap: these hits are never looked at
                const uint32_t j = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
                const uint32_t cj = __shfl(count, j, 64), fj = __shfl(first, j, 64), pj = __shfl(p, j, 64), rj = __shfl(rv, j, 64);
                const uint32_t onode = __shfl(one.node, j, 64), ooff = __shfl(one.offset, j, 64);
                for (uint32_t h0 = 0; h0 < cj; h0 += 64) {
                    if (n_seeds >= MZ_MAX_SEEDS) { truncated = true; break; }
                    unsigned long long key = 0; vgk_seed sd; sd.node = 0; sd.diff = 0;
                    if (h0 + lane < cj) {
                        MzPos qp; qp.node = onode; qp.offset = ooff;
                        if (fj != MZ_ONE) qp = P.index.pos[fj + h0 + lane];
                        sd = mz_seed(qp, pj, rj != 0u, k);
                        key = ((unsigned long long)sd.node << 32) | (uint32_t)sd.diff;
                    }
                    const uint32_t in_group = cj - h0 < 64 ? cj - h0 : 64;
                    for (uint32_t x = 0; x < in_group; ++x) {                // in hit order; all lanes agree on every decision
                        if (n_seeds >= MZ_MAX_SEEDS) { truncated = true; break; }
                        const unsigned long long kx = __shfl(key, x, 64);
                        const bool dup = __ballot(lane < n_seeds && seen[lane] == kx) != 0ull;
                        if (!dup) {
                            if (lane == x) { seen[n_seeds] = key; dst[n_seeds] = sd; }
                            ++n_seeds;
                            MZ_WAVE_SYNC();
                        }
                    }
                }
            }
            MZ_WAVE_SYNC();
        }
    }
    if (lane == 0) { P.counts[i] = n_seeds; if (P.mins) P.mins[i] = n_min | (truncated ? VGK_MINIMIZERS_TRUNCATED : 0u) | (skipped ? VGK_MINIMIZERS_POLICY_SKIPPED : 0u); }
}
__global__ void __launch_bounds__(256) minimizer_gather_kernel(const MinimizerParams P, const vgk_seed* slots) {
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (i >= P.n) return;
    const uint32_t at = P.first[i], cnt = P.first[i + 1] - at;
    if (lane < cnt) P.seeds[at + lane] = slots[(size_t)i * MZ_MAX_SEEDS + lane];
}

// ---- tail forests (tail_device.hpp): resident lanes take the tails in turn for the walks; one lane per tree node for the graph tables
__global__ void __launch_bounds__(64) tail_walk_kernel(const TailParams P, const uint32_t threads) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= threads) return;
    for (uint32_t i = t; i < P.n; i += threads) tail_walk_one(P, i, P.scratch[t]);
}
__global__ void __launch_bounds__(256) tail_stage_kernel(const TStageParams P, const int what, const uint32_t items) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < items) tstage_one(P, what, i);
}
__global__ void __launch_bounds__(256) rescue_requests_kernel(const RqParams P, const int what) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (what == RQ_FLAG) { if (p <= P.n_pairs) rq_flag_one(P, p); }
    else if (p < P.n_pairs) rq_emit_one(P, p);
}
// ---- seeding reads of any length (minimizer_device.hpp): a lane per read lists its minimizers, a lane per minimizer writes its seeds
__global__ void __launch_bounds__(64) minimizer_list_kernel(const MzListParams P) { mz_list_one(P, blockIdx.x * 64 + threadIdx.x); }
__global__ void __launch_bounds__(256) minimizer_seeds_of_kernel(const MzSeedsOfParams P) { mz_seeds_of_one(P, blockIdx.x * 256 + threadIdx.x); }

// ---- find_seeds' whole choice for reads of any length (minimizer_device.hpp: mz_choose_one is the rule and the checker): one wavefront per read.
// Cooperative: loading and ranking the list, the bitonic sort of (rank, key, position), the run boundaries, laying the shuffled runs out, the
// runs' hit sums, and every range operation on the two coverage bitmaps (a 64-bit word per lane, the "any bit set" test one ballot).  In one
// order, carried out by all lanes alike over uniform values (no divergence, nothing to hand from lane to lane): the downsampling sweep, Knuth's
// shuffle of the top runs, the sum of the base target and the filter pass, whose 64 next minimizers sit one in each lane's registers.
// The work arrays are LDS (ChooseLds: 13-bit positions, 16-bit indices) or a slab in HBM per workgroup (ChooseSlab), same code.
struct ChooseLds  { using ORD = uint32_t; using IDX = uint16_t; static constexpr uint32_t BITS = 13; };
struct ChooseSlab { using ORD = uint64_t; using IDX = uint32_t; static constexpr uint32_t BITS = 32; };
template <class T> struct ChooseWork {
    uint64_t* key; typename T::ORD* ord;          // the sort's records: key | rank << BITS | position (top bit: kept by the downsampling); afterwards ord = position | FLAG (first of its run) | KEPT
    typename T::ORD* tmp;                         // the shuffled top runs laid out
    uint32_t* hits; uint32_t* run_hits;           // in the final order: a minimizer's hits; at a run's first minimizer the run's
    typename T::IDX* start; typename T::IDX* perm; // the top runs: where each starts, their permutation
    typename T::IDX* off; typename T::IDX* dq;    // the downsampling sweep: read offsets in read order, its line
    uint64_t* cov; uint64_t* ovl;                 // covered (flanked), covered_by_minimizer
};
__device__ inline uint32_t choose_bc(uint32_t v, uint32_t j) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)j); }
__device__ inline double choose_bc(double v, uint32_t j) { const uint64_t u = (uint64_t)__double_as_longlong(v); return __longlong_as_double((long long)(((uint64_t)choose_bc((uint32_t)(u >> 32), j) << 32) | choose_bc((uint32_t)u, j))); }
__device__ inline uint64_t choose_word_mask(uint64_t w, uint64_t lo, uint64_t hi) {      // the bits of word w inside [lo, hi), hi > lo, w in [lo >> 6, (hi - 1) >> 6]
    uint64_t mask = ~0ull;
    if (w == (lo >> 6)) mask &= ~0ull << (lo & 63);
    if (w == ((hi - 1) >> 6)) mask &= ~0ull >> (63 - ((hi - 1) & 63));
    return mask;
}
__device__ inline void choose_mark(uint64_t* bm, uint64_t lo, uint64_t hi, uint32_t lane) {
    if (lo < hi) for (uint64_t w = (lo >> 6) + lane; w <= ((hi - 1) >> 6); w += 64) bm[w] |= choose_word_mask(w, lo, hi);
    __syncthreads();
}
__device__ inline bool choose_any(const uint64_t* bm, uint64_t lo, uint64_t hi, uint32_t lane) {
    bool hit = false;
    if (lo < hi) for (uint64_t w = (lo >> 6) + lane; w <= ((hi - 1) >> 6); w += 64) hit = hit || (bm[w] & choose_word_mask(w, lo, hi)) != 0;
    return __ballot(hit) != 0;
}
__device__ inline uint32_t choose_seed(const char* seq, uint64_t L, uint32_t lane) {      // seed = seed * 13 + byte over the read: a stretch per lane, then the stretches in order
    const uint64_t chunk = (L + 63) / 64, lo = lane * chunk < L ? lane * chunk : L, hi = lo + chunk < L ? lo + chunk : L;
    uint32_t part = 0, pw = 1;
    for (uint64_t i = lo; i < hi; ++i) { part = part * 13u + (uint32_t)(uint8_t)seq[i]; pw *= 13u; }
    uint32_t s = 0;
    for (uint32_t j = 0; j < 64; ++j) s = s * choose_bc(pw, j) + choose_bc(part, j);
    return s;
}
template <class T> __device__ void choose_read(const MzChooseParams& P, uint32_t r, const ChooseWork<T>& W, uint32_t lane) {
    using ORD = typename T::ORD; using IDX = typename T::IDX;
    constexpr uint32_t TOP = sizeof(ORD) * 8 - 1, BITS = T::BITS;
    constexpr ORD FLAG = (ORD)1 << TOP, KEPT = (ORD)1 << (TOP - 1), IMASK = ((ORD)1 << BITS) - 1;
    const MzChoosePolicy& Q = P.policy;
    const uint64_t a = P.min_off[r]; const uint32_t n = (uint32_t)(P.min_off[r + 1] - a);
    if (!n) return;
    const vgk_read_minimizer* m = P.mins + a; uint8_t* out = P.verdict + a;
    const char* seq = P.reads + P.read_off[r]; const uint64_t L = P.read_off[r + 1] - P.read_off[r]; const uint32_t k = P.k;
    uint32_t np = 1; while (np < n) np <<= 1;
    for (uint32_t i = lane; i < np; i += 64) {
        if (i < n) { const vgk_read_minimizer rec = m[i]; W.key[i] = rec.key; W.ord[i] = ((ORD)mz_choose_rank(Q, rec.hits) << BITS) | (ORD)i; W.off[i] = (IDX)rec.offset; }
        else { W.key[i] = ~0ull; W.ord[i] = (ORD)~FLAG; }
    }
    __syncthreads();
    // ---- window downsampling, in read order (what it keeps: the records' top bit)
    bool downsampling = false;
    const uint64_t window = mz_choose_window(Q, L, k);
    if (window) {
        const uint32_t nohit = 2u * Q.hard_hit_cap + 2u;
        mz_sample_minimal(n, k, window, L, W.dq, [&](uint32_t i) { return (uint64_t)W.off[i]; },
            [&](uint32_t x, uint32_t y) { const uint32_t px = (uint32_t)((W.ord[x] & ~FLAG) >> BITS), py = (uint32_t)((W.ord[y] & ~FLAG) >> BITS);
                                          return px != nohit && (px < py || (px == py && W.key[x] < W.key[y])); },
            [&](uint32_t i) { W.ord[i] |= FLAG; downsampling = true; });
        __syncthreads();
    }
    // ---- the order: a bitonic sort of the records, ascending (rank, key, position); the padding sorts last
    for (uint32_t kk = 2; kk <= np; kk <<= 1) for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
        for (uint32_t t = lane; t < np / 2; t += 64) {
            const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i | j;
            const ORD oi = W.ord[i], ol = W.ord[l]; const uint64_t ki = W.key[i], kl = W.key[l];
            const ORD ri = (oi & ~FLAG) >> BITS, rl = (ol & ~FLAG) >> BITS;
            const bool l_first = rl < ri || (rl == ri && (kl < ki || (kl == ki && (ol & IMASK) < (oi & IMASK))));
            if (l_first == ((i & kk) == 0)) { W.ord[i] = ol; W.ord[l] = oi; W.key[i] = kl; W.key[l] = ki; }
        }
        __syncthreads();
    }
    // ---- the runs (first of its key: FLAG) and the top tie: `elements` minimizers in `runs` runs, as the shim counts them
    const uint32_t rank0 = (uint32_t)((W.ord[0] & ~FLAG) >> BITS);
    __syncthreads();
    uint32_t elements = 0, runs = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t pos = base + lane; const bool valid = pos < n;
        const ORD o = valid ? W.ord[pos] : (ORD)0;
        const bool first = valid && (pos == 0 || W.key[pos] != W.key[pos - 1]), top = valid && (uint32_t)((o & ~FLAG) >> BITS) == rank0;
        if (valid) W.ord[pos] = (o & IMASK) | (first ? FLAG : (ORD)0) | ((o & FLAG) ? KEPT : (ORD)0);
        elements += (uint32_t)__popcll(__ballot(top)); runs += (uint32_t)__popcll(__ballot(top && first));
    }
    __syncthreads();
    while (elements < n && !(W.ord[elements] & FLAG)) ++elements;             // (the last top run ends where its key ends)
    if (runs >= 2u) {
        uint32_t found = 0;
        for (uint32_t base = 0; base < elements; base += 64) {
            const uint32_t pos = base + lane; const bool f = pos < elements && (W.ord[pos] & FLAG) != 0;
            const uint64_t b = __ballot(f);
            if (f) W.start[found + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = (IDX)pos;
            found += (uint32_t)__popcll(b);
        }
        for (uint32_t i = lane; i < runs; i += 64) W.perm[i] = (IDX)i;
        const uint32_t seed = choose_seed(seq, L, lane);
        __syncthreads();
        uint32_t x = mz_minstd_first(seed);
        for (uint32_t i = 1; i < runs; ++i) { x = mz_minstd_next(x); const uint32_t j = x % (i + 1u); const IDX t = W.perm[j]; W.perm[j] = W.perm[i]; W.perm[i] = t; }
        __syncthreads();
        uint32_t carry = 0;
        for (uint32_t base = 0; base < runs; base += 64) {
            const uint32_t i = base + lane; uint32_t s = 0, len = 0;
            if (i < runs) { const uint32_t q = W.perm[i]; s = W.start[q]; len = (q + 1u < runs ? (uint32_t)W.start[q + 1u] : elements) - s; }
            uint32_t inc = len;
            for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(inc, d); if (lane >= d) inc += v; }
            const uint32_t dst = carry + inc - len;
            for (uint32_t t = 0; t < len; ++t) W.tmp[dst + t] = W.ord[s + t];
            carry += choose_bc(inc, 63);
        }
        __syncthreads();
        for (uint32_t q = lane; q < elements; q += 64) W.ord[q] = W.tmp[q];
        __syncthreads();
    }
    // ---- hits in the final order, the runs' sums, clean bitmaps
    for (uint32_t q = lane; q < n; q += 64) W.hits[q] = m[(uint32_t)(W.ord[q] & IMASK)].hits;
    for (uint64_t w = lane; w < (L + 64) / 64; w += 64) { W.cov[w] = 0; W.ovl[w] = 0; }
    __syncthreads();
    for (uint32_t q = lane; q < n; q += 64) if (W.ord[q] & FLAG) {
        uint64_t s = 0; uint32_t e = q;
        do { s += W.hits[e]; ++e; } while (e < n && !(W.ord[e] & FLAG));
        W.run_hits[q] = s > 0xffffffffull ? 0xffffffffu : (uint32_t)s;
    }
    __syncthreads();
    const bool score_filter = Q.hit_cap != 0 || Q.fraction != 1.0;
    double target = 0.0, selected = 0.0;
    if (score_filter) {
        double sum = 0.0;
        for (uint32_t base = 0; base < n; base += 64) {
            const double sc = base + lane < n ? mz_choose_score(Q, W.hits[base + lane]) : 0.0;
            const uint32_t cnt = n - base < 64u ? n - base : 64u;
            for (uint32_t j = 0; j < cnt; ++j) sum = mz_add(sum, choose_bc(sc, j));
        }
        target = mz_add(mz_mul(sum, Q.fraction), 0.000001);
    }
    // ---- the filters, in score order, run by run
    const uint64_t by_read_length = Q.num_bp_per_min ? L / Q.num_bp_per_min : 0, budget = Q.max_unique_min > by_read_length ? Q.max_unique_min : by_read_length;
    uint64_t taken = 0; uint32_t worst_kept_hits = 0, run_hits = 0; bool taking_run = false;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t pos = base + lane; const bool valid = pos < n;
        const ORD o = valid ? W.ord[pos] : (ORD)0; const uint32_t idx = (uint32_t)(o & IMASK);
        const uint32_t my_hits = valid ? W.hits[pos] : 0u, my_run = valid && (o & FLAG) ? W.run_hits[pos] : 0u, my_off = valid ? m[idx].offset : 0u;
        const uint32_t my_flags = ((o & FLAG) ? 1u : 0u) | ((o & KEPT) ? 2u : 0u);
        const double my_score = mz_choose_score(Q, my_hits);
        uint32_t my_verdict = 0;
        const uint32_t cnt = n - base < 64u ? n - base : 64u;
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint32_t hits = choose_bc(my_hits, j), flags = choose_bc(my_flags, j); const uint64_t off = choose_bc(my_off, j);
            if (flags & 1u) { run_hits = choose_bc(my_run, j); taking_run = false; }
            uint32_t failed = MZ_TAKEN;
            if (downsampling && !(flags & 2u)) failed = MZ_DOWNSAMPLED;
            else if (!hits) failed = MZ_NO_HITS;
            else if (run_hits > Q.hard_hit_cap) failed = MZ_HARD_HIT_CAP;
            if (!failed && Q.exclude_overlapping) {
                const uint64_t e = off + k < L ? off + k : L, stop = off + k < L + 1 ? off + k : L + 1;
                if (((W.ovl[off >> 6] >> (off & 63)) & 1ull) || ((W.ovl[e >> 6] >> (e & 63)) & 1ull)) failed = MZ_OVERLAPPING;
                else choose_mark(W.ovl, off, stop, lane);
            }
            if (!failed && Q.max_unique_min != 0) {
                const uint64_t lo = off < Q.flank ? 0 : off - Q.flank, hi = off + k + Q.flank < L ? off + k + Q.flank : L;
                if (taken < budget) { choose_mark(W.cov, lo, hi, lane); if (hits > worst_kept_hits) worst_kept_hits = hits; }
                else if (hits > worst_kept_hits) failed = MZ_MAX_MIN;
                else if (choose_any(W.cov, lo, hi, lane)) failed = MZ_MAX_MIN;
                else choose_mark(W.cov, lo, hi, lane);
            }
            if (!failed && score_filter) {
                const double sc = choose_bc(my_score, j);
                if (hits <= Q.hit_cap || mz_add(selected, sc) <= target || taking_run) selected = mz_add(selected, sc);
                else { failed = MZ_HIT_CAP; target = selected; }
            }
            if (lane == j) my_verdict = failed;
            if (!failed) { taking_run = true; ++taken; }
        }
        if (valid) out[idx] = (uint8_t)(P.as_take ? (my_verdict ? 0u : 1u) : my_verdict);
    }
}
__global__ void __launch_bounds__(64) minimizer_choose_kernel(const MzChooseParams P) {
    __shared__ uint64_t key[MZ_CHOOSE_LDS_MAX];
    __shared__ uint32_t ord[MZ_CHOOSE_LDS_MAX];
    __shared__ uint16_t dq[MZ_CHOOSE_LDS_MAX];
    __shared__ uint64_t bits[MZ_CHOOSE_LDS_MAX / 4];      // before the sort the read offsets (16 bits each), after it the two bitmaps of MZ_CHOOSE_LDS_BASES + 1 bits
    static_assert((MZ_CHOOSE_LDS_BASES + 1) * 2 <= MZ_CHOOSE_LDS_MAX / 4 * 64 && MZ_CHOOSE_LDS_MAX <= (1u << ChooseLds::BITS) && MZ_CHOOSE_LDS_BASES < 65536, "the LDS layout of the choice");
    ChooseWork<ChooseLds> W;
    // once sorted, the records need their keys no longer: the keys' 32 KiB then hold the layout / the hits (16 KiB) and the top runs' tables / the runs' sums (16 KiB)
    W.key = key; W.ord = ord; W.tmp = (uint32_t*)key; W.hits = (uint32_t*)key; W.start = (uint16_t*)(key + MZ_CHOOSE_LDS_MAX / 2); W.perm = (uint16_t*)(key + MZ_CHOOSE_LDS_MAX / 4 * 3);
    W.run_hits = (uint32_t*)(key + MZ_CHOOSE_LDS_MAX / 2); W.off = (uint16_t*)bits; W.dq = dq; W.cov = bits; W.ovl = bits + MZ_CHOOSE_LDS_MAX / 8;
    choose_read<ChooseLds>(P, P.ids[blockIdx.x], W, threadIdx.x);
}
__global__ void __launch_bounds__(64) minimizer_choose_slab_kernel(const MzChooseParams P) {
    char* s = P.slab + (uint64_t)blockIdx.x * P.slab_stride; const uint64_t np = P.slab_np, words = P.slab_words;
    ChooseWork<ChooseSlab> W;
    W.key = (uint64_t*)s; s += 8 * np; W.ord = (uint64_t*)s; s += 8 * np; W.tmp = (uint64_t*)s; s += 8 * np; W.cov = (uint64_t*)s; s += 8 * words; W.ovl = (uint64_t*)s; s += 8 * words;
    W.hits = (uint32_t*)s; s += 4 * np; W.run_hits = (uint32_t*)s; s += 4 * np; W.start = (uint32_t*)s; s += 4 * np; W.perm = (uint32_t*)s; s += 4 * np; W.off = (uint32_t*)s; s += 4 * np; W.dq = (uint32_t*)s;
    for (uint32_t i = blockIdx.x; i < P.n; i += gridDim.x) { choose_read<ChooseSlab>(P, P.ids[i], W, threadIdx.x); __syncthreads(); }
}
// ---- chains of anchors (chain_items_device.hpp: ci_problem_one is the rule and the checker).  A lane per candidate transition applies the filter
// and counts its destination's group; after the prefix sums a lane per survivor claims a place in that group (an atomic: the order inside a group
// is free, the winner is a maximum) and leaves (from, jump) there, the jump looked up here, off the DP's serial path.
__global__ void __launch_bounds__(256) chain_items_legal_kernel(const CiParams P) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= P.n_cands) return;
    const CiProb q = P.probs[ci_problem_of(P.cand_off, P.n_problems, c)];
    const vgk_chain_candidate e = P.cands[c];
    uint32_t indel = CI_DROPPED, why = 0;
    if (e.from >= q.n || e.to >= q.n) atomicOr(P.flags, 1u);
    else indel = ci_legal(P.anchors[q.a_off + e.from], P.anchors[q.a_off + e.to], e.graph_distance, q.lookback, q.limit, &why);
    P.indel[c] = indel;
    if (indel != CI_DROPPED) atomicAdd(&P.count[q.a_off + e.to], 1u);
}
__global__ void __launch_bounds__(256) chain_items_scatter_kernel(const CiParams P) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= P.n_cands) return;
    const uint32_t indel = P.indel[c];
    if (indel == CI_DROPPED) return;
    const CiProb q = P.probs[ci_problem_of(P.cand_off, P.n_problems, c)];
    const vgk_chain_candidate e = P.cands[c];
    const uint64_t dest = q.a_off + e.to;
    const uint32_t pos = P.first[dest] + atomicAdd(&P.cursor[dest], 1u);
    P.grouped[pos] = CiEdge{e.from, P.jump[q.jump_off + indel]};
}
// The DP: one wavefront per problem, destinations in anchor order.  The next 64 destinations sit one in each lane's registers (points, paths, the
// bounds of their groups) and are broadcast as their turn comes; the lanes stride over a destination's group — its first 64 transitions are
// fetched while the destination before it is reduced —, the three-part key is reduced across the wave by shuffles, and lane 0 writes the entry.
__device__ inline uint32_t ci_bc(uint32_t v, uint32_t j) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)j); }
__device__ inline uint64_t ci_bc(uint64_t v, uint32_t j) { return ((uint64_t)ci_bc((uint32_t)(v >> 32), j) << 32) | ci_bc((uint32_t)v, j); }
__device__ void ci_dp_problem(const CiParams& P, uint32_t p, int32_t* sc, uint64_t* paths, uint32_t lane) {
    const CiProb q = P.probs[p]; const uint32_t n = q.n;
    const vgk_chain_anchor* a = P.anchors + q.a_off; const uint32_t* first = P.first + q.a_off;
    const int32_t rp = P.recombination_penalty, cb = P.consistency_bonus;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t i = base + lane;
        int32_t my_points = 0; uint64_t my_start = 0, my_end = 0; uint32_t my_g0 = 0, my_g1 = 0;
        if (i < n) { const vgk_chain_anchor x = a[i]; my_points = x.score + P.item_bonus; my_start = x.start_paths; my_end = x.end_paths; my_g0 = first[i]; my_g1 = first[i + 1]; }
        const uint32_t cnt = n - base < 64u ? n - base : 64u;
        CiEdge ahead{0u, 0};
        { const uint32_t b0 = ci_bc(my_g0, 0), b1 = ci_bc(my_g1, 0); if (b0 + lane < b1) ahead = P.grouped[b0 + lane]; }
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint32_t t = base + j;
            const int32_t points = (int32_t)ci_bc((uint32_t)my_points, j); const uint64_t start = ci_bc(my_start, j), end = ci_bc(my_end, j);
            const uint32_t b0 = ci_bc(my_g0, j), b1 = ci_bc(my_g1, j);
            const CiEdge cur = ahead;
            if (j + 1 < cnt) { const uint32_t nb0 = ci_bc(my_g0, j + 1), nb1 = ci_bc(my_g1, j + 1); if (nb0 + lane < nb1) ahead = P.grouped[nb0 + lane]; }
            CiKey best = ci_from_nowhere(points, cb);
            if (b0 + lane < b1) {
                const CiKey k = ci_candidate(sc[cur.from], paths[cur.from], cur.from, cur.jump, points, start, end, rp, cb);
                if (ci_key_greater(k, best)) best = k;
            }
            for (uint32_t g = b0 + 64u + lane; g < b1; g += 64u) {
                const CiEdge e = P.grouped[g];
                const CiKey k = ci_candidate(sc[e.from], paths[e.from], e.from, e.jump, points, start, end, rp, cb);
                if (ci_key_greater(k, best)) best = k;
            }
            uint32_t k0 = (uint32_t)best.eval ^ 0x80000000u, k1 = (uint32_t)best.score ^ 0x80000000u, k2 = best.source;
            for (int d = 32; d > 0; d >>= 1) {
                const uint32_t o0 = __shfl_xor(k0, d), o1 = __shfl_xor(k1, d), o2 = __shfl_xor(k2, d);
                if (o0 > k0 || (o0 == k0 && (o1 > k1 || (o1 == k1 && o2 > k2)))) { k0 = o0; k1 = o1; k2 = o2; }
            }
            const int32_t score = (int32_t)(k1 ^ 0x80000000u); const uint32_t source = k2;
            const uint64_t kept = source == CI_NOWHERE ? end : ci_paths_after(paths[source], start, end);
            if (lane == 0) { sc[t] = score; paths[t] = kept; P.t_score[q.a_off + t] = score; P.t_source[q.a_off + t] = source; }
            __syncthreads();
        }
    }
}
extern __shared__ uint64_t ci_lds[];
__global__ void __launch_bounds__(64) chain_items_dp_kernel(const CiParams P) {
    ci_dp_problem(P, P.ids[blockIdx.x], (int32_t*)(ci_lds + P.lds_np), ci_lds, threadIdx.x);
}
__global__ void __launch_bounds__(64) chain_items_dp_slab_kernel(const CiParams P) {
    char* s = P.slab + (uint64_t)blockIdx.x * P.slab_stride;
    for (uint32_t i = blockIdx.x; i < P.n; i += gridDim.x) { ci_dp_problem(P, P.ids[i], (int32_t*)(s + 8ull * P.slab_n), (uint64_t*)s, threadIdx.x); __syncthreads(); }
}
// The tracebacks: the same wavefront shape.  The starts are put in order by a bitonic sort of anchor numbers (ci_start_before over the table), lane 0
// walks them (every anchor is visited once), the tracebacks are sorted by penalty the same way, and a lane per chain writes it out with its two
// recombination passes.
template <class IDX> struct CiTraceWork { int32_t* score; uint32_t* source; int32_t* pen; uint32_t* used; IDX* order; IDX* tmp; IDX* obeg; IDX* begin; };
template <class IDX, class BEFORE> __device__ void ci_bitonic(IDX* order, uint32_t np, uint32_t lane, BEFORE before) {
    constexpr IDX PAD = (IDX)~(IDX)0;
    for (uint32_t kk = 2; kk <= np; kk <<= 1) for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
        for (uint32_t t = lane; t < np / 2; t += 64) {
            const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i | j;
            const IDX oi = order[i], ol = order[l];
            const bool l_first = ol != PAD && (oi == PAD || before((uint32_t)ol, (uint32_t)oi));
            if (l_first == ((i & kk) == 0)) { order[i] = ol; order[l] = oi; }
        }
        __syncthreads();
    }
}
template <class IDX, bool COPY> __device__ void ci_trace_problem(const CiParams& P, uint32_t p, const CiTraceWork<IDX>& W, uint32_t lane) {
    constexpr IDX PAD = (IDX)~(IDX)0;
    const CiProb q = P.probs[p]; const uint32_t n = q.n, base = (uint32_t)q.a_off;
    const vgk_chain_anchor* a = P.anchors + q.a_off; vgk_chain_found* out = P.chains + q.slot;
    if (!n || !P.max_chains) { if (lane == 0) { out[0] = vgk_chain_found{0, base, 0u, base, 0u, 0u}; P.n_chains[p] = 1u; } return; }
    uint32_t np = 1; while (np < n) np <<= 1;
    int32_t best = (int32_t)0x80000000;
    for (uint32_t i = lane; i < np; i += 64) {
        if (i < n) {
            const int32_t s = P.t_score[q.a_off + i];
            if (COPY) { W.score[i] = s; W.source[i] = P.t_source[q.a_off + i]; }
            best = s > best ? s : best; W.order[i] = (IDX)i;
        } else W.order[i] = PAD;
    }
    for (uint32_t w = lane; w < (n + 31u) / 32u; w += 64) W.used[w] = 0u;
    for (int d = 32; d > 0; d >>= 1) { const int32_t o = __shfl_xor(best, d); best = o > best ? o : best; }
    __syncthreads();
    ci_bitonic<IDX>(W.order, np, lane, [&](uint32_t x, uint32_t y) { return ci_start_before(W.score[x], W.source[x], x, W.score[y], W.source[y], y); });
    uint32_t n_tb = 0;
    if (lane == 0) n_tb = ci_walk<IDX>(n, W.order, W.score, W.source, a, P.item_bonus, best, W.used, W.tmp, W.pen, W.begin);
    n_tb = (uint32_t)__shfl((int)n_tb, 0);
    __syncthreads();
    uint32_t np2 = 1; while (np2 < n_tb) np2 <<= 1;
    for (uint32_t k = lane; k < np2; k += 64) W.order[k] = k < n_tb ? (IDX)k : PAD;
    __syncthreads();
    ci_bitonic<IDX>(W.order, np2, lane, [&](uint32_t x, uint32_t y) { return W.pen[x] < W.pen[y] || (W.pen[x] == W.pen[y] && x < y); });
    const uint32_t n_out = n_tb < P.max_chains ? n_tb : P.max_chains;
    if (lane == 0) {
        uint32_t at = 0;
        for (uint32_t k = 0; k < n_out; ++k) { const uint32_t tb = W.order[k]; W.obeg[k] = (IDX)at; at += (uint32_t)W.begin[tb + 1] - (uint32_t)W.begin[tb]; }
        P.n_chains[p] = n_out;
    }
    __syncthreads();
    for (uint32_t k = lane; k < n_out; k += 64) {
        const uint32_t tb = W.order[k], b = W.begin[tb], len = (uint32_t)W.begin[tb + 1] - b, at = base + (uint32_t)W.obeg[k];
        for (uint32_t i = 0; i < len; ++i) P.items[at + i] = W.tmp[b + len - 1u - i];
        uint32_t nr = 0, nl = 0;
        ci_rec_passes(a, P.items + at, len, P.rec_right + at, P.rec_left + at, &nr, &nl);
        out[k] = vgk_chain_found{best - W.pen[tb], at, len, at, nr, nl};
    }
}
__global__ void __launch_bounds__(64) chain_items_trace_kernel(const CiParams P) {
    const uint32_t np = P.lds_np;
    CiTraceWork<uint16_t> W;
    uint32_t* w = (uint32_t*)ci_lds;
    W.score = (int32_t*)w; w += np; W.source = w; w += np; W.pen = (int32_t*)w; w += np; W.used = w; w += np / 32u + 1u;
    uint16_t* h = (uint16_t*)w;
    W.order = h; h += np; W.tmp = h; h += np; W.obeg = h; h += np; W.begin = h;      // (begin: np + 2 entries)
    ci_trace_problem<uint16_t, true>(P, P.ids[blockIdx.x], W, threadIdx.x);
}
__global__ void __launch_bounds__(64) chain_items_trace_slab_kernel(const CiParams P) {
    uint32_t* w = (uint32_t*)(P.slab + (uint64_t)blockIdx.x * P.slab_stride);
    CiTraceWork<uint32_t> W;
    W.pen = (int32_t*)w; w += P.slab_n; W.used = w; w += P.slab_n / 32u + 1u; W.order = w; w += P.slab_np; W.tmp = w; w += P.slab_n; W.obeg = w; w += P.slab_n; W.begin = w;      // (begin: slab_n + 2 entries)
    for (uint32_t i = blockIdx.x; i < P.n; i += gridDim.x) {
        const uint32_t p = P.ids[i];
        W.score = P.t_score + P.probs[p].a_off; W.source = P.t_source + P.probs[p].a_off;      // the table where the DP left it
        ci_trace_problem<uint32_t, false>(P, p, W, threadIdx.x);
        __syncthreads();
    }
}
// ---- anchors from seeds and gapless extensions (extension_anchors_device.hpp: ea_problem_one is the rule and the checker).  A lane per seed makes
// its anchor; a wavefront per problem puts the problem's seeds in diagonal order (a bitonic sort of seed numbers: LDS, or the slab); a lane per extension
// walks its path and counts, then — behind the prefix sums — lists the seeds it contains; a wavefront per problem does what depends on the order of the
// extensions: their order (bitonic), the sweep with its used flags (lane 0: ea_extension, the very code of the serial statement), the anchors' order
// (bitonic) and the write-out across the lanes.
__global__ void __launch_bounds__(256) extension_anchors_seeds_kernel(const EaParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.n_seeds) return;
    vgk_chain_anchor a;
    if (ea_seed_anchor(P.seeds[i], P.n_oriented, P.node_tab, P.match, &a)) P.seed_anchor[i] = a;
    else atomicOr(P.flags, (uint32_t)EA_BAD_SEED);
}
__device__ void ea_sort_problem(const EaParams& P, uint32_t p, uint32_t* order, uint32_t lane) {
    const EaProb q = P.probs[p];
    if (!q.n_seeds || !q.n_ext) return;
    const vgk_anchor_seed* s = P.seeds + q.s_off;
    uint32_t np = 1; while (np < q.n_seeds) np <<= 1;
    for (uint32_t i = lane; i < np; i += 64) order[i] = i < q.n_seeds ? i : EA_NONE;
    __syncthreads();
    ci_bitonic<uint32_t>(order, np, lane, [&](uint32_t x, uint32_t y) { return ea_diag_before(s, x, y); });
    for (uint32_t i = lane; i < q.n_seeds; i += 64) P.sorted[q.s_off + i] = order[i];
}
__global__ void __launch_bounds__(64) extension_anchors_sort_kernel(const EaParams P) {
    ea_sort_problem(P, P.ids[blockIdx.x], (uint32_t*)ci_lds, threadIdx.x);
}
__global__ void __launch_bounds__(64) extension_anchors_sort_slab_kernel(const EaParams P) {
    uint32_t* order = (uint32_t*)(P.slab + (uint64_t)blockIdx.x * P.slab_stride);
    for (uint32_t i = blockIdx.x; i < P.n; i += gridDim.x) { ea_sort_problem(P, P.ids[i], order, threadIdx.x); __syncthreads(); }
}
__global__ void __launch_bounds__(256) extension_anchors_lists_kernel(const EaParams P, const int emit) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= P.n_ext) return;
    const EaProb q = P.probs[P.prob_of_ext[x]];
    if (emit) {
        uint32_t* list = P.ext_seeds + P.ext_first[x]; uint32_t at = 0;
        ea_ext_seeds(P.ext[x], P.nodes, P.node_tab, P.seeds + q.s_off, P.sorted + q.s_off, q.n_seeds, [&](uint32_t i) { list[at++] = i; });
    } else P.ext_count[x] = ea_ext_seeds(P.ext[x], P.nodes, P.node_tab, P.seeds + q.s_off, P.sorted + q.s_off, q.n_seeds, [](uint32_t) {});
}
__device__ void ea_anchors_problem(const EaParams& P, uint32_t p, uint32_t* order, uint32_t* used, uint32_t lane) {
    const EaProb q = P.probs[p];
    const vgk_anchor_seed* s = P.seeds + q.s_off; const vgk_extension* e = P.ext + q.e_off; const vgk_chain_anchor* sa = P.seed_anchor + q.s_off;
    vgk_chain_anchor* made = P.made + q.s_off; vgk_anchor_origin* origin = P.made_origin + q.s_off; uint32_t* rep = P.rep + q.s_off + q.e_off;
    uint32_t n_made = 0, n_rep = 0;
    if (P.from_seeds) {
        for (uint32_t i = lane; i < q.n_seeds; i += 64) ea_from_seed(sa[i], i, made, origin, rep);
        n_made = n_rep = q.n_seeds;
    } else {
        uint32_t n_full = 0;
        if (lane == 0) n_full = ea_full_length(q, e, P.max_mismatches, rep);
        n_full = (uint32_t)__shfl((int)n_full, 0);
        if (n_full) { if (lane == 0) { P.status[p] = VGK_ANCHORS_FULL_LENGTH; P.n_anchors[p] = 0u; P.n_rep[p] = n_full; } return; }
        uint32_t np = 1; while (np < q.n_ext) np <<= 1;
        for (uint32_t i = lane; i < np; i += 64) order[i] = i < q.n_ext ? i : EA_NONE;
        for (uint32_t w = lane; w < q.n_seeds / 32u + 1u; w += 64) used[w] = 0u;
        __syncthreads();
        ci_bitonic<uint32_t>(order, np, lane, [&](uint32_t x, uint32_t y) { return ea_ext_before(e, x, y); });
        if (lane == 0) {
            EaOut out{made, origin, rep, 0u, 0u};
            for (uint32_t k = 0; k < q.n_ext; ++k) {
                const uint32_t x = order[k], l0 = P.ext_first[q.e_off + x], l1 = P.ext_first[q.e_off + x + 1];
                ea_extension(e[x], x, P.mism + e[x].mism_begin, P.ext_seeds + l0, l1 - l0, s, sa, used, P.match, P.mismatch, out);
            }
            n_made = out.n_made; n_rep = out.n_rep;
        }
        n_made = (uint32_t)__shfl((int)n_made, 0); n_rep = (uint32_t)__shfl((int)n_rep, 0);
    }
    __syncthreads();
    uint32_t np = 1; while (np < n_made) np <<= 1;
    for (uint32_t i = lane; i < np; i += 64) order[i] = i < n_made ? i : EA_NONE;
    __syncthreads();
    ci_bitonic<uint32_t>(order, np, lane, [&](uint32_t x, uint32_t y) { return ea_anchor_before(made, x, y); });
    for (uint32_t k = lane; k < n_made; k += 64) { const uint32_t from = order[k]; P.anchors[q.s_off + k] = made[from]; P.origins[q.s_off + k] = origin[from]; }
    if (lane == 0) { P.status[p] = 0u; P.n_anchors[p] = n_made; P.n_rep[p] = n_rep; }
}
__global__ void __launch_bounds__(64) extension_anchors_kernel(const EaParams P) {
    uint32_t* order = (uint32_t*)ci_lds;
    ea_anchors_problem(P, P.ids[blockIdx.x], order, order + P.lds_np, threadIdx.x);
}
__global__ void __launch_bounds__(64) extension_anchors_slab_kernel(const EaParams P) {
    uint32_t* order = (uint32_t*)(P.slab + (uint64_t)blockIdx.x * P.slab_stride);
    for (uint32_t i = blockIdx.x; i < P.n; i += gridDim.x) { ea_anchors_problem(P, P.ids[i], order, order + P.slab_np, threadIdx.x); __syncthreads(); }
}
// ---- one Path per read (chain_device.hpp): a lane per read for the bounds and the composition, a wavefront per read for the dense copy
// ---- a short read's alignments from its extension set and its tails (read_alignments_device.hpp: ra_read_one is the rule and the checker).  A lane per
// read.  The selection's working words lie in LDS, one slice per lane at an odd stride (no two lanes of a wavefront in one bank), for sets of up to
// RA_LDS_EXT extensions; the reads with larger sets come in a launch of their own over slices of a slab in HBM.  Count and emit are the one composer.
__global__ void __launch_bounds__(64) read_alignments_select_kernel(const RaParams P) {
    __shared__ uint32_t work[64 * RA_LDS_STRIDE];
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t r = P.ids ? P.ids[i] : i;
    // (the resident form: every read in one launch; the few large sets take their slices of the slab, by the extensions before them)
    uint32_t* mine = work + threadIdx.x * RA_LDS_STRIDE;
    if (P.work && P.res[r].n_ext > RA_LDS_EXT) mine = P.work + 9ull * P.res[r].ext_begin + 4ull * r;
    ra_read_one(P, RA_RUN_SELECT, r, mine);
}
__global__ void __launch_bounds__(64) read_alignments_select_slab_kernel(const RaParams P) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < P.n) ra_read_one(P, RA_RUN_SELECT, P.ids[i], P.work + P.work_off[i]);
}
__global__ void __launch_bounds__(64) read_alignments_compose_kernel(const RaParams P, const int what) {
    const uint32_t r = blockIdx.x * 64 + threadIdx.x;
    if (r < (what == RA_RUN_TAILS ? P.n_tails : P.n_reads)) ra_read_one(P, what, r, nullptr);
}
// ---- a read's mapping quality (read_mapq_device.hpp: mq_region_one and mq_read_one are the rules and the checkers).  Agglomerations: a lane per
// minimizer.  The quality: a lane per read; the explored order and the c[] table lie in LDS, one slice per lane at an odd stride (no two lanes of a
// wavefront start in one bank), for reads of up to MQ_LDS_EXPLORED explored minimizers; the others come in a launch of their own over slices of a slab.
__global__ void __launch_bounds__(256) minimizer_regions_kernel(const MqRegionParams P) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < P.n_minimizers) mq_region_one(P, j);
}
__global__ void __launch_bounds__(64) read_mapq_kernel(const MqParams P) {
    __shared__ uint32_t work[64 * MQ_LDS_STRIDE];
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < P.n) mq_read_one(P, P.ids[i], work + threadIdx.x * MQ_LDS_STRIDE);
}
__global__ void __launch_bounds__(64) read_mapq_slab_kernel(const MqParams P) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < P.n) mq_read_one(P, P.ids[i], P.work + P.work_off[i]);
}
// ---- a pair's mapping qualities (pair_mapq_device.hpp: pm_candidate_score and pm_pair_one are the rules and the checkers).  The mates' caps: the
// sweep above without the scores' half (mq_cap_one), cap and verdict per read left in HBM.  Scores: a lane per candidate.  The pairs: a lane per pair;
// the order and the ordered scores lie in LDS, one slice per lane at an odd stride, for pairs of up to PM_LDS_CANDIDATES candidates; the others come
// in a launch of their own over slices of a slab.
__global__ void __launch_bounds__(64) explored_cap_kernel(const MqParams P) {
    __shared__ uint32_t work[64 * MQ_LDS_STRIDE];
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < P.n) mq_cap_one(P, P.ids[i], work + threadIdx.x * MQ_LDS_STRIDE);
}
__global__ void __launch_bounds__(64) explored_cap_slab_kernel(const MqParams P) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < P.n) mq_cap_one(P, P.ids[i], P.work + P.work_off[i]);
}
__global__ void __launch_bounds__(256) pair_score_kernel(const PmParams P) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < P.n_candidates) P.pair_score[j] = pm_candidate_score(P, P.cands[j]);
}
__global__ void __launch_bounds__(64) pair_mapq_kernel(const PmParams P) {
    __shared__ uint32_t work[64 * PM_LDS_STRIDE];
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < P.n) pm_pair_one(P, P.ids[i], work + threadIdx.x * PM_LDS_STRIDE);
}
__global__ void __launch_bounds__(64) pair_mapq_slab_kernel(const PmParams P) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < P.n) pm_pair_one(P, P.ids[i], P.work + P.work_off[i]);
}
// ---- a short read's funnel (read_funnel_device.hpp: rf_item_one is the rule and the checker).  A lane per cluster or set for the scoring, a lane per read
// for the walks, by P.what; a cluster's present bits and covered bitmap, a set's chain table, a walk's order lie in LDS, one slice per lane at an odd
// stride (no two lanes of a wavefront start in one bank), up to the FN_LDS_* limits; the items beyond them come in a launch of their own over slices of
// a slab.  The gather lays a walk's accepted items out at their prefix sums, a lane per read.
__global__ void __launch_bounds__(64) funnel_kernel(const FnParams P) {
    __shared__ uint32_t work[64 * FN_LDS_STRIDE];
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < P.n) rf_item_one(P, P.ids[i], work + threadIdx.x * FN_LDS_STRIDE);
}
__global__ void __launch_bounds__(64) funnel_slab_kernel(const FnParams P) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < P.n) rf_item_one(P, P.ids[i], P.work + P.work_off[i]);
}
__global__ void __launch_bounds__(64) funnel_gather_kernel(const FnParams P) {
    const uint32_t r = blockIdx.x * 64 + threadIdx.x;
    if (r < P.n_reads) rf_gather_one(P, r);
}
// ---- a chain's links (chain_links_device.hpp: cl_walk_one and cl_slot are the rule and the checker).  Only the walk is serial, a lane per chain; the
// checks, the counts and the write-out are a lane per item slot / distance entry / link slot, the sequences a wavefront per link.  No LDS.
__global__ void __launch_bounds__(256) chain_links_check_kernel(const ClParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < P.n_slots + P.n_dist) cl_check_one(P, i);
}
__global__ void __launch_bounds__(64) chain_links_walk_kernel(const ClParams P) {
    const uint32_t c = blockIdx.x * 64 + threadIdx.x;
    if (c < P.n_chains) cl_walk_one(P, c);
}
// the three counts of every link slot; their totals in 64 bits: summed over the wavefront, one atomic per wavefront and total
__global__ void __launch_bounds__(256) chain_links_count_kernel(const ClParams P) {
    const uint32_t ls = blockIdx.x * 256 + threadIdx.x;
    uint32_t out[3] = {0, 0, 0};
    if (ls < cl_link_slots(P)) cl_count_one(P, ls, out);
    unsigned long long t0 = out[0], t1 = out[1], t2 = out[2];
    for (int d = 32; d > 0; d >>= 1) { t0 += __shfl_xor(t0, d, 64); t1 += __shfl_xor(t1, d, 64); t2 += __shfl_xor(t2, d, 64); }
    if ((threadIdx.x & 63) == 0) {
        if (t0) atomicAdd(P.totals + 0, t0);
        if (t1) atomicAdd(P.totals + 1, t1);
        if (t2) atomicAdd(P.totals + 2, t2);
    }
}
// the write-out; anchor_score: a segmented sum — a wavefront's lanes of one chain are neighbours, so an inclusive scan that stops at the chain's first
// lane leaves the chain's share in its last lane of the wavefront, which adds it: one atomic per wavefront per chain (integers: any order, one sum)
__global__ void __launch_bounds__(256) chain_links_write_kernel(const ClParams P) {
    const uint32_t ls = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool live = ls < cl_link_slots(P);
    uint32_t chain = 0xffffffffu;
    long long share = 0;
    if (live) share = cl_write_one(P, ls, &chain);
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const long long up = __shfl_up(share, d, 64); const uint32_t up_chain = __shfl_up(chain, d, 64);
        if (lane >= d && up_chain == chain) share += up;
    }
    const uint32_t down_chain = __shfl_down(chain, 1, 64);
    if (live && share != 0 && (lane == 63 || down_chain != chain)) atomicAdd((unsigned long long*)&P.res[chain].anchor_score, (unsigned long long)share);
}
// a link's bases from its read: a wavefront per link; dwords where source and destination agree in alignment (bytes up to the first aligned
// destination and behind the last whole dword), bytes otherwise
__global__ void __launch_bounds__(256) chain_links_seq_kernel(const ClParams P) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= P.n_links) return;
    const vgk_chain_link L = P.links[i];
    const char* src = P.reads + P.read_off[P.chains[L.chain].read] + L.read_begin;
    char* dst = P.seqs + P.seq_off[i];
    const uint32_t len = L.length;
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 3) == 0) {
        uint32_t head = (uint32_t)((4 - ((uintptr_t)dst & 3)) & 3);
        if (head > len) head = len;
        if (lane < head) dst[lane] = src[lane];
        const uint32_t words = (len - head) / 4;
        const uint32_t* s4 = (const uint32_t*)(src + head); uint32_t* d4 = (uint32_t*)(dst + head);
        for (uint32_t k = lane; k < words; k += 64) d4[k] = s4[k];
        const uint32_t done = head + 4 * words;
        if (lane < len - done) dst[done + lane] = src[done + lane];
    } else {
        for (uint32_t k = lane; k < len; k += 64) dst[k] = src[k];
    }
}
// ---- a long read's mappings (pick_mappings_device.hpp: pick_alignment_one and pick_read_one are the rule and the checker).  The checks a lane per
// alignment and per chain, the statistics a lane per mapping slot with the two sums of an alignment as segmented wavefront sums, multiplicities and sort
// scores a lane per alignment; the pick a wavefront per read: all 64 lanes go through the one walk, share out an alignment's mappings for its fraction
// and its marks, and keep the walk's order and the used-node table in LDS — or, for the reads beyond the limits, in the block's slab.
__global__ void __launch_bounds__(256) pick_check_kernel(const PickParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (uint64_t)P.n_alns + P.n_chains) pick_check_one(P, i);
}
// a wavefront's lanes of one alignment are neighbours: an inclusive scan that stops at the alignment's first lane leaves its share in its last lane of
// the wavefront, which adds it: one atomic per wavefront, alignment and sum (integers: any order, one sum)
__global__ void __launch_bounds__(256) pick_stats_kernel(const PickParams P) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool live = s < P.n_slots;
    uint32_t aln = 0xffffffffu;
    unsigned long long share[2] = {0, 0};
    if (live) pick_stat_one(P, s, &aln, share);
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const unsigned long long up0 = __shfl_up(share[0], d, 64), up1 = __shfl_up(share[1], d, 64); const uint32_t up_aln = __shfl_up(aln, d, 64);
        if (lane >= d && up_aln == aln) { share[0] += up0; share[1] += up1; }
    }
    const uint32_t down_aln = __shfl_down(aln, 1, 64);
    if (live && (lane == 63 || down_aln != aln)) {
        if (share[0]) atomicAdd(P.sums + 2 * (uint64_t)aln, share[0]);
        if (share[1]) atomicAdd(P.sums + 2 * (uint64_t)aln + 1, share[1]);
    }
}
__global__ void __launch_bounds__(256) pick_alignments_kernel(const PickParams P) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < P.n_alns) pick_alignment_one(P, i);
}
// the 64 lanes of a pick.  LDS: the table is the block's own, a barrier orders its compare-and-swaps before the plain loads
struct PickWaveLds {
    uint32_t lane, lanes;
    __device__ unsigned long long sum(unsigned long long x) const { for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64); return x; }
    __device__ void sync() const { __syncthreads(); }
    __device__ uint32_t load(const uint32_t* p) const { return *p; }
    __device__ void store(uint32_t* p, uint32_t v) const { *p = v; }
    __device__ uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) const { return atomicCAS(p, expect, v); }
};
// the slab: the table lies in HBM, where compare-and-swap is done at L2; loads and stores of it go there too, past the CU's own cache
struct PickWaveSlab {
    uint32_t lane, lanes;
    __device__ unsigned long long sum(unsigned long long x) const { for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64); return x; }
    __device__ void sync() const { __threadfence(); __syncthreads(); }
    __device__ uint32_t load(const uint32_t* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ void store(uint32_t* p, uint32_t v) const { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) const { return atomicCAS(p, expect, v); }
};
__global__ void __launch_bounds__(64) pick_kernel(const PickParams P) {
    __shared__ uint32_t order[FN_LDS_ITEMS];
    __shared__ uint32_t table[PICK_LDS_SLOTS];
    pick_read_one(P, P.ids[blockIdx.x], order, table, PICK_LDS_SLOTS, PickWaveLds{threadIdx.x, 64u});
}
__global__ void __launch_bounds__(64) pick_slab_kernel(const PickParams P) {
    uint32_t* order = (uint32_t*)(P.slab + (uint64_t)blockIdx.x * P.slab_stride);
    for (uint32_t i = blockIdx.x; i < P.n; i += gridDim.x) { pick_read_one(P, P.ids[i], order, order + P.slab_items, P.slab_slots, PickWaveSlab{threadIdx.x, 64u}); __syncthreads(); }
}
__global__ void __launch_bounds__(64) chain_stitch_kernel(const CsParams P, const int what) {
    cs_one(P, what, blockIdx.x * 64 + threadIdx.x);
}
__global__ void __launch_bounds__(256) chain_gather_kernel(const CsParams P) {
    const uint32_t r = blockIdx.x * 4 + threadIdx.x / 64;
    if (r < P.n_reads) cs_gather_one(P, r, threadIdx.x & 63u, 64);
}
__global__ void __launch_bounds__(256) forest_flags_kernel(const ForestParams P) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v < P.n_nodes) forest_flags_one(P, v);
}
__global__ void __launch_bounds__(256) forest_emit_kernel(const ForestParams P) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v < P.n_nodes) forest_emit_one(P, v);
}

// ---- the WFA problems' sequences masked / flipped / laid out on the device: a wavefront per problem, four to a block
__global__ void __launch_bounds__(256) wfa_mask_kernel(const WProb* probs, const uint32_t* src_off, const char* raw, char* seqs, const uint32_t n) {
    const uint32_t i = blockIdx.x * 4 + threadIdx.x / 64;
    if (i < n) wfa_mask_one(probs, src_off, raw, seqs, i, threadIdx.x & 63u, 64);
}
// ---- wavefront alignment (wfa_device.hpp): the same launch shape
__global__ void __launch_bounds__(64, 4) wfa_kernel(const WfaParams P, const uint32_t threads) {
    __shared__ uint32_t node_end[W_NODES * 64];                    // [trie node][lane]: conflict-free, 8 KB per wavefront
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t < threads) wfa_thread(P, t, node_end + threadIdx.x, 64);
    if (P.producers_done) {                                        // run beside the wavefront kernel: this wavefront will hand nothing over any more
        __threadfence();                                           // (its list entries before the count the consumers trust)
        __builtin_amdgcn_wave_barrier();
        if (threadIdx.x == 0) atomicAdd(P.producers_done, 1u);
    }
}

// ---- wavefront alignment, one wavefront per problem (wfa_wave_device.hpp): trie nodes, possible penalties and the lanes' work lists in
//      LDS, the wavefront table / its log / the path pool in the wavefront's slab (workgroup-scope atomics: one wavefront = one workgroup)
struct WwXlHip {
    __device__ __forceinline__ unsigned long long ballot(bool flag) const { return __ballot(flag); }
    __device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t src) const { return (uint32_t)__shfl((int)v, (int)src, 64); }
    __device__ __forceinline__ unsigned long long reduce_min_u64(unsigned long long v) const {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { const unsigned long long o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
        return v;
    }
    __device__ __forceinline__ int32_t reduce_max(int32_t v) const {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { const int32_t o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
        return v;
    }
    __device__ __forceinline__ void fence() const { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }
    // the same for LDS alone: a wavefront's LDS instructions execute in order, so its lanes see each other's LDS writes once the compiler
    // keeps the order — no wait for the global stores in flight (a full fence after a step's table stores waits ~1.5 us for them)
    __device__ __forceinline__ void fence_lds() const { __builtin_amdgcn_wave_barrier(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }
    __device__ __forceinline__ unsigned long long load64(const unsigned long long* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ void store64(unsigned long long* p, unsigned long long v) const { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ unsigned long long cas64(unsigned long long* p, unsigned long long expect, unsigned long long desired) const {
        __hip_atomic_compare_exchange_strong(p, &expect, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return expect;                                                         // the value found there
    }
    __device__ __forceinline__ uint32_t add32(uint32_t* p, uint32_t v) const { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ uint32_t clock_us() const { return (uint32_t)(wall_clock64() / 100ull); }      // (the constant 100 MHz counter; statistics only)
    __device__ __forceinline__ void or32(uint32_t* p, uint32_t v) const { __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ uint32_t load32(const uint32_t* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};
__global__ void __launch_bounds__(64, VGK_WW_OCC) wfa_wave_kernel(const WwParams P) {
    __shared__ WwSharedBoth sh;
    WwXlHip xl;
    wfa_wave(P, blockIdx.x, threadIdx.x, sh, xl);
}

// ---- pinned gssw fill with full matrices (gssw_matrix_device.hpp): one wavefront per problem, R read rows per lane; the
//      one-thread-per-problem form remains for scorings with gap_open < gap_extend
// the k-best tracebacks of vgk_gssw_align_multi over the kept matrices: one lane per problem (gssw_multi_device.hpp)
__global__ void __launch_bounds__(64) banded_multi_kernel(const BandedMultiParams Q) {
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a < Q.P.n) banded_multi_one(Q, a);
}
__global__ void __launch_bounds__(64) gssw_multi_kernel(const GsswMultiParams P) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P.M.n) gssw_multi_one(P, i);
}
__global__ void __launch_bounds__(64) gssw_matrix_kernel(const GsswMatrixParams P) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < P.n) gssw_matrix_one(P, i);
}
// The same primitives over ONE ROW of 16 lanes (a DPP row): four problems share a wavefront, each in a row of its own.  Rows run loops
// of different lengths; a row is active or masked off as a whole, and nothing here reaches outside its row.
constexpr uint32_t XB_STAGE16 = 1024, XB_STAGE64 = 4096;          // graph bases staged in LDS per problem (xdrop_band_wave_lane)
struct XlDpp16 {
    uint8_t* stg; int32_t* cc; uint32_t cap = XB_STAGE16;
    __device__ __forceinline__ int32_t* col_cache() const { return cc; }
    __device__ __forceinline__ void lds_sync() const { __builtin_amdgcn_wave_barrier(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }
    __device__ __forceinline__ uint8_t* stage() const { return stg; }
    __device__ __forceinline__ uint32_t stage_cap() const { return cap; }
    __device__ __forceinline__ void stage_sync() const { __builtin_amdgcn_wave_barrier(); asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }
    __device__ __forceinline__ uint32_t width() const { return 16u; }
    __device__ __forceinline__ int32_t down(int32_t v) const { return __builtin_amdgcn_update_dpp(BNEG, v, 0x111 /* row_shr:1 */, 0xf, 0xf, false); }
    __device__ __forceinline__ int32_t scan_excl(int32_t v) const {       // exclusive max-scan over the row (XlDpp::scan_excl without the steps across rows)
        asm volatile("s_nop 4\n\tv_max_i32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1" : "+v"(v));
        return down(v);
    }
    __device__ __forceinline__ void fence() const { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }
    __device__ __forceinline__ unsigned long long ballot(bool flag) const { return (__ballot(flag) >> (threadIdx.x & 48u)) & 0xffffull; }
    __device__ __forceinline__ bool any(int32_t flag) const { return ballot(flag != 0) != 0ull; }
    __device__ __forceinline__ int32_t reduce_max(int32_t v) const {      // rotations inside the row (row_ror): no trip through the LDS crossbar
        int32_t o;
        o = __builtin_amdgcn_update_dpp(v, v, 0x128 /* row_ror:8 */, 0xf, 0xf, false); v = o > v ? o : v;
        o = __builtin_amdgcn_update_dpp(v, v, 0x124 /* row_ror:4 */, 0xf, 0xf, false); v = o > v ? o : v;
        o = __builtin_amdgcn_update_dpp(v, v, 0x122 /* row_ror:2 */, 0xf, 0xf, false); v = o > v ? o : v;
        o = __builtin_amdgcn_update_dpp(v, v, 0x121 /* row_ror:1 */, 0xf, 0xf, false); v = o > v ? o : v;
        return v;
    }
    __device__ __forceinline__ unsigned long long reduce_add(unsigned long long v) const {
#pragma unroll
        for (int d = 8; d > 0; d >>= 1) v += __shfl_xor(v, d, 16);
        return v;
    }
};
struct XlDppStaged : XlDpp {
    uint8_t* stg; int32_t* cc;
    __device__ __forceinline__ uint32_t width() const { return 64u; }
    __device__ __forceinline__ int32_t* col_cache() const { return cc; }
    __device__ __forceinline__ void lds_sync() const { __builtin_amdgcn_wave_barrier(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }
    __device__ __forceinline__ uint8_t* stage() const { return stg; }
    __device__ __forceinline__ uint32_t stage_cap() const { return XB_STAGE64; }
    __device__ __forceinline__ void stage_sync() const { __builtin_amdgcn_wave_barrier(); asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }
};
// (CT: the planes' cell type — int32_t, or int16_t when the call's bounds allow, GsswMatrixParams::xb_cell16)
template <class CT>
__global__ void __launch_bounds__(64) xdrop_band_kernel(const GsswMatrixParams P) {
    __shared__ uint8_t stg[XB_STAGE64];
    __shared__ int32_t cc[2 * 2 * 64 * 8];                       // two last columns (H | E) of up to 512 rows
    XlDppStaged xl; xl.stg = stg; xl.cc = cc;
    xdrop_band_wave_lane_t<CT>(P, P.xb_order ? P.xb_order[P.xb_n8 + P.xb_n16 + blockIdx.x] : blockIdx.x, threadIdx.x, xl);
}
// three wavefronts per SIMD (168 VGPRs, five spilled dwords): 26.2 -> 21.0 ms per 200 000 tails against the compiler's own 175 VGPRs = two;
// four (128 VGPRs, 38 spilled): the same 20.9 ms
#ifndef VGK_XB_OCC
#define VGK_XB_OCC 3
#endif
template <class CT>
__global__ void __launch_bounds__(64, VGK_XB_OCC) xdrop_band_kernel16(const GsswMatrixParams P) {
    __shared__ uint8_t stg[4 * XB_STAGE16];
    __shared__ int32_t cc[4 * 2 * 2 * 16 * 8];                   // per problem: two last columns (H | E) of up to 128 rows
    const uint32_t slot = blockIdx.x * 4u + (threadIdx.x >> 4);
    if (slot >= P.xb_n16) return;
    XlDpp16 xl; xl.stg = stg + (threadIdx.x >> 4) * XB_STAGE16; xl.cc = cc + (threadIdx.x >> 4) * (2 * 2 * 16 * 8);
    xdrop_band_wave_lane_t<CT>(P, P.xb_order[P.xb_n8 + slot], threadIdx.x & 15u, xl);
}
// the tracebacks of the X-drop band path, one lane per problem, in the fills' launch order (neighbours walk graphs of like size)
// the packed fill (xdrop_band_pk_lane): two rows to a register, half the registers, a quarter of the LDS (a word per row pair in the column
// cache, 512 staged bases per problem)
#ifndef VGK_XBP_OCC
#define VGK_XBP_OCC 4
#endif
constexpr uint32_t XBP_STAGE16 = 512;
__global__ void __launch_bounds__(64, VGK_XBP_OCC) xdrop_band_pk_kernel16(const GsswMatrixParams P) {
    __shared__ uint8_t stg[4 * XBP_STAGE16];
    __shared__ int32_t cc[4 * 2 * 2 * 16 * 4];
    const uint32_t slot = blockIdx.x * 4u + (threadIdx.x >> 4);
    if (slot >= P.xb_n16) return;
    XlDpp16 xl; xl.stg = stg + (threadIdx.x >> 4) * XBP_STAGE16; xl.cc = cc + (threadIdx.x >> 4) * (2 * 2 * 16 * 4); xl.cap = XBP_STAGE16;
    xdrop_band_pk_lane(P, P.xb_order[P.xb_n8 + slot], threadIdx.x & 15u, xl);
}
// The same over HALF a DPP row: eight problems share a wavefront, 8 lanes (64 rows) each — tails of at most 63 bases, which left half of a
// 16-lane row idle.  The DPP shifts stay row-wide; what would cross from lane 7 into lane 8 is masked: bank_mask for the shift by 4 (banks are
// four lanes), a select per lane for the shifts by 1 and 2; the maximum over the group is two quad permutes and a half-row mirror.
struct XlDpp8 {
    uint8_t* stg; int32_t* cc; uint32_t cap;
    __device__ __forceinline__ int32_t* col_cache() const { return cc; }
    __device__ __forceinline__ void lds_sync() const { __builtin_amdgcn_wave_barrier(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }
    __device__ __forceinline__ uint8_t* stage() const { return stg; }
    __device__ __forceinline__ uint32_t stage_cap() const { return cap; }
    __device__ __forceinline__ void stage_sync() const { __builtin_amdgcn_wave_barrier(); asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }
    __device__ __forceinline__ uint32_t width() const { return 8u; }
    __device__ __forceinline__ int32_t down(int32_t v) const {
        const int32_t r = __builtin_amdgcn_update_dpp(BNEG, v, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
        return (threadIdx.x & 7u) ? r : BNEG;
    }
    __device__ __forceinline__ int32_t scan_excl(int32_t v) const {       // exclusive max-scan over the group's 8 lanes
        const uint32_t l = threadIdx.x & 7u;
        int32_t t = __builtin_amdgcn_update_dpp(BNEG, v, 0x111 /* row_shr:1 */, 0xf, 0xf, false); t = l >= 1u ? t : BNEG; v = t > v ? t : v;
        t = __builtin_amdgcn_update_dpp(BNEG, v, 0x112 /* row_shr:2 */, 0xf, 0xf, false); t = l >= 2u ? t : BNEG; v = t > v ? t : v;
        t = __builtin_amdgcn_update_dpp(BNEG, v, 0x114 /* row_shr:4 */, 0xf, 0xa /* lanes 4-7 and 12-15 */, false); v = t > v ? t : v;
        return down(v);
    }
    __device__ __forceinline__ void fence() const { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }
    __device__ __forceinline__ unsigned long long ballot(bool flag) const { return (__ballot(flag) >> (threadIdx.x & 56u)) & 0xffull; }
    __device__ __forceinline__ bool any(int32_t flag) const { return ballot(flag != 0) != 0ull; }
    __device__ __forceinline__ int32_t reduce_max(int32_t v) const {
        int32_t o;
        o = __builtin_amdgcn_update_dpp(v, v, 0xb1 /* quad_perm:[1,0,3,2] */, 0xf, 0xf, false); v = o > v ? o : v;
        o = __builtin_amdgcn_update_dpp(v, v, 0x4e /* quad_perm:[2,3,0,1] */, 0xf, 0xf, false); v = o > v ? o : v;
        o = __builtin_amdgcn_update_dpp(v, v, 0x141 /* row_half_mirror */, 0xf, 0xf, false); v = o > v ? o : v;
        return v;
    }
    __device__ __forceinline__ unsigned long long reduce_add(unsigned long long v) const {
#pragma unroll
        for (int d = 4; d > 0; d >>= 1) v += __shfl_xor(v, d, 8);
        return v;
    }
};
constexpr uint32_t XBP_STAGE8 = 256;
__global__ void __launch_bounds__(64, VGK_XBP_OCC) xdrop_band_pk_kernel8(const GsswMatrixParams P) {
    __shared__ uint8_t stg[8 * XBP_STAGE8];
    __shared__ int32_t cc[8 * 2 * 2 * 8 * 4];
    const uint32_t slot = blockIdx.x * 8u + (threadIdx.x >> 3);
    if (slot >= P.xb_n8) return;
    XlDpp8 xl; xl.stg = stg + (threadIdx.x >> 3) * XBP_STAGE8; xl.cc = cc + (threadIdx.x >> 3) * (2 * 2 * 8 * 4); xl.cap = XBP_STAGE8;
    xdrop_band_pk_lane(P, P.xb_order[slot], threadIdx.x & 7u, xl);
}
__global__ void __launch_bounds__(64) xdrop_band_pk_kernel(const GsswMatrixParams P) {
    __shared__ uint8_t stg[XB_STAGE64];
    __shared__ int32_t cc[2 * 2 * 64 * 4];
    XlDppStaged xl; xl.stg = stg; xl.cc = cc;
    xdrop_band_pk_lane(P, P.xb_order ? P.xb_order[P.xb_n8 + P.xb_n16 + blockIdx.x] : blockIdx.x, threadIdx.x, xl);
}
template <class CT>
__global__ void __launch_bounds__(64) xdrop_band_walk_kernel(const GsswMatrixParams P) {
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k < P.n) xdrop_band_walk_one_t<CT>(P, P.xb_order ? P.xb_order[k] : k);
}
template <int R>
__global__ void __launch_bounds__(64) gssw_matrix_wave_kernel(const GsswMatrixParams P, const uint32_t rows_lo, const uint32_t rows_hi) {
    const uint32_t i = blockIdx.x;
    const uint32_t L = P.probs[i].L;
    if (L <= rows_lo || L > rows_hi) return;           // another rows-per-lane class takes this problem
    XlDpp xl;
    gssw_matrix_wave_lane<R>(P, i, threadIdx.x, xl);
}

// The wide route (gssw_wide_device.hpp): one workgroup of four wavefronts per problem; its 256 lanes run ONE skewed wavefront.  Inside a
// wavefront the row above arrives by DPP; lane 0 of wavefronts 1-3 takes it from the three words the last lane of the wavefront before
// left in LDS at the end of the previous step (double-buffered by step parity); one barrier per step keeps the four in step.
template <int K>
__global__ void __launch_bounds__(256) gssw_wide_kernel(const WideParams P) {
    __shared__ int32_t xh[2][4], xf[2][4];
    __shared__ uint32_t xi[2][4];
    const uint32_t i = P.order[P.order_begin + blockIdx.x];
    const WideProb d = P.probs[i];
    const uint32_t lane = threadIdx.x, wv = lane >> 6, wl = lane & 63u;
    uint32_t* tb = (d.flags & VGK_GSSW_TRACEBACK) ? P.tb + d.tb_off : nullptr;
    for (uint32_t strip = 0; strip < d.n_strips; ++strip) {
        WLane<K> s;
        wide_lane_init<K>(s, P, d, strip, lane);
        const uint32_t rows_left = d.L - strip * WIDE_LANES * (uint32_t)K;
        const uint32_t lanes_used = rows_left >= WIDE_LANES * (uint32_t)K ? WIDE_LANES : (rows_left + (uint32_t)K - 1u) / (uint32_t)K;
        const uint32_t n_steps = d.R + lanes_used - 1u;
        if (wl == 63u) { xh[0][wv] = xh[1][wv] = s.out_h; xf[0][wv] = xf[1][wv] = s.out_f; xi[0][wv] = xi[1][wv] = s.info; }      // "no column yet" for the wavefront after this one
        __syncthreads();
        for (uint32_t t = 0; t < n_steps; ++t) {
            int32_t rh = (int32_t)from_lane_above((uint32_t)s.out_h);
            int32_t rf = (int32_t)from_lane_above((uint32_t)s.out_f);
            uint32_t ri = from_lane_above(s.info);
            if (wl == 0 && wv > 0) { const uint32_t b = (t + 1u) & 1u; rh = xh[b][wv - 1]; rf = xf[b][wv - 1]; ri = xi[b][wv - 1]; }
            uint32_t* rec = tb ? tb + (uint64_t)strip * d.strip_dwords + ((uint64_t)t * WIDE_LANES + lane) * (K / 8) : nullptr;
            wide_lane_step<K>(s, P, d, strip, lane, t, rh, rf, ri, rec);
            if (wl == 63u) { const uint32_t b = t & 1u; xh[b][wv] = s.out_h; xf[b][wv] = s.out_f; xi[b][wv] = s.info; }
            __syncthreads();
        }
        unsigned long long key;
        if (wide_lane_best<K>(s, d, lane, key)) atomicMax(&P.best[i], key);
        __threadfence();            // this strip's carry row and saved columns -> the next strip's lanes
        __syncthreads();
    }
}
__global__ void __launch_bounds__(64) gssw_wide_walk_kernel(const WideParams P) {
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k < P.n) wide_walk_one(P, k);
}

class HipBackend final : public Backend {
public:
    int dev = 0; int n_launches = 1; hipStream_t stream = nullptr, copy = nullptr, fetch = nullptr, side[2] = {nullptr, nullptr}; hipEvent_t side_done[2] = {nullptr, nullptr}; hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipStream_t alt = nullptr; hipEvent_t evb[3] = {nullptr, nullptr, nullptr}; float ms_fill_b = 0.f, ms_walk_b = 0.f; bool pending_b = false, timed_walk_b = false, lane1_on_main = true;   // launch lane 1
    hipEvent_t fill_done[2] = {nullptr, nullptr}; bool fill_done_set[2] = {false, false};
    const bool walk_in_fill_order = std::getenv("VGAMD_WALK_PROBLEM_ORDER") == nullptr;
    const bool fills_take_turns = std::getenv("VGAMD_FILLS_TAKE_TURNS") != nullptr;   // experiment: a lane's fill waits for the other lane's fill, so that only a traceback
                                                                                     // runs beside a fill — no faster than one stream (the traceback takes the fill's wave slots); off
    hipDeviceProp_t prop;
    float ms_fill = 0.f, ms_walk = 0.f; bool timed_walk = false, pending = false;
    hipEvent_t sev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}}; bool sev_set[2] = {false, false}; float ms_refill[2] = {0.f, 0.f};      // the speculative fill's second fill (layout + fill), per launch lane
    float ms_gapless = 0.f, ms_wfa = 0.f, ms_xband = 0.f;
    float ms_bfill = 0.f, ms_bwalk = 0.f; hipEvent_t bev[3] = {nullptr, nullptr, nullptr};
    hipEvent_t xbev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};      // run_xdrop_band_async: start / end per slot
    hipEvent_t bbev[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};      // run_banded_async: start / fills done / walk done per slot
    void* scan_tmp = nullptr; size_t scan_tmp_bytes = 0;      // rocPRIM's scratch for scan_u32 (grow-only)
    void* mz_slots = nullptr; size_t mz_slots_bytes = 0;      // per-read seed slots of run_minimizer (grow-only)
    void* banded_slab = nullptr; size_t banded_slab_bytes = 0;      // the block states of the banded fill's HBM-state classes (grow-only)
    ~HipBackend() override {
        hipSetDevice(dev);
        for (auto& e : ev) if (e) hipEventDestroy(e);
        for (auto& e : bev) if (e) hipEventDestroy(e);
        for (auto& pair : xbev) for (auto& e : pair) if (e) hipEventDestroy(e);
        for (auto& trio : bbev) for (auto& e : trio) if (e) hipEventDestroy(e);
        for (auto& pair : sev) for (auto& e : pair) if (e) hipEventDestroy(e);
        if (scan_tmp) hipFree(scan_tmp);
        if (mz_slots) hipFree(mz_slots);
        if (banded_slab) hipFree(banded_slab);
        for (int i = 0; i < 2; ++i) { if (side[i]) hipStreamDestroy(side[i]); if (side_done[i]) hipEventDestroy(side_done[i]); }
        if (stream) hipStreamDestroy(stream);
        if (copy) hipStreamDestroy(copy);
        if (fetch) hipStreamDestroy(fetch);
        if (alt) hipStreamDestroy(alt);
        for (auto& e : evb) if (e) hipEventDestroy(e);
        for (auto& e : fill_done) if (e) hipEventDestroy(e);
    }
    const char* name() const override { return prop.name; }
    int compute_units() const override { return prop.multiProcessorCount; }
    size_t memory_bytes() const override { return prop.totalGlobalMem; }
    void* alloc(size_t bytes) override {
        hipSetDevice(dev);
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return nullptr;
        return p;
    }
    void release(void* p) override { if (p) { hipSetDevice(dev); hipFree(p); } }
    void* host_alloc(size_t bytes) override {
        hipSetDevice(dev);
        void* p = nullptr;
        if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) return nullptr;
        return p;
    }
    void host_release(void* p) override { if (p) { hipSetDevice(dev); hipHostFree(p); } }
    int host_register(const void* p, size_t bytes) override { hipSetDevice(dev); return hipHostRegister(const_cast<void*>(p), bytes, hipHostRegisterDefault) == hipSuccess ? VGK_OK : VGK_EINVAL; }
    int host_unregister(const void* p) override { hipSetDevice(dev); return hipHostUnregister(const_cast<void*>(p)) == hipSuccess ? VGK_OK : VGK_EINVAL; }
    int upload(void* dst, const void* src, size_t bytes) override {
        hipSetDevice(dev);
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int upload_side(void* dst, const void* src, size_t bytes) override {
        hipSetDevice(dev);
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, copy) == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    void* event_create() override {
        hipSetDevice(dev);
        hipEvent_t e = nullptr;
        return hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess ? (void*)e : nullptr;
    }
    void event_destroy(void* ev) override { if (ev) { hipSetDevice(dev); hipEventDestroy((hipEvent_t)ev); } }
    int event_record(void* ev) override {
        if (!ev) return VGK_OK;
        hipSetDevice(dev);
        return hipEventRecord((hipEvent_t)ev, stream) == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    bool event_done(void* ev) override {
        if (!ev) return false;
        hipSetDevice(dev);
        const hipError_t e = hipEventQuery((hipEvent_t)ev);
        if (e != hipSuccess && e != hipErrorNotReady) (void)hipGetLastError();
        return e == hipSuccess;
    }
    int event_wait(void* ev) override {
        if (!ev) return sync();
        hipSetDevice(dev);
        for (;;) {
            const hipError_t e = hipEventQuery((hipEvent_t)ev);
            if (e == hipSuccess) return VGK_OK;
            if (e != hipErrorNotReady) { (void)hipGetLastError(); return VGK_ENODEV; }
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
    }
    int fetch_after(void* ev) override {
        if (!ev) return VGK_OK;
        hipSetDevice(dev);
        return hipStreamWaitEvent(fetch, (hipEvent_t)ev, 0) == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int sync_fetch() override {
        hipSetDevice(dev);
        return hipStreamSynchronize(fetch) == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int download_fetch(void* dst, const void* src, size_t bytes) override {
        hipSetDevice(dev);
        if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, fetch) != hipSuccess) return VGK_ENODEV;
        return hipStreamSynchronize(fetch) == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int download_fetch_async(void* dst, const void* src, size_t bytes) override {
        hipSetDevice(dev);
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, fetch) == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    hipEvent_t side_mark = nullptr;
    int main_after_side() override {
        hipSetDevice(dev);
        if (!side_mark && hipEventCreateWithFlags(&side_mark, hipEventDisableTiming) != hipSuccess) return VGK_ENODEV;
        if (hipEventRecord(side_mark, copy) != hipSuccess || hipStreamWaitEvent(stream, side_mark, 0) != hipSuccess) return VGK_ENODEV;
        return VGK_OK;
    }
    int sync_side() override {
        hipSetDevice(dev);
        return hipStreamSynchronize(copy) == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int device_index() const override { return dev; }
    int download(void* dst, const void* src, size_t bytes) override {
        hipSetDevice(dev);
        if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) != hipSuccess) return VGK_ENODEV;
        return hipStreamSynchronize(stream) == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int zero(void* dst, size_t bytes) override {
        hipSetDevice(dev);
        if (bytes >= ((size_t)1 << 18) && ((uintptr_t)dst & 15u) == 0) {
            const size_t vecs = bytes / 16;
            const unsigned blocks = (unsigned)std::min<size_t>((vecs + 255) / 256, (size_t)std::max(1, prop.multiProcessorCount) * 8);
            hipLaunchKernelGGL(zero_kernel, dim3(blocks), dim3(256), 0, stream, (uint4*)dst, vecs, (unsigned char*)dst + vecs * 16, (uint32_t)(bytes - vecs * 16));
            return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
        }
        return hipMemsetAsync(dst, 0, bytes, stream) == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int sync() override {
        hipSetDevice(dev);
        return hipStreamSynchronize(stream) == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    size_t win_tmp_bytes(uint32_t n, uint32_t n_waves_cap) override { hipSetDevice(dev); return hip_win_tmp_bytes(n, n_waves_cap); }
    int win_stage1(const WinParams& P, void* tmp, size_t tmp_bytes) override { hipSetDevice(dev); return hip_win_stage1(P, tmp, tmp_bytes, copy); }
    int win_stage2(const WinParams& P, void* tmp, size_t tmp_bytes) override { hipSetDevice(dev); return hip_win_stage2(P, tmp, tmp_bytes, copy); }
    int download_side(void* dst, const void* src, size_t bytes) override {
        hipSetDevice(dev);
        if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, copy) != hipSuccess) return VGK_ENODEV;
        return hipStreamSynchronize(copy) == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int fill_side(void* dst, int byte, size_t bytes) override {
        hipSetDevice(dev);
        return hipMemsetAsync(dst, byte, bytes, copy) == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    // whether a speculative batch's second fill runs the kernels of its own (NOKEY: codes only, reads begun at their col0, and — GsswParams::refill_walk —
    // the walks of its reads): the x8 scale on stored codes; unscaled scorings, TB_REWALK and `fused` batches run it through the plain kernels
    static bool refill_own_kernel(const GsswParams& p) { return p.spec_fill == 2 && p.scale == 8 && p.tb_mode != TB_REWALK && !p.fused; }
    template <int K> int launch_fill_k(const GsswParams& p, hipStream_t stream) {
        const dim3 grid((p.wave_count + 3) / 4), block(256);
        const bool s8 = p.scale == 8, re = p.tb_mode == TB_REWALK;
        if (p.spec_fill == 1) {                                      // the first fill of a speculative batch: no codes
            if (s8 && p.key3 && p.row_off) hipLaunchKernelGGL((gssw_fill_kernel<K, true, false, false, true, false, true>), grid, block, 0, stream, p);
            else if (s8 && p.key3) hipLaunchKernelGGL((gssw_fill_kernel<K, true, false, false, true>), grid, block, 0, stream, p);
            else if (s8) hipLaunchKernelGGL((gssw_fill_kernel<K, true, false, false>), grid, block, 0, stream, p); else hipLaunchKernelGGL((gssw_fill_kernel<K, false, false, false>), grid, block, 0, stream, p);
            return VGK_OK;
        }
        if (refill_own_kernel(p)) { hipLaunchKernelGGL((gssw_fill_kernel<K, true, false, true, false, true>), grid, block, 0, stream, p); return VGK_OK; }      // (codes only: the end cells are the first fill's)
        if (re) { if (s8) hipLaunchKernelGGL((gssw_fill_kernel<K, true, true>), grid, block, 0, stream, p); else hipLaunchKernelGGL((gssw_fill_kernel<K, false, true>), grid, block, 0, stream, p); }
        else    { if (s8) hipLaunchKernelGGL((gssw_fill_kernel<K, true, false>), grid, block, 0, stream, p); else hipLaunchKernelGGL((gssw_fill_kernel<K, false, false>), grid, block, 0, stream, p); }
        return VGK_OK;
    }
    int launch_fill(const GsswParams& p, hipStream_t stream) {
        switch (p.K) {
            case 16: return launch_fill_k<16>(p, stream);
            case 19: return launch_fill_k<19>(p, stream);
            case 20: return launch_fill_k<20>(p, stream);
            case 24: return launch_fill_k<24>(p, stream);
            default: return VGK_EINVAL;
        }
    }
    // the recomputing tracebacks of one fill launch's reads (p.K / wave_begin / wave_count as for the fill); the grid covers every pair
    // of the batch (the launch's own count is a device-side fact for batches packed there): blocks beyond its reads leave at once
    template <int K> void launch_rewalk_k(const GsswParams& p, hipStream_t stream) {
        const dim3 grid(1024), block(64);                   // (the reads that left their band: a list in HBM whose length only the device knows; each lane takes every 65536th)
        if (p.scale == 8) hipLaunchKernelGGL((gssw_rewalk_kernel<K, true>), grid, block, 0, stream, p); else hipLaunchKernelGGL((gssw_rewalk_kernel<K, false>), grid, block, 0, stream, p);
    }
    template <int K> void launch_band_k(const GsswParams& p, hipStream_t stream) {
        const dim3 grid((p.wave_count + 3) / 4), block(256);
        if (p.scale == 8) hipLaunchKernelGGL((gssw_band_kernel<K, true>), grid, block, 0, stream, p); else hipLaunchKernelGGL((gssw_band_kernel<K, false>), grid, block, 0, stream, p);
    }
    void launch_walk(const GsswParams& p0, const FillLaunch* launches, uint32_t n, hipStream_t stream, int lane = 0) {
        sev_set[lane] = false;
        if (p0.tb_mode != TB_REWALK) {
            if (p0.walk_passes == 2) {
                hipLaunchKernelGGL(gssw_walk_first_kernel, dim3((2 * p0.n_pairs + 63) / 64), dim3(64), 0, stream, p0, walk_in_fill_order ? 1 : 0);
                if (p0.spec_fill) {
                    // the reads the first kernel left: wavefronts of their own, filled again with codes (their number is a device-side fact:
                    // the grids cover the most there can be, what lies beyond leaves at once)
                    const uint32_t max_waves = (p0.n_pairs + 64u / p0.refill_G - 1u) / (64u / p0.refill_G);
                    for (int k = 0; k < 2; ++k) if (!sev[lane][k]) hipEventCreate(&sev[lane][k]);
                    hipEventRecord(sev[lane][0], stream);
                    const uint32_t per_block = 4u * (64u / refill_layout_group(p0.refill_G));      // second-fill wavefronts a block of the layout lays out
                    hipLaunchKernelGGL(gssw_refill_layout_kernel, dim3((max_waves + per_block - 1u) / per_block), dim3(256), 0, stream, p0);
                    GsswParams p = p0;
                    p.spec_fill = 2; p.K = p0.refill_K; p.wave_begin = p0.refill_wave0; p.wave_count = max_waves; p.wave_limit = p0.refill_count;
                    launch_fill(p, stream);
                    hipEventRecord(sev[lane][1], stream); sev_set[lane] = true;
                    if (refill_own_kernel(p) && p.refill_walk) return;      // (its wavefronts have walked their reads)
                }
                hipLaunchKernelGGL(gssw_walk_missed_kernel, dim3((p0.n_problems + 255) / 256), dim3(256), 0, stream, p0);      // (lanes beyond the list's end leave at once)
            } else hipLaunchKernelGGL(gssw_walk_kernel, dim3((2 * p0.n_pairs + 255) / 256), dim3(256), 0, stream, p0, walk_in_fill_order ? 1 : 0);
            return;
        }
        GsswParams p = p0;
        for (uint32_t i = 0; i < n; ++i) {                              // the band records of every fill launch's wavefronts
            if (!launches[i].wave_count) continue;
            p.K = launches[i].K; p.wave_begin = launches[i].wave_begin; p.wave_count = launches[i].wave_count;
            switch (p.K) { case 16: launch_band_k<16>(p, stream); break; case 19: launch_band_k<19>(p, stream); break; case 20: launch_band_k<20>(p, stream); break; case 24: launch_band_k<24>(p, stream); break; default: break; }
        }
        hipLaunchKernelGGL(gssw_bandwalk_kernel, dim3((2 * p0.n_pairs + 255) / 256), dim3(256), 0, stream, p0);
        for (uint32_t i = 0; i < n; ++i) {                              // what left its band
            if (!launches[i].wave_count) continue;
            p.K = launches[i].K; p.wave_begin = launches[i].wave_begin; p.wave_count = launches[i].wave_count;
            switch (p.K) { case 16: launch_rewalk_k<16>(p, stream); break; case 19: launch_rewalk_k<19>(p, stream); break; case 20: launch_rewalk_k<20>(p, stream); break; case 24: launch_rewalk_k<24>(p, stream); break; default: break; }
        }
    }
    // One fill launch per rows-per-lane instantiation K (lanes-per-pair G is a per-wavefront value), then one traceback launch over all
    // reads.  (Running walk(c) under fill(c+1) on a second stream, and fusing the walk into the fill kernel,
    // were both measured slower than this plain sequence on MI355X — DESIGN.md §5; `fused` is kept as an option.  That was the whole-batch fill; the
    // second fill of a speculative batch walking its own reads, GsswParams::refill_walk, was measured on its own and is slower too: DESIGN.md §3a.)
    int run_gssw(const GsswParams& p0, const FillLaunch* launches, uint32_t n, bool walk) override {
        hipSetDevice(dev);
        n_launches = n ? (int)n : 1;
        if (p0.n_problems == 0 || n == 0) { ms_fill = ms_walk = 0; pending = false; return VGK_OK; }
        GsswParams p = p0;
        if (p0.restore_probs) hipLaunchKernelGGL(gssw_refill_restore_kernel, dim3((p0.n_problems + 255) / 256), dim3(256), 0, stream, p0);
        if (fills_take_turns && fill_done_set[1]) hipStreamWaitEvent(stream, fill_done[1], 0);       // (measured: DESIGN.md §5)
        hipEventRecord(ev[0], stream);
        // the (up to three) rows-per-lane instantiations are independent: side streams let a small bucket's
        // launch fill the CUs another bucket leaves idle; everything joins `stream` again before the walk
        for (uint32_t i = 0; i < n; ++i) {
            const FillLaunch& L = launches[i];
            p.K = L.K; p.wave_begin = L.wave_begin; p.wave_count = L.wave_count;
            if (L.wave_count == 0) continue;
            hipStream_t st = (i == 0 || i > 2) ? stream : side[i - 1];
            if (st != stream) hipStreamWaitEvent(st, ev[0], 0);
            int rc = launch_fill(p, st);
            if (rc) return rc;
            if (st != stream) { hipEventRecord(side_done[i - 1], st); hipStreamWaitEvent(stream, side_done[i - 1], 0); }
        }
        hipEventRecord(ev[1], stream);
        hipEventRecord(fill_done[0], stream); fill_done_set[0] = true;
        timed_walk = walk && (!p.fused || p.tb_mode == TB_REWALK);
        if (timed_walk) {
            launch_walk(p0, launches, n, stream);
            hipEventRecord(ev[2], stream);
        }
        pending = true;
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    // lane 1: a second launch stream with timing events of its own, for batches with a single fill launch (several rows-per-lane
    // launches share the side streams and stay on lane 0)
    int run_gssw_on(int lane, const GsswParams& p0, const FillLaunch* launches, uint32_t n, bool walk, void* done) override {
        hipSetDevice(dev);
        if (lane != 1 || n != 1 || p0.n_problems == 0) {
            if (lane == 1) lane1_on_main = true;
            if (hipMemsetAsync(p0.best, 0, ((size_t)p0.n_problems + 1) * sizeof(unsigned long long), stream) != hipSuccess) return VGK_ENODEV;
            int rc = run_gssw(p0, launches, n, walk);
            if (!rc && done) rc = hipEventRecord((hipEvent_t)done, stream) == hipSuccess ? VGK_OK : VGK_ENODEV;
            return rc;
        }
        lane1_on_main = false;
        if (hipMemsetAsync(p0.best, 0, ((size_t)p0.n_problems + 1) * sizeof(unsigned long long), alt) != hipSuccess) return VGK_ENODEV;
        GsswParams p = p0;
        p.K = launches[0].K; p.wave_begin = launches[0].wave_begin; p.wave_count = launches[0].wave_count;
        if (p0.restore_probs) hipLaunchKernelGGL(gssw_refill_restore_kernel, dim3((p0.n_problems + 255) / 256), dim3(256), 0, alt, p0);
        if (fills_take_turns && fill_done_set[0]) hipStreamWaitEvent(alt, fill_done[0], 0);
        hipEventRecord(evb[0], alt);
        if (p.wave_count) { const int rc = launch_fill(p, alt); if (rc) return rc; }
        hipEventRecord(evb[1], alt);
        hipEventRecord(fill_done[1], alt); fill_done_set[1] = true;
        timed_walk_b = walk && (!p.fused || p.tb_mode == TB_REWALK);
        if (timed_walk_b) {
            launch_walk(p0, launches, n, alt, 1);
            hipEventRecord(evb[2], alt);
        }
        pending_b = true;
        if (done && hipEventRecord((hipEvent_t)done, alt) != hipSuccess) return VGK_ENODEV;
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    double last_ms_on(int lane, int which) const override {
        if (which == 12) {                                           // the second fill of a speculative batch (0 when the last run had none)
            const int l = (lane == 1 && !lane1_on_main) ? 1 : 0;
            HipBackend* self = const_cast<HipBackend*>(this);
            if (!sev_set[l]) return 0.0;
            hipSetDevice(dev); hipStreamSynchronize(l ? alt : stream);
            float ms = 0.f; if (hipEventElapsedTime(&ms, sev[l][0], sev[l][1]) != hipSuccess) { (void)hipGetLastError(); ms = 0.f; }
            self->ms_refill[l] = ms; return ms;
        }
        if (lane != 1 || lane1_on_main || which > 2 || which < 0) return last_ms(which);
        HipBackend* self = const_cast<HipBackend*>(this);
        if (self->pending_b) {
            hipSetDevice(dev);
            hipStreamSynchronize(alt);
            hipEventElapsedTime(&self->ms_fill_b, evb[0], evb[1]);
            self->ms_walk_b = 0.f;
            if (timed_walk_b) hipEventElapsedTime(&self->ms_walk_b, evb[1], evb[2]);
            self->pending_b = false;
        }
        return which == 0 ? ms_fill_b : which == 1 ? ms_walk_b : 1.0;
    }
    int ops_offsets(const vgk_result* res, uint32_t n, uint32_t* offs, uint32_t* sums, uint64_t* total) override {
        hipSetDevice(dev);
        const uint32_t blocks = (n + OPS_SCAN_BLOCK - 1) / OPS_SCAN_BLOCK;
        unsigned long long* total_dev = (unsigned long long*)(sums + ((blocks + 2) & ~1u));       // 8-byte aligned, behind the block sums
        hipLaunchKernelGGL(ops_scan_kernel, dim3(blocks), dim3(256), 0, fetch, res, n, offs, sums);
        hipLaunchKernelGGL(ops_sums_kernel, dim3(1), dim3(256), 0, fetch, sums, blocks, total_dev);
        unsigned long long t = 0;
        if (hipMemcpyAsync(&t, total_dev, sizeof t, hipMemcpyDeviceToHost, fetch) != hipSuccess) return VGK_ENODEV;
        if (hipStreamSynchronize(fetch) != hipSuccess || hipGetLastError() != hipSuccess) return VGK_ENODEV;
        *total = t;
        return VGK_OK;
    }
    int ops_gather(const vgk_result* res, const vgk_op* ops, uint32_t n, const uint32_t* offs, const uint32_t* sums, vgk_result* out_res, vgk_op* out_ops) override {
        hipSetDevice(dev);
        hipLaunchKernelGGL(ops_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, fetch, res, ops, n, offs, sums, out_res, out_ops);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int run_banded(const BandedParams& p, const BandedLaunch* launches, uint32_t n) override {
        ms_bfill = ms_bwalk = 0.f;
        if (p.n == 0) return VGK_OK;
        const int rc = banded_launch(p, launches, n, bev);
        if (rc != VGK_OK) return rc;
        if (hipStreamSynchronize(stream) != hipSuccess || hipGetLastError() != hipSuccess) return VGK_ENODEV;
        hipEventElapsedTime(&ms_bfill, bev[0], bev[1]);
        hipEventElapsedTime(&ms_bwalk, bev[1], bev[2]);
        return VGK_OK;
    }
    int run_banded_async(const BandedParams& p, const BandedLaunch* launches, uint32_t n, int slot) override {
        if (p.n == 0) return VGK_OK;
        hipSetDevice(dev);
        hipEvent_t* ev = bbev[slot & 1];
        for (int k = 0; k < 3; ++k) if (!ev[k] && hipEventCreate(&ev[k]) != hipSuccess) return VGK_ENODEV;
        return banded_launch(p, launches, n, ev);
    }
    int run_banded_geometry(const BGeomParams& p) override {
        if (p.n == 0) return VGK_OK;
        hipSetDevice(dev);
        hipLaunchKernelGGL(banded_geometry_kernel, dim3((p.n + 63) / 64), dim3(64), 0, copy, p);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    double banded_ms(int slot, int which) override {
        hipEvent_t* ev = bbev[slot & 1]; float ms = 0.f;
        if (!ev[0] || hipEventElapsedTime(&ms, ev[which ? 1 : 0], ev[which ? 2 : 1]) != hipSuccess) { (void)hipGetLastError(); return 0.0; }
        return ms;
    }
    int banded_launch(const BandedParams& p, const BandedLaunch* launches, uint32_t n, hipEvent_t* bev) {
        hipSetDevice(dev);
        hipEventRecord(bev[0], stream);
        // the rows-per-lane classes are independent: the small ones run on the side streams under the big one
        for (uint32_t i = 0; i < n; ++i) {
            const BandedLaunch& L = launches[i];
            if (!L.count) continue;
            hipStream_t st = (i == 0 || i > 2 || L.R >= 64) ? stream : side[i - 1];      // (the HBM-state classes share one slab: one after the other on the main stream)
            if (st != stream) hipStreamWaitEvent(st, bev[0], 0);
            switch (L.R) {
                case 1:  launch_banded_fill<1>(p, L, st); break;
                case 2:  launch_banded_fill<2>(p, L, st); break;
                case 4:  launch_banded_fill<4>(p, L, st); break;
                case 8:  launch_banded_fill<8>(p, L, st); break;
                case 16: launch_banded_fill_blocks<2>(p, L, st); break;      // bands of more than 512 diagonals: blocks of 8 rows per lane (banded_fill_lane_blocks)
                case 32: launch_banded_fill_blocks<4>(p, L, st); break;
                case 64: case 128: case 256: case 512: {                     // 8 ... 64 blocks: their state in HBM (grow-only slab, one stretch per problem of the launch)
                    const uint32_t nb = L.R / 8u;
                    const size_t need = (size_t)L.count * ((size_t)nb * 3u * 8u + 3u * ((size_t)nb + 1u)) * 64u * sizeof(int32_t);
                    if (need > banded_slab_bytes) {
                        hipStreamSynchronize(stream); for (hipStream_t x : side) hipStreamSynchronize(x);
                        if (banded_slab) hipFree(banded_slab);
                        banded_slab = nullptr; banded_slab_bytes = 0;
                        if (hipMalloc(&banded_slab, need + need / 4) != hipSuccess) return VGK_ENOMEM;
                        banded_slab_bytes = need + need / 4;
                    }
                    if (p.quals) hipLaunchKernelGGL(banded_fill_blocks_any_kernel<true>, dim3(L.count), dim3(64), 0, stream, p, L.begin, nb, (int32_t*)banded_slab);
                    else         hipLaunchKernelGGL(banded_fill_blocks_any_kernel<false>, dim3(L.count), dim3(64), 0, stream, p, L.begin, nb, (int32_t*)banded_slab);
                    break; }
                default: return VGK_EINVAL;
            }
            if (st != stream) { hipEventRecord(side_done[i - 1], st); hipStreamWaitEvent(stream, side_done[i - 1], 0); }
        }
        hipEventRecord(bev[1], stream);
        if (!p.scores) hipLaunchKernelGGL(banded_walk_kernel, dim3((p.n + 63) / 64), dim3(64), 0, stream, p);      // k-best mode: the host walks the score matrices
        hipEventRecord(bev[2], stream);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    template <bool MG> void launch_gapless(const GaplessParams& p, uint32_t threads) {
        if (std::getenv("VGAMD_GAPLESS_SLAB_ONLY")) { hipLaunchKernelGGL(gapless_kernel<MG>, dim3((threads + 63) / 64), dim3(64), 0, stream, p, threads, 0); return; }
        hipLaunchKernelGGL(gapless_search_kernel<MG>, dim3((threads + 63) / 64), dim3(64), 0, stream, p, threads);
        // the rules over the searched reads and the slab kernel over the few G_RETRY reads touch different reads (the rules skip
        // G_RETRY, the slab kernel everything else; both take output space from the same atomic counters): side by side
        hipEventRecord(side_done[0], stream);
        hipStreamWaitEvent(side[0], side_done[0], 0);
        hipLaunchKernelGGL(gapless_kernel<MG>, dim3((threads + 63) / 64), dim3(64), 0, side[0], p, threads, 1);
        hipEventRecord(side_done[1], side[0]);
        hipLaunchKernelGGL(gapless_rules_kernel<MG>, dim3((p.n + 63) / 64), dim3(64), 0, stream, p);
        hipStreamWaitEvent(stream, side_done[1], 0);
    }
    int run_gapless(const GaplessParams& p, uint32_t threads) override {
        hipSetDevice(dev);
        ms_gapless = 0.f;
        if (!p.n || !threads) return VGK_OK;
        hipEventRecord(bev[0], stream);
        if (p.merge.on) launch_gapless<true>(p, threads); else launch_gapless<false>(p, threads);      // (the kernels without the merged-run code keep the plain search's registers)
        hipEventRecord(bev[1], stream);
        if (hipStreamSynchronize(stream) != hipSuccess || hipGetLastError() != hipSuccess) return VGK_ENODEV;
        hipEventElapsedTime(&ms_gapless, bev[0], bev[1]);
        return VGK_OK;
    }
    int run_gssw_matrix(const GsswMatrixParams& p) override {
        hipSetDevice(dev);
        if (!p.n) return VGK_OK;
        if (p.go < p.ge || std::getenv("VGAMD_MATRIX_THREADS")) hipLaunchKernelGGL(gssw_matrix_kernel, dim3((p.n + 63) / 64), dim3(64), 0, stream, p);
        else {      // one launch per rows-per-lane class; a wavefront whose problem belongs to another class returns at once
            hipLaunchKernelGGL((gssw_matrix_wave_kernel<2>), dim3(p.n), dim3(64), 0, stream, p, 0u, 128u);
            hipLaunchKernelGGL((gssw_matrix_wave_kernel<4>), dim3(p.n), dim3(64), 0, stream, p, 128u, 256u);
            hipLaunchKernelGGL((gssw_matrix_wave_kernel<8>), dim3(p.n), dim3(64), 0, stream, p, 256u, 512u);
            hipLaunchKernelGGL((gssw_matrix_wave_kernel<16>), dim3(p.n), dim3(64), 0, stream, p, 512u, 1024u);
        }
        if (hipStreamSynchronize(stream) != hipSuccess || hipGetLastError() != hipSuccess) return VGK_ENODEV;
        return VGK_OK;
    }
    int run_banded_multi(const BandedMultiParams& q) override {
        hipSetDevice(dev);
        if (!q.P.n) return VGK_OK;
        hipLaunchKernelGGL(banded_multi_kernel, dim3((q.P.n + 63) / 64), dim3(64), 0, stream, q);
        if (hipStreamSynchronize(stream) != hipSuccess || hipGetLastError() != hipSuccess) return VGK_ENODEV;
        return VGK_OK;
    }
    int run_gssw_multi(const GsswMultiParams& p) override {
        hipSetDevice(dev);
        if (!p.M.n) return VGK_OK;
        hipLaunchKernelGGL(gssw_multi_kernel, dim3((p.M.n + 63) / 64), dim3(64), 0, stream, p);
        if (hipStreamSynchronize(stream) != hipSuccess || hipGetLastError() != hipSuccess) return VGK_ENODEV;
        return VGK_OK;
    }
    int run_gssw_wide(const WideParams& p0, uint32_t n8, uint32_t n16) override {
        hipSetDevice(dev);
        if (!p0.n) return VGK_OK;
        WideParams p = p0;
        for (int k = 0; k < 3; ++k) if (!wev[k]) hipEventCreate(&wev[k]);
        hipEventRecord(wev[0], stream);
        if (n8) { p.order_begin = 0; p.order_count = n8; hipLaunchKernelGGL(gssw_wide_kernel<8>, dim3(n8), dim3(256), 0, stream, p); }
        if (n16) { p.order_begin = n8; p.order_count = n16; hipLaunchKernelGGL(gssw_wide_kernel<16>, dim3(n16), dim3(256), 0, stream, p); }
        hipEventRecord(wev[1], stream);
        hipLaunchKernelGGL(gssw_wide_walk_kernel, dim3((p.n + 63) / 64), dim3(64), 0, stream, p);
        hipEventRecord(wev[2], stream); wide_pending = true;
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int run_wide_windows(const WideWinParams& p, int what) override { hipSetDevice(dev); return hip_wide_windows(p, what, (uint32_t)std::max(1, prop.multiProcessorCount), stream); }
    int run_xdrop_band(const GsswMatrixParams& p) override {
        ms_xband = 0.f;
        if (!p.n) return VGK_OK;
        const int rc = run_xdrop_band_async(p, 0);
        if (rc != VGK_OK) return rc;
        if (hipStreamSynchronize(stream) != hipSuccess || hipGetLastError() != hipSuccess) return VGK_ENODEV;
        ms_xband = (float)xdrop_band_ms(0);
        return VGK_OK;
    }
    double xdrop_band_ms(int slot) override {
        float ms = 0.f;
        if (!xbev[slot & 1][0] || hipEventElapsedTime(&ms, xbev[slot & 1][0], xbev[slot & 1][1]) != hipSuccess) { (void)hipGetLastError(); return 0.0; }
        return ms;
    }
    int run_xdrop_band_async(const GsswMatrixParams& p, int slot) override {
        hipSetDevice(dev);
        if (!p.n) return VGK_OK;
        hipEvent_t* ev = xbev[slot & 1];
        for (int k = 0; k < 2; ++k) if (!ev[k] && hipEventCreate(&ev[k]) != hipSuccess) return VGK_ENODEV;
        hipEventRecord(ev[0], stream);
        auto launch = [&](auto cell) {
            using CT = decltype(cell);
            if (p.xb_order) {
                if (p.xb_n16) hipLaunchKernelGGL(xdrop_band_kernel16<CT>, dim3((p.xb_n16 + 3) / 4), dim3(64), 0, stream, p);
                if (p.xb_n64) hipLaunchKernelGGL(xdrop_band_kernel<CT>, dim3(p.xb_n64), dim3(64), 0, stream, p);
            } else hipLaunchKernelGGL(xdrop_band_kernel<CT>, dim3(p.n), dim3(64), 0, stream, p);
            if (p.xb_results) hipLaunchKernelGGL(xdrop_band_walk_kernel<CT>, dim3((p.n + 63) / 64), dim3(64), 0, stream, p);
        };
        if (p.xb_cell16 == 2) {
            if (p.xb_order) {
                if (p.xb_n8) hipLaunchKernelGGL(xdrop_band_pk_kernel8, dim3((p.xb_n8 + 7) / 8), dim3(64), 0, stream, p);
                if (p.xb_n16) hipLaunchKernelGGL(xdrop_band_pk_kernel16, dim3((p.xb_n16 + 3) / 4), dim3(64), 0, stream, p);
                if (p.xb_n64) hipLaunchKernelGGL(xdrop_band_pk_kernel, dim3(p.xb_n64), dim3(64), 0, stream, p);
            } else hipLaunchKernelGGL(xdrop_band_pk_kernel, dim3(p.n), dim3(64), 0, stream, p);
            if (p.xb_results) hipLaunchKernelGGL(xdrop_band_walk_kernel<uint16_t>, dim3((p.n + 63) / 64), dim3(64), 0, stream, p);
        } else if (p.xb_cell16) launch(int16_t{}); else launch(int32_t{});
        hipEventRecord(ev[1], stream);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int gapless_order(const GOrderParams& p, int stage) override {
        hipSetDevice(dev);
        if (!p.n) return VGK_OK;
        hipLaunchKernelGGL(gapless_order_kernel, dim3((p.n + 255) / 256), dim3(256), 0, stream, p, stage);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int gapless_seeded(const GSeededParams& p) override {
        hipSetDevice(dev);
        if (!p.n) return VGK_OK;
        hipLaunchKernelGGL(gapless_seeded_kernel, dim3((p.n + 255) / 256), dim3(256), 0, stream, p);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int sort_pairs_u32(const uint32_t* kin, uint32_t* kout, const uint32_t* vin, uint32_t* vout, uint32_t n, int bits) override {
        hipSetDevice(dev);
        if (!n) return VGK_OK;
        const size_t need = hip_sort_tmp_bytes(n);
        if (need > scan_tmp_bytes) {
            if (scan_tmp) { hipStreamSynchronize(stream); hipFree(scan_tmp); scan_tmp = nullptr; scan_tmp_bytes = 0; }
            if (hipMalloc(&scan_tmp, need + need / 4) != hipSuccess) return VGK_ENOMEM;
            scan_tmp_bytes = need + need / 4;
        }
        return hip_sort_pairs_u32(kin, kout, vin, vout, n, bits, scan_tmp, scan_tmp_bytes, stream);
    }
    int mask_reads(char* reads, size_t bytes) override {
        hipSetDevice(dev);
        if (!bytes) return VGK_OK;
        hipLaunchKernelGGL(mask_reads_kernel, dim3((unsigned)((bytes + 4095) / 4096)), dim3(256), 0, stream, reads, bytes);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int run_minimizer(const MinimizerParams& p) override {
        hipSetDevice(dev);
        if (!p.n) return VGK_OK;
        const size_t need = sizeof(vgk_seed) * (size_t)p.n * MZ_MAX_SEEDS;       // a slot of MZ_MAX_SEEDS seeds per read between the two launches
        if (need > mz_slots_bytes) {
            if (mz_slots) { hipStreamSynchronize(stream); hipFree(mz_slots); mz_slots = nullptr; mz_slots_bytes = 0; }
            if (hipMalloc(&mz_slots, need + need / 8) != hipSuccess) return VGK_ENOMEM;
            mz_slots_bytes = need + need / 8;
        }
        if (p.pass == 1) { if (p.hi > p.lo) hipLaunchKernelGGL(minimizer_kernel, dim3((p.hi - p.lo + 3) / 4), dim3(256), 0, stream, p, (vgk_seed*)mz_slots); }
        else hipLaunchKernelGGL(minimizer_gather_kernel, dim3((p.n + 3) / 4), dim3(256), 0, stream, p, (const vgk_seed*)mz_slots);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int run_tail_stage(const TStageParams& p, int what) override {
        hipSetDevice(dev);
        const uint32_t items = tstage_items(p, what);
        if (!items) return VGK_OK;
        hipLaunchKernelGGL(tail_stage_kernel, dim3((items + 255) / 256), dim3(256), 0, stream, p, what, items);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int run_minimizer_list(const MzListParams& p) override {
        hipSetDevice(dev);
        hipLaunchKernelGGL(minimizer_list_kernel, dim3((p.n + 64) / 64), dim3(64), 0, stream, p);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int run_minimizer_seeds_of(const MzSeedsOfParams& p) override {
        hipSetDevice(dev);
        hipLaunchKernelGGL(minimizer_seeds_of_kernel, dim3((p.n + 256) / 256), dim3(256), 0, stream, p);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    // one launch of a launch_split.hpp pair, wavefronts of 64 lanes: the kernel whose working set lies in LDS (lds_bytes of it dynamic), or its slab twin
    template <class P> int launch_lds_or_slab(void (*lds_kernel)(const P), void (*slab_kernel)(const P), bool slab, uint32_t grid, uint32_t lds_bytes, const P& p) {
        if (slab) hipLaunchKernelGGL(slab_kernel, dim3(grid), dim3(64), 0, stream, p);
        else hipLaunchKernelGGL(lds_kernel, dim3(grid), dim3(64), lds_bytes, stream, p);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int run_chain_items(const CiParams& p, int what, uint32_t blocks) override {
        hipSetDevice(dev);
        if (what == CI_RUN_LEGAL || what == CI_RUN_SCATTER) {
            if (!p.n_cands) return VGK_OK;
            const dim3 grid((uint32_t)((p.n_cands + 255) / 256));
            if (what == CI_RUN_LEGAL) hipLaunchKernelGGL(chain_items_legal_kernel, grid, dim3(256), 0, stream, p);
            else hipLaunchKernelGGL(chain_items_scatter_kernel, grid, dim3(256), 0, stream, p);
        } else {
            if (!blocks) return VGK_OK;
            if (!p.slab && (p.lds_np > CI_LDS_MAX || (p.lds_np & (p.lds_np - 1u)))) return VGK_EINVAL;
            if (what == CI_RUN_DP) return launch_lds_or_slab(chain_items_dp_kernel, chain_items_dp_slab_kernel, p.slab, blocks, ci_dp_lds_bytes(p.lds_np), p);
            if (what == CI_RUN_TRACE) return launch_lds_or_slab(chain_items_trace_kernel, chain_items_trace_slab_kernel, p.slab, blocks, ci_trace_lds_bytes(p.lds_np), p);
            return VGK_EINVAL;
        }
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int run_extension_anchors(const EaParams& p, int what, uint32_t blocks) override {
        hipSetDevice(dev);
        if (what == EA_RUN_SEEDS) {
            if (!p.n_seeds) return VGK_OK;
            hipLaunchKernelGGL(extension_anchors_seeds_kernel, dim3((uint32_t)((p.n_seeds + 255) / 256)), dim3(256), 0, stream, p);
        } else if (what == EA_RUN_COUNT || what == EA_RUN_EMIT) {
            if (!p.n_ext) return VGK_OK;
            hipLaunchKernelGGL(extension_anchors_lists_kernel, dim3((uint32_t)((p.n_ext + 255) / 256)), dim3(256), 0, stream, p, what == EA_RUN_EMIT ? 1 : 0);
        } else if (what == EA_RUN_SORT || what == EA_RUN_ANCHORS) {
            if (!blocks) return VGK_OK;
            if (!p.slab && (p.lds_np > std::max(EA_LDS_SEEDS, EA_LDS_EXT) || (p.lds_np & (p.lds_np - 1u)))) return VGK_EINVAL;
            const uint32_t lds = (uint32_t)ea_work_bytes(p.lds_np, EA_LDS_SEEDS);
            if (what == EA_RUN_SORT) return launch_lds_or_slab(extension_anchors_sort_kernel, extension_anchors_sort_slab_kernel, p.slab, blocks, lds, p);
            return launch_lds_or_slab(extension_anchors_kernel, extension_anchors_slab_kernel, p.slab, blocks, lds, p);
        } else return VGK_EINVAL;
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int run_read_alignments(const RaParams& p, int what) override {
        hipSetDevice(dev);
        if (what == RA_RUN_SELECT) {
            if (!p.n) return VGK_OK;
            return launch_lds_or_slab(read_alignments_select_kernel, read_alignments_select_slab_kernel, p.work && p.ids, (p.n + 63) / 64, 0, p);
        } else if (what == RA_RUN_COUNT || what == RA_RUN_EMIT || what == RA_RUN_TAILS) {
            const uint32_t items = what == RA_RUN_TAILS ? p.n_tails : p.n_reads;
            if (!items) return VGK_OK;
            hipLaunchKernelGGL(read_alignments_compose_kernel, dim3((items + 63) / 64), dim3(64), 0, stream, p, what);
        } else return VGK_EINVAL;
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int run_minimizer_regions(const MqRegionParams& p) override {
        hipSetDevice(dev);
        if (!p.n_minimizers) return VGK_OK;
        hipLaunchKernelGGL(minimizer_regions_kernel, dim3((uint32_t)((p.n_minimizers + 255) / 256)), dim3(256), 0, stream, p);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int run_read_mapq(const MqParams& p) override {
        hipSetDevice(dev);
        if (!p.n) return VGK_OK;
        return launch_lds_or_slab(read_mapq_kernel, read_mapq_slab_kernel, p.work, (p.n + 63) / 64, 0, p);
    }
    int run_explored_caps(const MqParams& p) override {
        hipSetDevice(dev);
        if (!p.n) return VGK_OK;
        return launch_lds_or_slab(explored_cap_kernel, explored_cap_slab_kernel, p.work, (p.n + 63) / 64, 0, p);
    }
    int run_pair_scores(const PmParams& p) override {
        hipSetDevice(dev);
        if (!p.n_candidates) return VGK_OK;
        hipLaunchKernelGGL(pair_score_kernel, dim3((uint32_t)((p.n_candidates + 255) / 256)), dim3(256), 0, stream, p);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int run_pair_mapq(const PmParams& p) override {
        hipSetDevice(dev);
        if (!p.n) return VGK_OK;
        return launch_lds_or_slab(pair_mapq_kernel, pair_mapq_slab_kernel, p.work, (p.n + 63) / 64, 0, p);
    }
    int run_funnel(const FnParams& p) override {
        hipSetDevice(dev);
        if (p.what == FN_RUN_GATHER) {
            if (!p.n_reads) return VGK_OK;
            hipLaunchKernelGGL(funnel_gather_kernel, dim3((p.n_reads + 63) / 64), dim3(64), 0, stream, p);
            return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
        }
        if (!p.n) return VGK_OK;
        return launch_lds_or_slab(funnel_kernel, funnel_slab_kernel, p.work, (p.n + 63) / 64, 0, p);
    }
    int run_chain_links(const ClParams& p, int what) override {
        hipSetDevice(dev);
        const uint64_t lanes = what == CL_RUN_CHECK ? p.n_slots + p.n_dist : what == CL_RUN_WALK ? p.n_chains : what == CL_RUN_SEQS ? p.n_links : cl_link_slots(p);
        if (!lanes) return VGK_OK;
        if (what == CL_RUN_CHECK) hipLaunchKernelGGL(chain_links_check_kernel, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, stream, p);
        else if (what == CL_RUN_WALK) hipLaunchKernelGGL(chain_links_walk_kernel, dim3((uint32_t)((lanes + 63) / 64)), dim3(64), 0, stream, p);
        else if (what == CL_RUN_COUNT) hipLaunchKernelGGL(chain_links_count_kernel, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, stream, p);
        else if (what == CL_RUN_WRITE) hipLaunchKernelGGL(chain_links_write_kernel, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, stream, p);
        else if (what == CL_RUN_SEQS) hipLaunchKernelGGL(chain_links_seq_kernel, dim3((uint32_t)((lanes + 3) / 4)), dim3(256), 0, stream, p);
        else return VGK_EINVAL;
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int run_pick_mappings(const PickParams& p, int what, uint32_t blocks) override {
        hipSetDevice(dev);
        if (what == PICK_RUN_PICK) {
            if (!blocks) return VGK_OK;
            return launch_lds_or_slab(pick_kernel, pick_slab_kernel, p.slab, blocks, 0, p);
        }
        const uint64_t lanes = what == PICK_RUN_CHECK ? (uint64_t)p.n_alns + p.n_chains : what == PICK_RUN_STATS ? p.n_slots : p.n_alns;
        if (!lanes) return VGK_OK;
        const dim3 grid((uint32_t)((lanes + 255) / 256));
        if (what == PICK_RUN_CHECK) hipLaunchKernelGGL(pick_check_kernel, grid, dim3(256), 0, stream, p);
        else if (what == PICK_RUN_STATS) hipLaunchKernelGGL(pick_stats_kernel, grid, dim3(256), 0, stream, p);
        else if (what == PICK_RUN_ALIGNMENTS) hipLaunchKernelGGL(pick_alignments_kernel, grid, dim3(256), 0, stream, p);
        else return VGK_EINVAL;
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int run_minimizer_choose(const MzChooseParams& p, uint32_t blocks) override {
        hipSetDevice(dev);
        if (!blocks) return VGK_OK;
        return launch_lds_or_slab(minimizer_choose_kernel, minimizer_choose_slab_kernel, p.slab, blocks, 0, p);
    }
    int run_wfa_mask(const WProb* probs, const uint32_t* src_off, const char* raw, char* seqs, uint32_t n) override {
        hipSetDevice(dev);
        if (n) hipLaunchKernelGGL(wfa_mask_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, probs, src_off, raw, seqs, n);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int run_chain_stitch(const CsParams& p, int what) override {
        hipSetDevice(dev);
        if (what == CS_GATHER) hipLaunchKernelGGL(chain_gather_kernel, dim3((p.n_reads + 3) / 4), dim3(256), 0, stream, p);
        else hipLaunchKernelGGL(chain_stitch_kernel, dim3((p.n_reads + 64) / 64), dim3(64), 0, stream, p, what);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int run_rescue_requests(const RqParams& p, int what) override {
        hipSetDevice(dev);
        hipLaunchKernelGGL(rescue_requests_kernel, dim3((p.n_pairs + 256) / 256), dim3(256), 0, stream, p, what);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int run_tail(const TailParams& p, uint32_t threads) override {
        hipSetDevice(dev);
        if (!p.n || !threads) return VGK_OK;
        hipLaunchKernelGGL(tail_walk_kernel, dim3((threads + 63) / 64), dim3(64), 0, stream, p, threads);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int scan_u32(const uint32_t* in, uint32_t* out, uint32_t n) override {
        hipSetDevice(dev);
        if (!n) return VGK_OK;
        const size_t need = hip_scan_tmp_bytes(n);
        if (need > scan_tmp_bytes) {
            if (scan_tmp) { hipStreamSynchronize(stream); hipFree(scan_tmp); scan_tmp = nullptr; scan_tmp_bytes = 0; }
            if (hipMalloc(&scan_tmp, need + need / 4) != hipSuccess) return VGK_ENOMEM;
            scan_tmp_bytes = need + need / 4;
        }
        return hip_scan_u32(in, out, n, scan_tmp, scan_tmp_bytes, stream);
    }
    int forest_flags(const ForestParams& p) override {
        hipSetDevice(dev);
        if (!p.n_nodes) return VGK_OK;
        hipLaunchKernelGGL(forest_flags_kernel, dim3((p.n_nodes + 255) / 256), dim3(256), 0, stream, p);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int forest_emit(const ForestParams& p) override {
        hipSetDevice(dev);
        if (!p.n_nodes) return VGK_OK;
        hipLaunchKernelGGL(forest_emit_kernel, dim3((p.n_nodes + 255) / 256), dim3(256), 0, stream, p);
        return hipGetLastError() == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    int fill(void* dst, int byte, size_t bytes) override {
        hipSetDevice(dev);
        return hipMemsetAsync(dst, byte, bytes, stream) == hipSuccess ? VGK_OK : VGK_ENODEV;
    }
    void watch(int which) override { hipSetDevice(dev); hipEventRecord(bev[which ? 1 : 0], stream); }
    double watch_ms() override { float ms = 0.f; hipEventElapsedTime(&ms, bev[0], bev[1]); return ms; }
    int run_wfa(const WfaParams& p, uint32_t threads) override {
        hipSetDevice(dev);
        ms_wfa = 0.f;
        if (!p.n || !threads) return VGK_OK;
        hipEventRecord(bev[0], stream);
        hipLaunchKernelGGL(wfa_kernel, dim3((threads + 63) / 64), dim3(64), 0, stream, p, threads);
        hipEventRecord(bev[1], stream);
        if (hipStreamSynchronize(stream) != hipSuccess || hipGetLastError() != hipSuccess) return VGK_ENODEV;
        hipEventElapsedTime(&ms_wfa, bev[0], bev[1]);
        return VGK_OK;
    }
    int run_wfa_wave(const WwParams& p, uint32_t waves) override {
        hipSetDevice(dev);
        if (!p.n_todo || !waves) return VGK_OK;
        hipEventRecord(bev[0], stream);
        hipLaunchKernelGGL(wfa_wave_kernel, dim3(waves), dim3(64), 0, stream, p);
        hipEventRecord(bev[1], stream);
        if (hipStreamSynchronize(stream) != hipSuccess || hipGetLastError() != hipSuccess) return VGK_ENODEV;
        float ms = 0.f; hipEventElapsedTime(&ms, bev[0], bev[1]);
        ms_wfa += ms;
        return VGK_OK;
    }
    bool wfa_concurrent() const override { return alt != nullptr; }
    int run_wfa_hybrid(const WfaParams& p, uint32_t threads, const WwParams& a, uint32_t waves) override {
        hipSetDevice(dev);
        ms_wfa = 0.f;
        if (!p.n || !threads || !waves) return VGK_OK;
        hipEventRecord(bev[0], stream);
        hipStreamWaitEvent(alt, bev[0], 0);                        // both start behind whatever the main stream held
        hipLaunchKernelGGL(wfa_kernel, dim3((threads + 63) / 64), dim3(64), 0, stream, p, threads);
        hipLaunchKernelGGL(wfa_wave_kernel, dim3(waves), dim3(64), 0, alt, a);
        hipEventRecord(bev[2], alt);
        hipStreamWaitEvent(stream, bev[2], 0);
        hipEventRecord(bev[1], stream);
        if (hipStreamSynchronize(stream) != hipSuccess || hipGetLastError() != hipSuccess) return VGK_ENODEV;
        hipEventElapsedTime(&ms_wfa, bev[0], bev[1]);
        return VGK_OK;
    }
    void reset_wfa_ms() override { ms_wfa = 0.f; }
    hipEvent_t wev[3] = {nullptr, nullptr, nullptr}; bool wide_pending = false; float ms_wide_fill = 0.f, ms_wide_walk = 0.f;
    double last_ms(int which) const override {
        if (which == 13 || which == 14) {                                // the wide route's last launch: fill | traceback
            HipBackend* self = const_cast<HipBackend*>(this);
            if (self->wide_pending) { hipSetDevice(dev); hipEventSynchronize(wev[2]); hipEventElapsedTime(&self->ms_wide_fill, wev[0], wev[1]); hipEventElapsedTime(&self->ms_wide_walk, wev[1], wev[2]); self->wide_pending = false; }
            return which == 13 ? ms_wide_fill : ms_wide_walk;
        }
        if (which == 6) return ms_wfa;
        if (which == 7) return ms_xband;
        if (which == 5) return ms_gapless;
        if (which == 3) return ms_bfill;
        if (which == 4) return ms_bwalk;
        HipBackend* self = const_cast<HipBackend*>(this);
        if (self->pending) {
            hipSetDevice(dev);
            hipStreamSynchronize(stream);
            hipEventElapsedTime(&self->ms_fill, ev[0], ev[1]);
            self->ms_walk = 0.f;
            if (timed_walk) hipEventElapsedTime(&self->ms_walk, ev[1], ev[2]);
            self->pending = false;
        }
        return which == 0 ? ms_fill : which == 1 ? ms_walk : (double)n_launches;
    }
};

Backend* make_backend(int device, std::string& err) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { err = std::string("no HIP device: ") + hipGetErrorString(e); return nullptr; }
    if (device < 0 || device >= n) { err = "HIP device index out of range"; return nullptr; }
    auto* b = new HipBackend();
    b->dev = device;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&b->prop, device) != hipSuccess) {
        err = "cannot select HIP device"; delete b; return nullptr; }
    // The side (copy) and fetch streams carry what the host WAITS for beside a main stream that is busy — small kernels (packers, the banded
    // geometry), descriptors up, results down: they get the device's highest stream priority, so that their work takes the slots a
    // saturating fill frees first instead of queueing behind all of its workgroups (VGAMD_STREAM_PRIORITY=0: all streams alike).
    int prio_least = 0, prio_greatest = 0;
    const bool use_prio = !(std::getenv("VGAMD_STREAM_PRIORITY") && std::atoi(std::getenv("VGAMD_STREAM_PRIORITY")) == 0) &&
                          hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) == hipSuccess && prio_greatest != prio_least;
    auto make_stream = [&](hipStream_t* st, bool high) {
        if (high && use_prio && hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio_greatest) == hipSuccess) return true;
        (void)hipGetLastError();
        return hipStreamCreateWithFlags(st, hipStreamNonBlocking) == hipSuccess;
    };
    if (!make_stream(&b->stream, false) || !make_stream(&b->copy, true) || !make_stream(&b->fetch, true) || !make_stream(&b->alt, false)) { err = "cannot create HIP stream"; delete b; return nullptr; }
    for (int i = 0; i < 2; ++i)
        if (hipStreamCreateWithFlags(&b->side[i], hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&b->side_done[i], hipEventDisableTiming) != hipSuccess) { err = "cannot create HIP side stream"; delete b; return nullptr; }
    for (auto& ev : b->bev) if (hipEventCreate(&ev) != hipSuccess) { err = "cannot create HIP event"; delete b; return nullptr; }
    for (auto& ev : b->ev) if (hipEventCreate(&ev) != hipSuccess) { err = "cannot create HIP event"; delete b; return nullptr; }
    for (auto& ev : b->evb) if (hipEventCreate(&ev) != hipSuccess) { err = "cannot create HIP event"; delete b; return nullptr; }
    for (auto& ev : b->fill_done) if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { err = "cannot create HIP event"; delete b; return nullptr; }
    return b;
}

}  // namespace vgk
