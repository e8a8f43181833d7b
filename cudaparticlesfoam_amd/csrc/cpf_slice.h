// One pass over a 4-byte cell-id array, a slice per workgroup: the shape the occupancy, recycling and tracer-age kernels share
// (cpf_occupancy.hip, cpf_recycle.hip, cpf_age.hip; cpf_handoff.hip's histogram takes count_runs).  A workgroup of kSliceBlock
// threads takes one contiguous slice with 16-byte loads, four ids per lane, all of a lane's loads in flight, and keeps it in
// registers.  What a kernel then does with its slice is one of three things, each written once here:
//   - sink_pass: ids whose bit is set in a mask become CPF_CELL_LOST, only changed quads are stored, the hits are summed;
//   - dead_mask / workgroup_any / wave_list: the slots with cell < 0 (or any other choice of a lane's elements) are gathered into
//     a list per wave, which the wave's lanes then take in turn;
//   - slice_window / window_bins: the ids are counted into LDS bins over the slice's window [lo, hi] of live ids and flushed as
//     contiguous global adds, or, where the window is wider than the bins, through a direct-mapped cache of (word, cell) pairs.
// The helpers that need LDS declare their own: a kernel's LDS is the sum of what it calls.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cpf.h"

namespace cpf {

constexpr int kSliceBlock = 256;                            // 4 waves
constexpr int kSliceLoads = 4;                              // 16-byte loads in flight per lane (the respawn kernels: one, see there)
constexpr int kSliceTrip = kSliceBlock * 4;                 // ids one round of loads covers
constexpr int slice_ids(int loads) { return kSliceTrip * loads; }   // ids per workgroup
// the respawn passes (cpf_recycle.hip, cpf_inlet.hip): one round of loads per workgroup: dead slots come in runs (a sink's cells are
// neighbours in a sorted cloud, a sort sends the dead to the tail), and a workgroup takes its dead 64 at a time per wave --
// measured, four rounds a workgroup made a run three times as slow
constexpr int kSpawnLoads = 1;                              // 16-byte loads per lane
constexpr int kSpawnSlice = slice_ids(kSpawnLoads);         // ids per workgroup
constexpr int kSinkLdsWords = 2048;                         // mask words staged in LDS: 8 KB, 65 536 cells -- half a slice's id bytes at most

// The launch of a slice pass over n > 0 ids: its grid, and whether `cell` is 16-byte aligned (a slice starts at a multiple of
// its length, so every full quad is then one aligned load / store).
struct SliceLaunch {
    int64_t blocks;
    bool vec;
    bool fits() const { return blocks <= (int64_t)INT32_MAX; }
};
inline SliceLaunch slice_launch(const void* cell, int64_t n, int loads = kSliceLoads) {
    return {(n + slice_ids(loads) - 1) / slice_ids(loads), (reinterpret_cast<uintptr_t>(cell) & 15u) == 0};
}

// lanes below this one whose bit is set in a wave-wide ballot
__device__ inline unsigned lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// the four ids at i .. i + 3 (past the end: `pad`); vec: `cell` is 16-byte aligned and i a multiple of 4
__device__ inline int4 load_quad(const int32_t* __restrict__ cell, int64_t i, int64_t n, bool vec, int pad) {
    if (vec && i + 3 < n) return *reinterpret_cast<const int4*>(cell + i);
    int4 q;
    q.x = (i < n) ? cell[i] : pad;
    q.y = (i + 1 < n) ? cell[i + 1] : pad;
    q.z = (i + 2 < n) ? cell[i + 2] : pad;
    q.w = (i + 3 < n) ? cell[i + 3] : pad;
    return q;
}

// a lane's quads of its workgroup's slice: quad k is the four ids at slice_base() + k * kSliceTrip
template <int kLoads>
__device__ inline int64_t slice_base() {
    return (int64_t)blockIdx.x * slice_ids(kLoads) + 4 * (int64_t)threadIdx.x;
}
template <int kLoads>
__device__ inline void load_slice(const int32_t* __restrict__ cell, int64_t n, bool vec, int pad, int4 (&v)[kLoads]) {
#pragma unroll
    for (int k = 0; k < kLoads; ++k) v[k] = load_quad(cell, slice_base<kLoads>() + (int64_t)k * kSliceTrip, n, vec, pad);
}

// The sink's pass over a slice.  The sink set is a bitmask over DERIVED cells; a mask of at most kSinkLdsWords words is staged in
// LDS while the loads are in flight (pitzDaily: 383 words), a larger one is read through L2 (a cell-sorted slice touches a handful
// of its words).  The hits of a wave are counted with ballot + popcount and summed per workgroup: returns that sum, in every
// thread, behind a barrier.  kHit: `hit` gets the lane's own hits, bit 4 k + j: element j of quad k was absorbed.  `v` gets the
// lane's quads as they were loaded, BEFORE the pass marked anybody (cpf_routes.hip asks a hit's cell for its sink group).
template <bool kVec, bool kHit>
__device__ inline unsigned sink_pass(int32_t* __restrict__ cell, int64_t n, const uint32_t* __restrict__ mask, int nDerived,
                                     int maskWords, unsigned& hit, int4 (&v)[kSliceLoads]) {
    __shared__ uint32_t sMask[kSinkLdsWords];
    __shared__ unsigned sHits;
    const int lane = threadIdx.x & 63;
    const int64_t base = slice_base<kSliceLoads>();
    load_slice(cell, n, kVec, 0, v);                        // (past the end: 0, which is neither in a sink nor dead)
    const bool staged = maskWords <= kSinkLdsWords;
    if (staged)
        for (int w = threadIdx.x; w < maskWords; w += kSliceBlock) sMask[w] = mask[w];
    if (threadIdx.x == 0) sHits = 0u;
    __syncthreads();
    // a live id (0 <= c < nDerived) whose bit is set; every other id -- CPF_CELL_LOST, CPF_CELL_FROZEN, ids beyond the mesh -- stays
    auto sunk = [&](int c) -> bool {
        if ((unsigned)c >= (unsigned)nDerived) return false;
        const uint32_t w = staged ? sMask[c >> 5] : mask[c >> 5];
        return ((w >> (c & 31)) & 1u) != 0u;
    };
    unsigned hits = 0;
    if (kHit) hit = 0u;
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k) {
        const int64_t i = base + (int64_t)k * kSliceTrip;
        const bool hx = sunk(v[k].x), hy = sunk(v[k].y), hz = sunk(v[k].z), hw = sunk(v[k].w);   // (past the end: id 0 read as "no")
        const bool bx = hx && i < n, by = hy && i + 1 < n, bz = hz && i + 2 < n, bw = hw && i + 3 < n;
        hits += (unsigned)__popcll(__ballot(bx)) + (unsigned)__popcll(__ballot(by)) + (unsigned)__popcll(__ballot(bz)) +
                (unsigned)__popcll(__ballot(bw));
        if (!(bx || by || bz || bw)) continue;
        if (kHit) hit |= ((bx ? 1u : 0u) | (by ? 2u : 0u) | (bz ? 4u : 0u) | (bw ? 8u : 0u)) << (4 * k);
        if (kVec && i + 3 < n) {
            int4 q = v[k];
            if (bx) q.x = CPF_CELL_LOST;
            if (by) q.y = CPF_CELL_LOST;
            if (bz) q.z = CPF_CELL_LOST;
            if (bw) q.w = CPF_CELL_LOST;
            *reinterpret_cast<int4*>(cell + i) = q;
        } else {
            if (bx) cell[i] = CPF_CELL_LOST;
            if (by) cell[i + 1] = CPF_CELL_LOST;
            if (bz) cell[i + 2] = CPF_CELL_LOST;
            if (bw) cell[i + 3] = CPF_CELL_LOST;
        }
    }
    // (hits is the wave's sum in every lane: the ballots are wave-wide)
    if (lane == 0 && hits != 0u) atomicAdd(&sHits, hits);
    __syncthreads();
    return sHits;
}
// (the same for a kernel that has no use for the loaded quads)
template <bool kVec, bool kHit>
__device__ inline unsigned sink_pass(int32_t* __restrict__ cell, int64_t n, const uint32_t* __restrict__ mask, int nDerived,
                                     int maskWords, unsigned& hit) {
    int4 v[kSliceLoads];
    return sink_pass<kVec, kHit>(cell, n, mask, nDerived, maskWords, hit, v);
}

// bit 4 k + j: element j of quad k is a dead slot, cell < 0 (past the end: pad the loads with 0)
template <int kLoads>
__device__ inline unsigned dead_mask(const int4 (&v)[kLoads]) {
    unsigned dead = 0;
#pragma unroll
    for (int k = 0; k < kLoads; ++k)
        dead |= ((v[k].x < 0 ? 1u : 0u) | (v[k].y < 0 ? 2u : 0u) | (v[k].z < 0 ? 4u : 0u) | (v[k].w < 0 ? 8u : 0u)) << (4 * k);
    return dead;
}

// whether `mine` holds in any thread of the workgroup, the same answer in all of them: on false the whole workgroup can leave
__device__ inline bool workgroup_any(bool mine) {
    __shared__ unsigned sAny;
    if (threadIdx.x == 0) sAny = 0u;
    __syncthreads();
    const unsigned long long any = __ballot(mine);
    if ((threadIdx.x & 63) == 0 && any != 0ull) sAny = 1u;
    __syncthreads();
    return sAny != 0u;
}

// The chosen elements of a lane's kLoads quads (bit 4 k + j of `chosen`: element j of quad k) are gathered into the wave's own
// list of slots within the slice (at most slice_ids(kLoads) / 4 entries), round- and then element-major; returns their number.
// The list may be read behind a __syncthreads().
template <int kLoads, class Slot>
__device__ inline unsigned wave_list(unsigned chosen, Slot* __restrict__ list) {
    unsigned total = 0;
#pragma unroll
    for (int k = 0; k < kLoads; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool mine = ((chosen >> (4 * k + j)) & 1u) != 0u;
            const unsigned long long b = __ballot(mine);
            if (mine) list[total + lanes_below(b)] = (Slot)(k * kSliceTrip + 4 * (int)threadIdx.x + j);
            total += (unsigned)__popcll(b);
        }
    return total;
}

// Adds weight w to the bin of every lane's id c (negative: none).  Runs of equal ids in the wave are taken kRounds times by their
// first lane -- one add of popcount * w --, what is left adds for itself.  Wave-uniform control flow.
template <int kRounds, class Add>
__device__ inline void count_runs(int c, unsigned w, int lane, Add add) {
    bool todo = c >= 0;
#pragma unroll 1
    for (int round = 0; round < kRounds; ++round) {
        const unsigned long long m = __ballot(todo);
        if (m == 0ull) return;
        const int leader = __ffsll((long long)m) - 1;
        const int cl = __builtin_amdgcn_readlane(c, leader);
        const unsigned long long same = __ballot(todo && c == cl);
        if (lane == leader) add(cl, (unsigned)__popcll(same) * w);
        if (c == cl) todo = false;
    }
    if (todo) add(c, w);
}

// The window [first, last] of the slice's live ids, over the lanes' mapped quads (not live: -1); returns last, the same in the
// whole workgroup: negative if the slice has no live id.
template <int kLoads>
__device__ inline int slice_window(const int4 (&v)[kLoads], int& first) {
    __shared__ int sLo[kSliceBlock / 64], sHi[kSliceBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned lo = 0xFFFFFFFFu;                              // (a negative id is a huge unsigned: the minimum skips it)
    int hi = -1;
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
        lo = min(min(lo, (unsigned)v[k].x), min(min((unsigned)v[k].y, (unsigned)v[k].z), (unsigned)v[k].w));
        hi = max(max(hi, v[k].x), max(max(v[k].y, v[k].z), v[k].w));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = min(lo, (unsigned)__shfl_xor((int)lo, d));
        hi = max(hi, __shfl_xor(hi, d));
    }
    if (lane == 0) { sLo[wave] = (int)lo; sHi[wave] = hi; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kSliceBlock / 64; ++w) {
        lo = min(lo, (unsigned)sLo[w]);
        hi = max(hi, sHi[w]);
    }
    first = (int)lo;
    return hi;
}

// kBins words of LDS over the window of slice_window.  count(add) has every lane call add(cell, word) for what its quads hold;
// flush(cell, word) adds a bin's non-zero sum to global memory.
//   - The window fits the bins (a cell-sorted cloud: a slice spans a handful of cells): bin = cell - first, and the flush is the
//     window alone, lane = cell, contiguous global adds, empty bins skipped.
//   - It does not: the bins become a direct-mapped cache of kBins / 2 (word, cell) pairs, words in the lower half, the 32-bit cell
//     ids behind them, bin = cell modulo kBins / 2.  An add claims its bin if it is free or holds the same cell; one that finds its
//     bin taken by another cell flushes for itself.  The flush walks the bins: neighbouring ids sit in neighbouring bins, so a band
//     of ids still leaves as contiguous adds.
template <class Word, int kBins, class Count, class Flush>
__device__ inline void window_bins(int first, int last, Count count, Flush flush) {
    constexpr int kTagBins = kBins / 2;
    const int width = last - first + 1;
    static_assert((kTagBins & (kTagBins - 1)) == 0, "bin = id & (kTagBins - 1)");
    __shared__ Word sBins[kBins];
    if (width <= kBins) {
        for (int b = threadIdx.x; b < width; b += kSliceBlock) sBins[b] = 0;
        __syncthreads();
        count([&](int c, Word w) { atomicAdd(&sBins[c - first], w); });
        __syncthreads();
        for (int b = threadIdx.x; b < width; b += kSliceBlock) {
            const Word w = sBins[b];
            if (w != 0) flush(first + b, w);
        }
    } else {
        Word* sWord = sBins;
        int* sTag = reinterpret_cast<int*>(sBins + kTagBins);
        for (int b = threadIdx.x; b < kTagBins; b += kSliceBlock) { sWord[b] = 0; sTag[b] = -1; }
        __syncthreads();
        count([&](int c, Word w) {
            const int b = c & (kTagBins - 1);
            const int held = atomicCAS(&sTag[b], -1, c);
            if (held == -1 || held == c) atomicAdd(&sWord[b], w);
            else flush(c, w);
        });
        __syncthreads();
        for (int b = threadIdx.x; b < kTagBins; b += kSliceBlock) {
            const Word w = sWord[b];
            if (w != 0) flush(sTag[b], w);
        }
    }
}

}  // namespace cpf
