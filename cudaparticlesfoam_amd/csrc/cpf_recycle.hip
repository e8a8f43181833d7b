// Recycling cloud (cpf_sink_apply*, cpf_respawn_box*): an open system without touching a step kernel.  Between launches a particle
// found in a SINK cell becomes CPF_CELL_LOST -- a dead slot, which every step kernel, frame, sort and occupancy sample already
// skips --, and dead slots get a fresh position in a SOURCE box and are located anew.  The cloud keeps its size and its ids
// (DESIGN.md "Recycling").
//
// Sink.  One pass over the 4-byte cell ids in the shape of occupancy_kernel: a workgroup takes one contiguous slice of kSinkSlice ids
// with 16-byte loads, four ids per lane, kSinkLoads loads in flight.  The sink set is a bitmask over DERIVED cells; a mask of at
// most kSinkLdsWords words is staged in LDS while the loads are in flight (pitzDaily: 383 words), a larger one is read through L2
// (a cell-sorted slice touches a handful of its words).  Only quads that changed are stored: almost all of the cloud is left
// unwritten.  The hits of a wave are counted with ballot + popcount, a workgroup adds its sum once to a 64-bit counter: integer
// sums, the same count whatever the order.
//
// Respawn.  A candidate is a slot with cell < 0; candidates are taken in ARRAY order up to maxCount.  Limited: (a) the candidates of
// every workgroup's slice are counted, (b) one workgroup turns the counts into exclusive offsets, (c) every lane recomputes its rank
// -- ballot prefix within the wave, wave offsets through LDS, the slice's offset from (b) -- and ranks below maxCount draw, locate
// and store.  Unlimited: (c) alone, every candidate is chosen.  The position is a pure function of (seed, gid, epoch)
// (cpf_philox.h, respawn_position): it does not depend on order, launch shape or rank.  The cell is the initial-locate rule
// (cpf_locate.h); a point outside the mesh leaves the slot dead (CPF_CELL_LOST, at the drawn point) and a candidate again.
#include <hip/hip_runtime.h>

#include "cpf_device.h"
#include "cpf_locate.h"
#include "cpf_philox.h"

namespace cpf {
namespace {

constexpr int kSinkBlock = 256;                             // 4 waves
constexpr int kSinkLoads = 4;                               // 16-byte loads in flight per lane
constexpr int kSinkTrip = kSinkBlock * 4;                   // ids one round of loads covers
constexpr int kSinkSlice = kSinkTrip * kSinkLoads;          // ids per workgroup
constexpr int kSinkLdsWords = 2048;                         // mask words staged in LDS: 8 KB, 65 536 cells -- half a slice's id bytes at most

constexpr int kSpawnBlock = 256;                            // 4 waves
// one round of loads per workgroup: dead slots come in runs (a sink's cells are neighbours in a sorted cloud, a sort sends the dead to
// the tail), and a workgroup takes its dead 64 at a time per wave -- measured, four rounds a workgroup made a run three times as slow
constexpr int kSpawnLoads = 1;                              // 16-byte loads per lane
constexpr int kSpawnTrip = kSpawnBlock * 4;                 // ids one round of loads covers
constexpr int kSpawnSlice = kSpawnTrip * kSpawnLoads;       // ids per workgroup
constexpr int kScanBlock = 1024;                            // the single workgroup of pass (b)

// lanes below this one whose bit is set in a wave-wide ballot
__device__ inline unsigned lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// the four ids at i .. i + 3 (past the end: 0, which is neither in a sink nor dead); vec: `cell` is 16-byte aligned
__device__ inline int4 load_quad(const int32_t* __restrict__ cell, int64_t i, int64_t n, bool vec) {
    if (vec && i + 3 < n) return *reinterpret_cast<const int4*>(cell + i);
    int4 q;
    q.x = (i < n) ? cell[i] : 0;
    q.y = (i + 1 < n) ? cell[i + 1] : 0;
    q.z = (i + 2 < n) ? cell[i + 2] : 0;
    q.w = (i + 3 < n) ? cell[i + 3] : 0;
    return q;
}

}  // namespace

// (outside the anonymous namespace, like the step kernels: tools/resource_usage.py lists kernels by their plain names)
// kVec: `cell` is 16-byte aligned (a slice starts at a multiple of kSinkSlice ids, so every full quad is one aligned load / store)
template <bool kVec>
__global__ __launch_bounds__(kSinkBlock) void sink_kernel(int32_t* __restrict__ cell, int64_t n, const uint32_t* __restrict__ mask,
                                                          int nDerived, int maskWords,
                                                          unsigned long long* __restrict__ absorbed) {
    __shared__ uint32_t sMask[kSinkLdsWords];
    __shared__ unsigned sHits;
    const int lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * kSinkSlice + 4 * (int64_t)threadIdx.x;
    int4 v[kSinkLoads];
#pragma unroll
    for (int k = 0; k < kSinkLoads; ++k) v[k] = load_quad(cell, base + (int64_t)k * kSinkTrip, n, kVec);
    const bool staged = maskWords <= kSinkLdsWords;
    if (staged)
        for (int w = threadIdx.x; w < maskWords; w += kSinkBlock) sMask[w] = mask[w];
    if (threadIdx.x == 0) sHits = 0u;
    __syncthreads();
    // a live id (0 <= c < nDerived) whose bit is set; every other id -- CPF_CELL_LOST, CPF_CELL_FROZEN, ids beyond the mesh -- stays
    auto sunk = [&](int c) -> bool {
        if ((unsigned)c >= (unsigned)nDerived) return false;
        const uint32_t w = staged ? sMask[c >> 5] : mask[c >> 5];
        return ((w >> (c & 31)) & 1u) != 0u;
    };
    unsigned hits = 0;
#pragma unroll
    for (int k = 0; k < kSinkLoads; ++k) {
        const int64_t i = base + (int64_t)k * kSinkTrip;
        const bool hx = sunk(v[k].x), hy = sunk(v[k].y), hz = sunk(v[k].z), hw = sunk(v[k].w);   // (past the end: id 0 read as "no")
        const bool bx = hx && i < n, by = hy && i + 1 < n, bz = hz && i + 2 < n, bw = hw && i + 3 < n;
        hits += (unsigned)__popcll(__ballot(bx)) + (unsigned)__popcll(__ballot(by)) + (unsigned)__popcll(__ballot(bz)) +
                (unsigned)__popcll(__ballot(bw));
        if (!(bx || by || bz || bw)) continue;
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
    if (threadIdx.x == 0 && sHits != 0u) atomicAdd(absorbed, (unsigned long long)sHits);
}

// pass (a) of a limited respawn: counts[b] = dead slots (cell < 0) in workgroup b's slice of kSpawnSlice ids
__global__ __launch_bounds__(kSpawnBlock) void respawn_count_kernel(const int32_t* __restrict__ cell, int64_t n, int vec,
                                                                    unsigned* __restrict__ counts) {
    __shared__ unsigned sDead;
    if (threadIdx.x == 0) sDead = 0u;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kSpawnSlice + 4 * (int64_t)threadIdx.x;
    int4 v[kSpawnLoads];
#pragma unroll
    for (int k = 0; k < kSpawnLoads; ++k) v[k] = load_quad(cell, base + (int64_t)k * kSpawnTrip, n, vec != 0);
    unsigned dead = 0;
#pragma unroll
    for (int k = 0; k < kSpawnLoads; ++k)
        dead += (unsigned)__popcll(__ballot(v[k].x < 0)) + (unsigned)__popcll(__ballot(v[k].y < 0)) +
                (unsigned)__popcll(__ballot(v[k].z < 0)) + (unsigned)__popcll(__ballot(v[k].w < 0));
    if ((threadIdx.x & 63) == 0 && dead != 0u) atomicAdd(&sDead, dead);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = sDead;
}

// pass (b): offsets[b] = counts[0] + ... + counts[b - 1], one workgroup, kScanBlock counts a round (their sum is below 2^31)
__global__ __launch_bounds__(kScanBlock) void respawn_scan_kernel(const unsigned* __restrict__ counts, unsigned* __restrict__ offsets,
                                                                  int nBlocks) {
    __shared__ unsigned sWave[kScanBlock / 64];
    __shared__ unsigned sCarry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) sCarry = 0u;
    __syncthreads();
    for (int b0 = 0; b0 < nBlocks; b0 += kScanBlock) {
        const int b = b0 + (int)threadIdx.x;
        const unsigned c = b < nBlocks ? counts[b] : 0u;
        unsigned incl = c;                                   // inclusive prefix within the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) sWave[wave] = incl;
        __syncthreads();
        unsigned before = sCarry;
        for (int w = 0; w < wave; ++w) before += sWave[w];
        if (b < nBlocks) offsets[b] = before + incl - c;
        __syncthreads();
        if (threadIdx.x == kScanBlock - 1) sCarry = before + incl;
        __syncthreads();
    }
}

struct SpawnBox { double lower[3], upper[3]; };

// pass (c): the dead slots whose rank in array order is below maxCount (offsets == nullptr: every dead slot) draw their position,
// are located and stored.  A workgroup without a dead slot leaves at once.  The chosen slots of a wave are first gathered into a
// list in LDS, a round of loads at a time, and the wave's lanes then take one slot each: with one particle in a hundred dead a
// wave draws and locates its two or three in ONE pass instead of once per element of a lane's quads.
// counters: [0] absorbed (the sink's), [1] drawn, [2] placed
__global__ __launch_bounds__(kSpawnBlock) void respawn_place_kernel(double* __restrict__ x, double* __restrict__ y, double* __restrict__ z,
                                                                    int32_t* __restrict__ cell, const int64_t* __restrict__ gid, int64_t n,
                                                                    int vec, SpawnBox box, const unsigned* __restrict__ offsets,
                                                                    int64_t maxCount, uint32_t seed, uint32_t epoch,
                                                                    const int32_t* __restrict__ cellOff, const double4* __restrict__ planes,
                                                                    GridView g, unsigned long long* __restrict__ counters) {
    __shared__ unsigned sWave[kSpawnLoads][kSpawnBlock / 64];   // dead slots per (round of loads, wave): the ranks of a limited respawn
    __shared__ int sList[kSpawnBlock / 64][256];                // per wave: the chosen slots of one round (at most 4 per lane)
    __shared__ unsigned sDrawn, sPlaced, sAny;
    // the grid and the box go through LDS: as kernel arguments they would sit in 60 scalar registers across the locate's loops
    __shared__ GridView sGrid;
    __shared__ SpawnBox sBox;
    const bool limited = offsets != nullptr;
    const int64_t first = limited ? (int64_t)offsets[blockIdx.x] : 0;
    if (limited && first >= maxCount) return;               // (the whole workgroup: nothing of this slice is chosen)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t blockBase = (int64_t)blockIdx.x * kSpawnSlice;
    int4 v[kSpawnLoads];
#pragma unroll
    for (int k = 0; k < kSpawnLoads; ++k) v[k] = load_quad(cell, blockBase + (int64_t)k * kSpawnTrip + 4 * (int64_t)threadIdx.x, n, vec != 0);
    unsigned dead = 0;                                      // bit 4 k + j: element j of quad k is a dead slot (past the end: load_quad gave 0)
#pragma unroll
    for (int k = 0; k < kSpawnLoads; ++k)
        dead |= ((v[k].x < 0 ? 1u : 0u) | (v[k].y < 0 ? 2u : 0u) | (v[k].z < 0 ? 4u : 0u) | (v[k].w < 0 ? 8u : 0u)) << (4 * k);
    if (threadIdx.x == 0) { sDrawn = 0u; sPlaced = 0u; sAny = 0u; }
    __syncthreads();
    const unsigned long long anyDead = __ballot(dead != 0u);
    if (lane == 0 && anyDead != 0ull) sAny = 1u;
    __syncthreads();
    if (sAny == 0u) return;                                 // (the whole workgroup: no dead slot in the slice)
    if (threadIdx.x == 0) { sGrid = g; sBox = box; }
    unsigned below[kSpawnLoads];                            // dead slots of the lanes below this one, per round
#pragma unroll
    for (int k = 0; k < kSpawnLoads; ++k) {
        unsigned total = 0;
        below[k] = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned long long b = __ballot(((dead >> (4 * k + j)) & 1u) != 0u);
            below[k] += lanes_below(b);
            total += (unsigned)__popcll(b);
        }
        if (lane == 0) sWave[k][wave] = total;
    }
    __syncthreads();
    unsigned chosen = dead;
    if (limited) {
        // array order = (round, lane, element): the slice's offset, the rounds before, the waves before, the lanes below, this lane's own
        chosen = 0u;
        int64_t rank0 = first;
#pragma unroll
        for (int k = 0; k < kSpawnLoads; ++k) {
            int64_t rank = rank0 + below[k];
#pragma unroll
            for (int w = 0; w < kSpawnBlock / 64; ++w) {
                if (w < wave) rank += sWave[k][w];
                rank0 += sWave[k][w];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((dead >> (4 * k + j)) & 1u) {
                    if (rank < maxCount) chosen |= 1u << (4 * k + j);
                    ++rank;
                }
        }
    }
    unsigned drawn = 0, placed = 0;
#pragma unroll 1
    for (int k = 0; k < kSpawnLoads; ++k) {
        // the wave's chosen slots of this round, element-major (any order will do: a position does not depend on it)
        unsigned total = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool mine = ((chosen >> (4 * k + j)) & 1u) != 0u;
            const unsigned long long b = __ballot(mine);
            if (mine) sList[wave][total + lanes_below(b)] = k * kSpawnTrip + 4 * (int)threadIdx.x + j;
            total += (unsigned)__popcll(b);
        }
        __syncthreads();                                    // (the list is the wave's own; the loop is the whole workgroup's)
        for (unsigned t = lane; t < total; t += 64) {
            const int64_t s = blockBase + sList[wave][t];
            double p[3];
            respawn_position(seed, (uint64_t)(gid ? gid[s] : s), epoch, sBox.lower, sBox.upper, p);
            const int found = locate_point(D3{p[0], p[1], p[2]}, cellOff, planes, sGrid);
            x[s] = p[0]; y[s] = p[1]; z[s] = p[2];
            cell[s] = found;
            placed += (unsigned)__popcll(__ballot(found >= 0));     // (lane 0 is in every pass that runs)
        }
        drawn += total;
        __syncthreads();
    }
    if (lane == 0 && drawn != 0u) { atomicAdd(&sDrawn, drawn); atomicAdd(&sPlaced, placed); }
    __syncthreads();
    if (threadIdx.x == 0 && sDrawn != 0u) {
        atomicAdd(&counters[1], (unsigned long long)sDrawn);
        if (sPlaced != 0u) atomicAdd(&counters[2], (unsigned long long)sPlaced);
    }
}

hipError_t sink_apply(hipStream_t st, int32_t* cell, int64_t n, const uint32_t* mask, int64_t nDerived,
                      unsigned long long* absorbed) {
    if (n <= 0) return hipSuccess;
    const int64_t blocks = (n + kSinkSlice - 1) / kSinkSlice;
    if (blocks > (int64_t)INT32_MAX || nDerived > (int64_t)INT32_MAX) return hipErrorInvalidValue;
    const int maskWords = (int)((nDerived + 31) / 32);
    if ((reinterpret_cast<uintptr_t>(cell) & 15u) == 0)
        hipLaunchKernelGGL(sink_kernel<true>, dim3((unsigned)blocks), dim3(kSinkBlock), 0, st, cell, n, mask, (int)nDerived, maskWords, absorbed);
    else
        hipLaunchKernelGGL(sink_kernel<false>, dim3((unsigned)blocks), dim3(kSinkBlock), 0, st, cell, n, mask, (int)nDerived, maskWords, absorbed);
    return hipGetLastError();
}

size_t respawn_scratch_bytes(int64_t n) {
    const int64_t blocks = (n + kSpawnSlice - 1) / kSpawnSlice;
    return (size_t)(blocks > 0 ? blocks : 1) * 2 * sizeof(unsigned);
}

hipError_t respawn_box(hipStream_t st, double* x, double* y, double* z, int32_t* cell, const int64_t* gid, int64_t n,
                       const double lower[3], const double upper[3], int64_t maxCount, uint32_t seed, uint32_t epoch,
                       const MeshView& m, const GridView& g, void* scratch, size_t scratchBytes, unsigned long long* counters) {
    if (n <= 0 || maxCount == 0) return hipSuccess;
    if (n >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const int64_t blocks = (n + kSpawnSlice - 1) / kSpawnSlice;
    const int vec = (reinterpret_cast<uintptr_t>(cell) & 15u) == 0 ? 1 : 0;
    SpawnBox box;
    for (int k = 0; k < 3; ++k) { box.lower[k] = lower[k]; box.upper[k] = upper[k]; }
    unsigned* offsets = nullptr;
    if (maxCount > 0 && maxCount < n) {                     // (maxCount >= n cannot bind: the unlimited pass alone)
        if (scratchBytes < respawn_scratch_bytes(n)) return hipErrorInvalidValue;
        unsigned* counts = static_cast<unsigned*>(scratch);
        offsets = counts + blocks;
        hipLaunchKernelGGL(respawn_count_kernel, dim3((unsigned)blocks), dim3(kSpawnBlock), 0, st, cell, n, vec, counts);
        hipLaunchKernelGGL(respawn_scan_kernel, dim3(1), dim3(kScanBlock), 0, st, counts, offsets, (int)blocks);
    }
    hipLaunchKernelGGL(respawn_place_kernel, dim3((unsigned)blocks), dim3(kSpawnBlock), 0, st, x, y, z, cell, gid, n, vec, box, offsets,
                       maxCount, seed, epoch, m.cellOff, m.planes, g, counters);
    return hipGetLastError();
}

}  // namespace cpf
