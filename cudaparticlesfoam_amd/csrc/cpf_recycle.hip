// Recycling cloud (cpf_sink_apply*, cpf_respawn_box*): an open system without touching a step kernel.  Between launches a particle
// found in a SINK cell becomes CPF_CELL_LOST -- a dead slot, which every step kernel, frame, sort and occupancy sample already
// skips --, and dead slots get a fresh position in a SOURCE box and are located anew.  The cloud keeps its size and its ids
// (DESIGN.md "Recycling").
//
// Sink.  cpf_slice.h's sink_pass over the 4-byte cell ids, a slice per workgroup: only quads that changed are stored, so almost all
// of the cloud is left unwritten, and a workgroup adds its hits once to a 64-bit counter: integer sums, the same count whatever
// the order.
//
// Respawn.  A candidate is a slot with cell < 0; candidates are taken in ARRAY order up to maxCount.  Limited: (a) the candidates of
// every workgroup's slice are counted, (b) one workgroup turns the counts into exclusive offsets, (c) every lane recomputes its rank
// -- ballot prefix within the wave, wave offsets through LDS, the slice's offset from (b) -- and ranks below maxCount draw, locate
// and store.  Unlimited: (c) alone, every candidate is chosen.  The position is a pure function of (seed, gid, epoch)
// (cpf_philox.h, respawn_position): it does not depend on order, launch shape or rank.  The cell is the initial-locate rule
// (cpf_locate.h); a point outside the mesh leaves the slot dead (CPF_CELL_LOST, at the drawn point) and a candidate again.
// The slice and the dead-slot mask are cpf_slice.h's.
#include <hip/hip_runtime.h>

#include "cpf_device.h"
#include "cpf_locate.h"
#include "cpf_philox.h"
#include "cpf_slice.h"

namespace cpf {
namespace {

// (kSpawnLoads, kSpawnSlice: cpf_slice.h -- cpf_inlet.hip's pass walks the same slices)
constexpr int kScanBlock = 1024;                            // the single workgroup of pass (b)

}  // namespace

// (outside the anonymous namespace, like the step kernels: tools/resource_usage.py lists kernels by their plain names)
// kVec: `cell` is 16-byte aligned
template <bool kVec>
__global__ __launch_bounds__(kSliceBlock) void sink_kernel(int32_t* __restrict__ cell, int64_t n, const uint32_t* __restrict__ mask,
                                                           int nDerived, int maskWords,
                                                           unsigned long long* __restrict__ absorbed) {
    unsigned none;
    const unsigned all = sink_pass<kVec, false>(cell, n, mask, nDerived, maskWords, none);
    if (threadIdx.x == 0 && all != 0u) atomicAdd(absorbed, (unsigned long long)all);
}

// pass (a) of a limited respawn: counts[b] = dead slots (cell < 0) in workgroup b's slice of kSpawnSlice ids
__global__ __launch_bounds__(kSliceBlock) void respawn_count_kernel(const int32_t* __restrict__ cell, int64_t n, int vec,
                                                                    unsigned* __restrict__ counts) {
    __shared__ unsigned sDead;
    if (threadIdx.x == 0) sDead = 0u;
    __syncthreads();
    int4 v[kSpawnLoads];
    load_slice(cell, n, vec != 0, 0, v);
    const unsigned mask = dead_mask(v);
    unsigned dead = 0;
#pragma unroll
    for (int b = 0; b < 4 * kSpawnLoads; ++b) dead += (unsigned)__popcll(__ballot(((mask >> b) & 1u) != 0u));
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
__global__ __launch_bounds__(kSliceBlock) void respawn_place_kernel(double* __restrict__ x, double* __restrict__ y, double* __restrict__ z,
                                                                    int32_t* __restrict__ cell, const int64_t* __restrict__ gid, int64_t n,
                                                                    int vec, SpawnBox box, const unsigned* __restrict__ offsets,
                                                                    int64_t maxCount, uint32_t seed, uint32_t epoch,
                                                                    const int32_t* __restrict__ cellOff, const double4* __restrict__ planes,
                                                                    GridView g, unsigned long long* __restrict__ counters) {
    __shared__ unsigned sWave[kSpawnLoads][kSliceBlock / 64];   // dead slots per (round of loads, wave): the ranks of a limited respawn
    __shared__ int sList[kSliceBlock / 64][256];                // per wave: the chosen slots of one round (at most 4 per lane)
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
    load_slice(cell, n, vec != 0, 0, v);
    const unsigned dead = dead_mask(v);
    // (workgroup_any and wave_list written out, one round at a time: the shared forms measured 0.2 - 1.3 % slower here)
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
            for (int w = 0; w < kSliceBlock / 64; ++w) {
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
            if (mine) sList[wave][total + lanes_below(b)] = k * kSliceTrip + 4 * (int)threadIdx.x + j;
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
    const SliceLaunch l = slice_launch(cell, n);
    if (!l.fits() || nDerived > (int64_t)INT32_MAX) return hipErrorInvalidValue;
    const int maskWords = (int)((nDerived + 31) / 32);
    const auto kernel = l.vec ? sink_kernel<true> : sink_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock), 0, st, cell, n, mask, (int)nDerived, maskWords, absorbed);
    return hipGetLastError();
}

size_t respawn_scratch_bytes(int64_t n) {
    const int64_t blocks = slice_launch(nullptr, n, kSpawnLoads).blocks;
    return (size_t)(blocks > 0 ? blocks : 1) * 2 * sizeof(unsigned);
}

hipError_t respawn_offsets(hipStream_t st, const int32_t* cell, int64_t n, int64_t maxCount, void* scratch, size_t scratchBytes,
                           const unsigned** offsets) {
    *offsets = nullptr;
    if (!(maxCount > 0 && maxCount < n)) return hipSuccess;     // (maxCount >= n cannot bind: the unlimited pass alone)
    if (scratchBytes < respawn_scratch_bytes(n)) return hipErrorInvalidValue;
    const SliceLaunch l = slice_launch(cell, n, kSpawnLoads);
    unsigned* counts = static_cast<unsigned*>(scratch);
    hipLaunchKernelGGL(respawn_count_kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock), 0, st, cell, n, l.vec ? 1 : 0, counts);
    hipLaunchKernelGGL(respawn_scan_kernel, dim3(1), dim3(kScanBlock), 0, st, counts, counts + l.blocks, (int)l.blocks);
    *offsets = counts + l.blocks;
    return hipGetLastError();
}

hipError_t respawn_box(hipStream_t st, double* x, double* y, double* z, int32_t* cell, const int64_t* gid, int64_t n,
                       const double lower[3], const double upper[3], int64_t maxCount, uint32_t seed, uint32_t epoch,
                       const MeshView& m, const GridView& g, void* scratch, size_t scratchBytes, unsigned long long* counters) {
    if (n <= 0 || maxCount == 0) return hipSuccess;
    if (n >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const SliceLaunch l = slice_launch(cell, n, kSpawnLoads);
    const int vec = l.vec ? 1 : 0;
    SpawnBox box;
    for (int k = 0; k < 3; ++k) { box.lower[k] = lower[k]; box.upper[k] = upper[k]; }
    const unsigned* offsets = nullptr;
    const hipError_t e = respawn_offsets(st, cell, n, maxCount, scratch, scratchBytes, &offsets);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(respawn_place_kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock), 0, st, x, y, z, cell, gid, n, vec, box, offsets,
                       maxCount, seed, epoch, m.cellOff, m.planes, g, counters);
    return hipGetLastError();
}

}  // namespace cpf
