// Per-cell occupancy (cpf_occupancy_sample*): acc[parent cell] += the number of entries of a cell array that claim it, one launch
// per sample, added in place into persistent 64-bit integer accumulators.  Integer sums do not depend on arrival order: the
// counts are the same bits whatever the order of the array and of the workgroups (DESIGN.md "Occupancy").
//
// Shape.  A workgroup takes one contiguous slice of kOccSlice ids with 16-byte loads, four ids per lane, and keeps it in registers;
// the derived -> parent map is applied as the ids arrive.  It finds the slice's [lo, hi] window of live ids:
//   - the window fits the LDS bins (a cell-sorted cloud: a slice spans a handful of cells): count into LDS -- a run of equal ids
//     in a wave is pre-counted with a ballot and costs one LDS atomic, as in cell_histogram_lds_kernel -- then flush the window
//     alone, lane = cell, contiguous 64-bit global adds, empty bins skipped;
//   - it does not (a cloud some cycles of diffusion past its sort on a 3-D mesh -- most of a slice in a narrow band of ids, a few
//     particles a whole row or layer of cells away --, a cloud sorted along the Morton curve, a sparse cloud over many cells, an
//     unsorted array): the bins become a direct-mapped cache of kOccTagBins (count, cell) pairs, bin = id modulo kOccTagBins.
//     A run claims its bin if it is free or holds the same cell; a run that finds its bin taken by another cell adds to global
//     memory itself, one add per run per wave.  The flush walks the bins: neighbouring ids sit in neighbouring bins, so the
//     band still leaves as contiguous adds.
// Nothing is staged in global memory: no per-block table, no scratch that grows with the mesh or the grid.
#include <hip/hip_runtime.h>

#include "cpf_device.h"

namespace cpf {
namespace {

constexpr int kOccBlock = 256;                              // 4 waves
constexpr int kOccLoads = 4;                                // 16-byte loads in flight per lane
constexpr int kOccTrip = kOccBlock * 4;                     // ids one round of loads covers
constexpr int kOccSlice = kOccTrip * kOccLoads;             // ids per workgroup
constexpr int kOccBins = 4096;                              // u32 LDS bins: 16 KB per workgroup (a bin holds at most kOccSlice)
constexpr int kOccTagBins = kOccBins / 2;                   // the same words as a cache: counts in the lower half, cell ids in the upper
static_assert((kOccTagBins & (kOccTagBins - 1)) == 0, "bin = id & (kOccTagBins - 1)");

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

// the four ids of one load: where every lane's four agree (the rule in a sorted cloud) they are counted once with weight 4
template <int kRounds, class Add>
__device__ inline void count_quad(const int4& q, int lane, Add add) {
    const bool mixed = !(q.x == q.y && q.y == q.z && q.z == q.w);
    if (__ballot(mixed) == 0ull) {
        count_runs<kRounds>(q.x, 4u, lane, add);
    } else {
        count_runs<kRounds>(q.x, 1u, lane, add);
        count_runs<kRounds>(q.y, 1u, lane, add);
        count_runs<kRounds>(q.z, 1u, lane, add);
        count_runs<kRounds>(q.w, 1u, lane, add);
    }
}

}  // namespace

// (outside the anonymous namespace, like the step kernels: tools/resource_usage.py lists kernels by their plain names)
// kVec: `cell` is 16-byte aligned (a slice starts at a multiple of kOccSlice ids, so every full quad is one aligned load)
template <bool kVec>
__global__ __launch_bounds__(kOccBlock) void occupancy_kernel(const int32_t* __restrict__ cell, int64_t n,
                                                              const int32_t* __restrict__ parentOf, int nDerived,
                                                              unsigned long long* __restrict__ acc) {
    __shared__ unsigned sBins[kOccBins];
    __shared__ int sLo[kOccBlock / 64], sHi[kOccBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * kOccSlice + 4 * (int64_t)threadIdx.x;
    int4 v[kOccLoads];
#pragma unroll
    for (int k = 0; k < kOccLoads; ++k) {
        const int64_t i = base + (int64_t)k * kOccTrip;
        if (kVec && i + 3 < n) {
            v[k] = *reinterpret_cast<const int4*>(cell + i);
        } else {
            v[k].x = (i < n) ? cell[i] : -1;
            v[k].y = (i + 1 < n) ? cell[i + 1] : -1;
            v[k].z = (i + 2 < n) ? cell[i + 2] : -1;
            v[k].w = (i + 3 < n) ? cell[i + 3] : -1;
        }
    }
    // derived -> parent; CPF_CELL_LOST, every other negative code and ids beyond the mesh become -1: not counted
    auto live = [&](int c) -> int {
        if ((unsigned)c >= (unsigned)nDerived) return -1;
        return parentOf ? parentOf[c] : c;
    };
    unsigned lo = 0xFFFFFFFFu;                                  // (a negative id is a huge unsigned: the minimum skips it)
    int hi = -1;
#pragma unroll
    for (int k = 0; k < kOccLoads; ++k) {
        v[k].x = live(v[k].x); v[k].y = live(v[k].y); v[k].z = live(v[k].z); v[k].w = live(v[k].w);
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
    for (int w = 0; w < kOccBlock / 64; ++w) {
        lo = min(lo, (unsigned)sLo[w]);
        hi = max(hi, sHi[w]);
    }
    if (hi < 0) return;                                         // no live id in the slice (the whole workgroup leaves)
    const int first = (int)lo, width = hi - first + 1;
    if (width <= kOccBins) {
        for (int b = threadIdx.x; b < width; b += kOccBlock) sBins[b] = 0u;
        __syncthreads();
        auto add = [&](int c, unsigned w) { atomicAdd(&sBins[c - first], w); };
#pragma unroll
        for (int k = 0; k < kOccLoads; ++k) count_quad<2>(v[k], lane, add);
        __syncthreads();
        for (int b = threadIdx.x; b < width; b += kOccBlock) {
            const unsigned k = sBins[b];
            if (k != 0u) atomicAdd(&acc[first + b], (unsigned long long)k);
        }
    } else {
        unsigned* sCount = sBins;
        int* sTag = reinterpret_cast<int*>(sBins + kOccTagBins);
        for (int b = threadIdx.x; b < kOccTagBins; b += kOccBlock) { sCount[b] = 0u; sTag[b] = -1; }
        __syncthreads();
        auto add = [&](int c, unsigned w) {
            const int b = c & (kOccTagBins - 1);
            const int held = atomicCAS(&sTag[b], -1, c);
            if (held == -1 || held == c) atomicAdd(&sCount[b], w);
            else atomicAdd(&acc[c], (unsigned long long)w);
        };
#pragma unroll
        for (int k = 0; k < kOccLoads; ++k) count_quad<2>(v[k], lane, add);
        __syncthreads();
        for (int b = threadIdx.x; b < kOccTagBins; b += kOccBlock) {
            const unsigned k = sCount[b];
            if (k != 0u) atomicAdd(&acc[sTag[b]], (unsigned long long)k);
        }
    }
}

hipError_t occupancy_accumulate(hipStream_t st, const int32_t* cell, int64_t n, const int32_t* parentOf, int64_t nDerived,
                                unsigned long long* acc) {
    if (n <= 0) return hipSuccess;
    const int64_t blocks = (n + kOccSlice - 1) / kOccSlice;
    if (blocks > (int64_t)INT32_MAX || nDerived > (int64_t)INT32_MAX) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(cell) & 15u) == 0)
        hipLaunchKernelGGL(occupancy_kernel<true>, dim3((unsigned)blocks), dim3(kOccBlock), 0, st, cell, n, parentOf, (int)nDerived, acc);
    else
        hipLaunchKernelGGL(occupancy_kernel<false>, dim3((unsigned)blocks), dim3(kOccBlock), 0, st, cell, n, parentOf, (int)nDerived, acc);
    return hipGetLastError();
}

}  // namespace cpf
