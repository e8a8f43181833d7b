// Patch source (cpf_respawn_source*): a dead slot is respawned on a triangulated surface instead of in a box (cpf_recycle.hip).
// The candidates, their order, the limited path and the counters are respawn_place_kernel's, and so is the shape of the pass:
// a slice of kSpawnSlice ids per workgroup, a workgroup without a dead slot leaves after its loads, a wave gathers its chosen
// slots into its LDS list and the lanes take one each.  What is new is the draw (cpf_philox.h: source_words, source_point): word 0
// of a slot's Philox block picks a triangle through the table's bounds hi[], and the triangle's 128-byte record gives the point.
//   - Bounds of at most kSourceLdsBounds entries are staged in LDS once a workgroup knows that it has a dead slot; the loads are
//     issued before the ballots that rank the slots.  The search is a branch-free lower bound of 12 steps on LDS.
//   - A larger table is searched in global memory (source_pick: the upper levels of the search stay in L2).
//   - A lane reads its record as eight 16-byte loads, all in flight before the first use.
#include <hip/hip_runtime.h>

#include "cpf_device.h"
#include "cpf_locate.h"
#include "cpf_philox.h"
#include "cpf_slice.h"

namespace cpf {

constexpr int kSourceLdsBounds = 4096;                      // bounds staged in LDS: 16 KB
constexpr int kSourceLdsSteps = 12;                         // 2^12 == kSourceLdsBounds
constexpr int kSourceStageLoads = kSourceLdsBounds / (4 * kSliceBlock);     // 16-byte loads per lane that stage them

// counters: [0] absorbed (the sink's), [1] drawn, [2] placed
__global__ __launch_bounds__(kSliceBlock) void inlet_place_kernel(double* __restrict__ x, double* __restrict__ y, double* __restrict__ z,
                                                                  int32_t* __restrict__ cell, const int64_t* __restrict__ gid, int64_t n,
                                                                  int vec, const double2* __restrict__ rec,
                                                                  const uint32_t* __restrict__ hi, int nKept,
                                                                  const unsigned* __restrict__ offsets, int64_t maxCount, uint32_t seed,
                                                                  uint32_t epoch, const int32_t* __restrict__ cellOff,
                                                                  const double4* __restrict__ planes, GridView g,
                                                                  unsigned long long* __restrict__ counters) {
    __shared__ uint32_t sHi[kSourceLdsBounds];                  // the staged bounds
    __shared__ unsigned sWave[kSpawnLoads][kSliceBlock / 64];   // dead slots per (round of loads, wave): the ranks of a limited respawn
    __shared__ int sList[kSliceBlock / 64][256];                // per wave: the chosen slots of one round (at most 4 per lane)
    __shared__ unsigned sDrawn, sPlaced, sAny;
    // the grid goes through LDS: as kernel arguments it would sit in scalar registers across the locate's loops
    __shared__ GridView sGrid;
    const bool limited = offsets != nullptr;
    const int64_t first = limited ? (int64_t)offsets[blockIdx.x] : 0;
    if (limited && first >= maxCount) return;               // (the whole workgroup: nothing of this slice is chosen)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t blockBase = (int64_t)blockIdx.x * kSpawnSlice;
    int4 v[kSpawnLoads];
    load_slice(cell, n, vec != 0, 0, v);
    const unsigned dead = dead_mask(v);
    if (threadIdx.x == 0) { sDrawn = 0u; sPlaced = 0u; sAny = 0u; }
    __syncthreads();
    const unsigned long long anyDead = __ballot(dead != 0u);
    if (lane == 0 && anyDead != 0ull) sAny = 1u;
    __syncthreads();
    if (sAny == 0u) return;                                 // (the whole workgroup: no dead slot in the slice)
    // the bounds' loads go out now and land in LDS behind the ballots (hi is padded to a multiple of 4 entries)
    const bool staged = nKept <= kSourceLdsBounds;
    uint4 h[kSourceStageLoads];
#pragma unroll
    for (int k = 0; k < kSourceStageLoads; ++k) {
        const int i = 4 * ((int)threadIdx.x + k * kSliceBlock);
        h[k] = make_uint4(0u, 0u, 0u, 0u);
        if (staged && i < nKept) h[k] = *reinterpret_cast<const uint4*>(hi + i);
    }
    if (threadIdx.x == 0) sGrid = g;
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
    if (staged) {
#pragma unroll
        for (int k = 0; k < kSourceStageLoads; ++k) {
            const int i = 4 * ((int)threadIdx.x + k * kSliceBlock);
            if (i < nKept) *reinterpret_cast<uint4*>(sHi + i) = h[k];
        }
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
    const int lastKept = nKept - 1;
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
            uint32_t c[4];
            source_words(seed, (uint64_t)(gid ? gid[s] : s), epoch, c);
            int tri;
            if (staged) {
                // first index with c[0] <= sHi[index]: entries past the table read as its last one, 0xFFFFFFFF, which is never below
                tri = 0;
#pragma unroll
                for (int step = kSourceLdsBounds >> 1, i = 0; i < kSourceLdsSteps; ++i, step >>= 1) {
                    const int probe = tri + step - 1;
                    const uint32_t bound = sHi[probe < lastKept ? probe : lastKept];
                    tri += bound < c[0] ? step : 0;
                }
            } else {
                tri = source_pick(hi, nKept, c[0]);
            }
            const double2* __restrict__ r = rec + (int64_t)tri * (kSourceDoubles / 2);
            double2 q[kSourceDoubles / 2];
#pragma unroll
            for (int i = 0; i < kSourceDoubles / 2; ++i) q[i] = r[i];
            double record[kSourceDoubles];
#pragma unroll
            for (int i = 0; i < kSourceDoubles / 2; ++i) { record[2 * i] = q[i].x; record[2 * i + 1] = q[i].y; }
            double p[3];
            source_point(c, record, p);
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

hipError_t respawn_source(hipStream_t st, double* x, double* y, double* z, int32_t* cell, const int64_t* gid, int64_t n,
                          const SourceView& src, int64_t maxCount, uint32_t seed, uint32_t epoch, const MeshView& m,
                          const GridView& g, void* scratch, size_t scratchBytes, unsigned long long* counters) {
    if (n <= 0 || maxCount == 0) return hipSuccess;
    if (n >= ((int64_t)1 << 31) || src.nKept <= 0 || !src.rec || !src.hi) return hipErrorInvalidValue;
    const SliceLaunch l = slice_launch(cell, n, kSpawnLoads);
    const unsigned* offsets = nullptr;
    const hipError_t e = respawn_offsets(st, cell, n, maxCount, scratch, scratchBytes, &offsets);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(inlet_place_kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock), 0, st, x, y, z, cell, gid, n, l.vec ? 1 : 0,
                       reinterpret_cast<const double2*>(src.rec), src.hi, (int)src.nKept, offsets, maxCount, seed, epoch, m.cellOff,
                       m.planes, g, counters);
    return hipGetLastError();
}

}  // namespace cpf
