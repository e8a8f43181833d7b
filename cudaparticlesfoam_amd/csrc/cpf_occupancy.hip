// Per-cell occupancy (cpf_occupancy_sample*): acc[parent cell] += the number of entries of a cell array that claim it, one launch
// per sample, added in place into persistent 64-bit integer accumulators.  Integer sums do not depend on arrival order: the
// counts are the same bits whatever the order of the array and of the workgroups (DESIGN.md "Occupancy").
//
// The pass is cpf_slice.h's: a slice of ids per workgroup, the window [lo, hi] of its live ids, 32-bit LDS bins over the window
// or, for a window wider than the bins (a cloud some cycles of diffusion past its sort on a 3-D mesh -- most of a slice in a
// narrow band of ids, a few particles a whole row or layer of cells away --, a cloud sorted along the Morton curve, a sparse cloud
// over many cells, an unsorted array), as a cache of (count, cell) pairs.  What is occupancy's own: the derived -> parent map
// applied as the ids arrive, and the count -- a run of equal ids in a wave is pre-counted with a ballot and costs one LDS atomic,
// one add per run per wave where a run goes to global memory itself.
// Nothing is staged in global memory: no per-block table, no scratch that grows with the mesh or the grid.
#include <hip/hip_runtime.h>

#include "cpf_device.h"
#include "cpf_slice.h"

namespace cpf {
namespace {

constexpr int kOccBins = 4096;                              // u32 LDS bins: 16 KB per workgroup (a bin holds at most a slice's ids)

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
// kVec: `cell` is 16-byte aligned
template <bool kVec>
__global__ __launch_bounds__(kSliceBlock) void occupancy_kernel(const int32_t* __restrict__ cell, int64_t n,
                                                                const int32_t* __restrict__ parentOf, int nDerived,
                                                                unsigned long long* __restrict__ acc) {
    const int lane = threadIdx.x & 63;
    int4 v[kSliceLoads];
    load_slice(cell, n, kVec, -1, v);
    // derived -> parent; CPF_CELL_LOST, every other negative code and ids beyond the mesh become -1: not counted
    auto live = [&](int c) -> int {
        if ((unsigned)c >= (unsigned)nDerived) return -1;
        return parentOf ? parentOf[c] : c;
    };
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k) {
        v[k].x = live(v[k].x); v[k].y = live(v[k].y); v[k].z = live(v[k].z); v[k].w = live(v[k].w);
    }
    int first;
    const int last = slice_window(v, first);
    if (last < 0) return;                                   // no live id in the slice (the whole workgroup leaves)
    window_bins<unsigned, kOccBins>(
        first, last,
        [&](auto add) {
#pragma unroll
            for (int k = 0; k < kSliceLoads; ++k) count_quad<2>(v[k], lane, add);
        },
        [&](int c, unsigned k) { atomicAdd(&acc[c], (unsigned long long)k); });
}

hipError_t occupancy_accumulate(hipStream_t st, const int32_t* cell, int64_t n, const int32_t* parentOf, int64_t nDerived,
                                unsigned long long* acc) {
    if (n <= 0) return hipSuccess;
    const SliceLaunch l = slice_launch(cell, n);
    if (!l.fits() || nDerived > (int64_t)INT32_MAX) return hipErrorInvalidValue;
    const auto kernel = l.vec ? occupancy_kernel<true> : occupancy_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock), 0, st, cell, n, parentOf, (int)nDerived, acc);
    return hipGetLastError();
}

}  // namespace cpf
