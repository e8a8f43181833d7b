// Tracer age (cpf_age_*): how long a particle of a recycled cloud has been live, without touching a step kernel, the sort or the
// recycling kernels.  birth[id] is a 32-bit stamp per PARTICLE ID -- the context's cycle counter when id last became live --, so
// neither sort moves it; an age is (uint32_t)(now - birth[id]), in cycles, and everything summed here is an integer: the same bits
// whatever the order of the cloud and of the workgroups (DESIGN.md "Age").  The three kernels are passes of cpf_slice.h; what is
// written here is what they do per particle.
//
// Absorb (age_absorb_kernel).  sink_pass plus the residence-time histogram.  A workgroup without a hit ends where sink_kernel
// ends.  Otherwise the hits of a wave are gathered into a list in LDS and the wave's lanes take them in turn, as
// respawn_place_kernel's do -- eight a lane at a time, every gid load and then every birth gather of a batch in flight before the
// first is used: the sink's cells are neighbours in a sorted cloud, so a few workgroups hold all the hits and their chain of
// dependent loads is the kernel's tail.  Per hit: gid[s], birth[gid], the bin, one add to a histogram of 32-bit bins in LDS (a
// slice has at most kAgeSlice hits).  Non-zero bins leave as 64-bit global adds.
//
// Stamp (age_stamp_kernel).  Before a respawn: birth[gid[s]] = now for every slot with cell < 0.  A slot the respawn leaves dead has
// no age and is stamped again before it can next become live.  A workgroup without a dead slot leaves after its loads; the dead of
// a wave go through the same list, so a run of dead slots reads its ids with consecutive lanes.
//
// Field (age_field_kernel).  slice_window and window_bins over the parents of the slice's live ids.  Every lane's gid loads and
// birth gathers are all issued before the first is used (16 gathers in flight per lane).  A bin is ONE 64-bit word,
// count << kAgeCountShift | age sum: a slice holds at most 2^12 particles of age < 2^32, so the sum stays below 2^44 and the count
// below 2^20 -- one LDS atomic per add, and no carry from the sum into the count.
#include <hip/hip_runtime.h>

#include "cpf_device.h"
#include "cpf_slice.h"

namespace cpf {
namespace {

constexpr int kAgeSlice = slice_ids(kSliceLoads);           // ids per workgroup
constexpr int kAgeMaxBins = 4096;                           // residence-time bins (cpf_age_enable's limit): 16 KB of dynamic LDS at most
constexpr int kAgeBatch = 8;                                // list entries a lane takes at a time
constexpr int kAgeBins = 2048;                              // 64-bit field bins in LDS: 16 KB per workgroup
constexpr int kAgeCountShift = 44;                          // a bin: count << 44 | age sum
static_assert(kAgeSlice <= (1 << 12), "a bin's age sum must stay below 2^44: at most 2^12 ages below 2^32");

// The wave's lanes take the entries of a wave_list kAgeBatch each at a time: f(ids, ok) gets the particle ids of the lane's
// entries (ok[b] false: no entry, or an id that is none of this cloud's -- ids[b] is 0 then, a valid index).  Every load of a batch
// is issued before the first is used: a slice where everybody is listed costs two passes of dependent loads, not sixteen.
template <class F>
__device__ inline void wave_take(const unsigned short* __restrict__ list, unsigned total, int64_t blockBase,
                                 const int64_t* __restrict__ gid, int64_t n, int lane, F f) {
#pragma unroll 1
    for (unsigned t0 = 0; t0 < total; t0 += 64 * kAgeBatch) {
        uint64_t ids[kAgeBatch];
        bool ok[kAgeBatch];
#pragma unroll
        for (int b = 0; b < kAgeBatch; ++b) {
            const unsigned t = t0 + 64 * b + lane;
            const int64_t s = blockBase + list[t < total ? t : 0];      // (entry 0 exists: total > 0)
            const uint64_t id = (uint64_t)(gid ? gid[s] : s);
            ok[b] = t < total && id < (uint64_t)n;
            ids[b] = ok[b] ? id : 0ull;
        }
        f(ids, ok);
    }
}

}  // namespace

// (outside the anonymous namespace, like the step kernels: tools/resource_usage.py lists kernels by their plain names)
// `cell` is 16-byte aligned (the context's own arrays are: the age entries have no _dev form).  Dynamic LDS: nBins 32-bit bins
__global__ __launch_bounds__(kSliceBlock) void age_absorb_kernel(int32_t* __restrict__ cell, const int64_t* __restrict__ gid,
                                                                 const uint32_t* __restrict__ birth, int64_t n,
                                                                 const uint32_t* __restrict__ mask, int nDerived, int maskWords,
                                                                 unsigned long long* __restrict__ absorbed, uint32_t now,
                                                                 uint32_t binCycles, int nBins, unsigned long long* __restrict__ hist) {
    extern __shared__ unsigned sHist[];
    __shared__ unsigned short sList[kSliceBlock / 64][kAgeSlice / 4];   // per wave: its hits (at most 16 per lane), slots within the slice
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned hit;
    const unsigned all = sink_pass<true, true>(cell, n, mask, nDerived, maskWords, hit);
    if (all == 0u) return;                                  // (the whole workgroup: sink_kernel's pass, nothing more)
    if (threadIdx.x == 0) atomicAdd(absorbed, (unsigned long long)all);
    for (int b = threadIdx.x; b < nBins; b += kSliceBlock) sHist[b] = 0u;
    const unsigned total = wave_list<kSliceLoads>(hit, sList[wave]);
    __syncthreads();
    wave_take(sList[wave], total, (int64_t)blockIdx.x * kAgeSlice, gid, n, lane, [&](const uint64_t* ids, const bool* ok) {
        uint32_t born[kAgeBatch];
#pragma unroll
        for (int b = 0; b < kAgeBatch; ++b) born[b] = birth[ids[b]];
#pragma unroll
        for (int b = 0; b < kAgeBatch; ++b)
            if (ok[b]) atomicAdd(&sHist[min((uint32_t)(now - born[b]) / binCycles, (uint32_t)(nBins - 1))], 1u);
    });
    __syncthreads();
    for (int b = threadIdx.x; b < nBins; b += kSliceBlock) {
        const unsigned k = sHist[b];
        if (k != 0u) atomicAdd(&hist[b], (unsigned long long)k);
    }
}

__global__ __launch_bounds__(kSliceBlock) void age_stamp_kernel(const int32_t* __restrict__ cell, const int64_t* __restrict__ gid,
                                                                uint32_t* __restrict__ birth, int64_t n, uint32_t now) {
    __shared__ unsigned short sList[kSliceBlock / 64][kAgeSlice / 4];   // per wave: its dead slots (at most 16 per lane)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int4 v[kSliceLoads];
    load_slice(cell, n, true, 0, v);
    const unsigned dead = dead_mask(v);
    if (!workgroup_any(dead != 0u)) return;                 // (the whole workgroup: no dead slot in the slice)
    const unsigned total = wave_list<kSliceLoads>(dead, sList[wave]);
    __syncthreads();
    wave_take(sList[wave], total, (int64_t)blockIdx.x * kAgeSlice, gid, n, lane, [&](const uint64_t* ids, const bool* ok) {
#pragma unroll
        for (int b = 0; b < kAgeBatch; ++b)
            if (ok[b]) birth[ids[b]] = now;
    });
}

// `cell` is 16-byte aligned
__global__ __launch_bounds__(kSliceBlock) void age_field_kernel(const int32_t* __restrict__ cell, const int64_t* __restrict__ gid,
                                                                const uint32_t* __restrict__ birth, int64_t n,
                                                                const int32_t* __restrict__ parentOf, int nDerived, uint32_t now,
                                                                unsigned long long* __restrict__ field) {
    const int64_t base = slice_base<kSliceLoads>();
    int4 v[kSliceLoads];
    load_slice(cell, n, true, -1, v);
    // the ids: gid is 8-byte elements behind a 256-byte aligned allocation or a caller's array -- plain 8-byte loads, four
    // consecutive per lane; past the end and ids that are none of this cloud's: id 0 (their slot is not live, see below)
    uint32_t id[kSliceLoads][4];
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t s = base + (int64_t)k * kSliceTrip + j;
            const uint64_t g = s < n ? (uint64_t)(gid ? gid[s] : s) : 0ull;
            id[k][j] = g < (uint64_t)n ? (uint32_t)g : 0xFFFFFFFFu;     // (n < 2^31)
        }
    uint32_t age[kSliceLoads][4];
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) age[k][j] = now - birth[id[k][j] != 0xFFFFFFFFu ? id[k][j] : 0u];
    // derived -> parent; CPF_CELL_LOST, every other negative code, ids beyond the mesh and slots without an id of this cloud become -1
    auto live = [&](int c, uint32_t i) -> int {
        if ((unsigned)c >= (unsigned)nDerived || i == 0xFFFFFFFFu) return -1;
        return parentOf ? parentOf[c] : c;
    };
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k) {
        v[k].x = live(v[k].x, id[k][0]); v[k].y = live(v[k].y, id[k][1]); v[k].z = live(v[k].z, id[k][2]); v[k].w = live(v[k].w, id[k][3]);
    }
    int first;
    const int last = slice_window(v, first);
    if (last < 0) return;                                   // no live id in the slice (the whole workgroup leaves)
    constexpr unsigned long long kOne = 1ull << kAgeCountShift, kSumMask = kOne - 1ull;
    window_bins<unsigned long long, kAgeBins>(
        first, last,
        // a lane's four ids: where they agree (the rule in a sorted cloud) one add carries all four
        [&](auto add) {
#pragma unroll
            for (int k = 0; k < kSliceLoads; ++k) {
                const int4& q = v[k];
                const uint32_t* a = age[k];
                if (q.x >= 0 && q.x == q.y && q.y == q.z && q.z == q.w) {
                    add(q.x, 4ull * kOne + ((unsigned long long)a[0] + a[1] + a[2] + a[3]));
                } else {
                    if (q.x >= 0) add(q.x, kOne + a[0]);
                    if (q.y >= 0) add(q.y, kOne + a[1]);
                    if (q.z >= 0) add(q.z, kOne + a[2]);
                    if (q.w >= 0) add(q.w, kOne + a[3]);
                }
            }
        },
        [&](int c, unsigned long long w) {
            atomicAdd(&field[2 * (size_t)c], w & kSumMask);
            atomicAdd(&field[2 * (size_t)c + 1], w >> kAgeCountShift);
        });
}

// (every launcher: `cell` must be 16-byte aligned, as the arrays of the context's own cloud are)
hipError_t age_absorb(hipStream_t st, int32_t* cell, const int64_t* gid, const uint32_t* birth, int64_t n, const uint32_t* mask,
                      int64_t nDerived, unsigned long long* absorbed, uint32_t now, int32_t binCycles, int32_t nBins,
                      unsigned long long* hist) {
    if (n <= 0) return hipSuccess;
    const SliceLaunch l = slice_launch(cell, n);
    if (!l.fits() || !l.vec || nDerived > (int64_t)INT32_MAX || binCycles < 1 || nBins < 1 || nBins > kAgeMaxBins)
        return hipErrorInvalidValue;
    const int maskWords = (int)((nDerived + 31) / 32);
    hipLaunchKernelGGL(age_absorb_kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock), (size_t)nBins * sizeof(unsigned), st, cell, gid,
                       birth, n, mask, (int)nDerived, maskWords, absorbed, now, (uint32_t)binCycles, (int)nBins, hist);
    return hipGetLastError();
}

hipError_t age_stamp(hipStream_t st, const int32_t* cell, const int64_t* gid, uint32_t* birth, int64_t n, uint32_t now) {
    if (n <= 0) return hipSuccess;
    const SliceLaunch l = slice_launch(cell, n);
    if (!l.fits() || !l.vec) return hipErrorInvalidValue;
    hipLaunchKernelGGL(age_stamp_kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock), 0, st, cell, gid, birth, n, now);
    return hipGetLastError();
}

hipError_t age_field(hipStream_t st, const int32_t* cell, const int64_t* gid, const uint32_t* birth, int64_t n,
                     const int32_t* parentOf, int64_t nDerived, uint32_t now, unsigned long long* field) {
    if (n <= 0) return hipSuccess;
    const SliceLaunch l = slice_launch(cell, n);
    if (n >= ((int64_t)1 << 31) || nDerived > (int64_t)INT32_MAX || !l.vec) return hipErrorInvalidValue;
    hipLaunchKernelGGL(age_field_kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock), 0, st, cell, gid, birth, n, parentOf, (int)nDerived,
                       now, field);
    return hipGetLastError();
}

}  // namespace cpf
