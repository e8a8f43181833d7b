// Exposure (cpf_exposure_*): what a particle of the context's own cloud accumulated on its way -- the integral of a cell field
// along its path -- and the distribution of that dose over the particles the sink absorbs, without touching a step kernel, the
// sort, the recycling kernels or the age, tag and route kernels.  dose[id] is one double per PARTICLE ID, so neither sort moves
// it; rate[d] is one double per DERIVED cell, the caller's field over the mesh as given, expanded on the host when it is set: one
// gather a particle, not parentOf and then the field.  Every id sits in exactly one slot, so dose[id] sees exactly one add a
// call, in call order, whatever the order of the cloud and of the workgroups: the same bits as numpy, without an atomic
// (DESIGN.md "Exposure").  The three kernels are passes of cpf_slice.h; what is written here is what they do per particle.
//
// Accumulate (exposure_accumulate_kernel).  dose[gid[s]] += scale * rate[cell[s]] for every live slot.  The slice with 16-byte
// loads, the ids alongside with 16-byte loads of two (gid is an allocation of the context's, so a quad of ids is 32-byte
// aligned), then all sixteen rate gathers of a lane, then -- for the elements whose rate is not zero only -- all dose loads, the
// adds, the stores.  An element whose rate is exactly 0 would add +0.0 to a dose that is never -0.0, the same bits: it touches no
// dose word.  A workgroup with no live slot, or with every rate zero (a zone field: all but the zone's few), leaves behind its
// loads and gathers.
//
// Absorb (exposure_absorb_kernel).  A READ-ONLY pass in front of whichever pass marks the absorbed (tag_transfer_kernel's place
// and shape): the slice, the sink's mask (staged in LDS up to kSinkLdsWords words, through L2 beyond), and a workgroup without a
// hit leaves.  Otherwise the hits of a wave go into a list in LDS and the wave's lanes take them in batches of kDoseBatch: every
// gid and cell load of a batch, then every dose[gid], origin[gid] and sinkGroup[cell] gather, in flight before the first use.
// Per hit one add to doseHist[origin][group][exposure_bin(dose)], 32-bit words in dynamic LDS (a slice has at most kDoseSlice
// hits; at most kDoseWords words, 16 KB); non-zero words leave as 64-bit global adds.  Without tagging origin and sinkGroup are
// null and both indices 0.
//
// Stamp (exposure_stamp_kernel).  age_stamp_kernel storing a double: before a respawn, dose[gid[s]] = +0.0 for every slot with
// cell < 0.
#include <hip/hip_runtime.h>

#include "cpf_device.h"
#include "cpf_exposure_bins.h"
#include "cpf_slice.h"

namespace cpf {
namespace {

constexpr int kDoseSlice = slice_ids(kSliceLoads);          // ids per workgroup
constexpr int kDoseMax = 16;                                // origins, and sink groups, at most (cpf_tag_enable's limit)
constexpr int kDoseWords = 4096;                            // histogram words at most (cpf_exposure_enable's limit): 16 KB of dynamic LDS
constexpr int kDoseBatch = 8;                               // list entries a lane takes at a time
constexpr uint32_t kNoId = 0xFFFFFFFFu;                     // a slot past the end, or one whose id is none of this cloud's
static_assert(kDoseSlice <= 0xFFFF + 1, "a list entry is a 16-bit slot within the slice");

// the ids of the quad of slots at s (a multiple of 4), as 32-bit numbers (n < 2^31): two 16-byte loads where the quad is whole
// (gid is 32-byte aligned there), 8-byte loads at the ragged end; gid null: the slots themselves
__device__ inline void load_ids(const int64_t* __restrict__ gid, int64_t s, int64_t n, uint32_t (&id)[4]) {
    uint64_t g[4];
    if (gid && s + 3 < n) {
        const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(gid + s), b = *reinterpret_cast<const ulonglong2*>(gid + s + 2);
        g[0] = a.x; g[1] = a.y; g[2] = b.x; g[3] = b.y;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = s + j < n ? (uint64_t)(gid ? gid[s + j] : s + j) : ~0ull;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) id[j] = g[j] < (uint64_t)n ? (uint32_t)g[j] : kNoId;
}

// The wave's lanes take the entries of a wave_list kDoseBatch each at a time: f(slots, ids, ok) gets the array slots and particle
// ids of the lane's entries (ok[b] false: no entry, or an id that is none of this cloud's -- slot and id are valid indices all the
// same).  Every gid load of a batch is issued before f runs.  (tag_take's shape, written again here: the existing kernel files
// keep their text.)
template <class F>
__device__ inline void dose_take(const unsigned short* __restrict__ list, unsigned total, int64_t blockBase,
                                 const int64_t* __restrict__ gid, int64_t n, int lane, F f) {
#pragma unroll 1
    for (unsigned t0 = 0; t0 < total; t0 += 64 * kDoseBatch) {
        int64_t slots[kDoseBatch];
        uint64_t ids[kDoseBatch];
        bool ok[kDoseBatch];
#pragma unroll
        for (int b = 0; b < kDoseBatch; ++b) {
            const unsigned t = t0 + 64 * b + lane;
            const int64_t s = blockBase + list[t < total ? t : 0];      // (entry 0 exists: total > 0)
            const uint64_t id = (uint64_t)(gid ? gid[s] : s);
            slots[b] = s;
            ok[b] = t < total && id < (uint64_t)n;
            ids[b] = ok[b] ? id : 0ull;
        }
        f(slots, ids, ok);
    }
}

}  // namespace

// (outside the anonymous namespace, like the step kernels: tools/resource_usage.py lists kernels by their plain names)
// `cell`, `gid` are the context's own arrays (16-byte aligned: the exposure entries have no _dev form); rate has nDerived entries,
// dose n.  No atomics: every id is in one slot.
__global__ __launch_bounds__(kSliceBlock) void exposure_accumulate_kernel(const int32_t* __restrict__ cell,
                                                                          const int64_t* __restrict__ gid,
                                                                          const double* __restrict__ rate,
                                                                          double* __restrict__ dose, int64_t n, int nDerived,
                                                                          double scale) {
    const int64_t base = slice_base<kSliceLoads>();
    int4 v[kSliceLoads];
    uint32_t id[kSliceLoads][4];
    // A slice that lies within the cloud -- every one but the last, the same answer in the whole workgroup -- takes load_slice's
    // and load_ids' 16-byte loads without their test for the ragged end: that test differs from lane to lane, so the compiler
    // joins its two sides quad by quad and waits for one quad's loads before it issues the next one's (eight round trips in a
    // row, seen in the listing); behind a branch that the whole workgroup takes alike all twelve loads are in flight together
    if (((int64_t)blockIdx.x + 1) * kDoseSlice <= n) {
#pragma unroll
        for (int k = 0; k < kSliceLoads; ++k) v[k] = *reinterpret_cast<const int4*>(cell + base + (int64_t)k * kSliceTrip);
#pragma unroll
        for (int k = 0; k < kSliceLoads; ++k) {
            const int64_t s = base + (int64_t)k * kSliceTrip;
            uint64_t g[4] = {(uint64_t)s, (uint64_t)s + 1, (uint64_t)s + 2, (uint64_t)s + 3};
            if (gid) {
                const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(gid + s), b = *reinterpret_cast<const ulonglong2*>(gid + s + 2);
                g[0] = a.x; g[1] = a.y; g[2] = b.x; g[3] = b.y;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) id[k][j] = g[j] < (uint64_t)n ? (uint32_t)g[j] : kNoId;
        }
    } else {
        load_slice(cell, n, true, -1, v);
#pragma unroll
        for (int k = 0; k < kSliceLoads; ++k) load_ids(gid, base + (int64_t)k * kSliceTrip, n, id[k]);
    }
    // every gather of the lane: CPF_CELL_LOST, every other negative code, ids beyond the mesh and slots past the end read cell 0,
    // a load that is there to be in flight
    double r[kSliceLoads][4];
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k) {
        const int c[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) r[k][j] = rate[(unsigned)c[j] < (unsigned)nDerived ? c[j] : 0];
    }
    // bit 4 k + j: element j of quad k is live, has an id of this cloud and a rate that is not zero
    unsigned nz = 0u;
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k) {
        const int c[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            nz |= ((unsigned)c[j] < (unsigned)nDerived && id[k][j] != kNoId && r[k][j] != 0.0 ? 1u : 0u) << (4 * k + j);
    }
    if (!workgroup_any(nz != 0u)) return;                   // (the whole workgroup: nothing to add in the slice)
    double d[kSliceLoads][4];
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((nz >> (4 * k + j)) & 1u) d[k][j] = dose[id[k][j]];
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((nz >> (4 * k + j)) & 1u) d[k][j] = d[k][j] + scale * r[k][j];
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((nz >> (4 * k + j)) & 1u) dose[id[k][j]] = d[k][j];
}

// Nothing of the cloud is written.  origin, sinkGroup null: no tagging, origin and group 0.  Dynamic LDS: nOrigins * nSinks * nBins
// 32-bit words
__global__ __launch_bounds__(kSliceBlock) void exposure_absorb_kernel(const int32_t* __restrict__ cell, const int64_t* __restrict__ gid,
                                                                      const double* __restrict__ dose,
                                                                      const uint8_t* __restrict__ origin, int64_t n,
                                                                      const uint32_t* __restrict__ mask, int nDerived, int maskWords,
                                                                      const uint8_t* __restrict__ sinkGroup, double invWidth,
                                                                      int nBins, int nOrigins, int nSinks,
                                                                      unsigned long long* __restrict__ hist) {
    extern __shared__ unsigned sDose[];                                 // [nOrigins][nSinks][nBins]
    __shared__ uint32_t sMask[kSinkLdsWords];
    __shared__ unsigned short sList[kSliceBlock / 64][kDoseSlice / 4];  // per wave: its hits (at most 16 per lane), slots within the slice
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = slice_base<kSliceLoads>();
    int4 v[kSliceLoads];
    load_slice(cell, n, true, 0, v);                        // (past the end: 0, and the test below asks for i < n as well)
    const bool staged = maskWords <= kSinkLdsWords;
    if (staged)
        for (int w = threadIdx.x; w < maskWords; w += kSliceBlock) sMask[w] = mask[w];
    __syncthreads();
    // sink_pass's test: a live id (0 <= c < nDerived) whose bit is set
    auto sunk = [&](int c) -> bool {
        if ((unsigned)c >= (unsigned)nDerived) return false;
        const uint32_t w = staged ? sMask[c >> 5] : mask[c >> 5];
        return ((w >> (c & 31)) & 1u) != 0u;
    };
    unsigned hit = 0u;
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k) {
        const int64_t i = base + (int64_t)k * kSliceTrip;
        const bool bx = sunk(v[k].x) && i < n, by = sunk(v[k].y) && i + 1 < n, bz = sunk(v[k].z) && i + 2 < n,
                   bw = sunk(v[k].w) && i + 3 < n;
        hit |= ((bx ? 1u : 0u) | (by ? 2u : 0u) | (bz ? 4u : 0u) | (bw ? 8u : 0u)) << (4 * k);
    }
    if (!workgroup_any(hit != 0u)) return;                  // (the whole workgroup: no hit in the slice)
    const int words = nOrigins * nSinks * nBins;            // (at most kDoseWords: the launcher's check)
    for (int w = threadIdx.x; w < words; w += kSliceBlock) sDose[w] = 0u;
    const unsigned total = wave_list<kSliceLoads>(hit, sList[wave]);
    __syncthreads();
    dose_take(sList[wave], total, (int64_t)blockIdx.x * kDoseSlice, gid, n, lane,
              [&](const int64_t* slots, const uint64_t* ids, const bool* ok) {
                  int c[kDoseBatch];
#pragma unroll
                  for (int b = 0; b < kDoseBatch; ++b) c[b] = cell[slots[b]];     // (a listed slot: 0 <= c < nDerived)
                  double d[kDoseBatch];
                  unsigned o[kDoseBatch], g[kDoseBatch];
#pragma unroll
                  for (int b = 0; b < kDoseBatch; ++b) {
                      d[b] = dose[ids[b]];
                      o[b] = origin ? origin[ids[b]] : 0u;
                      g[b] = sinkGroup ? sinkGroup[c[b]] : 0u;
                  }
#pragma unroll
                  for (int b = 0; b < kDoseBatch; ++b) {
                      if (!ok[b]) continue;
                      const int bin = exposure_bin(d[b], invWidth, nBins);
                      const unsigned ob = o[b] & (kDoseMax - 1), gb = g[b] & (kDoseMax - 1);     // (tag_transfer_kernel's reading)
                      if (bin < 0 || ob >= (unsigned)nOrigins || gb >= (unsigned)nSinks) continue;   // (no such word)
                      atomicAdd(&sDose[(ob * (unsigned)nSinks + gb) * (unsigned)nBins + (unsigned)bin], 1u);
                  }
              });
    __syncthreads();
    for (int w = threadIdx.x; w < words; w += kSliceBlock) {
        const unsigned k = sDose[w];
        if (k != 0u) atomicAdd(&hist[w], (unsigned long long)k);
    }
}

__global__ __launch_bounds__(kSliceBlock) void exposure_stamp_kernel(const int32_t* __restrict__ cell, const int64_t* __restrict__ gid,
                                                                     double* __restrict__ dose, int64_t n) {
    __shared__ unsigned short sList[kSliceBlock / 64][kDoseSlice / 4];  // per wave: its dead slots (at most 16 per lane)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int4 v[kSliceLoads];
    load_slice(cell, n, true, 0, v);
    const unsigned dead = dead_mask(v);
    if (!workgroup_any(dead != 0u)) return;                 // (the whole workgroup: no dead slot in the slice)
    const unsigned total = wave_list<kSliceLoads>(dead, sList[wave]);
    __syncthreads();
    dose_take(sList[wave], total, (int64_t)blockIdx.x * kDoseSlice, gid, n, lane,
              [&](const int64_t*, const uint64_t* ids, const bool* ok) {
#pragma unroll
                  for (int b = 0; b < kDoseBatch; ++b)
                      if (ok[b]) dose[ids[b]] = 0.0;
              });
}

// (every launcher: `cell` and `gid` must be 16-byte aligned, as the arrays of the context's own cloud are)
hipError_t exposure_accumulate(hipStream_t st, const int32_t* cell, const int64_t* gid, const double* rate, double* dose, int64_t n,
                               int64_t nDerived, double scale) {
    if (n <= 0) return hipSuccess;
    const SliceLaunch l = slice_launch(cell, n);
    if (n >= ((int64_t)1 << 31) || !l.fits() || !l.vec || (reinterpret_cast<uintptr_t>(gid) & 15u) != 0 || nDerived < 1 ||
        nDerived > (int64_t)INT32_MAX)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(exposure_accumulate_kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock), 0, st, cell, gid, rate, dose, n,
                       (int)nDerived, scale);
    return hipGetLastError();
}

hipError_t exposure_absorb(hipStream_t st, const int32_t* cell, const int64_t* gid, const double* dose, const uint8_t* origin, int64_t n,
                           const uint32_t* mask, int64_t nDerived, const uint8_t* sinkGroup, double invWidth, int32_t nBins,
                           int32_t nOrigins, int32_t nSinks, unsigned long long* hist) {
    if (n <= 0) return hipSuccess;
    const SliceLaunch l = slice_launch(cell, n);
    if (!l.fits() || !l.vec || nDerived < 1 || nDerived > (int64_t)INT32_MAX || nBins < 1 || nBins > kDoseWords || nOrigins < 1 ||
        nOrigins > kDoseMax || nSinks < 1 || nSinks > kDoseMax || (int64_t)nOrigins * nSinks * nBins > kDoseWords ||
        (origin == nullptr) != (sinkGroup == nullptr))
        return hipErrorInvalidValue;
    const int maskWords = (int)((nDerived + 31) / 32);
    hipLaunchKernelGGL(exposure_absorb_kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock),
                       (size_t)nOrigins * nSinks * nBins * sizeof(unsigned), st, cell, gid, dose, origin, n, mask, (int)nDerived,
                       maskWords, sinkGroup, invWidth, (int)nBins, (int)nOrigins, (int)nSinks, hist);
    return hipGetLastError();
}

hipError_t exposure_stamp(hipStream_t st, const int32_t* cell, const int64_t* gid, double* dose, int64_t n) {
    if (n <= 0) return hipSuccess;
    const SliceLaunch l = slice_launch(cell, n);
    if (!l.fits() || !l.vec) return hipErrorInvalidValue;
    hipLaunchKernelGGL(exposure_stamp_kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock), 0, st, cell, gid, dose, n);
    return hipGetLastError();
}

}  // namespace cpf
