// Tracer tags (cpf_tag_*): where a particle of a recycled cloud came from and where it went, without touching a step kernel, the
// sort, the recycling kernels or the age kernels.  origin[id] is one byte per PARTICLE ID -- the origin the respawn that last made
// id live gave it --, so neither sort moves it; sinkGroup[d] is one byte per DERIVED cell.  Everything summed here is an integer:
// the same bits whatever the order of the cloud and of the workgroups (DESIGN.md "Tags").  The three kernels are passes of
// cpf_slice.h; what is written here is what they do per particle.
//
// Transfer (tag_transfer_kernel).  A READ-ONLY pass that runs before the sink's: the slice, the sink's mask (staged in LDS up to
// kSinkLdsWords words, through L2 beyond), and a workgroup without a hit leaves.  Otherwise the hits of a wave go into a list in
// LDS and the wave's lanes take them in batches of kTagBatch -- every gid and cell load of a batch, then every origin[gid] and
// sinkGroup[cell] gather, in flight before the first use: the sink's cells are neighbours in a sorted cloud, so a few workgroups
// hold all the hits and their chains of dependent loads are the kernel's tail.  Per hit one add to a kTagMax x kTagMax matrix of
// 32-bit words in LDS (a slice has at most kTagSlice hits); non-zero entries leave as 64-bit global adds.
//
// Stamp (tag_stamp_kernel).  Before a respawn, for every slot with cell < 0: origin[gid] = boxOrigin (hi null: the box form), or
// originOfKept[source_pick(hi, nKept, source_words(seed, gid, epoch)[0])] (the source form) -- the triangle inlet_place_kernel is
// about to pick for that id, which is a pure function of (seed, id, epoch).  A workgroup without a dead slot leaves after its
// loads; the dead of a wave go through the list.  The bounds are searched where they lie, through the caches, by a lower bound of
// ceil(log2(nKept)) levels that every lane walks in step -- the eight searches of a lane's batch have their loads of a level in
// flight together, where source_pick's loop, whose trip count depends on the data, ran them one after the other (measured,
// 33 000 dead of 1e7 on 60 triangles: 0.024 -> 0.017 ms a call, next to age_stamp_kernel's 0.012).  Nothing is staged in LDS: the dead of a recycle point sit in a few workgroups, and the same text serves a table of
// any length (past inlet_place_kernel's 4096 staged bounds too).
//
// Field (tag_field_kernel).  occupancy_kernel over the VIRTUAL id parent * nOrigins + origin[gid]: slice_window and window_bins
// on 32-bit words (a slice has kTagSlice ids), the flush contiguous into [nParent][nOrigins].  Every lane's gid loads and origin
// gathers are all issued before the first is used (16 gathers in flight per lane).
#include <hip/hip_runtime.h>

#include "cpf_device.h"
#include "cpf_philox.h"
#include "cpf_slice.h"

namespace cpf {
namespace {

constexpr int kTagSlice = slice_ids(kSliceLoads);           // ids per workgroup
constexpr int kTagMax = 16;                                 // origins, and sink groups, at most (cpf_tag_enable's limit)
constexpr int kTagBatch = 8;                                // list entries a lane takes at a time
constexpr int kTagFieldBins = 4096;                         // 32-bit field bins in LDS: 16 KB per workgroup
static_assert(kTagSlice <= 0xFFFF + 1, "a list entry is a 16-bit slot within the slice");

// The wave's lanes take the entries of a wave_list kTagBatch each at a time: f(slots, ids, ok) gets the array slots and particle
// ids of the lane's entries (ok[b] false: no entry, or an id that is none of this cloud's -- slot and id are valid indices all the
// same).  Every gid load of a batch is issued before f runs.
template <class F>
__device__ inline void tag_take(const unsigned short* __restrict__ list, unsigned total, int64_t blockBase,
                                const int64_t* __restrict__ gid, int64_t n, int lane, F f) {
#pragma unroll 1
    for (unsigned t0 = 0; t0 < total; t0 += 64 * kTagBatch) {
        int64_t slots[kTagBatch];
        uint64_t ids[kTagBatch];
        bool ok[kTagBatch];
#pragma unroll
        for (int b = 0; b < kTagBatch; ++b) {
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
// `cell` is 16-byte aligned (the context's own arrays are: the tag entries have no _dev form).  Nothing of the cloud is written.
__global__ __launch_bounds__(kSliceBlock) void tag_transfer_kernel(const int32_t* __restrict__ cell, const int64_t* __restrict__ gid,
                                                                   const uint8_t* __restrict__ origin, int64_t n,
                                                                   const uint32_t* __restrict__ mask, int nDerived, int maskWords,
                                                                   const uint8_t* __restrict__ sinkGroup,
                                                                   unsigned long long* __restrict__ transfer, int nSinks) {
    __shared__ uint32_t sMask[kSinkLdsWords];
    __shared__ unsigned short sList[kSliceBlock / 64][kTagSlice / 4];   // per wave: its hits (at most 16 per lane), slots within the slice
    __shared__ unsigned sT[kTagMax * kTagMax];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = slice_base<kSliceLoads>();
    int4 v[kSliceLoads];
    load_slice(cell, n, true, 0, v);                        // (past the end: 0, and the test below asks for i < n as well)
    const bool staged = maskWords <= kSinkLdsWords;
    if (staged)
        for (int w = threadIdx.x; w < maskWords; w += kSliceBlock) sMask[w] = mask[w];
    sT[threadIdx.x] = 0u;
    static_assert(kTagMax * kTagMax == kSliceBlock, "one matrix entry per thread");
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
    const unsigned total = wave_list<kSliceLoads>(hit, sList[wave]);
    __syncthreads();
    tag_take(sList[wave], total, (int64_t)blockIdx.x * kTagSlice, gid, n, lane,
             [&](const int64_t* slots, const uint64_t* ids, const bool* ok) {
                 int c[kTagBatch];
#pragma unroll
                 for (int b = 0; b < kTagBatch; ++b) c[b] = cell[slots[b]];      // (a listed slot: 0 <= c < nDerived)
                 unsigned o[kTagBatch], g[kTagBatch];
#pragma unroll
                 for (int b = 0; b < kTagBatch; ++b) {
                     o[b] = origin[ids[b]];
                     g[b] = sinkGroup[c[b]];
                 }
#pragma unroll
                 for (int b = 0; b < kTagBatch; ++b)
                     if (ok[b]) atomicAdd(&sT[(o[b] & (kTagMax - 1)) * kTagMax + (g[b] & (kTagMax - 1))], 1u);
             });
    __syncthreads();
    const unsigned k = sT[threadIdx.x];
    const int o = threadIdx.x / kTagMax, g = threadIdx.x % kTagMax;
    if (k != 0u && g < nSinks) atomicAdd(&transfer[o * nSinks + g], (unsigned long long)k);
}

// hi null: the box form, everybody gets boxOrigin; else the source form over the bounds hi[nKept] and originOfKept[nKept]
__global__ __launch_bounds__(kSliceBlock) void tag_stamp_kernel(const int32_t* __restrict__ cell, const int64_t* __restrict__ gid,
                                                                uint8_t* __restrict__ origin, int64_t n,
                                                                const uint32_t* __restrict__ hi, int nKept,
                                                                const uint8_t* __restrict__ originOfKept, uint32_t seed,
                                                                uint32_t epoch, int boxOrigin) {
    __shared__ unsigned short sList[kSliceBlock / 64][kTagSlice / 4];   // per wave: its dead slots (at most 16 per lane)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int4 v[kSliceLoads];
    load_slice(cell, n, true, 0, v);
    const unsigned dead = dead_mask(v);
    if (!workgroup_any(dead != 0u)) return;                 // (the whole workgroup: no dead slot in the slice)
    const unsigned total = wave_list<kSliceLoads>(dead, sList[wave]);
    __syncthreads();
    const int levels = nKept > 1 ? 32 - __builtin_clz((unsigned)(nKept - 1)) : 0;      // 2^levels >= nKept
    tag_take(sList[wave], total, (int64_t)blockIdx.x * kTagSlice, gid, n, lane,
             [&](const int64_t* slots, const uint64_t* ids, const bool* ok) {
                 if (hi == nullptr) {
#pragma unroll
                     for (int b = 0; b < kTagBatch; ++b)
                         if (ok[b]) origin[ids[b]] = (uint8_t)boxOrigin;
                     return;
                 }
                 // the draw keys on the id the respawn keys on: gid[s], whatever it is (an id beyond the cloud has no entry)
                 uint32_t w0[kTagBatch];
#pragma unroll
                 for (int b = 0; b < kTagBatch; ++b) {
                     uint32_t c[4];
                     source_words(seed, ids[b], epoch, c);
                     w0[b] = c[0];
                 }
                 // source_pick's answer, the first t with w0 <= hi[t], by a lower bound whose trip count is the table's alone:
                 // the batch's searches go in step, eight loads in flight a level (entries past the table read as its last one,
                 // 0xFFFFFFFF, which is never below)
                 int tri[kTagBatch];
#pragma unroll
                 for (int b = 0; b < kTagBatch; ++b) tri[b] = 0;
#pragma unroll 1
                 for (int step = levels - 1; step >= 0; --step) {
                     uint32_t bound[kTagBatch];
#pragma unroll
                     for (int b = 0; b < kTagBatch; ++b) bound[b] = hi[min(tri[b] + (1 << step) - 1, nKept - 1)];
#pragma unroll
                     for (int b = 0; b < kTagBatch; ++b) tri[b] += bound[b] < w0[b] ? (1 << step) : 0;
                 }
                 unsigned o[kTagBatch];
#pragma unroll
                 for (int b = 0; b < kTagBatch; ++b) o[b] = originOfKept[tri[b]];
#pragma unroll
                 for (int b = 0; b < kTagBatch; ++b)
                     if (ok[b]) origin[ids[b]] = (uint8_t)o[b];
             });
}

// `cell` is 16-byte aligned; field is [nParent][nOrigins]
__global__ __launch_bounds__(kSliceBlock) void tag_field_kernel(const int32_t* __restrict__ cell, const int64_t* __restrict__ gid,
                                                                const uint8_t* __restrict__ origin, int64_t n,
                                                                const int32_t* __restrict__ parentOf, int nDerived, int nOrigins,
                                                                unsigned long long* __restrict__ field) {
    const int64_t base = slice_base<kSliceLoads>();
    int4 v[kSliceLoads];
    load_slice(cell, n, true, -1, v);
    // the ids, as age_field_kernel reads them: plain 8-byte loads, four consecutive per lane; past the end and ids that are none
    // of this cloud's: no id (their slot is not counted, see below)
    uint32_t id[kSliceLoads][4];
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t s = base + (int64_t)k * kSliceTrip + j;
            const uint64_t g = s < n ? (uint64_t)(gid ? gid[s] : s) : ~0ull;
            id[k][j] = g < (uint64_t)n ? (uint32_t)g : 0xFFFFFFFFu;     // (n < 2^31)
        }
    unsigned org[kSliceLoads][4];
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) org[k][j] = origin[id[k][j] != 0xFFFFFFFFu ? id[k][j] : 0u];
    // derived -> parent -> virtual id; CPF_CELL_LOST, every other negative code, ids beyond the mesh, slots without an id of this
    // cloud and origins beyond nOrigins (cpf_tag_set_origins refuses them) become -1
    auto live = [&](int c, uint32_t i, unsigned o) -> int {
        if ((unsigned)c >= (unsigned)nDerived || i == 0xFFFFFFFFu || o >= (unsigned)nOrigins) return -1;
        return (parentOf ? parentOf[c] : c) * nOrigins + (int)o;
    };
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k) {
        v[k].x = live(v[k].x, id[k][0], org[k][0]); v[k].y = live(v[k].y, id[k][1], org[k][1]);
        v[k].z = live(v[k].z, id[k][2], org[k][2]); v[k].w = live(v[k].w, id[k][3], org[k][3]);
    }
    int first;
    const int last = slice_window(v, first);
    if (last < 0) return;                                   // nothing to count in the slice (the whole workgroup leaves)
    window_bins<unsigned, kTagFieldBins>(
        first, last,
        // a lane's four ids: where they agree (a sorted cloud fed by one origin) one add carries all four
        [&](auto add) {
#pragma unroll
            for (int k = 0; k < kSliceLoads; ++k) {
                const int4& q = v[k];
                if (q.x >= 0 && q.x == q.y && q.y == q.z && q.z == q.w) {
                    add(q.x, 4u);
                } else {
                    if (q.x >= 0) add(q.x, 1u);
                    if (q.y >= 0) add(q.y, 1u);
                    if (q.z >= 0) add(q.z, 1u);
                    if (q.w >= 0) add(q.w, 1u);
                }
            }
        },
        [&](int c, unsigned w) { atomicAdd(&field[(size_t)c], (unsigned long long)w); });
}

// (every launcher: `cell` must be 16-byte aligned, as the arrays of the context's own cloud are)
hipError_t tag_transfer(hipStream_t st, const int32_t* cell, const int64_t* gid, const uint8_t* origin, int64_t n, const uint32_t* mask,
                        int64_t nDerived, const uint8_t* sinkGroup, int32_t nOrigins, int32_t nSinks, unsigned long long* transfer) {
    if (n <= 0) return hipSuccess;
    const SliceLaunch l = slice_launch(cell, n);
    if (!l.fits() || !l.vec || nDerived > (int64_t)INT32_MAX || nOrigins < 1 || nOrigins > kTagMax || nSinks < 1 || nSinks > kTagMax)
        return hipErrorInvalidValue;
    const int maskWords = (int)((nDerived + 31) / 32);
    hipLaunchKernelGGL(tag_transfer_kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock), 0, st, cell, gid, origin, n, mask, (int)nDerived,
                       maskWords, sinkGroup, transfer, (int)nSinks);
    return hipGetLastError();
}

hipError_t tag_stamp(hipStream_t st, const int32_t* cell, const int64_t* gid, uint8_t* origin, int64_t n, const uint32_t* hi,
                     int32_t nKept, const uint8_t* originOfKept, uint32_t seed, uint32_t epoch, int32_t boxOrigin) {
    if (n <= 0) return hipSuccess;
    const SliceLaunch l = slice_launch(cell, n);
    if (!l.fits() || !l.vec || (hi && (nKept < 1 || !originOfKept)) || boxOrigin < 0 || boxOrigin >= kTagMax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tag_stamp_kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock), 0, st, cell, gid, origin, n, hi, (int)nKept,
                       originOfKept, seed, epoch, (int)boxOrigin);
    return hipGetLastError();
}

hipError_t tag_field(hipStream_t st, const int32_t* cell, const int64_t* gid, const uint8_t* origin, int64_t n, const int32_t* parentOf,
                     int64_t nDerived, int64_t nParent, int32_t nOrigins, unsigned long long* field) {
    if (n <= 0) return hipSuccess;
    const SliceLaunch l = slice_launch(cell, n);
    if (n >= ((int64_t)1 << 31) || nDerived > (int64_t)INT32_MAX || !l.fits() || !l.vec || nOrigins < 1 || nOrigins > kTagMax ||
        nParent * nOrigins >= ((int64_t)1 << 31))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(tag_field_kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock), 0, st, cell, gid, origin, n, parentOf, (int)nDerived,
                       (int)nOrigins, field);
    return hipGetLastError();
}

}  // namespace cpf
