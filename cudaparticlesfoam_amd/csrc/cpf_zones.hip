// Zones (cpf_zone_*): how much of the context's own cloud goes from one compartment of the mesh to another between two samples,
// and how long a visit lasts -- the exchange matrix a compartment model asks of a CFD run -- without touching a step kernel, the
// sort, the recycling kernels or the age, tag, route and exposure kernels.  last[id] is one byte per PARTICLE ID, the zone the
// particle was in at the last sample (kZoneOutside: none since enable, or since a respawn made it a candidate), so neither sort
// moves it; zoneOf[d] is one byte per DERIVED cell, the caller's map over the mesh as given, expanded on the host when it is set:
// one gather a particle, not parentOf and then the map.  Every id sits in exactly one slot, so last[id] is read and written by one
// lane a call: no atomic; the table is integer sums, the same bits as numpy whatever the order of the cloud and of the workgroups
// (DESIGN.md "Zones").  The three kernels are passes of cpf_slice.h; what is written here is what they do per particle.
//
// Sample (zone_sample_kernel).  For every live slot: p = last[gid[s]] (outside: nZones), z = zoneOf[cell[s]], flow[p][z] += 1, and
// last = z where p != z.  The slice and the ids with 16-byte loads (exposure_accumulate_kernel's way: one question a workgroup
// whether the slice lies within the cloud, then twelve loads without a per-lane test), then all sixteen zoneOf and all sixteen last
// gathers of a lane before the first use.  A workgroup with no live slot leaves.  The counts go into (nZones + 1)^2 32-bit words of
// dynamic LDS (a slice has 4096 slots: no word overflows), runs of equal (p, z) in a wave first (count_runs): behind a sort a
// whole wave usually holds ONE pair, one LDS add and not 64 to one address.  Non-zero words leave as 64-bit global adds.  last[id]
// is stored only where it changes: in steady state a few per cent of the cloud.
//
// Leave (zone_leave_kernel).  A READ-ONLY pass in front of whichever pass marks the absorbed (exposure_absorb_kernel's place and
// shape): the slice, the sink's mask (staged in LDS up to kSinkLdsWords words, through L2 beyond), and a workgroup without a hit
// leaves.  Otherwise the hits of a wave go into a list in LDS and the wave's lanes take them in batches of kZoneBatch: every gid
// load of a batch, then every last[gid] gather, in flight before the first use.  Per hit one add to a word of LDS per p; non-zero
// words leave as 64-bit global adds to flow[p][nZones].
//
// Stamp (zone_stamp_kernel).  age_stamp_kernel storing a byte: before a respawn, last[gid[s]] = kZoneOutside for every slot with
// cell < 0.
#include <hip/hip_runtime.h>

#include "cpf_device.h"
#include "cpf_slice.h"

namespace cpf {
namespace {

constexpr int kZoneSlice = slice_ids(kSliceLoads);          // ids per workgroup
constexpr int kZoneMax = 63;                                // zones at most (cpf_zone_enable's limit): 64 x 64 words, 16 KB of dynamic LDS
constexpr int kZoneBatch = 8;                               // list entries a lane takes at a time
constexpr unsigned kZoneOutside = 0xFFu;                    // last[id]: in no zone at the last sample
constexpr uint32_t kNoId = 0xFFFFFFFFu;                     // a slot past the end, or one whose id is none of this cloud's
static_assert(kZoneSlice <= 0xFFFF + 1, "a list entry is a 16-bit slot within the slice");
static_assert((kZoneMax + 1) * (kZoneMax + 1) <= 4096, "the table is staged in at most 4096 words of LDS");

// the ids of the quad of slots at s (a multiple of 4), as 32-bit numbers (n < 2^31): two 16-byte loads where the quad is whole
// (gid is 32-byte aligned there), 8-byte loads at the ragged end; gid null: the slots themselves
__device__ inline void zone_ids(const int64_t* __restrict__ gid, int64_t s, int64_t n, uint32_t (&id)[4]) {
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

// The wave's lanes take the entries of a wave_list kZoneBatch each at a time: f(ids, ok) gets the particle ids of the lane's
// entries (ok[b] false: no entry, or an id that is none of this cloud's -- the id is a valid index all the same).  Every gid load
// of a batch is issued before f runs.  (dose_take's shape, written again here: the existing kernel files keep their text.)
template <class F>
__device__ inline void zone_take(const unsigned short* __restrict__ list, unsigned total, int64_t blockBase,
                                 const int64_t* __restrict__ gid, int64_t n, int lane, F f) {
#pragma unroll 1
    for (unsigned t0 = 0; t0 < total; t0 += 64 * kZoneBatch) {
        uint64_t ids[kZoneBatch];
        bool ok[kZoneBatch];
#pragma unroll
        for (int b = 0; b < kZoneBatch; ++b) {
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
// `cell`, `gid` are the context's own arrays (16-byte aligned: the zone entries have no _dev form); zoneOf has nDerived bytes, each
// below nZones; last n bytes.  Dynamic LDS: (nZones + 1)^2 32-bit words.  No atomics on last: every id is in one slot.
__global__ __launch_bounds__(kSliceBlock) void zone_sample_kernel(const int32_t* __restrict__ cell, const int64_t* __restrict__ gid,
                                                                  const uint8_t* __restrict__ zoneOf, uint8_t* __restrict__ last,
                                                                  int64_t n, int nDerived, int nZones,
                                                                  unsigned long long* __restrict__ flow) {
    extern __shared__ unsigned sFlow[];                     // [nZones + 1][nZones + 1]
    const int lane = threadIdx.x & 63;
    const int64_t base = slice_base<kSliceLoads>();
    int4 v[kSliceLoads];
    uint32_t id[kSliceLoads][4];
    // a slice that lies within the cloud -- every one but the last, the same answer in the whole workgroup -- takes its twelve
    // 16-byte loads without the test for the ragged end, all in flight together (see exposure_accumulate_kernel)
    if (((int64_t)blockIdx.x + 1) * kZoneSlice <= n) {
#pragma unroll
        for (int k = 0; k < kSliceLoads; ++k) v[k] = *reinterpret_cast<const int4*>(cell + base + (int64_t)k * kSliceTrip);
        // (the test for a null gid ONCE, round the eight loads: asked per quad it cuts the loads into blocks, and the compiler
        // waited for the first ten loads before it issued the last two -- seen in the listing)
        if (gid) {
            ulonglong2 a[kSliceLoads], b[kSliceLoads];
#pragma unroll
            for (int k = 0; k < kSliceLoads; ++k) {
                const int64_t s = base + (int64_t)k * kSliceTrip;
                a[k] = *reinterpret_cast<const ulonglong2*>(gid + s);
                b[k] = *reinterpret_cast<const ulonglong2*>(gid + s + 2);
            }
#pragma unroll
            for (int k = 0; k < kSliceLoads; ++k) {
                const uint64_t g[4] = {a[k].x, a[k].y, b[k].x, b[k].y};
#pragma unroll
                for (int j = 0; j < 4; ++j) id[k][j] = g[j] < (uint64_t)n ? (uint32_t)g[j] : kNoId;
            }
        } else {
#pragma unroll
            for (int k = 0; k < kSliceLoads; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) id[k][j] = (uint32_t)(base + (int64_t)k * kSliceTrip + j);      // (below n: the slice is whole)
        }
    } else {
        load_slice(cell, n, true, -1, v);
#pragma unroll
        for (int k = 0; k < kSliceLoads; ++k) zone_ids(gid, base + (int64_t)k * kSliceTrip, n, id[k]);
    }
    // every gather of the lane: CPF_CELL_LOST, every other negative code, ids beyond the mesh and slots past the end read cell 0
    // and id 0, loads that are there to be in flight
    unsigned z[kSliceLoads][4], p[kSliceLoads][4];
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k) {
        const int c[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) z[k][j] = zoneOf[(unsigned)c[j] < (unsigned)nDerived ? c[j] : 0];
    }
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) p[k][j] = last[id[k][j] != kNoId ? id[k][j] : 0u];
    // bit 4 k + j: element j of quad k is live and has an id of this cloud
    unsigned live = 0u;
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k) {
        const int c[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) live |= ((unsigned)c[j] < (unsigned)nDerived && id[k][j] != kNoId ? 1u : 0u) << (4 * k + j);
    }
    if (!workgroup_any(live != 0u)) return;                 // (the whole workgroup: nobody to count in the slice)
    const int side = nZones + 1, words = side * side;       // (at most 64 x 64: the launcher's check)
    for (int w = threadIdx.x; w < words; w += kSliceBlock) sFlow[w] = 0u;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool mine = ((live >> (4 * k + j)) & 1u) != 0u;
            // kZoneOutside is row nZones; so is any other byte that is no zone (cpf_zone_set_last refuses them), and a zone byte
            // beyond the map's range (cpf_set_zone_map refuses them) counts as the last zone: no add leaves the table
            const unsigned pp = p[k][j] < (unsigned)nZones ? p[k][j] : (unsigned)nZones;
            const unsigned zz = z[k][j] < (unsigned)nZones ? z[k][j] : (unsigned)nZones - 1u;
            count_runs<2>(mine ? (int)(pp * (unsigned)side + zz) : -1, 1u, lane, [&](int key, unsigned w) { atomicAdd(&sFlow[key], w); });
            if (mine && p[k][j] != zz) last[id[k][j]] = (uint8_t)zz;
        }
    __syncthreads();
    for (int w = threadIdx.x; w < words; w += kSliceBlock) {
        const unsigned k = sFlow[w];
        if (k != 0u) atomicAdd(&flow[w], (unsigned long long)k);
    }
}

// Nothing of the cloud and nothing of last is written: flow[p][nZones] += 1 for everybody the sink is about to absorb
__global__ __launch_bounds__(kSliceBlock) void zone_leave_kernel(const int32_t* __restrict__ cell, const int64_t* __restrict__ gid,
                                                                 const uint8_t* __restrict__ last, int64_t n,
                                                                 const uint32_t* __restrict__ mask, int nDerived, int maskWords,
                                                                 int nZones, unsigned long long* __restrict__ flow) {
    __shared__ unsigned sOut[kZoneMax + 1];                             // [nZones + 1] by p
    __shared__ uint32_t sMask[kSinkLdsWords];
    __shared__ unsigned short sList[kSliceBlock / 64][kZoneSlice / 4];  // per wave: its hits (at most 16 per lane), slots within the slice
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
    if (threadIdx.x <= (unsigned)nZones) sOut[threadIdx.x] = 0u;        // (nZones <= kZoneMax: the launcher's check)
    const unsigned total = wave_list<kSliceLoads>(hit, sList[wave]);
    __syncthreads();
    zone_take(sList[wave], total, (int64_t)blockIdx.x * kZoneSlice, gid, n, lane, [&](const uint64_t* ids, const bool* ok) {
        unsigned p[kZoneBatch];
#pragma unroll
        for (int b = 0; b < kZoneBatch; ++b) p[b] = last[ids[b]];
#pragma unroll
        for (int b = 0; b < kZoneBatch; ++b)
            if (ok[b]) atomicAdd(&sOut[p[b] < (unsigned)nZones ? p[b] : (unsigned)nZones], 1u);
    });
    __syncthreads();
    if (threadIdx.x <= (unsigned)nZones) {
        const unsigned k = sOut[threadIdx.x];
        if (k != 0u) atomicAdd(&flow[(int)threadIdx.x * (nZones + 1) + nZones], (unsigned long long)k);
    }
}

__global__ __launch_bounds__(kSliceBlock) void zone_stamp_kernel(const int32_t* __restrict__ cell, const int64_t* __restrict__ gid,
                                                                 uint8_t* __restrict__ last, int64_t n) {
    __shared__ unsigned short sList[kSliceBlock / 64][kZoneSlice / 4];  // per wave: its dead slots (at most 16 per lane)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int4 v[kSliceLoads];
    load_slice(cell, n, true, 0, v);
    const unsigned dead = dead_mask(v);
    if (!workgroup_any(dead != 0u)) return;                 // (the whole workgroup: no dead slot in the slice)
    const unsigned total = wave_list<kSliceLoads>(dead, sList[wave]);
    __syncthreads();
    zone_take(sList[wave], total, (int64_t)blockIdx.x * kZoneSlice, gid, n, lane, [&](const uint64_t* ids, const bool* ok) {
#pragma unroll
        for (int b = 0; b < kZoneBatch; ++b)
            if (ok[b]) last[ids[b]] = (uint8_t)kZoneOutside;
    });
}

// (every launcher: `cell` and `gid` must be 16-byte aligned, as the arrays of the context's own cloud are)
hipError_t zone_sample(hipStream_t st, const int32_t* cell, const int64_t* gid, const uint8_t* zoneOf, uint8_t* last, int64_t n,
                       int64_t nDerived, int32_t nZones, unsigned long long* flow) {
    if (n <= 0) return hipSuccess;
    const SliceLaunch l = slice_launch(cell, n);
    if (n >= ((int64_t)1 << 31) || !l.fits() || !l.vec || (reinterpret_cast<uintptr_t>(gid) & 15u) != 0 || nDerived < 1 ||
        nDerived > (int64_t)INT32_MAX || nZones < 1 || nZones > kZoneMax)
        return hipErrorInvalidValue;
    const size_t words = (size_t)(nZones + 1) * (size_t)(nZones + 1);
    hipLaunchKernelGGL(zone_sample_kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock), words * sizeof(unsigned), st, cell, gid, zoneOf,
                       last, n, (int)nDerived, (int)nZones, flow);
    return hipGetLastError();
}

hipError_t zone_leave(hipStream_t st, const int32_t* cell, const int64_t* gid, const uint8_t* last, int64_t n, const uint32_t* mask,
                      int64_t nDerived, int32_t nZones, unsigned long long* flow) {
    if (n <= 0) return hipSuccess;
    const SliceLaunch l = slice_launch(cell, n);
    if (!l.fits() || !l.vec || nDerived < 1 || nDerived > (int64_t)INT32_MAX || nZones < 1 || nZones > kZoneMax)
        return hipErrorInvalidValue;
    const int maskWords = (int)((nDerived + 31) / 32);
    hipLaunchKernelGGL(zone_leave_kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock), 0, st, cell, gid, last, n, mask, (int)nDerived,
                       maskWords, (int)nZones, flow);
    return hipGetLastError();
}

hipError_t zone_stamp(hipStream_t st, const int32_t* cell, const int64_t* gid, uint8_t* last, int64_t n) {
    if (n <= 0) return hipSuccess;
    const SliceLaunch l = slice_launch(cell, n);
    if (!l.fits() || !l.vec) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zone_stamp_kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock), 0, st, cell, gid, last, n);
    return hipGetLastError();
}

}  // namespace cpf
