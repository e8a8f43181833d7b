// Sink log (cpf_sink_log_*): one 64-byte record for every particle of the context's own cloud that cpf_sink_apply absorbs -- who,
// when, where and with what state: the list the age histogram, the transfer matrix, the route and dose histograms and the
// "outside" column of the zone table are reductions of -- appended to a buffer on the device, without touching a step kernel, the
// sort, the recycling kernels or the age, tag, route, exposure and zone kernels.  It keeps no state per particle: a record is
// made of what the cloud and the other groups' tables hold at the apply (DESIGN.md "Sink log").
//
// The one kernel (sink_log_kernel) is a READ-ONLY pass of cpf_slice.h in front of everything else cpf_sink_apply runs
// (zone_leave_kernel's place and shape): the slice, the sink's mask (staged in LDS up to kSinkLdsWords words, through L2 beyond),
// sink_pass's test, and a workgroup without a hit leaves.  Otherwise the hits of a wave go into the wave's list in LDS, the four
// totals into four words of LDS, and ONE thread makes ONE returning 64-bit add of their sum on the cursor: the workgroup's base.
// A wave's base is that plus the totals of the waves before it.  Every workgroup with a hit reserves, whether its records fit or
// not, so the cursor counts everybody; nobody waits for another workgroup.  The wave's lanes then take its list in batches of
// kLogBatch: every gid and cell load of a batch, then x, y, z of the slot and every gather by id and by cell, in flight before
// the first use.  Entry t of the list becomes record base + t: four 16-byte stores a lane, neighbouring lanes write neighbouring
// records (a wave-instruction covers 64 records 64 bytes apart; the four together fill 4 KB whole), indices >= capacity are
// skipped.  The order of the records is whichever workgroup reserved first: cpf_sink_log_read sorts on the host.
#include <hip/hip_runtime.h>

#include "cpf_device.h"
#include "cpf_slice.h"

namespace cpf {
namespace {

constexpr int kLogSlice = slice_ids(kSliceLoads);           // ids per workgroup
constexpr int kLogWaves = kSliceBlock / 64;
constexpr int kLogBatch = 4;                                // list entries a lane takes at a time (some twenty registers each)
static_assert(kLogSlice <= 0xFFFF + 1, "a list entry is a 16-bit slot within the slice");
static_assert(sizeof(cpf_sink_record) == 4 * sizeof(uint4), "a record is four 16-byte stores");

__device__ inline uint32_t lo32(double d) { return (uint32_t)(unsigned long long)__double_as_longlong(d); }
__device__ inline uint32_t hi32(double d) { return (uint32_t)((unsigned long long)__double_as_longlong(d) >> 32); }

}  // namespace

// (outside the anonymous namespace, like the step kernels: tools/resource_usage.py lists kernels by their plain names)
__global__ __launch_bounds__(kSliceBlock) void sink_log_kernel(const SinkLogView a, int nDerived, int maskWords) {
    __shared__ uint32_t sMask[kSinkLdsWords];
    __shared__ unsigned short sList[kLogWaves][kLogSlice / 4];          // per wave: its hits (at most 16 per lane), slots within the slice
    __shared__ unsigned sTotal[kLogWaves];                              // the reservation: the waves' totals ...
    __shared__ unsigned long long sBase;                                // ... and what the cursor held before their sum was added
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = slice_base<kSliceLoads>(), n = a.n;
    const uint32_t* __restrict__ mask = a.mask;
    int4 v[kSliceLoads];
    load_slice(a.cell, n, true, 0, v);                      // (past the end: 0, and the test below asks for i < n as well)
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
    if (!workgroup_any(hit != 0u)) return;                  // (the whole workgroup: no hit in the slice, no reservation)
    const unsigned total = wave_list<kSliceLoads>(hit, sList[wave]);
    if (lane == 0) sTotal[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned sum = 0u;
#pragma unroll
        for (int w = 0; w < kLogWaves; ++w) sum += sTotal[w];
        sBase = atomicAdd(a.cursor, (unsigned long long)sum);           // (sum > 0: somebody had a hit)
    }
    __syncthreads();
    unsigned long long first = sBase;                       // the index of the wave's entry 0
    for (int w = 0; w < wave; ++w) first += sTotal[w];
    if (first >= (unsigned long long)a.capacity) return;    // (the wave: none of its records fits; no barrier follows)
    const int64_t blockBase = (int64_t)blockIdx.x * kLogSlice;
    const unsigned short* __restrict__ list = sList[wave];
    uint4* __restrict__ out = reinterpret_cast<uint4*>(a.rec);
    const uint32_t tail = a.fields << 24;
#pragma unroll 1
    for (unsigned t0 = 0; t0 < total; t0 += 64 * kLogBatch) {
        int64_t s[kLogBatch];
        uint64_t g[kLogBatch];
        int c[kLogBatch];
        bool ok[kLogBatch];
#pragma unroll
        for (int b = 0; b < kLogBatch; ++b) {
            const unsigned t = t0 + 64 * b + lane;
            ok[b] = t < total;
            s[b] = blockBase + list[ok[b] ? t : 0];         // (entry 0 exists: total > 0; every entry is a slot below n)
            g[b] = (uint64_t)s[b];
        }
        // (every test for a null table ONCE, round the loads of a batch: asked per load it cuts them into blocks with a wait
        // at the end of each -- seen in the listing)
        if (a.gid) {
#pragma unroll
            for (int b = 0; b < kLogBatch; ++b) g[b] = (uint64_t)a.gid[s[b]];
        }
#pragma unroll
        for (int b = 0; b < kLogBatch; ++b) c[b] = a.cell[s[b]];
        double x[kLogBatch], y[kLogBatch], z[kLogBatch], dose[kLogBatch];
        uint32_t birth[kLogBatch], origin[kLogBatch], zone[kLogBatch], group[kLogBatch];
        int parent[kLogBatch];
#pragma unroll
        for (int b = 0; b < kLogBatch; ++b) { x[b] = a.x[s[b]]; y[b] = a.y[s[b]]; z[b] = a.z[s[b]]; }
        // the gathers by id and by cell: an id that is none of this cloud's reads entry 0 (and is recorded with the off values);
        // the cell is the one the test above accepted (nobody writes during the pass), clamped all the same
        uint64_t id[kLogBatch];
        int d[kLogBatch];
#pragma unroll
        for (int b = 0; b < kLogBatch; ++b) {
            id[b] = g[b] < (uint64_t)n ? g[b] : 0ull;
            d[b] = (unsigned)c[b] < (unsigned)nDerived ? c[b] : 0;
            birth[b] = a.now; origin[b] = 0xFFu; dose[b] = 0.0; zone[b] = 0xFFu; group[b] = 0xFFu; parent[b] = d[b];
        }
        if (a.birth) {
#pragma unroll
            for (int b = 0; b < kLogBatch; ++b) birth[b] = a.birth[id[b]];
        }
        if (a.origin) {
#pragma unroll
            for (int b = 0; b < kLogBatch; ++b) origin[b] = a.origin[id[b]];
        }
        if (a.dose) {
#pragma unroll
            for (int b = 0; b < kLogBatch; ++b) dose[b] = a.dose[id[b]];
        }
        if (a.last) {
#pragma unroll
            for (int b = 0; b < kLogBatch; ++b) zone[b] = a.last[id[b]];
        }
        if (a.sinkGroup) {
#pragma unroll
            for (int b = 0; b < kLogBatch; ++b) group[b] = a.sinkGroup[d[b]];
        }
        if (a.parentOf) {
#pragma unroll
            for (int b = 0; b < kLogBatch; ++b) parent[b] = a.parentOf[d[b]];
        }
#pragma unroll
        for (int b = 0; b < kLogBatch; ++b) {
            const unsigned long long k = first + t0 + 64 * b + lane;
            if (!ok[b] || k >= (unsigned long long)a.capacity) continue;
            if (g[b] >= (uint64_t)n) { birth[b] = a.now; origin[b] = 0xFFu; dose[b] = 0.0; zone[b] = 0xFFu; }
            uint4* __restrict__ r = out + 4 * k;
            r[0] = make_uint4((uint32_t)g[b], (uint32_t)(g[b] >> 32), a.apply, a.now);
            r[1] = make_uint4(lo32(x[b]), hi32(x[b]), lo32(y[b]), hi32(y[b]));
            r[2] = make_uint4(lo32(z[b]), hi32(z[b]), lo32(dose[b]), hi32(dose[b]));
            r[3] = make_uint4(a.now - birth[b], (uint32_t)parent[b], origin[b] | (group[b] << 8) | (zone[b] << 16) | tail, 0u);
        }
    }
}

// (`cell` and `rec` must be 16-byte aligned, as the arrays of the context's own cloud and the log's buffer are)
hipError_t sink_log(hipStream_t st, const SinkLogView& v, int64_t nDerived) {
    if (v.n <= 0) return hipSuccess;
    const SliceLaunch l = slice_launch(v.cell, v.n);
    if (v.n >= ((int64_t)1 << 31) || !l.fits() || !l.vec || (reinterpret_cast<uintptr_t>(v.rec) & 15u) != 0 || !v.rec || !v.cursor ||
        !v.mask || !v.x || !v.y || !v.z || v.capacity < 1 || nDerived < 1 || nDerived > (int64_t)INT32_MAX || v.fields > 0xFFu)
        return hipErrorInvalidValue;
    const int maskWords = (int)((nDerived + 31) / 32);
    hipLaunchKernelGGL(sink_log_kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock), 0, st, v, (int)nDerived, maskWords);
    return hipGetLastError();
}

}  // namespace cpf
