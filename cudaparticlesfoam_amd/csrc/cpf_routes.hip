// Routes (cpf_route_*): the residence time of a recycled cloud's tracer per ROUTE, route = origin x sink group -- what tracer age
// (cpf_age.hip) and tracer tags (cpf_tags.hip) answer separately, read together.  Nothing new is kept per particle: birth[id] is
// age's, origin[id] and sinkGroup[d] are tags'.  Everything summed here is an integer: the same bits whatever the order of the
// cloud and of the workgroups (DESIGN.md "Routes").  The two kernels are passes of cpf_slice.h; what is written here is what they
// do per particle.
//
// Absorb (route_absorb_kernel).  ONE pass in place of tag_transfer_kernel + age_absorb_kernel: sink_pass, and a workgroup without a
// hit ends where sink_kernel ends.  Otherwise:
//   - the sink GROUP of a hit belongs to the DERIVED cell the slot held before the pass marked it, which only the lane that loaded
//     the quad still has (sink_pass hands its loaded quads out).  That lane issues the sinkGroup gathers of its hit elements
//     -- sixteen byte loads, all in flight, the elements without a hit at cell 0 -- right
//     behind the pass and lays the bytes down in LDS by slot, one word per quad (4 KB; a list of the cells themselves would take
//     16 KB, and with the staged tables below the workgroup's 64 KB would not hold it);
//   - the hits of a wave go into a wave_list and the wave's lanes take them in batches of kRouteBatch: every gid load of a batch,
//     then every birth[gid] and origin[gid] gather, in flight before the first use; the group comes from LDS by the listed slot;
//   - per hit one add each to the kRouteMax x kRouteMax transfer matrix, to the nBins age histogram and to the joint histogram
//     [nOrigins][nSinks][nBins].  The joint one is staged in LDS behind the age histogram when it has at most kRouteJointWords
//     words.  A larger one is added to where it lies, through L2 -- behind window_bins' direct-mapped cache, in the same
//     kRouteJointWords words: kRouteJointWords / 2 (count, word index) pairs, an add claims the pair of its index modulo that
//     if it is free or holds the same index and goes to global memory for itself otherwise.  The absorbed of a slice share a
//     few dozen (route, bin) words, so nearly every add stays in LDS (measured, 33 000 absorbed of 1e7, 2 x 2 x 4096: one
//     64-bit global add per hit made the call 0.250 ms, 4.3 times the two-pass path's; see DESIGN.md 5.10 for the cache's).
//     All LDS words are 32-bit (a slice has at most kRouteSlice hits); non-zero ones leave as 64-bit global adds.
// Static LDS: sink_pass's mask and sum, the four lists, the group bytes, the matrix.  Dynamic: nBins words, and the joint
// histogram's or the cache's -- 32 KB at most.
//
// Field (route_field_kernel).  age_field_kernel over tag_field_kernel's VIRTUAL id parent * nOrigins + origin[gid]: slice_window and
// window_bins on the 64-bit word count << 44 | age sum, kRouteBins bins, a wider window through the direct-mapped cache; the
// flush is contiguous into [nParent][nOrigins][2].  All of a lane's 16 gid loads are issued first, then its 16 birth and its 16
// origin gathers, before the first use: 48 loads in flight a lane, which the register file holds without a spill (see
// tests/test_build_resources_routes.py), so the batch is NOT halved.
#include <hip/hip_runtime.h>

#include "cpf_device.h"
#include "cpf_slice.h"

namespace cpf {
namespace {

constexpr int kRouteSlice = slice_ids(kSliceLoads);         // ids per workgroup
constexpr int kRouteMax = 16;                               // origins, and sink groups, at most (cpf_tag_enable's limit)
constexpr int kRouteMaxBins = 4096;                         // residence-time bins at most (cpf_age_enable's limit)
constexpr int kRouteJointWords = 4096;                      // the joint histogram is staged in LDS up to this many 32-bit words
constexpr int kRouteBatch = 8;                              // list entries a lane takes at a time
constexpr int kRouteBins = 2048;                            // 64-bit field bins in LDS: 16 KB per workgroup
constexpr int kRouteCountShift = 44;                        // a bin: count << 44 | age sum
static_assert(kRouteSlice <= 0xFFFF + 1, "a list entry is a 16-bit slot within the slice");
static_assert(kRouteSlice <= (1 << 12), "a bin's age sum must stay below 2^44: at most 2^12 ages below 2^32");

// The wave's lanes take the entries of a wave_list kRouteBatch each at a time: f(local, ids, ok) gets the slots WITHIN THE SLICE
// and the particle ids of the lane's entries (ok[b] false: no entry, or an id that is none of this cloud's -- slot and id are
// valid indices all the same).  Every gid load of a batch is issued before f runs.  (tag_take's shape, written again here: the
// existing kernel files keep their text.)
template <class F>
__device__ inline void route_take(const unsigned short* __restrict__ list, unsigned total, int64_t blockBase,
                                  const int64_t* __restrict__ gid, int64_t n, int lane, F f) {
#pragma unroll 1
    for (unsigned t0 = 0; t0 < total; t0 += 64 * kRouteBatch) {
        unsigned local[kRouteBatch];
        uint64_t ids[kRouteBatch];
        bool ok[kRouteBatch];
#pragma unroll
        for (int b = 0; b < kRouteBatch; ++b) {
            const unsigned t = t0 + 64 * b + lane;
            local[b] = list[t < total ? t : 0];                         // (entry 0 exists: total > 0)
            const int64_t s = blockBase + local[b];
            const uint64_t id = (uint64_t)(gid ? gid[s] : s);
            ok[b] = t < total && id < (uint64_t)n;
            ids[b] = ok[b] ? id : 0ull;
        }
        f(local, ids, ok);
    }
}

}  // namespace

// (outside the anonymous namespace, like the step kernels: tools/resource_usage.py lists kernels by their plain names)
// `cell` is 16-byte aligned (the context's own arrays are: the route entries have no _dev form).  Dynamic LDS: nBins 32-bit bins,
// then the joint histogram's jointWords 32-bit words, or (jointWords 0: it is added to in global memory) kRouteJointWords words
// of cache
__global__ __launch_bounds__(kSliceBlock) void route_absorb_kernel(int32_t* __restrict__ cell, const int64_t* __restrict__ gid,
                                                                   const uint32_t* __restrict__ birth,
                                                                   const uint8_t* __restrict__ origin, int64_t n,
                                                                   const uint32_t* __restrict__ mask, int nDerived, int maskWords,
                                                                   const uint8_t* __restrict__ sinkGroup,
                                                                   unsigned long long* __restrict__ absorbed, uint32_t now,
                                                                   uint32_t binCycles, int nBins, int nOrigins, int nSinks,
                                                                   int jointWords, unsigned long long* __restrict__ hist,
                                                                   unsigned long long* __restrict__ transfer,
                                                                   unsigned long long* __restrict__ routeHist) {
    extern __shared__ unsigned sDyn[];                                  // [nBins] the age histogram | the joint one, or its cache
    __shared__ unsigned short sList[kSliceBlock / 64][kRouteSlice / 4]; // per wave: its hits (at most 16 per lane), slots within the slice
    __shared__ uint32_t sGroup[kRouteSlice / 4];                        // a byte per slot of the slice: the sink group of a hit
    __shared__ unsigned sT[kRouteMax * kRouteMax];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int4 v[kSliceLoads];                                    // the ids as they were BEFORE the pass marked them
    unsigned hit;
    const unsigned all = sink_pass<true, true>(cell, n, mask, nDerived, maskWords, hit, v);
    if (all == 0u) return;                                  // (the whole workgroup: sink_kernel's pass, nothing more)
    if (threadIdx.x == 0) atomicAdd(absorbed, (unsigned long long)all);
    // the groups of this lane's hits (a hit: 0 <= cell < nDerived); no hit: cell 0, a load that is there to be in flight
    unsigned grp[kSliceLoads][4];
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k) {
        const unsigned h = hit >> (4 * k);
        grp[k][0] = sinkGroup[(h & 1u) ? v[k].x : 0];
        grp[k][1] = sinkGroup[(h & 2u) ? v[k].y : 0];
        grp[k][2] = sinkGroup[(h & 4u) ? v[k].z : 0];
        grp[k][3] = sinkGroup[(h & 8u) ? v[k].w : 0];
    }
    constexpr int kPairs = kRouteJointWords / 2;
    static_assert((kPairs & (kPairs - 1)) == 0, "pair = word index & (kPairs - 1)");
    unsigned* sHist = sDyn;
    unsigned* sJoint = sDyn + nBins;                        // staged: the words themselves; else kPairs counts, then kPairs indices
    int* sIndex = reinterpret_cast<int*>(sJoint + kPairs);
    const bool staged = jointWords != 0;
    for (int b = threadIdx.x; b < nBins + (staged ? jointWords : kPairs); b += kSliceBlock) sDyn[b] = 0u;
    if (!staged)
        for (int b = threadIdx.x; b < kPairs; b += kSliceBlock) sIndex[b] = -1;
    sT[threadIdx.x] = 0u;
    static_assert(kRouteMax * kRouteMax == kSliceBlock, "one matrix entry per thread");
    const unsigned total = wave_list<kSliceLoads>(hit, sList[wave]);
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k)                   // slot k * kSliceTrip + 4 * thread + j is byte j of word k * kSliceBlock + thread
        sGroup[k * kSliceBlock + threadIdx.x] = (grp[k][0] & 0xFFu) | ((grp[k][1] & 0xFFu) << 8) | ((grp[k][2] & 0xFFu) << 16) | (grp[k][3] << 24);
    __syncthreads();
    const uint8_t* sGroupOf = reinterpret_cast<const uint8_t*>(sGroup);
    route_take(sList[wave], total, (int64_t)blockIdx.x * kRouteSlice, gid, n, lane,
               [&](const unsigned* local, const uint64_t* ids, const bool* ok) {
                   uint32_t born[kRouteBatch];
                   unsigned o[kRouteBatch], g[kRouteBatch];
#pragma unroll
                   for (int b = 0; b < kRouteBatch; ++b) {
                       born[b] = birth[ids[b]];
                       o[b] = origin[ids[b]];
                       g[b] = sGroupOf[local[b]];
                   }
#pragma unroll
                   for (int b = 0; b < kRouteBatch; ++b) {
                       if (!ok[b]) continue;
                       const unsigned bin = min((uint32_t)(now - born[b]) / binCycles, (uint32_t)(nBins - 1));
                       atomicAdd(&sT[(o[b] & (kRouteMax - 1)) * kRouteMax + (g[b] & (kRouteMax - 1))], 1u);     // tag_transfer_kernel's add
                       atomicAdd(&sHist[bin], 1u);                                                             // age_absorb_kernel's
                       if (o[b] >= (unsigned)nOrigins || g[b] >= (unsigned)nSinks) continue;                   // (no such route)
                       const unsigned w = (o[b] * (unsigned)nSinks + g[b]) * (unsigned)nBins + bin;
                       if (staged) {
                           atomicAdd(&sJoint[w], 1u);
                       } else {
                           const int pair = (int)(w & (unsigned)(kPairs - 1));
                           const int held = atomicCAS(&sIndex[pair], -1, (int)w);       // (w < 2^20)
                           if (held == -1 || held == (int)w) atomicAdd(&sJoint[pair], 1u);
                           else atomicAdd(&routeHist[w], 1ull);
                       }
                   }
               });
    __syncthreads();
    for (int b = threadIdx.x; b < nBins; b += kSliceBlock) {
        const unsigned k = sHist[b];
        if (k != 0u) atomicAdd(&hist[b], (unsigned long long)k);
    }
    {
        const unsigned k = sT[threadIdx.x];
        const int o = threadIdx.x / kRouteMax, g = threadIdx.x % kRouteMax;
        if (k != 0u && g < nSinks) atomicAdd(&transfer[o * nSinks + g], (unsigned long long)k);
    }
    for (int w = threadIdx.x; w < (staged ? jointWords : kPairs); w += kSliceBlock) {
        const unsigned k = sJoint[w];
        if (k != 0u) atomicAdd(&routeHist[staged ? w : sIndex[w]], (unsigned long long)k);
    }
}

// `cell` is 16-byte aligned; field is [nParent][nOrigins][2] = age sum, count
__global__ __launch_bounds__(kSliceBlock) void route_field_kernel(const int32_t* __restrict__ cell, const int64_t* __restrict__ gid,
                                                                  const uint32_t* __restrict__ birth,
                                                                  const uint8_t* __restrict__ origin, int64_t n,
                                                                  const int32_t* __restrict__ parentOf, int nDerived, int nOrigins,
                                                                  uint32_t now, unsigned long long* __restrict__ field) {
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
    uint32_t age[kSliceLoads][4];
    unsigned org[kSliceLoads][4];
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) age[k][j] = birth[id[k][j] != 0xFFFFFFFFu ? id[k][j] : 0u];
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) org[k][j] = origin[id[k][j] != 0xFFFFFFFFu ? id[k][j] : 0u];
#pragma unroll
    for (int k = 0; k < kSliceLoads; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) age[k][j] = now - age[k][j];
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
    constexpr unsigned long long kOne = 1ull << kRouteCountShift, kSumMask = kOne - 1ull;
    window_bins<unsigned long long, kRouteBins>(
        first, last,
        // a lane's four ids: where they agree (a sorted cloud fed by one origin) one add carries all four
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
            atomicAdd(&field[2 * (size_t)c + 1], w >> kRouteCountShift);
        });
}

// (both launchers: `cell` must be 16-byte aligned, as the arrays of the context's own cloud are)
hipError_t route_absorb(hipStream_t st, int32_t* cell, const int64_t* gid, const uint32_t* birth, const uint8_t* origin, int64_t n,
                        const uint32_t* mask, int64_t nDerived, const uint8_t* sinkGroup, unsigned long long* absorbed, uint32_t now,
                        int32_t binCycles, int32_t nBins, int32_t nOrigins, int32_t nSinks, unsigned long long* hist,
                        unsigned long long* transfer, unsigned long long* routeHist) {
    if (n <= 0) return hipSuccess;
    const SliceLaunch l = slice_launch(cell, n);
    if (!l.fits() || !l.vec || nDerived < 1 || nDerived > (int64_t)INT32_MAX || binCycles < 1 || nBins < 1 || nBins > kRouteMaxBins ||
        nOrigins < 1 || nOrigins > kRouteMax || nSinks < 1 || nSinks > kRouteMax)
        return hipErrorInvalidValue;
    const int maskWords = (int)((nDerived + 31) / 32);
    const int words = nOrigins * nSinks * nBins;            // (at most 2^20)
    const int jointWords = words <= kRouteJointWords ? words : 0;
    hipLaunchKernelGGL(route_absorb_kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock),
                       (size_t)(nBins + (jointWords ? jointWords : kRouteJointWords)) * sizeof(unsigned), st,
                       cell, gid, birth, origin, n, mask, (int)nDerived, maskWords, sinkGroup, absorbed, now, (uint32_t)binCycles,
                       (int)nBins, (int)nOrigins, (int)nSinks, jointWords, hist, transfer, routeHist);
    return hipGetLastError();
}

hipError_t route_field(hipStream_t st, const int32_t* cell, const int64_t* gid, const uint32_t* birth, const uint8_t* origin, int64_t n,
                       const int32_t* parentOf, int64_t nDerived, int64_t nParent, int32_t nOrigins, uint32_t now,
                       unsigned long long* field) {
    if (n <= 0) return hipSuccess;
    const SliceLaunch l = slice_launch(cell, n);
    if (n >= ((int64_t)1 << 31) || nDerived > (int64_t)INT32_MAX || !l.fits() || !l.vec || nOrigins < 1 || nOrigins > kRouteMax ||
        nParent * nOrigins >= ((int64_t)1 << 31))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(route_field_kernel, dim3((unsigned)l.blocks), dim3(kSliceBlock), 0, st, cell, gid, birth, origin, n, parentOf,
                       (int)nDerived, (int)nOrigins, now, field);
    return hipGetLastError();
}

}  // namespace cpf
