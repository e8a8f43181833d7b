// Tracer age (cpf_age_*): how long a particle of a recycled cloud has been live, without touching a step kernel, the sort or the
// recycling kernels.  birth[id] is a 32-bit stamp per PARTICLE ID -- the context's cycle counter when id last became live --, so
// neither sort moves it; an age is (uint32_t)(now - birth[id]), in cycles, and everything summed here is an integer: the same bits
// whatever the order of the cloud and of the workgroups (DESIGN.md "Age").
//
// Absorb (age_absorb_kernel).  sink_kernel's pass (cpf_recycle.hip: a slice of kAgeSlice ids per workgroup, 16-byte loads four in
// flight, the mask staged in LDS up to kAgeLdsWords words and read through L2 beyond, only changed quads stored) plus the residence-
// time histogram.  A workgroup without a hit ends where sink_kernel ends.  Otherwise the hits of a wave are gathered into a list in
// LDS and the wave's lanes take them in turn, as respawn_place_kernel's do -- eight a lane at a time, every gid load and then every
// birth gather of a batch in flight before the first is used: the sink's cells are neighbours in a sorted cloud, so a few
// workgroups hold all the hits and their chain of dependent loads is the kernel's tail.  Per hit: gid[s], birth[gid], the bin, one
// add to a histogram of 32-bit bins in LDS (a slice has at most kAgeSlice hits).  Non-zero bins leave as 64-bit global adds.
//
// Stamp (age_stamp_kernel).  Before a respawn: birth[gid[s]] = now for every slot with cell < 0.  A slot the respawn leaves dead has
// no age and is stamped again before it can next become live.  A workgroup without a dead slot leaves after its loads; the dead of
// a wave go through the same list, so a run of dead slots reads its ids with consecutive lanes.
//
// Field (age_field_kernel).  occupancy_kernel's shape (cpf_occupancy.hip): a slice of ids, derived -> parent, the window [lo, hi] of
// the slice's live ids, bins in LDS from the window's start, a contiguous flush.  Every lane's gid loads and birth gathers are all
// issued before the first is used (16 gathers in flight per lane).  A bin is ONE 64-bit word, count << kAgeCountShift | age sum:
// a slice holds at most 2^12 particles of age < 2^32, so the sum stays below 2^44 and the count below 2^20 -- one LDS atomic
// per add, and no carry from the sum into the count.  A window wider than the bins turns them into a direct-mapped cache of
// (word, cell) pairs, as occupancy's does; a particle that finds its bin taken by another cell adds to global memory itself.
#include <hip/hip_runtime.h>

#include "cpf_device.h"

namespace cpf {
namespace {

constexpr int kAgeBlock = 256;                              // 4 waves
constexpr int kAgeLoads = 4;                                // 16-byte loads of cell ids in flight per lane
constexpr int kAgeTrip = kAgeBlock * 4;                     // ids one round of loads covers
constexpr int kAgeSlice = kAgeTrip * kAgeLoads;             // ids per workgroup
constexpr int kAgeLdsWords = 2048;                          // mask words staged in LDS, as the sink's
constexpr int kAgeMaxBins = 4096;                           // residence-time bins (cpf_age_enable's limit): 16 KB of dynamic LDS at most
constexpr int kAgeBatch = 8;                                // list entries a lane takes at a time
constexpr int kAgeBins = 2048;                              // 64-bit field bins in LDS: 16 KB per workgroup
constexpr int kAgeTagBins = kAgeBins / 2;                   // as a cache: words in the lower half, cell ids (32-bit) in the third quarter
constexpr int kAgeCountShift = 44;                          // a bin: count << 44 | age sum
static_assert((kAgeTagBins & (kAgeTagBins - 1)) == 0, "bin = id & (kAgeTagBins - 1)");
static_assert(kAgeSlice <= (1 << 12), "a bin's age sum must stay below 2^44: at most 2^12 ages below 2^32");

// lanes below this one whose bit is set in a wave-wide ballot
__device__ inline unsigned lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// the four ids at i .. i + 3 (past the end: `pad`); `cell` is 16-byte aligned and i a multiple of 4: a full quad is one aligned load
__device__ inline int4 load_quad(const int32_t* __restrict__ cell, int64_t i, int64_t n, int pad) {
    if (i + 3 < n) return *reinterpret_cast<const int4*>(cell + i);
    int4 q;
    q.x = (i < n) ? cell[i] : pad;
    q.y = (i + 1 < n) ? cell[i + 1] : pad;
    q.z = (i + 2 < n) ? cell[i + 2] : pad;
    q.w = (i + 3 < n) ? cell[i + 3] : pad;
    return q;
}

// The chosen elements of a lane's four quads (bit 4 k + j of `chosen`: element j of quad k) are gathered into the wave's own list
// of slots within the slice (at most kAgeSlice / 4 entries); returns their number.  The list may be read behind a __syncthreads().
__device__ inline unsigned wave_list(unsigned chosen, unsigned short* __restrict__ list, int lane) {
    unsigned total = 0;
#pragma unroll
    for (int k = 0; k < kAgeLoads; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool mine = ((chosen >> (4 * k + j)) & 1u) != 0u;
            const unsigned long long b = __ballot(mine);
            if (mine) list[total + lanes_below(b)] = (unsigned short)(k * kAgeTrip + 4 * (int)threadIdx.x + j);
            total += (unsigned)__popcll(b);
        }
    return total;
}

// The wave's lanes take the list's entries kAgeBatch each at a time: f(ids, ok) gets the particle ids of the lane's entries (ok[b]
// false: no entry, or an id that is none of this cloud's -- ids[b] is 0 then, a valid index).  Every load of a batch is issued
// before the first is used: a slice where everybody is listed costs two passes of dependent loads, not sixteen.
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
__global__ __launch_bounds__(kAgeBlock) void age_absorb_kernel(int32_t* __restrict__ cell, const int64_t* __restrict__ gid,
                                                               const uint32_t* __restrict__ birth, int64_t n,
                                                               const uint32_t* __restrict__ mask, int nDerived, int maskWords,
                                                               unsigned long long* __restrict__ absorbed, uint32_t now,
                                                               uint32_t binCycles, int nBins, unsigned long long* __restrict__ hist) {
    extern __shared__ unsigned sHist[];
    __shared__ uint32_t sMask[kAgeLdsWords];
    __shared__ unsigned short sList[kAgeBlock / 64][kAgeSlice / 4];     // per wave: its hits (at most 16 per lane), slots within the slice
    __shared__ unsigned sHits;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t blockBase = (int64_t)blockIdx.x * kAgeSlice;
    const int64_t base = blockBase + 4 * (int64_t)threadIdx.x;
    int4 v[kAgeLoads];
#pragma unroll
    for (int k = 0; k < kAgeLoads; ++k) v[k] = load_quad(cell, base + (int64_t)k * kAgeTrip, n, 0);
    const bool staged = maskWords <= kAgeLdsWords;
    if (staged)
        for (int w = threadIdx.x; w < maskWords; w += kAgeBlock) sMask[w] = mask[w];
    if (threadIdx.x == 0) sHits = 0u;
    __syncthreads();
    // a live id (0 <= c < nDerived) whose bit is set; every other id -- CPF_CELL_LOST, CPF_CELL_FROZEN, ids beyond the mesh -- stays
    auto sunk = [&](int c) -> bool {
        if ((unsigned)c >= (unsigned)nDerived) return false;
        const uint32_t w = staged ? sMask[c >> 5] : mask[c >> 5];
        return ((w >> (c & 31)) & 1u) != 0u;
    };
    unsigned hits = 0, hit = 0;                             // hit, bit 4 k + j: element j of quad k was absorbed
#pragma unroll
    for (int k = 0; k < kAgeLoads; ++k) {
        const int64_t i = base + (int64_t)k * kAgeTrip;
        const bool hx = sunk(v[k].x), hy = sunk(v[k].y), hz = sunk(v[k].z), hw = sunk(v[k].w);   // (past the end: id 0 read as "no")
        const bool bx = hx && i < n, by = hy && i + 1 < n, bz = hz && i + 2 < n, bw = hw && i + 3 < n;
        hits += (unsigned)__popcll(__ballot(bx)) + (unsigned)__popcll(__ballot(by)) + (unsigned)__popcll(__ballot(bz)) +
                (unsigned)__popcll(__ballot(bw));
        if (!(bx || by || bz || bw)) continue;
        hit |= ((bx ? 1u : 0u) | (by ? 2u : 0u) | (bz ? 4u : 0u) | (bw ? 8u : 0u)) << (4 * k);
        if (i + 3 < n) {
            int4 q = v[k];
            if (bx) q.x = CPF_CELL_LOST;
            if (by) q.y = CPF_CELL_LOST;
            if (bz) q.z = CPF_CELL_LOST;
            if (bw) q.w = CPF_CELL_LOST;
            *reinterpret_cast<int4*>(cell + i) = q;
        } else {
            if (bx) cell[i] = CPF_CELL_LOST;
            if (by) cell[i + 1] = CPF_CELL_LOST;
            if (bz) cell[i + 2] = CPF_CELL_LOST;
            if (bw) cell[i + 3] = CPF_CELL_LOST;
        }
    }
    // (hits is the wave's sum in every lane: the ballots are wave-wide)
    if (lane == 0 && hits != 0u) atomicAdd(&sHits, hits);
    __syncthreads();
    const unsigned all = sHits;
    if (all == 0u) return;                                  // (the whole workgroup: sink_kernel's pass, nothing more)
    if (threadIdx.x == 0) atomicAdd(absorbed, (unsigned long long)all);
    for (int b = threadIdx.x; b < nBins; b += kAgeBlock) sHist[b] = 0u;
    const unsigned total = wave_list(hit, sList[wave], lane);
    __syncthreads();
    wave_take(sList[wave], total, blockBase, gid, n, lane, [&](const uint64_t* ids, const bool* ok) {
        uint32_t born[kAgeBatch];
#pragma unroll
        for (int b = 0; b < kAgeBatch; ++b) born[b] = birth[ids[b]];
#pragma unroll
        for (int b = 0; b < kAgeBatch; ++b)
            if (ok[b]) atomicAdd(&sHist[min((uint32_t)(now - born[b]) / binCycles, (uint32_t)(nBins - 1))], 1u);
    });
    __syncthreads();
    for (int b = threadIdx.x; b < nBins; b += kAgeBlock) {
        const unsigned k = sHist[b];
        if (k != 0u) atomicAdd(&hist[b], (unsigned long long)k);
    }
}

__global__ __launch_bounds__(kAgeBlock) void age_stamp_kernel(const int32_t* __restrict__ cell, const int64_t* __restrict__ gid,
                                                              uint32_t* __restrict__ birth, int64_t n, uint32_t now) {
    __shared__ unsigned short sList[kAgeBlock / 64][kAgeSlice / 4];     // per wave: its dead slots (at most 16 per lane)
    __shared__ unsigned sAny;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t blockBase = (int64_t)blockIdx.x * kAgeSlice;
    int4 v[kAgeLoads];
#pragma unroll
    for (int k = 0; k < kAgeLoads; ++k) v[k] = load_quad(cell, blockBase + (int64_t)k * kAgeTrip + 4 * (int64_t)threadIdx.x, n, 0);
    unsigned dead = 0;                                      // bit 4 k + j: element j of quad k is a dead slot (past the end: load_quad gave 0)
#pragma unroll
    for (int k = 0; k < kAgeLoads; ++k)
        dead |= ((v[k].x < 0 ? 1u : 0u) | (v[k].y < 0 ? 2u : 0u) | (v[k].z < 0 ? 4u : 0u) | (v[k].w < 0 ? 8u : 0u)) << (4 * k);
    if (threadIdx.x == 0) sAny = 0u;
    __syncthreads();
    const unsigned long long anyDead = __ballot(dead != 0u);
    if (lane == 0 && anyDead != 0ull) sAny = 1u;
    __syncthreads();
    if (sAny == 0u) return;                                 // (the whole workgroup: no dead slot in the slice)
    const unsigned total = wave_list(dead, sList[wave], lane);
    __syncthreads();
    wave_take(sList[wave], total, blockBase, gid, n, lane, [&](const uint64_t* ids, const bool* ok) {
#pragma unroll
        for (int b = 0; b < kAgeBatch; ++b)
            if (ok[b]) birth[ids[b]] = now;
    });
}

// `cell` is 16-byte aligned
__global__ __launch_bounds__(kAgeBlock) void age_field_kernel(const int32_t* __restrict__ cell, const int64_t* __restrict__ gid,
                                                              const uint32_t* __restrict__ birth, int64_t n,
                                                              const int32_t* __restrict__ parentOf, int nDerived, uint32_t now,
                                                              unsigned long long* __restrict__ field) {
    __shared__ unsigned long long sBins[kAgeBins];
    __shared__ int sLo[kAgeBlock / 64], sHi[kAgeBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * kAgeSlice + 4 * (int64_t)threadIdx.x;
    int4 v[kAgeLoads];
#pragma unroll
    for (int k = 0; k < kAgeLoads; ++k) v[k] = load_quad(cell, base + (int64_t)k * kAgeTrip, n, -1);
    // the ids: gid is 8-byte elements behind a 256-byte aligned allocation or a caller's array -- plain 8-byte loads, four
    // consecutive per lane; past the end and ids that are none of this cloud's: id 0 (their slot is not live, see below)
    uint32_t id[kAgeLoads][4];
#pragma unroll
    for (int k = 0; k < kAgeLoads; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t s = base + (int64_t)k * kAgeTrip + j;
            const uint64_t g = s < n ? (uint64_t)(gid ? gid[s] : s) : 0ull;
            id[k][j] = g < (uint64_t)n ? (uint32_t)g : 0xFFFFFFFFu;     // (n < 2^31)
        }
    uint32_t age[kAgeLoads][4];
#pragma unroll
    for (int k = 0; k < kAgeLoads; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) age[k][j] = now - birth[id[k][j] != 0xFFFFFFFFu ? id[k][j] : 0u];
    // derived -> parent; CPF_CELL_LOST, every other negative code, ids beyond the mesh and slots without an id of this cloud become -1
    auto live = [&](int c, uint32_t i) -> int {
        if ((unsigned)c >= (unsigned)nDerived || i == 0xFFFFFFFFu) return -1;
        return parentOf ? parentOf[c] : c;
    };
    unsigned lo = 0xFFFFFFFFu;                                  // (a negative id is a huge unsigned: the minimum skips it)
    int hi = -1;
#pragma unroll
    for (int k = 0; k < kAgeLoads; ++k) {
        v[k].x = live(v[k].x, id[k][0]); v[k].y = live(v[k].y, id[k][1]); v[k].z = live(v[k].z, id[k][2]); v[k].w = live(v[k].w, id[k][3]);
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
    for (int w = 0; w < kAgeBlock / 64; ++w) {
        lo = min(lo, (unsigned)sLo[w]);
        hi = max(hi, sHi[w]);
    }
    if (hi < 0) return;                                         // no live id in the slice (the whole workgroup leaves)
    constexpr unsigned long long kOne = 1ull << kAgeCountShift, kSumMask = kOne - 1ull;
    // a lane's four ids: where they agree (the rule in a sorted cloud) one add carries all four
    auto quad = [&](const int4& q, const uint32_t* a, auto add) {
        if (q.x >= 0 && q.x == q.y && q.y == q.z && q.z == q.w) {
            add(q.x, 4ull * kOne + ((unsigned long long)a[0] + a[1] + a[2] + a[3]));
        } else {
            if (q.x >= 0) add(q.x, kOne + a[0]);
            if (q.y >= 0) add(q.y, kOne + a[1]);
            if (q.z >= 0) add(q.z, kOne + a[2]);
            if (q.w >= 0) add(q.w, kOne + a[3]);
        }
    };
    auto to_field = [&](int c, unsigned long long w) {
        atomicAdd(&field[2 * (size_t)c], w & kSumMask);
        atomicAdd(&field[2 * (size_t)c + 1], w >> kAgeCountShift);
    };
    const int first = (int)lo, width = hi - first + 1;
    if (width <= kAgeBins) {
        for (int b = threadIdx.x; b < width; b += kAgeBlock) sBins[b] = 0ull;
        __syncthreads();
        auto add = [&](int c, unsigned long long w) { atomicAdd(&sBins[c - first], w); };
#pragma unroll
        for (int k = 0; k < kAgeLoads; ++k) quad(v[k], age[k], add);
        __syncthreads();
        for (int b = threadIdx.x; b < width; b += kAgeBlock) {
            const unsigned long long w = sBins[b];
            if (w != 0ull) to_field(first + b, w);
        }
    } else {
        unsigned long long* sWord = sBins;
        int* sTag = reinterpret_cast<int*>(sBins + kAgeTagBins);
        for (int b = threadIdx.x; b < kAgeTagBins; b += kAgeBlock) { sWord[b] = 0ull; sTag[b] = -1; }
        __syncthreads();
        auto add = [&](int c, unsigned long long w) {
            const int b = c & (kAgeTagBins - 1);
            const int held = atomicCAS(&sTag[b], -1, c);
            if (held == -1 || held == c) atomicAdd(&sWord[b], w);
            else to_field(c, w);
        };
#pragma unroll
        for (int k = 0; k < kAgeLoads; ++k) quad(v[k], age[k], add);
        __syncthreads();
        for (int b = threadIdx.x; b < kAgeTagBins; b += kAgeBlock) {
            const unsigned long long w = sWord[b];
            if (w != 0ull) to_field(sTag[b], w);
        }
    }
}

// (every launcher: `cell` must be 16-byte aligned, as the arrays of the context's own cloud are)
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

hipError_t age_absorb(hipStream_t st, int32_t* cell, const int64_t* gid, const uint32_t* birth, int64_t n, const uint32_t* mask,
                      int64_t nDerived, unsigned long long* absorbed, uint32_t now, int32_t binCycles, int32_t nBins,
                      unsigned long long* hist) {
    if (n <= 0) return hipSuccess;
    const int64_t blocks = (n + kAgeSlice - 1) / kAgeSlice;
    if (blocks > (int64_t)INT32_MAX || nDerived > (int64_t)INT32_MAX || binCycles < 1 || nBins < 1 || nBins > kAgeMaxBins ||
        !aligned16(cell))
        return hipErrorInvalidValue;
    const int maskWords = (int)((nDerived + 31) / 32);
    hipLaunchKernelGGL(age_absorb_kernel, dim3((unsigned)blocks), dim3(kAgeBlock), (size_t)nBins * sizeof(unsigned), st, cell, gid,
                       birth, n, mask, (int)nDerived, maskWords, absorbed, now, (uint32_t)binCycles, (int)nBins, hist);
    return hipGetLastError();
}

hipError_t age_stamp(hipStream_t st, const int32_t* cell, const int64_t* gid, uint32_t* birth, int64_t n, uint32_t now) {
    if (n <= 0) return hipSuccess;
    const int64_t blocks = (n + kAgeSlice - 1) / kAgeSlice;
    if (blocks > (int64_t)INT32_MAX || !aligned16(cell)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(age_stamp_kernel, dim3((unsigned)blocks), dim3(kAgeBlock), 0, st, cell, gid, birth, n, now);
    return hipGetLastError();
}

hipError_t age_field(hipStream_t st, const int32_t* cell, const int64_t* gid, const uint32_t* birth, int64_t n,
                     const int32_t* parentOf, int64_t nDerived, uint32_t now, unsigned long long* field) {
    if (n <= 0) return hipSuccess;
    if (n >= ((int64_t)1 << 31) || nDerived > (int64_t)INT32_MAX || !aligned16(cell)) return hipErrorInvalidValue;
    const int64_t blocks = (n + kAgeSlice - 1) / kAgeSlice;
    hipLaunchKernelGGL(age_field_kernel, dim3((unsigned)blocks), dim3(kAgeBlock), 0, st, cell, gid, birth, n, parentOf, (int)nDerived,
                       now, field);
    return hipGetLastError();
}

}  // namespace cpf
