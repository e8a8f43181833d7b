// The re-sort by cell (cpf_sort_by_cell*; gfx950 / CDNA4, wave64): keys and 32-byte records, a key sort -- this library's radix
// sort ("sort_method" 2, the default) or hipcub::DeviceRadixSort (0, the order the tests compare with) -- then ONE tail for both:
// the occupied-cell census, the gather out of the records, the velocity triples.
#include "cpf_device.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace cpf {

static inline dim3 grid_for(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

__global__ void iota_kernel(int32_t* p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) p[i] = (int32_t)i;
}
__global__ void gather3_kernel(const double* __restrict__ src, double* __restrict__ dst,
                               const int32_t* __restrict__ perm, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) {
        const int64_t j = perm[i];
        dst[3 * i] = src[3 * j]; dst[3 * i + 1] = src[3 * j + 1]; dst[3 * i + 2] = src[3 * j + 2];
    }
}

// ------------------------------------------------------------------------------------------------
// sort by cell: radix sort (cell, index) pairs on the low bits only, then gather every array.
// Stable and deterministic, so the order of particles is reproducible run to run.
// ------------------------------------------------------------------------------------------------
// Sort key = (cell, position inside the cell's bounding box quantised per axis): particles that share a wave then
// also share a neighbourhood INSIDE the cell, so they cross the same faces in the same round.  The bit layout
// (bits per axis, axis significance) is chosen at mesh ingest (cpf_mesh.cpp): 4 x 4 x 4 for 3-D meshes, 4 x 32 for
// a 2-D case like pitzDaily.  Measured on the bench cloud: rounds per wave 2.68 (cell only) -> 2.31 -> 2.23.
struct SubKey { int bits[3]; int order[3]; };
#ifndef CPF_SORT_XCD
#define CPF_SORT_XCD 1
#endif
// (the particle's (x, y, z, id) also goes out as ONE 32-byte record, which the sort's gather then fetches with one L2 transaction
// instead of four -- see sort_by_cell)
struct __attribute__((aligned(16))) Pair64 { double a, b; };
__device__ __forceinline__ void put_aos(double* __restrict__ aos, int64_t i, double px, double py, double pz, const int64_t* __restrict__ gid) {
    Pair64* rec = reinterpret_cast<Pair64*>(aos) + 2 * i;
    rec[0] = Pair64{px, py};
    rec[1] = Pair64{pz, __longlong_as_double(gid ? gid[i] : 0ll)};
}
__device__ __forceinline__ uint32_t sort_key_of(double px, double py, double pz, int32_t c, const float* __restrict__ cellBox,
                                                const int32_t* __restrict__ rank, const SubKey& sk, int subBits) {
    if (c < 0) return 0xFFFFFFFFu;                          // lost / frozen particles go to the tail
    const float* b = cellBox + 6 * (int64_t)c;              // lo.xyz, 2^bits / extent.xyz
    const float r[3] = {((float)px - b[0]) * b[3], ((float)py - b[1]) * b[4], ((float)pz - b[2]) * b[5]};
    uint32_t sub = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = sk.order[k];
        const int q = min((1 << sk.bits[a]) - 1, max(0, (int)(a == 0 ? r[0] : (a == 1 ? r[1] : r[2]))));
        sub = (sub << sk.bits[a]) | (uint32_t)q;
    }
    // (rank: the cell's place along the mesh layer's Morton curve instead of its id -- sparse clouds, see sort_by_cell)
    return ((uint32_t)(rank ? rank[c] : c) << subBits) | sub;
}
__global__ void sort_keys_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                 const double* __restrict__ z, const int32_t* __restrict__ cell,
                                 const float* __restrict__ cellBox, const int32_t* __restrict__ rank, SubKey sk, int subBits,
                                 uint32_t* __restrict__ keys, int64_t n, const int64_t* __restrict__ gid, double* __restrict__ aos) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double px = x[i], py = y[i], pz = z[i];
    put_aos(aos, i, px, py, pz, gid);
    keys[i] = sort_key_of(px, py, pz, cell[i], cellBox, rank, sk, subBits);
}
// the gather out of the 32-byte records: positions and id with one transaction; the cell out of the sorted key, or fetched.
// kGatherItems destinations per thread, all their record loads in flight at once: the chain permutation -> record -> store is
// two memory latencies long.  MEASURED: 1 / 2 / 4 / 8 destinations per thread: 0.58 / 0.54 / 0.53-0.54 / 0.53-0.55 ms per sort of 1e7
// (pitzDaily), 0.26-0.27 / 0.244-0.248 / 0.255 / 0.258 of 4e6 (TJunction).
// The permutation, the keys and the output arrays are streamed past the caches (non-temporal loads / stores: the L2 is for the
// records' lines): -1.4 % (pitzDaily), -2.9 % (TJunction) per sort, three alternating runs each.
#ifndef CPF_GATHER_ITEMS
#define CPF_GATHER_ITEMS 2
#endif
#ifndef CPF_GATHER_NT
#define CPF_GATHER_NT 1
#endif
constexpr int kGatherItems = CPF_GATHER_ITEMS;
__global__ __launch_bounds__(kBlock) void gather_aos_kernel(const double* __restrict__ aos, const int32_t* __restrict__ cell,
                                                            double* __restrict__ ox, double* __restrict__ oy, double* __restrict__ oz,
                                                            int32_t* __restrict__ ocell, int64_t* __restrict__ ogid,
                                                            const int32_t* __restrict__ perm, const uint32_t* __restrict__ keys, int nSub, int64_t n,
                                                            bool cellFromKey) {
    // (workgroups go to the 8 XCDs in turn: give every XCD one contiguous eighth of the destinations, so that the records of
    //  a 128-byte source line -- whose destinations are neighbours -- are fetched into ONE L2; the grid is 8 * ceil(blocks / 8))
#if CPF_SORT_XCD
    const int64_t per = gridDim.x >> 3;
    const int64_t i0 = (((int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3)) * kBlock * kGatherItems) + threadIdx.x;
#else
    const int64_t i0 = (int64_t)blockIdx.x * kBlock * kGatherItems + threadIdx.x;
#endif
    int64_t j[kGatherItems]; uint32_t k[kGatherItems];
#pragma unroll
    for (int u = 0; u < kGatherItems; ++u) {
        const int64_t i = i0 + (int64_t)u * kBlock;
#if CPF_GATHER_NT
        j[u] = i < n ? __builtin_nontemporal_load(perm + i) : 0;
        k[u] = (cellFromKey && i < n) ? __builtin_nontemporal_load(keys + i) : 0xFFFFFFFFu;
#else
        j[u] = i < n ? perm[i] : 0;
        k[u] = (cellFromKey && i < n) ? keys[i] : 0xFFFFFFFFu;
#endif
    }
    Pair64 lo[kGatherItems], hi[kGatherItems]; int32_t cc[kGatherItems];
#pragma unroll
    for (int u = 0; u < kGatherItems; ++u) {
        const Pair64* rec = reinterpret_cast<const Pair64*>(aos) + 2 * j[u];
        lo[u] = rec[0]; hi[u] = rec[1];
        cc[u] = (cellFromKey && k[u] != 0xFFFFFFFFu) ? (int32_t)(k[u] >> nSub) : cell[j[u]];
    }
#pragma unroll
    for (int u = 0; u < kGatherItems; ++u) {
        const int64_t i = i0 + (int64_t)u * kBlock;
        if (i < n) {
#if CPF_GATHER_NT
            __builtin_nontemporal_store(lo[u].a, ox + i); __builtin_nontemporal_store(lo[u].b, oy + i); __builtin_nontemporal_store(hi[u].a, oz + i);
            __builtin_nontemporal_store(cc[u], ocell + i);
            if (ogid) __builtin_nontemporal_store((int64_t)__double_as_longlong(hi[u].b), ogid + i);
#else
            ox[i] = lo[u].a; oy[i] = lo[u].b; oz[i] = hi[u].a;
            ocell[i] = cc[u];
            if (ogid) ogid[i] = __double_as_longlong(hi[u].b);
#endif
        }
    }
}
static inline dim3 grid8_for(int64_t n) { const int64_t b = (n + kBlock * kGatherItems - 1) / (kBlock * kGatherItems); return dim3((unsigned)((b + 7) / 8 * 8)); }
__global__ void copy_cells_kernel(int32_t* __restrict__ cell, const int32_t* __restrict__ sc, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) cell[i] = sc[i];
}

// ------------------------------------------------------------------------------------------------
// The key sort, hand-written (round 5; option "sort_method" 2, the default; 0 = hipcub::DeviceRadixSort): a stable LSD radix sort
// of (key, index) pairs with digits of <= 8 bits (as many passes as the library's) as chunked counting sorts.
//   * The cloud is cut into up to 1024 contiguous chunks of whole 4096-element tiles, one workgroup (4 waves) each.  Inside a tile
//     wave w owns elements [1024 w, 1024 (w + 1)) and ranks them in order against private per-wave counters in LDS: stability then
//     needs no ordering BETWEEN waves -- wave w's elements rank behind those of the waves before it.  Lanes with equal digits find
//     each other with one ballot per digit bit; rank = the counter + the peers before me; the group's first lane advances the counter.
//   * One pass over [wave][bin] turns the counters into first positions; the tile is written to LDS in digit order and copied out
//     with the bins' running global positions, so that every bin receives ONE contiguous run per tile (a first version with
//     11-bit digits and no reorder wrote 8 bytes per 64-byte line on a random digit: 0.65 ms per 1e7; docs/experiments.md).
//   * Per pass: rt_hist_kernel (per-chunk digit counts, bin-major: 16-byte loads, a tile's worth in flight per thread),
//     rt_scan_kernel (one wave per bin over the chunks), rt_scatter_kernel.  The first pass reads no index array (the index is the
//     position), the last writes no keys unless the gather wants the cell from them.
// MEASURED (profiles/r05_sort_breakdown.json; 1e7 particles on pitzDaily sorted 25 cycles of D = 1.5e-5 ago): counts 10-13 us, scan
// 5, scatter 56 per pass -- 0.54 ms per sort against 0.64 with the library's onesweep passes (88 us each); TJunction, 4e6 particles,
// 24 key bits: 0.24 against 0.27.  The scatter is bound by its own ranking arithmetic (8 ballots and ~65 vector instructions per
// element: coalesced stores instead of the scatter, or no loads at all, change its time by < 7 %); 256 x 16, 256 x 8, 512 x 8 and
// 512 x 16 threads x items tie.
// ------------------------------------------------------------------------------------------------
struct SortPlan {
    int passes, bits[4], shift[4];
    int nChunks;
    int64_t chunk;       // elements per chunk: whole tiles
};
static inline size_t sort_al(size_t b) { return (b + 255) & ~(size_t)255; }
#ifndef CPF_RT_STHREADS
#define CPF_RT_STHREADS 256
#endif
#ifndef CPF_RT_SITEMS
#define CPF_RT_SITEMS 16
#endif
constexpr int kRtThreads = 256, kRtWaves = 4, kRtMaxBits = 8, kRtMaxChunks = 1024;        // the counting and scanning kernels
constexpr int kRtSThreads = CPF_RT_STHREADS, kRtSWaves = kRtSThreads / 64, kRtItems = CPF_RT_SITEMS, kRtTile = kRtSThreads * kRtItems;   // the scatter
static_assert(kRtTile % (kRtThreads * 4) == 0, "a tile is whole batches of the counting kernel's 16-byte loads");
static SortPlan rt_plan(int64_t n, int endBit) {
    SortPlan p{};
    p.passes = (endBit + kRtMaxBits - 1) / kRtMaxBits;
    const int d = (endBit + p.passes - 1) / p.passes;
    for (int k = 0; k < p.passes; ++k) { p.shift[k] = k * d; p.bits[k] = std::min(d, endBit - k * d); }
    int64_t chunk = (n + kRtMaxChunks - 1) / kRtMaxChunks;
    chunk = std::max<int64_t>(kRtTile, (chunk + kRtTile - 1) / kRtTile * kRtTile);
    p.chunk = chunk;
    p.nChunks = (int)((n + chunk - 1) / chunk);
    return p;
}

// counts of one digit per chunk, BIN-major: counts[bin * stride + chunk].  A chunk is whole tiles of 4096 keys, the key buffers
// are 256-byte aligned: every thread has its 16-byte loads of a tile in flight at once (one memory latency per tile, not one per
// key), counts in per-wave private LDS histograms; a wave whose 64 x 4 keys share a digit (the high digits of an almost sorted
// cloud) adds them with one atomic.
constexpr int kRtHistBatch = 4;       // uint4 loads in flight per thread: 4 x 4 x 256 = 4096 keys
__global__ __launch_bounds__(kRtThreads) void rt_hist_kernel(const uint32_t* __restrict__ keys, int64_t n, int64_t chunk, int shift, int bits,
                                                             uint32_t* __restrict__ counts, int stride) {
    extern __shared__ unsigned sH[];                    // [kRtWaves][bins]
    const int bins = 1 << bits;
    const int wave = threadIdx.x >> 6;
    for (int b = threadIdx.x; b < kRtWaves * bins; b += kRtThreads) sH[b] = 0u;
    __syncthreads();
    unsigned* mine = sH + wave * bins;
    const uint32_t mask = (uint32_t)bins - 1u;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = min(n, lo + chunk);
    for (int64_t t0 = lo; t0 < hi; t0 += (int64_t)kRtHistBatch * 4 * kRtThreads) {
        uint4 v[kRtHistBatch];
#pragma unroll
        for (int u = 0; u < kRtHistBatch; ++u) {
            const int64_t i = t0 + ((int64_t)u * kRtThreads + threadIdx.x) * 4;
            if (i + 3 < hi) v[u] = *reinterpret_cast<const uint4*>(keys + i);
            else {
                v[u].x = i < hi ? keys[i] : 0u; v[u].y = i + 1 < hi ? keys[i + 1] : 0u; v[u].z = i + 2 < hi ? keys[i + 2] : 0u; v[u].w = 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < kRtHistBatch; ++u) {
            const int64_t i = t0 + ((int64_t)u * kRtThreads + threadIdx.x) * 4;
            const int live = (int)max<int64_t>(0, min<int64_t>(4, hi - i));
            const uint32_t d0 = (v[u].x >> shift) & mask, d1 = (v[u].y >> shift) & mask, d2 = (v[u].z >> shift) & mask, d3 = (v[u].w >> shift) & mask;
            const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)d0);
            const bool same = live == 4 && d0 == first && d1 == first && d2 == first && d3 == first;
            if (__ballot(same) == ~0ull) {
                if ((threadIdx.x & 63) == 0) atomicAdd(&mine[first], 256u);
            } else {
                if (live > 0) atomicAdd(&mine[d0], 1u);
                if (live > 1) atomicAdd(&mine[d1], 1u);
                if (live > 2) atomicAdd(&mine[d2], 1u);
                if (live > 3) atomicAdd(&mine[d3], 1u);
            }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += kRtThreads) {
        unsigned c = 0;
#pragma unroll
        for (int w = 0; w < kRtWaves; ++w) c += sH[w * bins + b];
        counts[(int64_t)b * stride + blockIdx.x] = c;
    }
}
// counts[bin][chunk] -> the bin's elements in the chunks BEFORE this one (in place); totals[bin] = the bin's size.  One wave per
// bin: a lane sums its run of consecutive chunks, one shuffle scan across the lanes, the run is written back.
__global__ __launch_bounds__(kRtThreads) void rt_scan_kernel(uint32_t* __restrict__ counts, int nChunks, int stride, int bins,
                                                             uint32_t* __restrict__ totals) {
    const int bin = blockIdx.x * kRtWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (bin >= bins) return;
    constexpr int PER = kRtMaxChunks / 64;               // 16
    uint32_t* row = counts + (int64_t)bin * stride;
    uint32_t v[PER]; uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) { const int c = lane * PER + k; v[k] = c < nChunks ? row[c] : 0u; sum += v[k]; }
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t up = __shfl_up(incl, off, 64); if (lane >= off) incl += up; }
    uint32_t run = incl - sum;
#pragma unroll
    for (int k = 0; k < PER; ++k) { const int c = lane * PER + k; if (c < nChunks) row[c] = run; run += v[k]; }
    if (lane == 63) totals[bin] = incl;
}

template <int BITS>
__global__ __launch_bounds__(kRtSThreads) void rt_scatter_kernel(const uint32_t* __restrict__ keysIn, const int32_t* __restrict__ idxIn,
                                                                uint32_t* __restrict__ keysOut, int32_t* __restrict__ idxOut, int64_t n,
                                                                int64_t chunk, int shift, const uint32_t* __restrict__ before, int stride,
                                                                const uint32_t* __restrict__ totals) {
    constexpr int BINS = 1 << BITS;
    __shared__ uint32_t sKey[kRtTile];
    __shared__ int32_t sIdx[kRtTile];
    __shared__ unsigned sCnt[kRtSWaves][BINS];          // per tile: the waves' digit counts, then their first positions in the tile
    __shared__ unsigned sBinStart[BINS + 1];           // per tile: first position of a bin inside the tile
    __shared__ unsigned sGlobal[BINS];                 // running: where the bin's next element of this chunk goes
    __shared__ unsigned sScan[kRtSThreads];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t mask = (uint32_t)BINS - 1u;
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    // bin starts of the whole array = exclusive scan of the totals (BINS <= 256 == kRtThreads), + what the chunks before this one hold
    {
        const unsigned tot = threadIdx.x < BINS ? totals[threadIdx.x] : 0u;
        unsigned incl = tot;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const unsigned up = __shfl_up(incl, off, 64); if (lane >= off) incl += up; }
        if (lane == 63) sScan[wave] = incl;
        __syncthreads();
        unsigned base = 0;
        for (int w = 0; w < wave; ++w) base += sScan[w];
        if (threadIdx.x < BINS) sGlobal[threadIdx.x] = base + incl - tot + before[(int64_t)threadIdx.x * stride + blockIdx.x];
        __syncthreads();                                   // (sScan is used again by the first tile)
    }
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = min(n, lo + chunk);
    for (int64_t t0 = lo; t0 < hi; t0 += kRtTile) {
        const int tileN = (int)min<int64_t>(kRtTile, hi - t0);
        for (int b = lane; b < BINS; b += 64) sCnt[wave][b] = 0u;
        __syncthreads();                                   // (also: the previous tile's copy-out has left sKey / sIdx / sBinStart)
        // ---- load the wave's 1024 elements, rank them in order against the wave's counters
        uint32_t k[kRtItems]; int32_t v[kRtItems]; unsigned rnk[kRtItems];
        const int sub = wave * (kRtTile / kRtSWaves);
#pragma unroll
        for (int s = 0; s < kRtItems; ++s) {
            const int j = sub + s * 64 + lane;
            const int64_t i = t0 + j;
            k[s] = j < tileN ? keysIn[i] : 0xFFFFFFFFu;
            v[s] = j < tileN ? (idxIn ? idxIn[i] : (int32_t)i) : 0;
        }
#pragma unroll
        for (int s = 0; s < kRtItems; ++s) {
            const int j = sub + s * 64 + lane;
            const bool live = j < tileN;
            const uint32_t d = (k[s] >> shift) & mask;
            unsigned long long same = __ballot(live);
#pragma unroll
            for (int b = 0; b < BITS; ++b) {
                const unsigned long long one = __ballot(((d >> b) & 1u) != 0u);
                same &= ((d >> b) & 1u) ? one : ~one;
            }
            if (live) {
                const unsigned first = sCnt[wave][d];           // (every lane of the group reads before its first lane writes)
                rnk[s] = first + (unsigned)__popcll(same & lt);
                if ((same & lt) == 0ull) sCnt[wave][d] = first + (unsigned)__popcll(same);
            } else rnk[s] = 0;
        }
        __syncthreads();
        // ---- counts -> the waves' first positions inside each bin; bins' first positions inside the tile
        unsigned binCount = 0;
        if (threadIdx.x < BINS) {
            unsigned run = 0;
#pragma unroll
            for (int w = 0; w < kRtSWaves; ++w) { const unsigned c = sCnt[w][threadIdx.x]; sCnt[w][threadIdx.x] = run; run += c; }
            binCount = run;
        }
        {   // exclusive scan of binCount over the bins (BINS <= 256 == kRtThreads)
            unsigned incl = binCount;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) { const unsigned up = __shfl_up(incl, off, 64); if (lane >= off) incl += up; }
            if (lane == 63) sScan[wave] = incl;
            __syncthreads();
            unsigned base = 0;
            for (int w = 0; w < wave; ++w) base += sScan[w];
            if (threadIdx.x < BINS) sBinStart[threadIdx.x] = base + incl - binCount;
        }
        __syncthreads();
        // ---- the tile in digit order in LDS
#pragma unroll
        for (int s = 0; s < kRtItems; ++s) {
            const int j = sub + s * 64 + lane;
            if (j < tileN) {
                const uint32_t d = (k[s] >> shift) & mask;
                const unsigned pos = sBinStart[d] + sCnt[wave][d] + rnk[s];
                sKey[pos] = k[s]; sIdx[pos] = v[s];
            }
        }
        __syncthreads();
        // ---- out: element j of the ordered tile is the (j - start of its bin)-th of its bin in this tile
        for (int j = threadIdx.x; j < tileN; j += kRtSThreads) {
            const uint32_t kk = sKey[j];
            const uint32_t d = (kk >> shift) & mask;
            const unsigned g = sGlobal[d] + ((unsigned)j - sBinStart[d]);
            if (keysOut) keysOut[g] = kk;
            idxOut[g] = sIdx[j];
        }
        __syncthreads();
        if (threadIdx.x < BINS) sGlobal[threadIdx.x] += binCount;
    }
}

// how many cells hold particles: the runs of equal cell ids in the sorted keys (lost / frozen particles -- the all-ones key --
// do not count).  out[0] += runs, out[1] += live particles
__global__ __launch_bounds__(kBlock) void count_cell_runs_kernel(const uint32_t* __restrict__ keys, int64_t n, int nSub, uint32_t lostKey,
                                                                 unsigned long long* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool live = false, start = false;
    if (i < n) {
        const uint32_t k = keys[i];
        live = k != lostKey;
        start = live && (i == 0 || (keys[i - 1] >> nSub) != (k >> nSub));
    }
    const unsigned runs = (unsigned)__popcll(__builtin_amdgcn_ballot_w64(start)), alive = (unsigned)__popcll(__builtin_amdgcn_ballot_w64(live));
    __shared__ unsigned sR, sA;
    if (threadIdx.x == 0) { sR = 0; sA = 0; }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { atomicAdd(&sR, runs); atomicAdd(&sA, alive); }
    __syncthreads();
    if (threadIdx.x == 0 && (sR | sA)) { atomicAdd(&out[0], (unsigned long long)sR); atomicAdd(&out[1], (unsigned long long)sA); }
}

// ------------------------------------------------------------------------------------------------
// The host side.  The caller's scratch, one layout for both key sorts, every buffer 256-byte aligned:
//   keys[0] | keys[1] | idx[0] | idx[1] | aux | stage
// ------------------------------------------------------------------------------------------------
constexpr size_t kRtCountsBytes = (size_t)kRtMaxChunks * (1u << kRtMaxBits) * 4, kRtTotalsBytes = (1u << kRtMaxBits) * 4;
struct SortScratch {
    uint32_t* keys[2];      // 4 n bytes each
    int32_t* idx[2];        // 4 n bytes each
    char* aux;              // method 0: the library's temporary storage, auxBytes of it; else the per-chunk counts, then the totals
    size_t auxBytes;
    double* stage;          // 32 n bytes: the (x, y, z, id) records, then the velocity triples
    size_t bytes;           // all of it
};
static SortScratch carve_sort_scratch(void* scratch, int64_t n, int endBit, int method) {
    SortScratch s{};
    size_t off = 0;
    auto take = [&](size_t b) { char* p = scratch ? (char*)scratch + off : nullptr; off += sort_al(b); return p; };
    for (auto& k : s.keys) k = (uint32_t*)take(4 * (size_t)n);
    for (auto& i : s.idx) i = (int32_t*)take(4 * (size_t)n);
    if (method == 0)
        (void)hipcub::DeviceRadixSort::SortPairs(nullptr, s.auxBytes, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                           (const int32_t*)nullptr, (int32_t*)nullptr, (int)n, 0, endBit);
    else
        s.auxBytes = sort_al(kRtCountsBytes) + kRtTotalsBytes;
    s.aux = take(s.auxBytes);
    s.stage = (double*)take(32 * (size_t)n);
    s.bytes = off;
    return s;
}
size_t sort_scratch_bytes(int64_t n, int endBit) {
    return std::max(carve_sort_scratch(nullptr, n, endBit, 0).bytes, carve_sort_scratch(nullptr, n, endBit, 2).bytes);
}

// What a key sort hands to the tail.  Both take the keys in keys[0] and sort the low endBit bits of them (they cover the cell bits
// + sub-cell bits; the all-ones key of lost / frozen particles sorts last).
struct SortedPairs {
    const uint32_t* keys;   // sorted; null where nobody wanted them
    const int32_t* perm;    // element i of the sorted cloud is element perm[i] of the unsorted one
    int32_t* spent;         // the index buffer that does not hold perm: the in-place form routes the cells through it
};
static hipError_t rt_sort_pairs(hipStream_t st, const SortScratch& s, int64_t n, int endBit, bool keepKeys, SortedPairs* out) {
    const SortPlan p = rt_plan(n, endBit);
    uint32_t* counts = (uint32_t*)s.aux;
    uint32_t* totals = (uint32_t*)(s.aux + sort_al(kRtCountsBytes));
    const int stride = kRtMaxChunks;
    const uint32_t* kin = s.keys[0]; const int32_t* iin = nullptr;
    for (int k = 0; k < p.passes; ++k) {
        const int bins = 1 << p.bits[k];
        hipLaunchKernelGGL(rt_hist_kernel, dim3(p.nChunks), dim3(kRtThreads), (size_t)kRtWaves * bins * 4, st, kin, n, p.chunk, p.shift[k], p.bits[k],
                           counts, stride);
        hipLaunchKernelGGL(rt_scan_kernel, dim3((bins + kRtWaves - 1) / kRtWaves), dim3(kRtThreads), 0, st, counts, p.nChunks, stride, bins, totals);
        const bool last = k == p.passes - 1;
        uint32_t* kout = s.keys[kin == s.keys[0]];
        int32_t* iout = s.idx[iin == s.idx[0]];
        uint32_t* ko = (last && !keepKeys) ? nullptr : kout;
#define CPF_RT_LAUNCH(B) hipLaunchKernelGGL(rt_scatter_kernel<B>, dim3(p.nChunks), dim3(kRtSThreads), 0, st, kin, iin, ko, iout, n, p.chunk, p.shift[k], counts, stride, totals)
        switch (p.bits[k]) {
            case 1: CPF_RT_LAUNCH(1); break; case 2: CPF_RT_LAUNCH(2); break; case 3: CPF_RT_LAUNCH(3); break; case 4: CPF_RT_LAUNCH(4); break;
            case 5: CPF_RT_LAUNCH(5); break; case 6: CPF_RT_LAUNCH(6); break; case 7: CPF_RT_LAUNCH(7); break; default: CPF_RT_LAUNCH(8); break;
        }
#undef CPF_RT_LAUNCH
        kin = kout; iin = iout;
    }
    *out = {keepKeys ? kin : nullptr, iin, s.idx[iin == s.idx[0]]};
    return hipGetLastError();
}
// (the library reads the indices it sorts along with the keys: sort_by_cell has written 0 ... n - 1 to idx[0])
static hipError_t library_sort_pairs(hipStream_t st, const SortScratch& s, int64_t n, int endBit, SortedPairs* out) {
    size_t tmpBytes = s.auxBytes;
    *out = {s.keys[1], s.idx[1], s.idx[0]};
    return hipcub::DeviceRadixSort::SortPairs(s.aux, tmpBytes, s.keys[0], s.keys[1], s.idx[0], s.idx[1], (int)n, 0, endBit, st);
}

// Out arrays (ox ... ogid) given: the sorted cloud is written there and the input arrays are left alone -- no staging,
// no copy back (a fifth of the sort's time); the caller swaps its buffers.  All null: in place.
// method 0: the library radix sort (the order tests compare with); otherwise this library's own.
hipError_t sort_by_cell(hipStream_t st, double* x, double* y, double* z, int32_t* cell, int64_t* gid, double* vel3,
                        int64_t n, int endBit, const float* cellBox, const int* subBits, const int* subOrder,
                        void* scratch, size_t scratchBytes, double* ox, double* oy, double* oz, int32_t* ocell,
                        int64_t* ogid, unsigned long long* occupied, const int32_t* rank, int method) {
    if (n <= 1) return hipSuccess;
    SubKey sk;
    for (int k = 0; k < 3; ++k) { sk.bits[k] = subBits[k]; sk.order[k] = subOrder[k]; }
    const int nSub = subBits[0] + subBits[1] + subBits[2];
    const SortScratch s = carve_sort_scratch(scratch, n, endBit, method);
    if (s.bytes > scratchBytes) return hipErrorInvalidValue;
    // ---- keys and records (the library's index array first: our own sort takes an element's position for its index)
    if (method == 0) hipLaunchKernelGGL(iota_kernel, grid_for(n), dim3(kBlock), 0, st, s.idx[0], n);
    hipLaunchKernelGGL(sort_keys_kernel, grid_for(n), dim3(kBlock), 0, st, x, y, z, cell, cellBox, rank, sk, nSub, s.keys[0], n, gid, s.stage);
    // ---- the key sort
    // (a live particle's cell out of its sorted key: only where no cell bit was shifted out of the 32-bit key)
    const bool cellFromKey = rank == nullptr && endBit < 32;
    SortedPairs r{};
    hipError_t e = method == 0 ? library_sort_pairs(st, s, n, endBit, &r)
                               : rt_sort_pairs(st, s, n, endBit, occupied != nullptr || cellFromKey, &r);
    if (e != hipSuccess) return e;
    // ---- the census
    if (occupied != nullptr) {
        e = hipMemsetAsync(occupied, 0, 16, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(count_cell_runs_kernel, grid_for(n), dim3(kBlock), 0, st, r.keys, n, nSub, 0xFFFFFFFFu, occupied);    // (sort_keys_kernel's lost key)
    }
    // ---- the gather.  In place: the records ARE the copy -- positions and ids go straight back; the cells pass through the spent
    // index buffer
    const bool inPlace = ox == nullptr;
    if (inPlace) { ox = x; oy = y; oz = z; ocell = r.spent; ogid = gid; }
    hipLaunchKernelGGL(gather_aos_kernel, grid8_for(n), dim3(kBlock), 0, st, s.stage, cell, ox, oy, oz, ocell, gid ? ogid : nullptr, r.perm, r.keys,
                       nSub, n, cellFromKey);
    if (inPlace) hipLaunchKernelGGL(copy_cells_kernel, grid_for(n), dim3(kBlock), 0, st, cell, r.spent, n);
    // ---- the velocity triples, through the stage the records have left
    if (vel3) {
        hipLaunchKernelGGL(gather3_kernel, grid_for(n), dim3(kBlock), 0, st, vel3, s.stage, r.perm, n);
        e = hipMemcpyAsync(vel3, s.stage, 24 * (size_t)n, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

}  // namespace cpf
