// Flux table (cpf_source_follow; include/cpf.h "flux table"): the patch source's bounds hi[] and slab depths rec[][13] as a
// function of the current U, recomputed on the stream each time the velocity changes.  The arithmetic is cpf_inflow.h's, shared
// with cpf_source_flux_host; here is who computes what.
//   - A table of at most kInflowFused records takes ONE launch of one workgroup, a record per lane, everything in registers: the
//     terms, the maximum across the workgroup, the quanta, their scan, the bounds.  An inlet has tens to thousands of triangles.
//   - A larger one takes four launches of kInflowBlock lanes, a record per lane and a tile of kInflowBlock records per workgroup:
//     flux (terms to scratch, one 64-bit atomicMax per workgroup on the bit pattern: non-negative doubles order like their bits),
//     sums (the tiles' sums of quanta), scan (one workgroup over the tiles' sums, as respawn_scan_kernel), apply.
// No workgroup waits for another one: what a pass needs of the pass before has been written when its launch starts.
// With wmax == 0 nothing of the table is written and the skipped counter goes up by one.
#include <hip/hip_runtime.h>

#include "cpf_device.h"
#include "cpf_inflow.h"
#include "cpf_philox.h"

namespace cpf {

constexpr int kInflowBlock = 256;                           // lanes of a workgroup of the four passes == records of its tile
constexpr int kInflowFused = 1024;                          // records the fused kernel takes == its lanes

// one record's terms: nIn as two 16-byte loads (columns 8..9 and 10..11), its area and owner, U of the owner (uStride doubles a cell)
__device__ __forceinline__ InflowTerm inflow_load(const double2* rec, const double* __restrict__ area,
                                                  const int32_t* __restrict__ owner, const double* __restrict__ U, int uStride, int k,
                                                  double scale) {
    const double2* r = rec + (int64_t)k * (kSourceDoubles / 2);
    const double2 a = r[4], b = r[5];
    const double ar = area[k];
    const double* __restrict__ u = U + (int64_t)owner[k] * uStride;
    const double ux = u[0], uy = u[1], uz = u[2];
    return inflow_term(ux, uy, uz, a.y, b.x, b.y, ar, scale);
}

// the maximum of `bits` over the workgroup, in every lane (sWave: one word per wave)
template <int kBlock>
__device__ __forceinline__ unsigned long long inflow_block_max(unsigned long long bits, unsigned long long* sWave) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(bits, d, 64);
        bits = o > bits ? o : bits;
    }
    if (lane == 0) sWave[wave] = bits;
    __syncthreads();
    unsigned long long m = 0ull;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) m = sWave[w] > m ? sWave[w] : m;
    __syncthreads();                                        // (sWave is used again)
    return m;
}

// the inclusive running sum of q over the workgroup; *total: the workgroup's sum, in every lane
template <int kBlock>
__device__ __forceinline__ unsigned long long inflow_block_scan(unsigned long long q, unsigned long long* sWave,
                                                                unsigned long long* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long incl = q;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) sWave[wave] = incl;
    __syncthreads();
    unsigned long long before = 0ull, all = 0ull;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
        const unsigned long long s = sWave[w];
        if (w < wave) before += s;
        all += s;
    }
    __syncthreads();
    *total = all;
    return before + incl;
}

// slots: [0] the bit pattern of wmax (the four passes), [1] Q_last (the four passes), [2] refreshes skipped for zero inflow
__global__ __launch_bounds__(kInflowFused) void inflow_fused_kernel(double* rec, uint32_t* __restrict__ hi,
                                                                    const double* __restrict__ area, const int32_t* __restrict__ owner,
                                                                    const double* __restrict__ U, int uStride, int nKept, double scale,
                                                                    unsigned long long* __restrict__ slots) {
    __shared__ unsigned long long sWave[kInflowFused / 64];
    const int k = (int)threadIdx.x;
    const bool mine = k < nKept;
    InflowTerm t{0.0, 0.0};
    if (mine) t = inflow_load(reinterpret_cast<const double2*>(rec), area, owner, U, uStride, k, scale);
    const unsigned long long wmaxBits = inflow_block_max<kInflowFused>((unsigned long long)inflow_bits(t.w), sWave);
    if (wmaxBits == 0ull) {                                 // (the whole workgroup)
        if (threadIdx.x == 0) atomicAdd(&slots[2], 1ull);
        return;
    }
    const int E = inflow_exponent(__longlong_as_double((long long)wmaxBits));
    const unsigned long long q = mine ? (unsigned long long)inflow_quantum(t.w, E) : 0ull;
    unsigned long long last;
    const unsigned long long Q = inflow_block_scan<kInflowFused>(q, sWave, &last);
    if (mine) {
        hi[k] = inflow_bound(Q, last);
        if (scale > 0.0) rec[(int64_t)k * kSourceDoubles + 13] = t.span;
    }
}

__global__ __launch_bounds__(kInflowBlock) void inflow_flux_kernel(const double2* __restrict__ rec, const double* __restrict__ area,
                                                                   const int32_t* __restrict__ owner, const double* __restrict__ U,
                                                                   int uStride, int nKept, double scale, double* __restrict__ w,
                                                                   double* __restrict__ span, unsigned long long* __restrict__ slots) {
    __shared__ unsigned long long sWave[kInflowBlock / 64];
    const int k = (int)blockIdx.x * kInflowBlock + (int)threadIdx.x;
    InflowTerm t{0.0, 0.0};
    if (k < nKept) {
        t = inflow_load(rec, area, owner, U, uStride, k, scale);
        w[k] = t.w;
        span[k] = t.span;
    }
    const unsigned long long m = inflow_block_max<kInflowBlock>((unsigned long long)inflow_bits(t.w), sWave);
    if (threadIdx.x == 0 && m != 0ull) atomicMax(&slots[0], m);
}

__global__ __launch_bounds__(kInflowBlock) void inflow_sums_kernel(const double* __restrict__ w, int nKept,
                                                                   const unsigned long long* __restrict__ slots,
                                                                   unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long sWave[kInflowBlock / 64];
    const unsigned long long wmaxBits = slots[0];
    if (wmaxBits == 0ull) return;                           // (the whole workgroup)
    const int E = inflow_exponent(__longlong_as_double((long long)wmaxBits));
    const int k = (int)blockIdx.x * kInflowBlock + (int)threadIdx.x;
    const unsigned long long q = k < nKept ? (unsigned long long)inflow_quantum(w[k], E) : 0ull;
    unsigned long long total;
    (void)inflow_block_scan<kInflowBlock>(q, sWave, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: offsets[b] = sums[0] + ... + sums[b-1], slots[1] = their total
__global__ __launch_bounds__(kInflowBlock) void inflow_scan_kernel(const unsigned long long* __restrict__ sums,
                                                                   unsigned long long* __restrict__ offsets, int nBlocks,
                                                                   unsigned long long* __restrict__ slots) {
    __shared__ unsigned long long sWave[kInflowBlock / 64];
    if (slots[0] == 0ull) return;                           // (the sums were not written)
    unsigned long long carry = 0ull;
    for (int b0 = 0; b0 < nBlocks; b0 += kInflowBlock) {
        const int b = b0 + (int)threadIdx.x;
        const unsigned long long c = b < nBlocks ? sums[b] : 0ull;
        unsigned long long total;
        const unsigned long long incl = inflow_block_scan<kInflowBlock>(c, sWave, &total);
        if (b < nBlocks) offsets[b] = carry + incl - c;
        carry += total;
    }
    if (threadIdx.x == 0) slots[1] = carry;
}

__global__ __launch_bounds__(kInflowBlock) void inflow_apply_kernel(double* __restrict__ rec, uint32_t* __restrict__ hi,
                                                                    const double* __restrict__ w, const double* __restrict__ span,
                                                                    int nKept, double scale, const unsigned long long* __restrict__ offsets,
                                                                    unsigned long long* __restrict__ slots) {
    __shared__ unsigned long long sWave[kInflowBlock / 64];
    const unsigned long long wmaxBits = slots[0];
    if (wmaxBits == 0ull) {                                 // (the whole workgroup)
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&slots[2], 1ull);
        return;
    }
    const int E = inflow_exponent(__longlong_as_double((long long)wmaxBits));
    const int k = (int)blockIdx.x * kInflowBlock + (int)threadIdx.x;
    const bool mine = k < nKept;
    const unsigned long long q = mine ? (unsigned long long)inflow_quantum(w[k], E) : 0ull;
    unsigned long long total;
    const unsigned long long Q = offsets[blockIdx.x] + inflow_block_scan<kInflowBlock>(q, sWave, &total);
    if (mine) {
        hi[k] = inflow_bound(Q, slots[1]);
        if (scale > 0.0) rec[(int64_t)k * kSourceDoubles + 13] = span[k];
    }
}

int64_t inflow_blocks(int64_t nKept) { return (nKept + kInflowBlock - 1) / kInflowBlock; }

hipError_t inflow_refresh(hipStream_t st, const InflowView& v, const double* U, int uStride) {
    if (v.nKept <= 0 || v.nKept > (1 << 24) || !v.rec || !v.hi || !v.area || !v.owner || !v.w || !v.sums || !v.slots || !U)
        return hipErrorInvalidValue;
    if (v.nKept <= kInflowFused) {
        hipLaunchKernelGGL(inflow_fused_kernel, dim3(1), dim3(kInflowFused), 0, st, v.rec, v.hi, v.area, v.owner, U, uStride, v.nKept,
                           v.depthScale, v.slots);
        return hipGetLastError();
    }
    const int nBlocks = (int)inflow_blocks(v.nKept);
    double* span = v.w + v.nKept;
    unsigned long long* offsets = v.sums + nBlocks;
    const hipError_t e = hipMemsetAsync(v.slots, 0, 8, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(inflow_flux_kernel, dim3((unsigned)nBlocks), dim3(kInflowBlock), 0, st, reinterpret_cast<const double2*>(v.rec),
                       v.area, v.owner, U, uStride, v.nKept, v.depthScale, v.w, span, v.slots);
    hipLaunchKernelGGL(inflow_sums_kernel, dim3((unsigned)nBlocks), dim3(kInflowBlock), 0, st, v.w, v.nKept, v.slots, v.sums);
    hipLaunchKernelGGL(inflow_scan_kernel, dim3(1), dim3(kInflowBlock), 0, st, v.sums, offsets, nBlocks, v.slots);
    hipLaunchKernelGGL(inflow_apply_kernel, dim3((unsigned)nBlocks), dim3(kInflowBlock), 0, st, v.rec, v.hi, v.w, span, v.nKept,
                       v.depthScale, offsets, v.slots);
    return hipGetLastError();
}

}  // namespace cpf
