// The flux table's arithmetic (include/cpf.h "patch source", "flux table"), one text for the kernels of cpf_inflow.hip and for
// cpf_source_flux_host: every floating-point operation is a rounding of its own (-ffp-contract=off on both sides), the scaling
// and the running sums are integer work, so a parallel scan and a sequential loop give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

namespace cpf {

__host__ __device__ __forceinline__ uint64_t inflow_bits(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint64_t)__double_as_longlong(v);
#else
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
#endif
}
__host__ __device__ __forceinline__ bool inflow_finite(double v) { return ((inflow_bits(v) >> 52) & 0x7FFu) != 0x7FFu; }

// w = area * max(U . nIn, 0) and span = s * max(U . nIn, 0): a NaN product of U counts as no inflow, a term that is not finite as 0
struct InflowTerm { double w, span; };
__host__ __device__ __forceinline__ InflowTerm inflow_term(double ux, double uy, double uz, double nx, double ny, double nz, double area,
                                                           double s) {
    const double a = ux * nx, b = uy * ny, c = uz * nz;
    const double ab = a + b;
    const double un = ab + c;
    const double v = un > 0.0 ? un : 0.0;
    InflowTerm t;
    t.w = area * v;
    t.span = s * v;
    if (!inflow_finite(t.w)) t.w = 0.0;
    if (!inflow_finite(t.span)) t.span = 0.0;
    return t;
}

// E of wmax = f * 2^E, f in [0.5, 1), from the exponent bits; wmax > 0 and finite, subnormal or not
__host__ __device__ __forceinline__ int inflow_exponent(double wmax) {
    const uint64_t b = inflow_bits(wmax);
    const int e = (int)((b >> 52) & 0x7FFu);
    if (e != 0) return e - 1022;
    return -1074 + (64 - __builtin_clzll((unsigned long long)b));       // b is the significand, of p bits: wmax in [2^(p-1), 2^p) * 2^-1074
}

// q = floor(w * 2^(32 - E)), exactly: the significand shifted.  0 <= w <= wmax < 2^E, so q < 2^32.
__host__ __device__ __forceinline__ uint64_t inflow_quantum(double w, int E) {
    const uint64_t b = inflow_bits(w);
    const int e = (int)((b >> 52) & 0x7FFu);
    const uint64_t frac = b & 0xFFFFFFFFFFFFFull;
    const uint64_t m = e != 0 ? frac | (1ull << 52) : frac;            // w = m * 2^((e ? e : 1) - 1075)
    const int shift = (e != 0 ? e : 1) - 1075 + 32 - E;                 // at most 32 - 53 + ... : m << shift stays below 2^32
    if (shift >= 0) return m << shift;
    return shift <= -64 ? 0ull : m >> -shift;
}

// hi of a running sum Q out of Qlast > 0: b = 2^32 at the end, else min(2^32, floor(((double)Q / (double)Qlast) * 2^32)), each of the
// two conversions, the division and the product one IEEE operation; hi = max(b, 1) - 1
__host__ __device__ __forceinline__ uint32_t inflow_bound(uint64_t Q, uint64_t Qlast) {
    const uint64_t full = 1ull << 32;
    uint64_t b = full;
    if (Q != Qlast) {
        const double num = (double)Q, den = (double)Qlast;
        const double share = num / den;
        const double scaled = share * 4294967296.0;
        b = (uint64_t)scaled;                                           // (non-negative: the conversion is the floor)
        if (b > full) b = full;
    }
    return (uint32_t)((b > 1 ? b : 1) - 1);
}

}  // namespace cpf
