// Philox4x32 and the respawn positions drawn from it: shared by the step kernels' kick (cpf_walk.h, normal3), the recycling
// kernels (cpf_recycle.hip, cpf_inlet.hip) and, on the host, cpf_respawn_positions_host and cpf_source_positions_host
// (cpf_api.cpp) -- one text for the device and the host.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cpf {

// Philox4x32-10 (Salmon et al. SC'11) keyed by (seed, "CPF1"), counter (gid, step): replaces the
// 48-byte-per-particle cuRAND XORWOW state of cuda/particles.cu:524-575 with nothing at all.
// Philox4x32-R (Salmon et al., SC'11).  R = 7: the variant with the fewest rounds that the paper reports as passing the
// whole of BigCrush ("Crush-resistant"; R = 10 is Random123's default, with a safety margin).  Each round is two
// quarter-rate 32 x 32 -> 64 multiplies (v_mad_u64_u32) and four XORs per lane and the streaming kernel is bound by its
// vector ALU: measured on one box (pitzDaily, D = 1.5e-5, 1e7 particles) 10 -> 7 rounds = 0.1865 -> 0.1825 ms per launch;
// the deviates as a whole (this + Box-Muller below) are 0.052 of the 0.188 ms (A/B build that returns constants instead).
// oracle/cellwalk.c states the same function; its known-answer test runs at R = 10, where Random123 publishes vectors.
#ifndef CPF_PHILOX_ROUNDS
#define CPF_PHILOX_ROUNDS 7
#endif
__host__ __device__ __forceinline__ void philox4x32(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < CPF_PHILOX_ROUNDS; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// Where a respawned particle goes (cpf_respawn_box*): a pure function of (seed, gid, epoch) -- one Philox block, counter
// (gid low, gid high, epoch, 0), key (seed, "CPF2": the kick's stream is keyed "CPF1", so the two never meet); word k gives
// u_k = w_k * 2^-32 in [0, 1) exactly, and pos_k = lower_k + u_k * (upper_k - lower_k) with every operation rounded on its own
// (-ffp-contract=off; the host's compile of this text has it too).
__host__ __device__ __forceinline__ void respawn_position(uint32_t seed, uint64_t gid, uint32_t epoch, const double lower[3],
                                                          const double upper[3], double pos[3]) {
    uint32_t c[4] = {(uint32_t)gid, (uint32_t)(gid >> 32), epoch, 0u};
    philox4x32(c, seed, 0x43504632u);
    for (int k = 0; k < 3; ++k) {
        const double u = (double)c[k] * 2.3283064365386963e-10;      // 2^-32
        const double span = upper[k] - lower[k];
        const double off = u * span;
        pos[k] = lower[k] + off;
    }
}

// Where a particle respawned on a patch source goes (cpf_respawn_source*; the table: cpf_source_table_host): one Philox block,
// counter (gid low, gid high, epoch, 0), key (seed, "CPF3": neither the box's stream nor the kick's).  Word 0 picks the triangle,
// the first t with w0 <= hi[t] (source_pick; the kernel searches its LDS copy instead); words 1 and 2 the point in it, word 3
// the depth along the inward normal.  A record is kSourceDoubles doubles: A[3] | e1[3] | e2[3] | nIn[3] | d0 | d1 - d0 | index | 0.
constexpr int kSourceDoubles = 16;
__host__ __device__ __forceinline__ void source_words(uint32_t seed, uint64_t gid, uint32_t epoch, uint32_t c[4]) {
    c[0] = (uint32_t)gid; c[1] = (uint32_t)(gid >> 32); c[2] = epoch; c[3] = 0u;
    philox4x32(c, seed, 0x43504633u);
}
// lower bound over the non-decreasing hi[0 .. n-1] -- strictly increasing as built, with equal neighbours once the table follows U
// (include/cpf.h "flux table") -- (hi[n-1] == 0xFFFFFFFF: there always is one)
__host__ __device__ __forceinline__ int source_pick(const uint32_t* __restrict__ hi, int n, uint32_t w0) {
    int lo = 0, len = n;
    while (len > 1) {
        const int half = len >> 1;
        if (hi[lo + half - 1] < w0) { lo += half; len -= half; }
        else len = half;
    }
    return lo;
}
// The fold keeps (u1, u2) in the triangle: w1 + w2 > 2^32 mirrors both, as 64-bit integers; u = w * 2^-32 is exact.  Every
// product and sum below is a rounding of its own, in this order (-ffp-contract=off on both sides).
__host__ __device__ __forceinline__ void source_point(const uint32_t c[4], const double rec[kSourceDoubles], double pos[3]) {
    uint64_t w1 = c[1], w2 = c[2];
    if (w1 + w2 > ((uint64_t)1 << 32)) { w1 = ((uint64_t)1 << 32) - w1; w2 = ((uint64_t)1 << 32) - w2; }
    const double u1 = (double)w1 * 2.3283064365386963e-10, u2 = (double)w2 * 2.3283064365386963e-10;      // 2^-32
    const double ud = (double)c[3] * 2.3283064365386963e-10;
    const double dspan = ud * rec[13];
    const double d = rec[12] + dspan;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double a1 = u1 * rec[3 + k];
        const double s1 = rec[k] + a1;
        const double a2 = u2 * rec[6 + k];
        const double s2 = s1 + a2;
        const double a3 = d * rec[9 + k];
        pos[k] = s2 + a3;
    }
}

}  // namespace cpf
