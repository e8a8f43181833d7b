// HIP kernels (gfx950 / CDNA4, wave64) for the per-timestep particle loop, and their launchers.
//
// One fused kernel per Lagrangian cycle replaces the reference's five launches + five device
// syncs (src/advect.H:96-161): advect -> Brownian kick -> locate (plane-exit walk) -> wall
// reflect -> move.  The walk runs on the polyMesh cells themselves (CSR face slots with
// precomputed inward planes), not on a 12-tets-per-cell decomposition, and needs no BVH.
//
// Arithmetic contract ("Numerics, the oracle, and what is pinned"): fp64 like the reference (cuda/common.h:26);
// dot products and axpy use explicit fma(), nothing else may be contracted (-ffp-contract=off),
// divisions are IEEE.  tests/ compare bit-for-bit with an independent CPU statement.
#include "cpf_device.h"

#include "cpf_locate.h"
#include "cpf_walk.h"

#include <algorithm>

namespace cpf {

// ------------------------------------------------------------------------------------------------
// fused step: one thread per particle, nCyc cycles per launch (1 = the reference's per-cycle
// structure; >1 keeps the particle in registers between cycles)
// ------------------------------------------------------------------------------------------------

template <class TRACER, bool BROWNIAN, bool REFLECT, bool STORE_VEL, bool VERTEX = false>
__device__ __forceinline__ void particle_cycles(const TRACER& tr, const MeshView& m, D3& P, int& cur, D3& v,
                                                uint64_t id, double dt, double sigma, uint32_t step0, int nCyc,
                                                uint32_t seed, StepStats& st, const VertexField* vf = nullptr) {
    for (int c = 0; c < nCyc; ++c) {
        if (cur < 0) { cur = CPF_CELL_FROZEN; break; }           // lost in the previous cycle: w = 0
        // ---- advect (cuda/particles.cu:355-362): disp = (P + dt*U[cell]) - P
        D3 Pn;
        if (VERTEX) {
            // (no tet of the cell holds P -- degenerate decomposition: the reference switches the particle off, :262-266)
            if (!vertex_velocity(*vf, P, cur, v)) { cur = CPF_CELL_FROZEN; break; }
            Pn = {P.x + dt * v.x, P.y + dt * v.y, P.z + dt * v.z};       // multiply, round, add: what the staged advect does
        } else {
            const double4 u = tr.velocity(cur);
            v = {u.x, u.y, u.z};
            Pn = axpy(dt, v, P);
        }
        ++st.steps;
        D3 disp = {Pn.x - P.x, Pn.y - P.y, Pn.z - P.z};
        if (BROWNIAN) {                                          // particles.cu:560-569
            const D3 xi = normal3(id, step0 + (uint32_t)c, seed);
            disp = axpy(sigma, xi, disp);
        }
        // ---- locate + reflect (ConvexQuery.cu:135-216, :320-436)
        D3 E = {P.x + disp.x, P.y + disp.y, P.z + disp.z};
        bool folded = false;
        if (BROWNIAN && REFLECT && m.zThin) {                    // one cell thick in z: cpf_walk.h, fold_z
            const int s0 = m.cellOff[cur];
            bool clear;
            const int nb = fold_z(E.z, m.planes[s0 + 4], m.planes[s0 + 5], clear);
            st.refl += nb;
            if (nb & 1) v.z = -v.z;
            folded = nb != 0;
        }
        D3 S = P, hit = P;
        int token = INT32_MIN, next = cur, outSlot = 0;
        bool reflected = false;
        for (int j = 0; j < kMaxReflect; ++j) {
            for (int h = 0; h < kMaxHops; ++h) {
                next = tr.trace(S, E, cur, token, outSlot);
                ++st.hops;
                if (next == cur || next < 0) break;
                token = cur;
                cur = next;
            }
            if (next >= 0 || !REFLECT) break;
            // wall: mirror end point and velocity about the boundary face (ConvexQuery.cu:286-309)
            hit = S; reflected = true; ++st.refl;
            const double4 pl = m.planes[outSlot];
            const D3 nn = {pl.x, pl.y, pl.z};
            const double sd = dot3(pl, E) - pl.w;
            E = axpy(-2.0 * sd, nn, E);
            v = axpy(-2.0 * dot3(pl, v), nn, v);
            token = next;
        }
        // ---- move (particles.cu:693-701); reflected: p = P_hit, disp = P_end - P_hit
        if (reflected) P = {hit.x + (E.x - hit.x), hit.y + (E.y - hit.y), hit.z + (E.z - hit.z)};
        else P = {P.x + disp.x, P.y + disp.y, folded ? E.z : P.z + disp.z};
        if (next < 0) { next = CPF_CELL_LOST; ++st.lost; }
        cur = next;
    }
}

template <int VARIANT, bool BROWNIAN, bool REFLECT, bool STORE_VEL>
__global__ __launch_bounds__(kBlock) void step_kernel(double* __restrict__ x, double* __restrict__ y,
                                                      double* __restrict__ z, int32_t* __restrict__ cell,
                                                      const int64_t* __restrict__ gid, double* __restrict__ vel,
                                                      int64_t n, double dt, double sigma, uint32_t step0, int nCyc,
                                                      uint32_t seed, MeshView m,
                                                      unsigned long long* __restrict__ counters) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    StepStats st = {0, 0, 0, 0};
    if (i < n) {
        int cur = cell[i];
        if (cur >= 0) {
            D3 P = {x[i], y[i], z[i]};
            D3 v = {0, 0, 0};
            const uint64_t id = gid ? (uint64_t)gid[i] : (uint64_t)i;
            const GlobalTracer<VARIANT> tr{m};
            particle_cycles<GlobalTracer<VARIANT>, BROWNIAN, REFLECT, STORE_VEL>(tr, m, P, cur, v, id, dt, sigma, step0,
                                                                                 nCyc, seed, st);
            x[i] = P.x; y[i] = P.y; z[i] = P.z;
            cell[i] = cur;
            if (STORE_VEL) { vel[3 * i] = v.x; vel[3 * i + 1] = v.y; vel[3 * i + 2] = v.z; }
        } else if (cur == CPF_CELL_LOST) {
            cell[i] = CPF_CELL_FROZEN;
        }
    }
    __shared__ unsigned sCnt[4];
    flush_stats(st, counters, sCnt);
}

// The fused cycle with the "VertexVelocity" advect (cuda/particles.cu:428-437; CPF_STEP_VERTEX_VELOCITY): the generic walk
// with the velocity interpolated at the particle's position.  Same stages in the same order as the reference's five calls with
// that mode, one launch; the advect shares its arithmetic with cpf_stage_advect_vertex (tests assert equality).
template <bool BROWNIAN, bool REFLECT, bool STORE_VEL>
__global__ __launch_bounds__(kBlock) void step_kernel_vertex(double* __restrict__ x, double* __restrict__ y,
                                                             double* __restrict__ z, int32_t* __restrict__ cell,
                                                             const int64_t* __restrict__ gid, double* __restrict__ vel,
                                                             int64_t n, double dt, double sigma, uint32_t step0, int nCyc,
                                                             uint32_t seed, MeshView m, VertexField vf,
                                                             unsigned long long* __restrict__ counters) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    StepStats st = {0, 0, 0, 0};
    if (i < n) {
        int cur = cell[i];
        if (cur >= 0) {
            D3 P = {x[i], y[i], z[i]};
            D3 v = {0, 0, 0};
            const uint64_t id = gid ? (uint64_t)gid[i] : (uint64_t)i;
            const GlobalTracer<kVariantGeneric> tr{m};
            particle_cycles<GlobalTracer<kVariantGeneric>, BROWNIAN, REFLECT, STORE_VEL, true>(tr, m, P, cur, v, id, dt, sigma, step0,
                                                                                               nCyc, seed, st, &vf);
            x[i] = P.x; y[i] = P.y; z[i] = P.z;
            cell[i] = cur;
            if (STORE_VEL) { vel[3 * i] = v.x; vel[3 * i + 1] = v.y; vel[3 * i + 2] = v.z; }
        } else if (cur == CPF_CELL_LOST) {
            cell[i] = CPF_CELL_FROZEN;
        }
    }
    __shared__ unsigned sCnt[4];
    flush_stats(st, counters, sCnt);
}

// ------------------------------------------------------------------------------------------------
// Wave-cooperative variant (all-hex meshes).  Mesh data lives in packed 256-byte cell records
// (6 planes | U | 6 neighbour ids).  Each round, a wave finds the distinct cells its busy lanes sit in
// (ballot + readlane), fetches up to four whole records with ONE coalesced 16-byte-per-lane load
// (16 lanes per record) into its private LDS slots, and every lane then reads its cell's planes with
// ds_read_b128 (same-cell lanes broadcast).  That replaces 18 scattered per-lane gathers per visit
// and their serialised round trips by a single L2 round trip per visit.  Lanes whose cell did not
// get a slot (more than four distinct cells in the wave: unsorted clouds) read the record directly
// from global memory in the same round, so every busy lane advances every round.
// The walk is written as a wave-synchronous state machine; per lane it performs exactly the loop
// nest of particle_cycles (<= 50 hops per segment, <= 5 reflections), in the same arithmetic order.
// ------------------------------------------------------------------------------------------------
constexpr int kCoopSlots = 4;
#ifndef CPF_COOP_BLOCK
#define CPF_COOP_BLOCK 128
#endif
constexpr int kCoopBlock = CPF_COOP_BLOCK;   // waves of a block share nothing but the dispatch slot

// Waves per SIMD the register allocator must make room for.  The plain cycle (no Brownian kick, no stored velocity,
// no statistics) fits 72 VGPRs = 7 waves; measured time follows T = 0.10 ms + 0.59 ms / waves on the bench cloud,
// i.e. the kernel is bound by the length of each wave's dependent chain, and resident waves are what hides it.
template <bool BROWNIAN, bool STORE_VEL, bool STATS>
struct CoopOccupancy { static constexpr int waves = (!STORE_VEL && !STATS) ? 7 : 1; };

template <bool BROWNIAN, bool REFLECT, bool STORE_VEL, bool STATS>
__global__ __launch_bounds__(kCoopBlock, (CoopOccupancy<BROWNIAN, STORE_VEL, STATS>::waves)) void step_kernel_coop(double* __restrict__ x, double* __restrict__ y,
                                                           double* __restrict__ z, int32_t* __restrict__ cell,
                                                           const int64_t* __restrict__ gid, double* __restrict__ vel,
                                                           int64_t n, double dt, double sigma, uint32_t step0,
                                                           int nCyc, uint32_t seed, MeshView m,
                                                           unsigned long long* __restrict__ counters) {
    __shared__ double4 sRec[kCoopBlock / 64][kCoopSlots][8];
    __shared__ unsigned sCnt[4];
    // Per-lane end point E and last wall hit point, parked in LDS between rounds (SoA: conflict-free).  Neither is
    // needed while the six planes are tested, and the kernel's speed is set by waves per SIMD: 12 VGPRs less
    // is one more resident wave.  A lane only ever reads back what it wrote itself, so no barrier is involved.
    __shared__ double sLane[6][kCoopBlock];            // one array: one address register + immediate offsets
    double(*sE)[kCoopBlock] = sLane;
    double(*sHit)[kCoopBlock] = sLane + 3;
    const int tid = threadIdx.x;
    const int lane = threadIdx.x & 63;
    double4(*slots)[8] = sRec[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];   // wave-uniform: lives in SGPRs
    const int64_t i = (int64_t)blockIdx.x * kCoopBlock + threadIdx.x;
    int cur = (i < n) ? cell[i] : CPF_CELL_FROZEN;
    const bool wasLost = cur == CPF_CELL_LOST;
    const bool hadParticle = cur >= 0;
    bool valid = hadParticle;
    D3 P = {0, 0, 0}, v = {0, 0, 0};
    if (valid) P = {x[i], y[i], z[i]};
    const uint64_t id = (valid && gid) ? (uint64_t)gid[i] : (uint64_t)i;
    StepStats st = {0, 0, 0, 0};

    for (int c = 0; c < nCyc; ++c) {
        if (valid && cur < 0) { cur = CPF_CELL_FROZEN; valid = false; }      // lost in the previous cycle: w = 0
        bool busy = valid;
        bool needAdvect = busy, reflected = false, lostNow = false;
        int token = INT32_MIN, h = 0, j = 0;
        D3 S = P;
        if (STATS && busy) ++st.steps;
        if (BROWNIAN && busy) {
            // Philox + Box-Muller (fp64 log / sqrt / sincos: a few hundred instructions and many registers) run HERE,
            // with almost nothing else live, and leave the three deviates in the lane's wall-hit LDS slot, which is
            // not needed before the first reflection and the kick is consumed in the first round.  Inside the round
            // loop they cost the whole walk its occupancy (97 VGPRs = 4 waves).
            const D3 xi = normal3(id, step0 + (uint32_t)c, seed);
            sHit[0][tid] = xi.x; sHit[1][tid] = xi.y; sHit[2][tid] = xi.z;
        }
        while (ballot64(busy) != 0ull) {
            // ---- distinct cells of the busy lanes -> slots (wave-uniform scalars)
            const unsigned long long busyMask = ballot64(busy);
            const D3 Epre = {sE[0][tid], sE[1][tid], sE[2][tid]};                  // requested before the cell discovery: its LDS round trip hides behind it (2 %)
            unsigned long long todo = busyMask;
            int myslot = -1, c0 = -1, c1 = -1, c2 = -1, c3 = -1;
#pragma unroll
            for (int k = 0; k < kCoopSlots; ++k) {
                if (todo != 0ull) {
                    const int leader = __ffsll((long long)todo) - 1;
                    const int ck = __builtin_amdgcn_readlane(cur, leader);
                    if (busy && cur == ck) myslot = k;
                    // the compare mask itself, combined in the scalar unit (see ballot64)
                    todo &= ~(__builtin_amdgcn_uicmp((unsigned)cur, (unsigned)ck, 32 /* eq */) & busyMask);
                    if (k == 0) c0 = ck; else if (k == 1) c1 = ck; else if (k == 2) c2 = ck; else c3 = ck;
                }
            }
            // ---- one coalesced load: lanes 16g..16g+15 copy record g (256 B) into LDS slot g
            const int g = lane >> 4;
            const int cg = g == 0 ? c0 : (g == 1 ? c1 : (g == 2 ? c2 : c3));
            if (cg >= 0) {
                // scalar base + 32-bit lane offset (records of up to 2^24 cells): no 64-bit address kept per lane
                const unsigned off = (unsigned)cg * 256u + (unsigned)(lane & 15) * 16u;
                const double2 val = *reinterpret_cast<const double2*>(reinterpret_cast<const char*>(m.cellRec) + off);
                reinterpret_cast<double2*>(slots[g])[lane & 15] = val;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // ---- every busy lane does one cell visit
            if (busy) {
                int next, outSlot = 0;
                D3 E = S;
                if (!needAdvect) E = Epre;
                if (myslot >= 0) {
                    const double4* rec = slots[myslot];
                    if (needAdvect) {
                        const double4 u = rec[6];
                        v = {u.x, u.y, u.z};
                    }
                    if (needAdvect) {
                        const D3 Pn = axpy(dt, v, P);                              // particles.cu:355-362
                        D3 disp = {Pn.x - P.x, Pn.y - P.y, Pn.z - P.z};
                        if (BROWNIAN) {                                            // the deviates drawn before the round loop
                            const D3 xi = {sHit[0][tid], sHit[1][tid], sHit[2][tid]};
                            disp = axpy(sigma, xi, disp);
                        }
                        E = {P.x + disp.x, P.y + disp.y, P.z + disp.z};
                        if (BROWNIAN && REFLECT && m.zThin) {                      // one cell thick in z: cpf_walk.h, fold_z
                            bool clear;
                            const int nb = fold_z(E.z, rec[4], rec[5], clear);
                            if (STATS) st.refl += nb;
                            if (STORE_VEL && (nb & 1)) v.z = -v.z;
                        }
                        sE[0][tid] = E.x; sE[1][tid] = E.y; sE[2][tid] = E.z;
                        needAdvect = false;
                    }
                    next = trace_lds6(S, E, cur, rec, token, outSlot, m.zPairLast != 0);
                } else {
                    // no slot: more than kCoopSlots distinct cells in the wave (a cloud that is not kept sorted).
                    // Per-lane gathers keep such a wave moving; letting these lanes wait for a free slot instead
                    // measured 1.7x slower on an unsorted cloud and no faster on a sorted one.
                    const double4* rec = m.cellRec + 8 * (int64_t)cur;
                    if (needAdvect) {
                        const double4 u = rec[6];
                        v = {u.x, u.y, u.z};
                        const D3 Pn = axpy(dt, v, P);
                        D3 disp = {Pn.x - P.x, Pn.y - P.y, Pn.z - P.z};
                        if (BROWNIAN) {                                            // the deviates drawn before the round loop
                            const D3 xi = {sHit[0][tid], sHit[1][tid], sHit[2][tid]};
                            disp = axpy(sigma, xi, disp);
                        }
                        E = {P.x + disp.x, P.y + disp.y, P.z + disp.z};
                        if (BROWNIAN && REFLECT && m.zThin) {
                            bool clear;
                            const int nb = fold_z(E.z, rec[4], rec[5], clear);
                            if (STATS) st.refl += nb;
                            if (STORE_VEL && (nb & 1)) v.z = -v.z;
                        }
                        sE[0][tid] = E.x; sE[1][tid] = E.y; sE[2][tid] = E.z;
                        needAdvect = false;
                    }
                    next = trace_fixed<6, false>(S, E, cur, rec, reinterpret_cast<const int32_t*>(rec + 7), token, outSlot, 0);
                }
                if (STATS) ++st.hops;
                if (next == cur) {
                    busy = false;                                                  // segment ends in this cell
                } else if (next < 0) {                                             // boundary face
                    if (!REFLECT) { busy = false; lostNow = true; }
                    else {
                        // mirror end point and velocity about the wall (ConvexQuery.cu:286-309)
                        sHit[0][tid] = S.x; sHit[1][tid] = S.y; sHit[2][tid] = S.z;
                        reflected = true; if (STATS) ++st.refl;
                        // the wall's plane is fetched here, by the few lanes that reflect: reading it after every
                        // visit cost 2 KB of LDS return bandwidth per wave-round, and LDS bandwidth is what the
                        // throughput-bound part of this kernel's time consists of
                        const double4 wallPlane = myslot >= 0 ? slots[myslot][outSlot] : m.cellRec[8 * (int64_t)cur + outSlot];
                        const D3 nn = {wallPlane.x, wallPlane.y, wallPlane.z};
                        const double sd = dot3(wallPlane, E) - wallPlane.w;
                        E = axpy(-2.0 * sd, nn, E);
                        sE[0][tid] = E.x; sE[1][tid] = E.y; sE[2][tid] = E.z;
                        v = axpy(-2.0 * dot3(wallPlane, v), nn, v);
                        token = next;
                        h = 0;
                        if (++j == kMaxReflect) { busy = false; lostNow = true; }  // still on a wall after 5 bounces
                    }
                } else {
                    token = cur;
                    cur = next;
                    if (++h == kMaxHops) busy = false;                             // hop cap: keep the last cell
                }
            }
            __builtin_amdgcn_wave_barrier();                                       // slots are rewritten next round
        }
        // ---- move (particles.cu:693-701); reflected: p = P_hit, disp = P_end - P_hit; else P + disp == E
        if (valid) {
            const D3 E = {sE[0][tid], sE[1][tid], sE[2][tid]};
            if (reflected) {
                const D3 hit = {sHit[0][tid], sHit[1][tid], sHit[2][tid]};
                P = {hit.x + (E.x - hit.x), hit.y + (E.y - hit.y), hit.z + (E.z - hit.z)};
            } else P = E;
            if (lostNow) { cur = CPF_CELL_LOST; if (STATS) ++st.lost; }
        }
    }
    // the particle index again, from the block id (kept out of the long-lived registers on purpose)
    unsigned bid = blockIdx.x;
    asm volatile("" : "+s"(bid));
    const int64_t io = (int64_t)bid * kCoopBlock + threadIdx.x;
    if (hadParticle) {
        x[io] = P.x; y[io] = P.y; z[io] = P.z;
        cell[io] = cur;
        if (STORE_VEL) { vel[3 * io] = v.x; vel[3 * io + 1] = v.y; vel[3 * io + 2] = v.z; }
    } else if (wasLost) {
        cell[io] = CPF_CELL_FROZEN;
    }
    if (STATS) flush_stats(st, counters, sCnt);
}

hipError_t launch_step(const StepPlan& p, hipStream_t st, double* x, double* y, double* z, int32_t* cell, const int64_t* gid,
                       double* vel, int64_t n, double dt, double D, uint32_t step0, int nCyc, uint32_t seed, const MeshView& m,
                       unsigned long long* counters, const VertexField* vf, StreamState& ss, bool zSettled, hipEvent_t evStart,
                       hipEvent_t evStop) {
    if (n <= 0) return hipSuccess;
    const double sigma = p.brown ? sqrt(2.00 * D * dt) : 0.0;   // particles.cu:564
    if (p.kernel == StepPlan::kStream || p.kernel == StepPlan::kStreamVertex)
        return launch_step_stream(p, st, x, y, z, cell, gid, vel, n, dt, sigma, step0, nCyc, seed, m, counters, vf, ss, zSettled,
                                  evStart, evStop);
    if (p.kernel == StepPlan::kVertex && vf == nullptr) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
    const auto walk = [&](auto V) {
        with_bools([&](auto B, auto R, auto SV) {
            hipLaunchKernelGGL((step_kernel<V, B, R, SV>), grid, dim3(kBlock), 0, st, x, y, z, cell, gid, vel, n, dt, sigma, step0,
                               nCyc, seed, m, counters);
        }, p.brown, p.reflect, p.storeVel);
    };
    switch (p.kernel) {
#ifdef CPF_EXPERIMENTS
        case StepPlan::kAhead: return launch_step_ahead(p, st, x, y, z, cell, n, dt, m, counters, ss, vel);
        case StepPlan::kFixed: walk(std::integral_constant<int, kVariantFixed>{}); break;
        case StepPlan::kFixedScalar: walk(std::integral_constant<int, kVariantFixedScalar>{}); break;
#endif
        case StepPlan::kCoop:
            // statistics are a template flag here: the four per-lane counters cost registers, and registers are waves
            with_bools([&](auto B, auto R, auto SV, auto ST) {
                hipLaunchKernelGGL((step_kernel_coop<B, R, SV, ST>), dim3((unsigned)((n + kCoopBlock - 1) / kCoopBlock)),
                                   dim3(kCoopBlock), 0, st, x, y, z, cell, gid, vel, n, dt, sigma, step0, nCyc, seed, m, counters);
            }, p.brown, p.reflect, p.storeVel, p.stats);
            break;
        case StepPlan::kVertex:
            with_bools([&](auto B, auto R, auto SV) {
                hipLaunchKernelGGL((step_kernel_vertex<B, R, SV>), grid, dim3(kBlock), 0, st, x, y, z, cell, gid, vel, n, dt, sigma,
                                   step0, nCyc, seed, m, *vf, counters);
            }, p.brown, p.reflect, p.storeVel);
            break;
        default: walk(std::integral_constant<int, kVariantGeneric>{});
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Stage-by-stage kernels on the REFERENCE's own array layouts (Particle = double4 AoS, vec4d
// disps / vels, int ids), one per wrapper of third_party/RTXAdvect/cuda/common.h and
// query/ConvexQuery.h, for hosts that keep the reference's five-call cycle (compat shims).
// ids are cell ids here (reference: tet ids, cell = tet / 12); the wall encoding between
// locate and reflect is the reference's: -(cell at the START of the step + 1).
// The fused step_kernel above is the same arithmetic in the same order (tests assert equality).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void stage_advect_kernel(double4* __restrict__ P, const int32_t* __restrict__ ids,
                                                              double4* __restrict__ vels, double4* __restrict__ disps,
                                                              double dt, int64_t n, MeshView m) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double4 p = P[i];
    if (!p.w) return;
    const int id = ids[i];
    if (id < 0) { p.w = 0.0; P[i] = p; return; }                 // particles.cu:333-338
    const double4 u = m.U[id];
    const D3 v = {u.x, u.y, u.z}, Pp = {p.x, p.y, p.z};
    const D3 Pn = axpy(dt, v, Pp);
    vels[i] = make_double4(v.x, v.y, v.z, -1.0);
    disps[i] = make_double4(Pn.x - Pp.x, Pn.y - Pp.y, Pn.z - Pp.z, -1.0);
}

// "VertexVelocity" advect (cuda/particles.cu:244-313) on cell ids; see cpf_stage_advect_vertex in include/cpf.h.
// Plain products and sums in the reference's order (no fma: the file is built with -ffp-contract=off), so that
// oracle/cellwalk.c's cw_advect_vertex is reproduced bit for bit.
__global__ __launch_bounds__(kBlock) void stage_advect_vertex_kernel(double4* __restrict__ P, const int32_t* __restrict__ ids,
                                                                     double4* __restrict__ vels, double4* __restrict__ disps,
                                                                     double dt, int64_t n, VertexField f) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double4 p = P[i];
    if (!p.w) return;
    const int c = ids[i];
    if (c < 0) { p.w = 0.0; P[i] = p; return; }                  // particles.cu:262-266
    D3 v;
    if (!vertex_velocity(f, D3{p.x, p.y, p.z}, c, v)) { p.w = 0.0; P[i] = p; return; }
    const D3 Pn = {p.x + dt * v.x, p.y + dt * v.y, p.z + dt * v.z};
    vels[i] = make_double4(v.x, v.y, v.z, -1.0);
    disps[i] = make_double4(Pn.x - p.x, Pn.y - p.y, Pn.z - p.z, -1.0);
}

__global__ __launch_bounds__(kBlock) void stage_brownian_kernel(const double4* __restrict__ P,
                                                                double4* __restrict__ disps, double sigma, int64_t n,
                                                                uint32_t step, uint32_t seed) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (!P[i].w) return;
    double4 d = disps[i];
    const D3 r = axpy(sigma, normal3((uint64_t)i, step, seed), D3{d.x, d.y, d.z});
    disps[i] = make_double4(r.x, r.y, r.z, d.w);
}

__global__ __launch_bounds__(kBlock) void stage_locate_kernel(const double4* __restrict__ P,
                                                              const double4* __restrict__ disps,
                                                              int32_t* __restrict__ ids, int64_t n, MeshView m) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double4 p = P[i];
    if (!p.w) return;
    const int start = ids[i];
    if (start < 0) return;
    const double4 d = disps[i];
    const D3 E = {p.x + d.x, p.y + d.y, p.z + d.z};
    D3 S = {p.x, p.y, p.z};
    int cur = start, next = start, token = INT32_MIN, outSlot = 0;
    for (int h = 0; h < kMaxHops; ++h) {
        next = trace_in_cell(S, E, cur, m, token, outSlot);
        if (next == cur || next < 0) break;
        token = cur;
        cur = next;
    }
    ids[i] = next < 0 ? -(start + 1) : next;                      // ConvexQuery.cu:204-215
}

__global__ __launch_bounds__(kBlock) void stage_reflect_kernel(int32_t* __restrict__ ids, double4* __restrict__ P,
                                                               double4* __restrict__ vels, double4* __restrict__ disps,
                                                               int64_t n, MeshView m) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double4 p = P[i];
    if (!p.w) return;
    const int id = ids[i];
    if (id >= 0) return;                                          // only particles that hit a wall
    double4 d = disps[i], vv = vels[i];
    D3 S = {p.x, p.y, p.z};
    D3 E = {p.x + d.x, p.y + d.y, p.z + d.z};
    D3 v = {vv.x, vv.y, vv.z};
    D3 hit = {-1.0, -1.0, -1.0};                                  // ConvexQuery.cu:352
    int cur = -id - 1, next = cur, token = INT32_MIN, outSlot = 0;
    for (int j = 0; j < kMaxReflect; ++j) {
        for (int h = 0; h < kMaxHops; ++h) {
            next = trace_in_cell(S, E, cur, m, token, outSlot);
            if (next == cur || next < 0) break;
            token = cur;
            cur = next;
        }
        if (next >= 0) break;
        hit = S;
        const double4 pl = m.planes[outSlot];
        const D3 nn = {pl.x, pl.y, pl.z};
        const double sd = dot3(pl, E) - pl.w;
        E = axpy(-2.0 * sd, nn, E);
        v = axpy(-2.0 * dot3(pl, v), nn, v);
        token = next;
    }
    P[i] = make_double4(hit.x, hit.y, hit.z, p.w);
    disps[i] = make_double4(E.x - hit.x, E.y - hit.y, E.z - hit.z, d.w);
    vels[i] = make_double4(v.x, v.y, v.z, vv.w);
    ids[i] = next < 0 ? CPF_CELL_LOST : next;
}

__global__ __launch_bounds__(kBlock) void stage_move_kernel(double4* __restrict__ P, double4* __restrict__ disps,
                                                            int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double4 p = P[i];
    if (!p.w) return;
    double4 d = disps[i];
    p.x += d.x; p.y += d.y; p.z += d.z;
    d.x = 0.0; d.y = 0.0; d.z = 0.0;
    P[i] = p; disps[i] = d;
}

__global__ __launch_bounds__(kBlock) void aos_to_soa_kernel(const double4* __restrict__ P, double* x, double* y,
                                                            double* z, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) { const double4 p = P[i]; x[i] = p.x; y[i] = p.y; z[i] = p.z; }
}
__global__ __launch_bounds__(kBlock) void soa_to_aos_kernel(const double* x, const double* y, const double* z,
                                                            double4* __restrict__ P, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) P[i] = make_double4(x[i], y[i], z[i], 1.0);
}

static inline dim3 grid_of(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

hipError_t launch_stage_advect(hipStream_t st, double* P, const int32_t* ids, double* vels, double* disps, double dt,
                               int64_t n, const MeshView& m) {
    if (n > 0) hipLaunchKernelGGL(stage_advect_kernel, grid_of(n), dim3(kBlock), 0, st, (double4*)P, ids, (double4*)vels, (double4*)disps, dt, n, m);
    return hipGetLastError();
}
// "ConstantVelocity" advect (cuda/particles.cu:376-399): the particle's own stored velocity, first-order Euler
__global__ __launch_bounds__(kBlock) void stage_advect_const_kernel(double4* __restrict__ P, const int32_t* __restrict__ ids,
                                                                    const double4* __restrict__ vels, double4* __restrict__ disps,
                                                                    double dt, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double4 p = P[i];
    if (!p.w) return;
    if (ids[i] < 0) { p.w = 0.0; P[i] = p; return; }             // particles.cu:390-394
    const double4 v = vels[i];
    disps[i] = make_double4(v.x * dt, v.y * dt, v.z * dt, -1.0);  // particles.cu:398
}
hipError_t launch_stage_advect_const(hipStream_t st, double* P, const int32_t* ids, const double* vels, double* disps, double dt,
                                     int64_t n) {
    if (n > 0) hipLaunchKernelGGL(stage_advect_const_kernel, grid_of(n), dim3(kBlock), 0, st, (double4*)P, ids, (const double4*)vels, (double4*)disps, dt, n);
    return hipGetLastError();
}
hipError_t launch_stage_advect_vertex(hipStream_t st, double* P, const int32_t* ids, double* vels, double* disps, double dt,
                                      int64_t n, const double* pos, const int32_t* tets, int tetsPerCell,
                                      const double* vertVel, const double* cone, const double* apex) {
    if (n > 0)
        hipLaunchKernelGGL(stage_advect_vertex_kernel, grid_of(n), dim3(kBlock), 0, st, (double4*)P, ids, (double4*)vels,
                           (double4*)disps, dt, n, VertexField{pos, tets, vertVel, tetsPerCell, cone, reinterpret_cast<const double4*>(apex)});
    return hipGetLastError();
}

// the cone-locate tables of the "VertexVelocity" advect (see VertexField): per tet the rows of the inverse of [B-A C-A D-A] --
// (B-A, C-A, D-A) coordinates of P - A, a guess only -- and 1 / det4(A, B, C, D) by the expressions vertex_velocity() itself uses
__global__ __launch_bounds__(kBlock) void vertex_cone_tables_kernel(const double* __restrict__ pos, const int32_t* __restrict__ tets,
                                                                    int64_t nTets, int tetsPerCell, double* __restrict__ cone,
                                                                    double4* __restrict__ apex) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nTets) return;
    auto ld = [](const double* a, int k) { return D3{a[3 * (int64_t)k], a[3 * (int64_t)k + 1], a[3 * (int64_t)k + 2]}; };
    const int32_t* ix = tets + 4 * t;
    const D3 A = ld(pos, ix[0]), B = ld(pos, ix[1]), C = ld(pos, ix[2]), D = ld(pos, ix[3]);
    const double den = det4(A, B, C, D);
    const D3 b = {B.x - A.x, B.y - A.y, B.z - A.z}, c = {C.x - A.x, C.y - A.y, C.z - A.z}, d = {D.x - A.x, D.y - A.y, D.z - A.z};
    const D3 cd = {c.y * d.z - c.z * d.y, c.z * d.x - c.x * d.z, c.x * d.y - c.y * d.x};
    const D3 db = {d.y * b.z - d.z * b.y, d.z * b.x - d.x * b.z, d.x * b.y - d.y * b.x};
    const D3 bc = {b.y * c.z - b.z * c.y, b.z * c.x - b.x * c.z, b.x * c.y - b.y * c.x};
    const double vol = b.x * cd.x + b.y * cd.y + b.z * cd.z;
    const double s = vol != 0.0 ? 1.0 / vol : 0.0;
    double* g = cone + kConeDoubles * t;
    g[0] = cd.x * s; g[1] = cd.y * s; g[2] = cd.z * s;
    g[3] = db.x * s; g[4] = db.y * s; g[5] = db.z * s;
    g[6] = bc.x * s; g[7] = bc.y * s; g[8] = bc.z * s;
    g[9] = den == 0.0 ? 0.0 : 1. / den;        // (a mesh with a flat tet is not admitted to the cone locate: cpf_set_tets)
    g[10] = B.x; g[11] = B.y; g[12] = B.z; g[13] = C.x; g[14] = C.y; g[15] = C.z; g[16] = D.x; g[17] = D.y; g[18] = D.z;
    g[31] = 0.0;
    if (t % tetsPerCell == 0) apex[t / tetsPerCell] = make_double4(A.x, A.y, A.z, 0.0);
}
// the velocity part of the tet records: [19..30] = the velocities of the tet's four vertices (every cpf_set_vertex_velocity)
__global__ __launch_bounds__(kBlock) void vertex_record_velocity_kernel(const int32_t* __restrict__ tets, const double* __restrict__ vel,
                                                                        int64_t nTets, double* __restrict__ cone) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= 4 * nTets) return;
    const int64_t t = i >> 2;
    const int k = (int)(i & 3);
    const int64_t vtx = tets[i];
    double* g = cone + kConeDoubles * t + 19 + 3 * k;
    g[0] = vel[3 * vtx]; g[1] = vel[3 * vtx + 1]; g[2] = vel[3 * vtx + 2];
}
hipError_t launch_vertex_cone_tables(hipStream_t st, const double* pos, const int32_t* tets, int64_t nTets, int tetsPerCell, double* cone,
                                     double* apex) {
    if (nTets > 0) hipLaunchKernelGGL(vertex_cone_tables_kernel, grid_of(nTets), dim3(kBlock), 0, st, pos, tets, nTets, tetsPerCell, cone, (double4*)apex);
    return hipGetLastError();
}
hipError_t launch_vertex_record_velocity(hipStream_t st, const int32_t* tets, const double* vel, int64_t nTets, double* cone) {
    if (nTets > 0) hipLaunchKernelGGL(vertex_record_velocity_kernel, grid_of(4 * nTets), dim3(kBlock), 0, st, tets, vel, nTets, cone);
    return hipGetLastError();
}
hipError_t launch_stage_brownian(hipStream_t st, const double* P, double* disps, double dt, int64_t n, double D,
                                 uint32_t step, uint32_t seed) {
    if (n > 0 && D > 0.0)
        hipLaunchKernelGGL(stage_brownian_kernel, grid_of(n), dim3(kBlock), 0, st, (const double4*)P, (double4*)disps, sqrt(2.00 * D * dt), n, step, seed);
    return hipGetLastError();
}
hipError_t launch_stage_locate(hipStream_t st, const double* P, const double* disps, int32_t* ids, int64_t n,
                               const MeshView& m) {
    if (n > 0) hipLaunchKernelGGL(stage_locate_kernel, grid_of(n), dim3(kBlock), 0, st, (const double4*)P, (const double4*)disps, ids, n, m);
    return hipGetLastError();
}
hipError_t launch_stage_reflect(hipStream_t st, int32_t* ids, double* P, double* vels, double* disps, int64_t n,
                                const MeshView& m) {
    if (n > 0) hipLaunchKernelGGL(stage_reflect_kernel, grid_of(n), dim3(kBlock), 0, st, ids, (double4*)P, (double4*)vels, (double4*)disps, n, m);
    return hipGetLastError();
}
hipError_t launch_stage_move(hipStream_t st, double* P, double* disps, int64_t n) {
    if (n > 0) hipLaunchKernelGGL(stage_move_kernel, grid_of(n), dim3(kBlock), 0, st, (double4*)P, (double4*)disps, n);
    return hipGetLastError();
}
hipError_t launch_aos_to_soa(hipStream_t st, const double* P, double* x, double* y, double* z, int64_t n) {
    if (n > 0) hipLaunchKernelGGL(aos_to_soa_kernel, grid_of(n), dim3(kBlock), 0, st, (const double4*)P, x, y, z, n);
    return hipGetLastError();
}
hipError_t launch_soa_to_aos(hipStream_t st, const double* x, const double* y, const double* z, double* P, int64_t n) {
    if (n > 0) hipLaunchKernelGGL(soa_to_aos_kernel, grid_of(n), dim3(kBlock), 0, st, x, y, z, (double4*)P, n);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// initial locate: bin grid + point-in-convex-cell plane test (replaces OptiX query + baryQuery,
// query/RTQuery.cu:295-310).  Lowest-numbered containing cell wins (bins list cells ascending).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void locate_initial_kernel(const double* __restrict__ x,
                                                                const double* __restrict__ y,
                                                                const double* __restrict__ z,
                                                                int32_t* __restrict__ cell, int64_t n, MeshView m,
                                                                GridView g) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    cell[i] = locate_point(D3{x[i], y[i], z[i]}, m.cellOff, m.planes, g);   // (cpf_locate.h: shared with the respawn kernel)
}

hipError_t launch_locate_initial(hipStream_t st, const double* x, const double* y, const double* z, int32_t* cell,
                                 int64_t n, const MeshView& m, const GridView& g) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(locate_initial_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, x, y,
                       z, cell, n, m, g);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// seeding: cudaInitParticles (cuda/particles.cu:78-108) + LCG<16> (owl/common/math/random.h:56-91)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void seed_box_kernel(double* __restrict__ x, double* __restrict__ y,
                                                          double* __restrict__ z, int64_t first, int64_t n,
                                                          D3 lower, D3 size, int order) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    const int64_t id = first + k;
    uint32_t v0 = (uint32_t)(id % 128), v1 = (uint32_t)(id / 128), s0 = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        s0 += 0x9e3779b9u;
        v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + s0) ^ ((v1 >> 5) + 0xc8013ea4u);
        v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7e95761eu);
    }
    uint32_t state = v0;
    float r[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        state = 1664525u * state + 1013904223u;
        r[q] = ldexpf((float)state, -32);
    }
    if (order) { const float t = r[0]; r[0] = r[2]; r[2] = t; }
    x[k] = lower.x + (double)r[0] * size.x;
    y[k] = lower.y + (double)r[1] * size.y;
    z[k] = lower.z + (double)r[2] * size.z;
}

hipError_t launch_seed_box(hipStream_t st, double* x, double* y, double* z, int64_t first, int64_t n,
                           const double lower[3], const double upper[3], int order) {
    if (n <= 0) return hipSuccess;
    const D3 lo = {lower[0], lower[1], lower[2]};
    const D3 sz = {upper[0] - lower[0], upper[1] - lower[1], upper[2] - lower[2]};
    hipLaunchKernelGGL(seed_box_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, x, y, z,
                       first, n, lo, sz, order);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// small utility kernels
// ------------------------------------------------------------------------------------------------
__global__ void iota64_kernel(int64_t* p, int64_t n, int64_t first) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) p[i] = first + i;
}
// AoS <-> SoA conversion for the reference-shaped accessors (Particle = double4)
__global__ void unpack_xyz_kernel(const double* __restrict__ xyz, double* x, double* y, double* z, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) { x[i] = xyz[3 * i]; y[i] = xyz[3 * i + 1]; z[i] = xyz[3 * i + 2]; }
}
// scatter back to original-id order: out[gid] = (x,y,z,w)
__global__ void pack_by_gid_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                   const double* __restrict__ z, const int32_t* __restrict__ cell,
                                   const int64_t* __restrict__ gid, const double* __restrict__ vel,
                                   double* __restrict__ xyzw, int32_t* __restrict__ cellOut,
                                   double* __restrict__ velOut, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t g = gid[i];
    const int32_t c = cell[i];
    if (xyzw) {
        xyzw[4 * g] = x[i]; xyzw[4 * g + 1] = y[i]; xyzw[4 * g + 2] = z[i];
        xyzw[4 * g + 3] = (c == CPF_CELL_FROZEN) ? 0.0 : 1.0;
    }
    if (cellOut) cellOut[g] = c;
    if (velOut) {
        velOut[4 * g] = vel ? vel[3 * i] : 0.0; velOut[4 * g + 1] = vel ? vel[3 * i + 1] : 0.0;
        velOut[4 * g + 2] = vel ? vel[3 * i + 2] : 0.0; velOut[4 * g + 3] = -1.0;   // particles.cu:361
    }
}
// (zFlag: may be null; set to 1 if any cell's velocity has a z component -- what decides the flat walk, cpf_walk.h)
__global__ void u3_to_u4_kernel(const double* __restrict__ u3, double4* __restrict__ u4, int64_t nCells, unsigned long long* zFlag) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= nCells) return;
    const double uz = u3[3 * c + 2];
    u4[c] = make_double4(u3[3 * c], u3[3 * c + 1], uz, 0.0);
    if (zFlag != nullptr && !(uz == 0.0)) *zFlag = 1ull;          // (NaN counts as a component; every writer writes the same value)
}
// packed 256-byte cell records for all-hex meshes: [0..5] planes, [6] U, [7] six neighbour ids + pad
__global__ void build_cell_records_kernel(const double4* __restrict__ planes, const int32_t* __restrict__ nbr,
                                          const double4* __restrict__ U, double4* __restrict__ rec, int64_t nCells) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= nCells) return;
    double4* r = rec + 8 * c;
#pragma unroll
    for (int s = 0; s < 6; ++s) r[s] = planes[6 * c + s];
    r[6] = U[c];
    int32_t* nb = reinterpret_cast<int32_t*>(r + 7);
#pragma unroll
    for (int s = 0; s < 6; ++s) nb[s] = nbr[6 * c + s];
    nb[6] = 0; nb[7] = 0;
}
// records of a mesh that is not all-hex (layout: cpf_walk.h "cell records").  recB[c] (may be null): index of the cell's
// SECOND record (slots 6..11 of a cell with 7..12 slots), behind the nCells first ones; -1 = none
__global__ void build_cell_records_mixed_kernel(const int32_t* __restrict__ cellOff, const double4* __restrict__ planes,
                                                const int32_t* __restrict__ nbr, const double4* __restrict__ U,
                                                const int32_t* __restrict__ recB, double4* __restrict__ rec, int64_t nCells) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= nCells) return;
    const int s0 = cellOff[c], nf = cellOff[c + 1] - s0;
    const int second = recB ? recB[c] : -1;
    double4* r = rec + 8 * c;
    int32_t* nb = reinterpret_cast<int32_t*>(r + 7);
    const double4 nullPlane = make_double4(0.0, 0.0, 0.0, -1.0);
    const bool header = nf > 6 && second < 0;
    for (int s = 0; s < 6; ++s) {
        const bool real = !header && s < nf;
        r[s] = real ? planes[s0 + s] : nullPlane;
        nb[s] = real ? nbr[s0 + s] : kNullNbr;
    }
    r[6] = U[c];
    nb[6] = 0; nb[7] = 0;
    if (header) { nb[0] = kBigCellMark; nb[1] = s0; nb[2] = nf; }
    if (second >= 0) {
        nb[6] = kTwoRecMark; nb[7] = second;
        double4* r2 = rec + 8 * (int64_t)second;
        int32_t* nb2 = reinterpret_cast<int32_t*>(r2 + 7);
        for (int s = 0; s < 6; ++s) {
            const bool real = 6 + s < nf;
            r2[s] = real ? planes[s0 + 6 + s] : nullPlane;
            nb2[s] = real ? nbr[s0 + 6 + s] : kNullNbr;
        }
        r2[6] = U[c];
        nb2[6] = 0; nb2[7] = 0;
    }
}
// (box: the mesh's box records, or null -- U sits in doubles 10..12 of each, cpf_walk.h "box records")
__global__ void update_record_velocity_kernel(const double4* __restrict__ U, double4* __restrict__ rec, double* __restrict__ box,
                                              int64_t nCells) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= nCells) return;
    const double4 u = U[c];
    rec[8 * c + 6] = u;
    if (box != nullptr) { box[16 * c + 10] = u.x; box[16 * c + 11] = u.y; box[16 * c + 12] = u.z; }
}
__global__ void count_negative_kernel(const int32_t* __restrict__ cell, int64_t n, unsigned long long* out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned v = (i < n && cell[i] < 0) ? 1u : 0u;
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(out, (unsigned long long)v);
}

hipError_t launch_iota64(hipStream_t st, int64_t* p, int64_t n, int64_t first) {
    if (n > 0) hipLaunchKernelGGL(iota64_kernel, grid_of(n), dim3(kBlock), 0, st, p, n, first);
    return hipGetLastError();
}
hipError_t launch_unpack_xyz(hipStream_t st, const double* xyz, double* x, double* y, double* z, int64_t n) {
    if (n > 0) hipLaunchKernelGGL(unpack_xyz_kernel, grid_of(n), dim3(kBlock), 0, st, xyz, x, y, z, n);
    return hipGetLastError();
}
hipError_t launch_pack_by_gid(hipStream_t st, const double* x, const double* y, const double* z, const int32_t* cell,
                              const int64_t* gid, const double* vel, double* xyzw, int32_t* cellOut, double* velOut,
                              int64_t n) {
    if (n > 0)
        hipLaunchKernelGGL(pack_by_gid_kernel, grid_of(n), dim3(kBlock), 0, st, x, y, z, cell, gid, vel, xyzw, cellOut,
                           velOut, n);
    return hipGetLastError();
}
hipError_t launch_u3_to_u4(hipStream_t st, const double* u3, double4* u4, int64_t nCells, unsigned long long* zFlag) {
    if (nCells > 0) hipLaunchKernelGGL(u3_to_u4_kernel, grid_of(nCells), dim3(kBlock), 0, st, u3, u4, nCells, zFlag);
    return hipGetLastError();
}
hipError_t launch_build_cell_records(hipStream_t st, const double4* planes, const int32_t* nbr, const double4* U,
                                     double4* rec, int64_t nCells) {
    if (nCells > 0) hipLaunchKernelGGL(build_cell_records_kernel, grid_of(nCells), dim3(kBlock), 0, st, planes, nbr, U, rec, nCells);
    return hipGetLastError();
}
hipError_t launch_build_cell_records_mixed(hipStream_t st, const int32_t* cellOff, const double4* planes, const int32_t* nbr,
                                           const double4* U, const int32_t* recB, double4* rec, int64_t nCells) {
    if (nCells > 0) hipLaunchKernelGGL(build_cell_records_mixed_kernel, grid_of(nCells), dim3(kBlock), 0, st, cellOff, planes, nbr, U, recB, rec, nCells);
    return hipGetLastError();
}
hipError_t launch_update_record_velocity(hipStream_t st, const double4* U, double4* rec, double* box, int64_t nCells) {
    if (nCells > 0) hipLaunchKernelGGL(update_record_velocity_kernel, grid_of(nCells), dim3(kBlock), 0, st, U, rec, box, nCells);
    return hipGetLastError();
}
hipError_t launch_count_negative(hipStream_t st, const int32_t* cell, int64_t n, unsigned long long* out) {
    if (n > 0) hipLaunchKernelGGL(count_negative_kernel, grid_of(n), dim3(kBlock), 0, st, cell, n, out);
    return hipGetLastError();
}

// (the re-sort by cell -- its kernels, scratch layout and host side -- is cpf_sort.hip)

}  // namespace cpf
