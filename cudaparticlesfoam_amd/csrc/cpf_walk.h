// Device-side helpers shared by the step kernels (cpf_kernels.hip, cpf_stream.hip): the plane-exit test of one
// cell visit in its three data-source flavours, the Philox/Box-Muller deviates and the statistics reduction.
// Arithmetic contract: see the head of cpf_kernels.hip (explicit fma() only, -ffp-contract=off, IEEE division).
#pragma once
#include "cpf_accept.h"      // kTol, is_group, face_accept: the acceptance rule itself
#include "cpf_device.h"
#include "cpf_philox.h"    // philox4x32

namespace cpf {

// Wave-wide vote on a bool.  HIP's ballot64(int) first turns the predicate into 0/1 in a VGPR and compares it
// again (two VALU instructions per vote on a kernel that is VALU-issue bound); the builtin takes the i1 as is.
__device__ __forceinline__ unsigned long long ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// ------------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------------
struct D3 { double x, y, z; };

__device__ __forceinline__ double dot3(const double4& n, const D3& v) {
    return fma(n.z, v.z, fma(n.y, v.y, n.x * v.x));
}
__device__ __forceinline__ double dot3(const D3& n, const D3& v) {
    return fma(n.z, v.z, fma(n.y, v.y, n.x * v.x));
}
// signed plane distance (Cf - P).n = d - n.P as one fma chain (<= 0 on the inner side of the face)
__device__ __forceinline__ double plane_dist(const double4& pl, const D3& P) {
    return fma(-pl.z, P.z, fma(-pl.y, P.y, fma(-pl.x, P.x, pl.w)));
}
__device__ __forceinline__ D3 axpy(double s, const D3& a, const D3& b) {
    return {fma(s, a.x, b.x), fma(s, a.y, b.y), fma(s, a.z, b.z)};
}

constexpr int kMaxHops = 50;       // query/ConvexQuery.cu:169
constexpr int kMaxReflect = 5;     // query/ConvexQuery.cu:353

// FACE GROUPS, rule 2 (cpf_accept.h): the cell entered through a group slot is chosen at the exit point X -- the piece whose
// CELL holds X best: the smallest maximum, over that cell's slots, of X's signed plane distance; the first piece on equal
// scores (a rare path: per-lane reads of the CSR tables).
__device__ __forceinline__ int resolve_group(int code, const D3& X, const int32_t* __restrict__ cellOff, const double4* __restrict__ planes,
                                             const int32_t* __restrict__ groupOff, const int32_t* __restrict__ groupNbr) {
    const int g = code - kGroupBase;
    const int k0 = groupOff[g], k1 = groupOff[g + 1];
    double bestScore = 1e301;
    int pick = groupNbr[k0];
    for (int k = k0; k < k1; ++k) {
        const int nb = groupNbr[k];
        double score = -1e300;
        const int q0 = cellOff[nb], q1 = cellOff[nb + 1];
        for (int q = q0; q < q1; ++q) {
            const double d = plane_dist(planes[q], X);
            if (d > score) score = d;
        }
        if (score < bestScore) { bestScore = score; pick = nb; }
    }
    return pick;
}

// THIN z-LAYERED MESHES AND THE BROWNIAN KICK (MeshView::zThin: every cell is a hex whose slots 4, 5 are boundary faces with
// normals exactly along z -- a 2-D case extruded one cell thick, both tutorials' pitzDaily).  With the kick 5-10 % of the
// particles cross the front or back plane per cycle; the reference walks each of them to the plane, mirrors the end point
// and walks on (ConvexQuery.cu:286-309).  The side faces of such a mesh have nz == 0 exactly, so the cells a segment
// crosses depend on its x-y projection alone, and mirroring about a z plane leaves that projection alone: the end point
// can be mirrored about the planes BEFORE the walk -- same cells, same final point (E' = E - 2 (n.E - d) n, the
// reference's own formula, applied to the end point instead of at the hit) -- and the walk never meets the planes.  In exact
// arithmetic the two are the same trajectory; in floating point the final z differs by the rounding of the hit point the
// reference passes through (parity with the kick is statistical by contract, SURVEY.md 8c: the generator differs).  Only
// with the kick and reflecting walls; D = 0 runs keep the reference's order of operations bit for bit.
// Returns the number of mirrorings (statistics; an odd number flips the stored velocity's z).
// `clear`: the mirrored end point lies between the planes with a margin of 1e-9 of the slab's thickness.  Then NO visit of
// this particle's walk can accept a z face, in the reference's own arithmetic: from inside, fd = z_wall - S.z and den =
// fl(E.z - S.z) have equal signs only if the segment heads for that plane, and then |den| <= (|S.z - z_wall| - margin)(1 +
// 2^-53) < |fd|, so fl(fd / den) > 1 and the face is rejected (cpf_walk.h, trace_fixed: the <= 1 test is exact); the
// planes of all cells of such a mesh agree to 1e-12 of the thickness (cpf_mesh.cpp), far inside the margin, and a
// reflection off a side wall (nz == 0 exactly) leaves E.z alone.  A wave whose lanes are all clear may therefore leave both
// z faces out of its rounds -- bit-identical to testing them.
__device__ __forceinline__ int fold_z(double& ez, const double4& pa, const double4& pb, bool& clear) {
    const double za = pa.w * pa.z, zb = pb.w * pb.z;          // plane (0, 0, nz, d), nz = +-1: z = d / nz = d * nz, exactly
    const double lo = fmin(za, zb), hi = fmax(za, zb);
    int nb = 0;
#pragma unroll 1
    for (int k = 0; k < kMaxReflect && ballot64(ez < lo || ez > hi) != 0ull; ++k) {
        if (ez < lo) { ez = fma(-2.0, ez - lo, ez); ++nb; }
        else if (ez > hi) { ez = fma(-2.0, ez - hi, ez); ++nb; }
    }
    const double margin = 1e-9 * (hi - lo);
    clear = ez > lo + margin && ez < hi - margin;
    return nb;
}
// ... with the START point of the segment.  The argument above is about a segment that starts between the planes ("from inside").
// A particle that begins its cycle beyond one of them -- by a rounding of the last move's hit + (E - hit), or because its caller
// put it there -- heads back in with fd and den of equal signs and a tiny |fd|: the reference's walk accepts that z face, so a
// wave that leaves the z faces out would give such a lane other bits than a wave that tests them, and the result would depend
// on which particles share a wave (tests/test_gpu_vertex_cycle.py: a sorted cloud against an unsorted one).  Such a lane is
// not clear, whatever its end point; on a plane (sz == lo or hi) fd is 0 and the face is rejected as from inside.
__device__ __forceinline__ int fold_z(double& ez, const double sz, const double4& pa, const double4& pb, bool& clear) {
    const int nb = fold_z(ez, pa, pb, clear);
    const double za = pa.w * pa.z, zb = pb.w * pb.z;
    clear = clear && sz >= fmin(za, zb) && sz <= fmax(za, zb);
    return nb;
}

// Same test for meshes whose cells all have NF faces (every mesh the reference can run is all-hex,
// src/initCuda.H:64): slot s of cell c is 6c+s, loads are issued back to back, and the IEEE
// division is only executed for faces that can still be accepted.  The pre-filter is EXACT, not
// approximate: with fd and den of equal sign, fl(fd/den) <= 1  <=>  |fd| <= |den| (1 is
// representable and rounding is monotone; |fd| > |den| gives a quotient >= 1 + 2^-52), a zero or
// opposite-sign pair can never give dT > tol, and den == 0 / NaN fall out of every comparison
// exactly like the isinf -> -1 substitution of ConvexQuery.cu:89.
// `pl`/`nb` may be wave-uniform pointers (scalar loads, one fetch per wave) or per-lane ones.
// GROUPS: the mesh may hold face groups -- such a slot is only left with den < 0 (see above)
// AHEAD: request that many planes (and all neighbour ids) before the first test and keep that many in flight -- per-lane
// gathers from L2 / HBM, where six dependent round trips are the cost of the visit
template <int NF, bool SKIP_ZERO_DEN, bool GROUPS = false, int AHEAD = 0>
__device__ __forceinline__ int trace_fixed(D3& S, const D3& E, int cur, const double4* __restrict__ pl,
                                           const int32_t* __restrict__ nb, int token, int& outSlot, int slotBase) {
    const D3 P0 = S;
    const D3 Pd = {E.x - P0.x, E.y - P0.y, E.z - P0.z};
    int next = cur, best = -1;
    double dTmin = 1.1;
    double4 ahead[AHEAD > 0 ? AHEAD : 1];
    int nbAll[AHEAD > 0 ? NF : 1];
    if (AHEAD > 0) {
#pragma unroll
        for (int s = 0; s < AHEAD; ++s) ahead[s] = pl[s];
#pragma unroll
        for (int s = 0; s < NF; ++s) nbAll[s] = nb[s];
#pragma unroll
        for (int s = 0; s < AHEAD; ++s) asm volatile("" : "+v"(ahead[s].x), "+v"(ahead[s].y), "+v"(ahead[s].z), "+v"(ahead[s].w));
    }
#pragma unroll
    for (int s = 0; s < NF; ++s) {
        double4 p;
        if (AHEAD > 0) {
            constexpr int A = AHEAD > 0 ? AHEAD : 1;
            p = ahead[s % A];
            if (s + AHEAD < NF) ahead[s % A] = pl[s + AHEAD];
        } else p = pl[s];
        const double den = dot3(p, Pd);
        // no lane of the wave moves across this face's plane (den == +-0 exactly, e.g. the front/back
        // faces of a one-cell-thick mesh, or wall-parallel faces in aligned flow): dT would be +-inf
        // (-> -1) or NaN, never accepted (ConvexQuery.cu:86-95), so the face costs nothing more
        // (only worth a branch when the planes are already on chip: it would serialise global gathers)
        if (SKIP_ZERO_DEN && ballot64(den != 0.0) == 0ull) continue;
        const int bs = AHEAD > 0 ? nbAll[s] : nb[s];
        const double fd = plane_dist(p, P0);
        // |fd| <= |den| (one compare with abs modifiers) and equal sign bits (integer test); zeros and
        // NaNs that slip through give dT = 0 / NaN and fail dT > tol below, as in the reference
        const bool c1 = fabs(fd) <= fabs(den), c2 = (__double2hiint(fd) ^ __double2hiint(den)) >= 0;
        const bool c3 = fd < kTol, c4 = bs != token && !(GROUPS && is_group(bs) && !(den < 0.0));
        const bool cand = c1 && c2 && c3 && c4;
        // wave-uniform skip: hipcc would otherwise if-convert and run the ~12-instruction IEEE division for
        // every face of every lane; most faces have no candidate lane at all.  The vote is the AND of the four
        // compare masks (scalar ALU); voting on `cand` itself makes the compiler rebuild it as 0/1 in a VGPR.
        if ((ballot64(c1) & ballot64(c2) & ballot64(c3) & __builtin_amdgcn_uicmp((unsigned)bs, (unsigned)token, 33 /* ne */)) != 0ull) {
            if (cand) {
                const double dT = fd / den;
                if (dT > kTol && dT < dTmin) { dTmin = dT; next = bs; best = s; }
            }
        }
    }
    if (best >= 0) {                   // exit point of the LAST accepted face == the smallest dT
        S = axpy(dTmin, Pd, P0);
        outSlot = slotBase + best;
    }
    return next;
}

// The same six-face test for a hex record sitting in LDS (wave-cooperative kernel).  Identical arithmetic and
// acceptance order; what differs is the SCHEDULE: the planes are fetched two at a time in straight-line code
// before the wave-uniform skips, so a round pays three LDS round trips instead of six (the per-face branches keep
// the compiler from hoisting the reads itself, and this kernel is bound by the length of each wave's dependent
// chain, not by instruction issue).
// ZERO_SKIP: try the zero-denominator skip at all -- pointless (a compare and a branch per face) once every particle
// has a displacement along every axis, i.e. with the Brownian kick; results are the same with or without it.
// FLAT: the two-term den and fd of the flat walk (see below): the plane's nz == +-0 exactly and is not read.
// The wave vote is cheap and a superset, the exact test runs only where it can matter.  A lane can be accepted only if
// |fd| <= |den| with equal signs and fd < tol: from inside (fd < 0) that means den <= fd; every other acceptable lane has
// fd >= 0 (on or outside the plane: the face it came in through, or an entry point rounded across a neighbouring face).
// (den <= fd) | (fd >= 0) is therefore a superset of the candidates -- two compares per face instead of five, two scalar
// operations instead of five -- and the exact predicate (cpf_accept.h, face_accept) decides inside the branch.
__device__ __forceinline__ unsigned long long face_vote(double den, double fd, int bs, int token) {
    return (ballot64(den <= fd) | ballot64(fd >= 0.0)) & __builtin_amdgcn_uicmp((unsigned)bs, (unsigned)token, 33 /* ne */);
}
template <bool ZERO_SKIP, bool GROUPS = false, bool FLAT = false>
__device__ __forceinline__ void face_test(const double4& p, int bs, const D3& P0, const D3& Pd, int token, int s,
                                          double& dTmin, int& next, int& best) {
    const double den = FLAT ? fma(p.y, Pd.y, p.x * Pd.x) : dot3(p, Pd);
    if (ZERO_SKIP && ballot64(den != 0.0) == 0ull) return;          // see trace_fixed: nobody crosses this plane
    const double fd = FLAT ? fma(-p.y, P0.y, fma(-p.x, P0.x, p.w)) : plane_dist(p, P0);
    if (face_vote(den, fd, bs, token) != 0ull) face_accept<GROUPS>(den, fd, bs, token, s, dTmin, next, best);
}

// The plane offsets are requested together with the normals (the empty asm pins them): left alone, the compiler sinks
// their LDS reads behind the first wave-uniform skip of each pair -- one more LDS round trip on the wave's dependent
// chain per pair.  Measured at steady clocks: 1-2 % on the 3-D meshes (no face is skipped there before its offset is
// needed), nothing either way on pitzDaily.
#define CPF_PIN_W(a, b) asm volatile("" : "+v"(a.w), "+v"(b.w));
// ONE PAIR of a cell record (see "cell records" below): the two face tests of slots s and s + 1, whose planes and int2 of
// neighbours the caller has just fetched -- in its own straight-line code, which is what keeps the two LDS reads together.
template <bool ZERO_SKIP, bool GROUPS, bool FLAT = false>
__device__ __forceinline__ void record_pair(double4& pa, double4& pb, const int2 b, int s, const D3& P0, const D3& Pd, int token, double& dTmin, int& next, int& best) {
    CPF_PIN_W(pa, pb)
    face_test<ZERO_SKIP, GROUPS, FLAT>(pa, b.x, P0, Pd, token, s, dTmin, next, best);
    face_test<ZERO_SKIP, GROUPS, FLAT>(pb, b.y, P0, Pd, token, s + 1, dTmin, next, best);
}
// zLast (wave-uniform; MeshView::zPairLast): slots 4 and 5 are the cell's two faces with an exactly z-parallel normal.
// When no active lane moves in z (Pd.z == +-0 exactly: 2-D flow on a z-extruded mesh, no diffusion) both denominators
// are exactly +-0 for every lane -- nx == ny == 0 leaves den = nz * 0 -- so neither face can be accepted
// (ConvexQuery.cu:86-95) and ONE test replaces two plane fetches, two denominators and two votes.  Exact, not
// approximate: it is the zero-denominator skip of face_test, decided for the pair up front.
// zNever (wave-uniform): no active lane can leave through a z face at all (the Brownian kick on a one-cell-thick mesh with
// every end point mirrored clear of the planes: fold_z) -- the pair is left out whatever Pd.z is.
template <bool ZERO_SKIP = true, bool GROUPS = false>
__device__ __forceinline__ int trace_lds6(D3& S, const D3& E, int cur, const double4* rec, int token, int& outSlot, bool zLast = false,
                                          bool zNever = false) {
    const D3 P0 = S;
    const D3 Pd = {E.x - P0.x, E.y - P0.y, E.z - P0.z};
    int next = cur, best = -1;
    double dTmin = 2.0;                 // any start value > 1 is equivalent (candidates have dT <= 1); 2.0 is an inline constant
    const int2* nb = reinterpret_cast<const int2*>(rec + 7);
    { double4 p0 = rec[0], p1 = rec[1]; record_pair<ZERO_SKIP, GROUPS>(p0, p1, nb[0], 0, P0, Pd, token, dTmin, next, best); }
    { double4 p2 = rec[2], p3 = rec[3]; record_pair<ZERO_SKIP, GROUPS>(p2, p3, nb[1], 2, P0, Pd, token, dTmin, next, best); }
    if (!(zNever || (zLast && ballot64(Pd.z != 0.0) == 0ull))) {
        double4 p4 = rec[4], p5 = rec[5]; record_pair<ZERO_SKIP, GROUPS>(p4, p5, nb[2], 4, P0, Pd, token, dTmin, next, best);
    }
    if (best >= 0) {
        S = axpy(dTmin, Pd, P0);
        outSlot = best;
    }
    return next;
}

// ONE RECORD of a visit on a mesh with two-record cells (7 ... 12 slots, see "cell records" below): the six face tests of the
// record -- slots base .. base + 5 of the cell, base = 0 or 6 -- continuing from (dTmin, next, best) and leaving the exit
// point to the caller, which concludes after the cell's last record.  Same tests, same order, same strict "<" as one pass
// over the cell's slots.  (The LOOKUP 2 instantiation runs EVERY visit through this one instance -- an ordinary cell is a
// first record that is also the last --: three inlined copies of the six tests cost the instantiation 25 % on a mesh without
// a single big cell.)
template <bool ZERO_SKIP, bool GROUPS>
__device__ __forceinline__ void trace_lds6_record(const D3& P0, const D3& Pd, const double4* rec, int token, int base, double& dTmin, int& next, int& best) {
    const int2* nb = reinterpret_cast<const int2*>(rec + 7);
    { double4 p0 = rec[0], p1 = rec[1]; record_pair<ZERO_SKIP, GROUPS>(p0, p1, nb[0], base + 0, P0, Pd, token, dTmin, next, best); }
    { double4 p2 = rec[2], p3 = rec[3]; record_pair<ZERO_SKIP, GROUPS>(p2, p3, nb[1], base + 2, P0, Pd, token, dTmin, next, best); }
    { double4 p4 = rec[4], p5 = rec[5]; record_pair<ZERO_SKIP, GROUPS>(p4, p5, nb[2], base + 4, P0, Pd, token, dTmin, next, best); }
}

// FLAT WALK (MeshView::zSide0 + a velocity field without a z component + no Brownian kick: a 2-D case as both tutorials'
// pitzDaily run it with D = 0): the mesh is z-layered with its z faces in slots 4, 5 (zPairLast) and the four side faces of
// every cell have nz == 0 EXACTLY; no particle has a displacement in z (Pd.z == +-0 exactly: dt * 0 added to and subtracted
// from P.z, and a mirror about a wall with nz == 0 leaves E.z alone).  Then, bit for bit: the z faces have den == +-0 for
// every lane and are never accepted (the zLast shortcut of trace_lds6, here decided at launch instead of per round), and a
// side face's den = fma(nz, Pd.z, t) = t and fd = fma(-nz, P0.z, u) = u up to the sign of a zero result, which no comparison
// sees -- two FMAs per face that need not be issued, a vote and a branch per round that need not be taken, and no z in the walk.
// (face_test<.., FLAT>; S.z is left alone: fma(dT, +-0, P0.z) is P0.z)
//
// SETTLED Z (CPF_STEP_Z_SETTLED: what admits a flat launch to the body without z, below).  What one flat cycle does to a live particle's z is a function f of z
// alone: the advect gives Pn.z = z + dt * u.z with u.z == +-0 and dt finite (cpf_step_dev refuses any other), disp.z = Pn.z - z,
// E.z = z + disp.z; the walk never moves S.z; a mirror about a side wall adds -2 sd * nz with nz == +-0 (a wall is only ever a
// side face here, and sd is finite for finite z -- see "not settled" below for the others: a lane with a non-finite x or y never
// meets a face, dT = fd / den is then NaN or infinite);
// the move gives E.z, or hit.z + (E.z - hit.z) with hit.z == z.  Case by case, in round-to-nearest:
//   * z finite and non-zero: every zero added is exact and z + (+0) == z -- f(z) = z, the same bits;
//   * z == +0: +0 + (+-0) == +0 -- f(+0) = +0;  z == -0: disp.z = (+-0) - (-0) = +0 and -0 + (+0) == +0 -- f(-0) = +0;
//   * z == +-inf: disp.z = inf - inf is NaN -- f(+-inf) = NaN;  z NaN: f(z) is NaN.
// So f(f(z)) == f(z) for every z but NaN, and for a NaN as well provided the ALU maps a NaN operand to the same NaN every time
// -- it either propagates the (quieted) operand or returns the default NaN, both idempotent -- which is all the NaN case needs:
// no comparison of the walk reads z, x, y and the cell do not depend on it, and the argument only requires that a second
// application give the bits the first one gave.  Lanes that are frozen or lost (cell < 0) store what they loaded, so they
// keep their z whichever way; a lane lost DURING a cycle (no-reflect wall, five bounces) gets the move first, i.e. f(z), then
// is frozen for good.  Hence: after one flat launch of at least one cycle that streamed z, every particle's z in memory is a
// fixed point of f (or belongs to a particle no flat cycle steps again), and every later flat launch may leave z in memory as
// it is -- the bits a streaming launch would have written.  What ends it: anything that writes x, y, z or cell other than a
// sort (a sort only permutes) -- a particle set or seeded anew, a frozen particle revived by cpf_locate_initial, hand-off
// arrivals -- and any launch that is not the flat walk (the kick, a field with a z component, the vertex advect).  Only -0 and
// +-inf are rewritten by the first cycle; NaN needs the idempotence above, finite non-zero z needs nothing.
//
// NOT SETTLED: A LIVE PARTICLE WHOSE Z IS NOT FINITE (round 8).  "sd is finite" above argues from x and y and holds for finite z
// only.  The flat walk's face tests do not read z, so a live particle with z == NaN (+-inf is NaN after its first flat cycle)
// does reach a wall, and the mirror's sd = dot3(plane, E) - w = fma(nz, NaN, ...) - w is NaN: the launch that streams z turns
// its x and y into NaN, a launch that leaves z alone computes with z = 0 and reflects it.  x and y DO depend on z there.  So
// a cloud that may hold such a particle is not called settled: the flat launch that streams z reports one (StreamArgs::zBad, a
// pinned word the cloud's owner reads behind that launch, once, before the first launch that would leave z alone -- no pass
// over the cloud), and flat launches keep streaming z for as long as one is reported.
//
// THE BODY WITHOUT Z (stream_body's ZSET, step_kernel_stream_flat: what a flat launch on a settled cloud runs).  Round 7 ran
// such a launch on the three-coordinate body behind a run-time flag, with z = 0.0 in place of the z it did not load (the flag went
// in round 14: "no z" is the template parameter alone).  Every z term is then a product or a
// sum of zeros, and dropping it gives the same bits in x, y and the cell, for every input:
//   * advect, displacement, end point, move: z components only; x and y never read them;
//   * the mirror: sd = dot3(plane, E) - w = fma(nz, E.z, t) - w with t = fma(ny, E.y, nx * E.x), nz == +-0, E.z == +-0.  The
//     product is +-0 and t + (+-0) == t unless t is itself a zero, where only the sign of that zero can change; sd = t - w then
//     differs at most in the sign of a zero result (w == 0), and so does the factor -2 sd.  E.x' = fma(-2 sd, nx, E.x) with
//     E.x != 0 adds a zero product to a non-zero addend: the same bits.  E.z' = fma(-2 sd, nz, E.z) is a zero: not kept.
//     (What is left: t == -0, w == 0 and an end point coordinate that is itself a zero -- an end point exactly at the origin, with
//     x == -0, on a wall through the origin.  Only then could the sign of a stored zero differ.  No comparison reads it either.);
//   * the velocity mirror, v' = v - 2 dot3(plane, v) n with v.z == +-0, nz == +-0: the same argument term by term; the
//     body keeps all three components of v as they were (only a launch that stores velocities reads them at all);
//   * no comparison of the walk reads a z or the sign of a zero (trace_lds4_flat below reads x and y only).
// What is left in memory: z untouched, the bits a streaming launch would have written (the fixed-point argument above).
// KEEP_Z: the flat walk under the kick, below.
//
// FLAT WALK UNDER THE KICK (round 6; KEEP_Z).  With the Brownian kick every particle moves in z, so the flat walk above does not apply --
// but on a one-cell-thick mesh whose side faces have nz == 0 exactly (zThin && zSide0), once fold_z has mirrored every lane's end
// point clear of the z planes (`zFold && !zUnclear`: the condition that already drops the z pair from trace_lds6), the four
// side faces are all that is tested, and their dropped terms are 0 * finite: den = fma(0, Pd.z, t) = t and fd = fma(-0, P0.z, u)
// = u up to the sign of a zero, which no comparison sees (E.z and P0.z are finite: a lane with a NaN or infinite end point is
// never `clear`).  The exit point keeps its z: S = P0 + dT * Pd with the real Pd.z.  Same bits as trace_lds6(..., zNever = true).
//
// THE FACE BLOCK IN HAND-WRITTEN ISA (FACE_ASM; the body without z only: step_kernel_stream_flat, stream_body's kFaceAsm).  The C++ face
// test computes every predicate into a scalar register pair and combines them on the scalar ALU -- a vote of three compares, a
// scalar compare and a branch, then the exact predicate's four compares, four scalar operations, a saveexec and a branch, then
// two more compares, an AND and a saveexec: 14 scalar-issue instructions per face with a candidate lane, in a kernel whose
// scalar pipe is the busier one (docs/experiments.md, round 9).  v_cmpx narrows EXEC itself, so a chain of them is an AND that
// costs the scalar pipe nothing: save EXEC, c4, c3, c12 (cpf_accept.h, face_accept_chain: c1 and c2 as one comparison of the bit
// patterns -- the same accepted set, argued there), ONE branch over the division, the division as hipcc expands fd / den (correctly rounded: the same bits), dT > tol,
// dT < dTmin, three moves, restore EXEC -- three scalar-issue instructions per face, candidate or not, and seven vector
// instructions for a face without a candidate lane (as many as the C++ vote), 24 for one with (28).  den and fd stay in C++: the
// compiler interleaves the two chains of a pair.
// Wait states, by hand (the compiler's hazard recogniser does not look inside the string):
//   * v_div_scale writes VCC, v_div_fmas reads it: four states wanted, six instructions lie between;
//   * v_rcp_f64 (transcendental unit) -> its first reader: one independent instruction between, as hipcc schedules it;
//   * a VALU write of EXEC (v_cmpx) -> a lane-crossing read (DPP, v_readlane, v_readfirstlane, v_permlane): five states.  None
//     is in the block; behind the last v_cmpx of either path lie a branch and a scalar move at the least before compiler code
//     resumes, and tests/test_build_resources_flat_face.py holds that no such instruction follows a block within five.
//   * v_cmpx -> s_cbranch_execz and v_cmpx -> VALU under the new mask need none (hipcc emits both back to back).
template <int SLOT>
__device__ __forceinline__ void face_accept_flat_asm(double den, double fd, int bs, int token, double& dTmin, int& next, int& best) {
    double q0, q1, q2, q3;                 // the division's temporaries; dT ends up in q0
    unsigned long long keep;
    const double tol = kTol;
    asm volatile(
        "s_mov_b64 %[keep], exec\n\t"
        "v_cmpx_ne_u32_e32 vcc, %[bs], %[tok]\n\t"               // c4
        "v_cmpx_gt_f64_e32 vcc, %[tol], %[fd]\n\t"               // c3
        "v_cmpx_le_u64_e32 vcc, %[fd], %[den]\n\t"               // c12
        "s_cbranch_execz .Lcpf_face_%=\n\t"
        "v_div_scale_f64 %[q0], vcc, %[den], %[den], %[fd]\n\t"
        "v_rcp_f64_e32 %[q1], %[q0]\n\t"
        "v_div_scale_f64 %[q2], vcc, %[fd], %[den], %[fd]\n\t"
        "v_fma_f64 %[q3], -%[q0], %[q1], 1.0\n\t"
        "v_fmac_f64_e32 %[q1], %[q1], %[q3]\n\t"
        "v_fma_f64 %[q3], -%[q0], %[q1], 1.0\n\t"
        "v_fmac_f64_e32 %[q1], %[q1], %[q3]\n\t"
        "v_mul_f64 %[q3], %[q2], %[q1]\n\t"
        "v_fma_f64 %[q0], -%[q0], %[q3], %[q2]\n\t"
        "v_div_fmas_f64 %[q0], %[q0], %[q1], %[q3]\n\t"
        "v_div_fixup_f64 %[q0], %[q0], %[den], %[fd]\n\t"
        "v_cmpx_lt_f64_e32 vcc, %[tol], %[q0]\n\t"               // dT > tol
        "v_cmpx_lt_f64_e32 vcc, %[q0], %[dtm]\n\t"               // dT < dTmin
        "v_mov_b64_e32 %[dtm], %[q0]\n\t"
        "v_mov_b32_e32 %[nx], %[bs]\n\t"
        "v_mov_b32_e32 %[bst], %[slot]\n"
        ".Lcpf_face_%=:\n\t"
        "s_mov_b64 exec, %[keep]"
        : [dtm] "+v"(dTmin), [nx] "+v"(next), [bst] "+v"(best), [q0] "=&v"(q0), [q1] "=&v"(q1), [q2] "=&v"(q2), [q3] "=&v"(q3),
          [keep] "=&s"(keep)
        : [den] "v"(den), [fd] "v"(fd), [bs] "v"(bs), [tok] "v"(token), [tol] "s"(tol), [slot] "n"(SLOT)
        : "vcc");
}
// ONE PAIR, FACE_ASM: record_pair<.., FLAT> with the face block above -- same planes, same den and fd, same order.
template <int SLOT>
__device__ __forceinline__ void record_pair_flat_asm(double4& pa, double4& pb, const int2 b, const D3& P0, const D3& Pd, int token, double& dTmin, int& next, int& best) {
    CPF_PIN_W(pa, pb)
    const double denA = fma(pa.y, Pd.y, pa.x * Pd.x), fdA = fma(-pa.y, P0.y, fma(-pa.x, P0.x, pa.w));
    const double denB = fma(pb.y, Pd.y, pb.x * Pd.x), fdB = fma(-pb.y, P0.y, fma(-pb.x, P0.x, pb.w));
    face_accept_flat_asm<SLOT>(denA, fdA, b.x, token, dTmin, next, best);
    face_accept_flat_asm<SLOT + 1>(denB, fdB, b.y, token, dTmin, next, best);
}
//
// THE EXIT POINT WITHOUT ITS SELECT (EXIT_ALWAYS, round 15; the body without z only).  `if (best >= 0) { S = P0 + dTmin * Pd; outSlot =
// best; }` is a compare and four selects per visit, and `best = -1` a move, for the sake of the lanes that accepted no face: theirs
// keep S and outSlot.  In stream_body's ZSET round nobody reads either of such a lane, so the body computes S = fma(dTmin, Pd, P0)
// with dTmin still 2.0 for them, leaves `best` unset until a face is accepted, and hands it out as it is.  The argument:
//   * next and best are written together, by an accepted face only (face_accept_flat_asm: three moves under one EXEC), so a lane
//     that accepted none returns next == cur.  outcome_flat ends it (endsM): its busy bit is cleared, it makes no further visit in this
//     cycle, and cycle_end -- which every lane with cur >= 0 runs, and a visiting lane was busy, so cur >= 0, and ending leaves cur as it
//     was -- writes S_ = E, or hit + (E - hit) with the PARKED hit point, before anything reads S_: park_hit(S_) and the mirror read
//     it in the wall branch (an accepted wall face), the next visit's P0 belongs to a lane that is still busy (it crossed or was
//     mirrored: an accepted face).  outSlot is read for the wall's plane alone, under next < 0: an accepted face (next == cur >= 0
//     otherwise).  No load is issued from an unset outSlot: the read stands inside the region of the lanes with next < 0.
//   * hop cap: a lane reaches it by crossing -- an accepted face, a proper S_; it is done and cycle_end overwrites S_ all the same.
//   * five bounces: every bounce is an accepted wall face; park_hit and the mirror read a proper S_, the sixth visit never happens.
//   * a wall without reflection: accepted; S_ is not read (no park_hit), j = kMaxReflect, and cycle_end (REFLECT false) writes S_ = E.
//   * fused cycles: cycle_end closes every cycle of the launch, and the next cycle's first visit starts from the S_ it wrote; the
//     tile's result is that S_ too.  A launch of zero cycles has no busy lane and makes no visit.
//   * non-finite Pd (x, y or the record's velocity not finite): every comparison of the face block that reads den, fd or dT is an
//     ordered one and fails, no face is accepted, next == cur: the first case.  S_ holds a NaN until cycle_end writes E over it -- the
//     bits it wrote before, for E and the parked hit point do not come from S_ of this visit.
//   * lanes that are not visiting -- not busy, or left without a slot in a round that is no gather round -- are outside the EXEC
//     mask of the region the visit stands in: their S_ is not written at all.
// (Round 13 measured the select under a narrowed EXEC instead: 9 vector instructions fewer, 4 scalar more, no gain.)
template <bool ZERO_SKIP, bool KEEP_Z = false, bool FACE_ASM = false, bool EXIT_ALWAYS = false>
__device__ __forceinline__ int trace_lds4_flat(D3& S, const D3& E, int cur, const double4* rec, int token, int& outSlot) {
    static_assert(!(FACE_ASM && (KEEP_Z || ZERO_SKIP)), "the hand-written face block is the body without z's, without the zero-denominator vote");
    static_assert(!EXIT_ALWAYS || FACE_ASM, "the exit point without its select: argued for the body without z and its face block");
    const D3 P0 = S;
    const D3 Pd = {E.x - P0.x, E.y - P0.y, KEEP_Z ? E.z - P0.z : 0.0};
    int next = cur, best = -1;
    if constexpr (EXIT_ALWAYS) asm volatile("" : "=v"(best));          // (unset: no move; read only where a face block has written it)
    double dTmin = 2.0;
    const int2* nb = reinterpret_cast<const int2*>(rec + 7);
    if constexpr (FACE_ASM) {
        { double4 p0 = rec[0], p1 = rec[1]; record_pair_flat_asm<0>(p0, p1, nb[0], P0, Pd, token, dTmin, next, best); }
        { double4 p2 = rec[2], p3 = rec[3]; record_pair_flat_asm<2>(p2, p3, nb[1], P0, Pd, token, dTmin, next, best); }
    } else {
    { double4 p0 = rec[0], p1 = rec[1]; record_pair<ZERO_SKIP, false, true>(p0, p1, nb[0], 0, P0, Pd, token, dTmin, next, best); }
    { double4 p2 = rec[2], p3 = rec[3]; record_pair<ZERO_SKIP, false, true>(p2, p3, nb[1], 2, P0, Pd, token, dTmin, next, best); }
    }
    if (EXIT_ALWAYS || best >= 0) {
        if (KEEP_Z) S = axpy(dTmin, Pd, P0);
        else { S.x = fma(dTmin, Pd.x, P0.x); S.y = fma(dTmin, Pd.y, P0.y); }
        outSlot = best;
    }
    return next;
}

// The same six face tests, two faces per wave-uniform decision: both denominators and both plane distances are computed
// up front (four independent FMA chains instead of two short ones between branches), then ONE test decides whether either
// face has a candidate lane.  No zero-denominator skip: a lane with den == 0 is a candidate only with fd >= 0, and is then
// rejected by the exact predicate (|fd| <= |den| leaves fd == 0, whose quotient is NaN) exactly as in face_test.  More
// vector instructions where faces used to be skipped for zero denominators (2-D cases), fewer branches and shorter
// dependent chains everywhere: used where every face is live anyway (3-D meshes, the Brownian kick).
__device__ __forceinline__ void face_pair_test(const double4& pa, const double4& pb, int2 b, const D3& P0, const D3& Pd, int token,
                                               int s, double& dTmin, int& next, int& best) {
    const double denA = dot3(pa, Pd), denB = dot3(pb, Pd);
    const double fdA = plane_dist(pa, P0), fdB = plane_dist(pb, P0);
    const unsigned long long mA = face_vote(denA, fdA, b.x, token), mB = face_vote(denB, fdB, b.y, token);
    if ((mA | mB) != 0ull) {
        if (mA != 0ull) face_accept<false>(denA, fdA, b.x, token, s, dTmin, next, best);
        if (mB != 0ull) face_accept<false>(denB, fdB, b.y, token, s + 1, dTmin, next, best);
    }
}
__device__ __forceinline__ int trace_lds6_paired(D3& S, const D3& E, int cur, const double4* rec, int token, int& outSlot, bool zLast = false) {
    const D3 P0 = S;
    const D3 Pd = {E.x - P0.x, E.y - P0.y, E.z - P0.z};
    int next = cur, best = -1;
    double dTmin = 2.0;
    const int2* nb = reinterpret_cast<const int2*>(rec + 7);
    { const double4 p0 = rec[0], p1 = rec[1]; face_pair_test(p0, p1, nb[0], P0, Pd, token, 0, dTmin, next, best); }
    { const double4 p2 = rec[2], p3 = rec[3]; face_pair_test(p2, p3, nb[1], P0, Pd, token, 2, dTmin, next, best); }
    if (!(zLast && ballot64(Pd.z != 0.0) == 0ull)) {          // see trace_lds6
        const double4 p4 = rec[4], p5 = rec[5]; face_pair_test(p4, p5, nb[2], P0, Pd, token, 4, dTmin, next, best);
    }
    if (best >= 0) {
        S = axpy(dTmin, Pd, P0);
        outSlot = best;
    }
    return next;
}

// Cell records (MeshView::cellRec, 256 bytes per cell = 8 double4): [0..5] the planes of face slots 0..5, [6] U,
// [7] six neighbour ids (int32) + two spare words.  On meshes that are not all-hex (MeshView::mixed):
//   * a cell with FEWER than 6 faces (prism, tet, pyramid) is padded with null faces -- plane (0, 0, 0, -1), neighbour
//     kNullNbr: den == 0 and fd == -1 for every particle, so the face can never be accepted (ConvexQuery.cu:86-95) and
//     the six-slot tests give what the walk over its real faces gives, in the same slot order;
//   * a cell with MORE than 6 faces (next to a 2:1 refinement: 7 ... 24) has a HEADER record: neighbour word 0 =
//     kBigCellMark, word 1 = its first CSR slot, word 2 = its face count, null planes, U as usual.  A lane in such a
//     cell walks the CSR tables (planes / nbr in global memory) with trace_csr -- same arithmetic, same slot order.
// The reference cannot run such meshes at all (src/initCuda.H:64: tetsPerCell = 12).
//   * a cell with 7 ... 12 slots (true polyhedra: a pentagonal prism has seven planes, a polyDualMesh cell a dozen) has TWO
//     records: the first holds slots 0..5 and U, spare word 6 = kTwoRecMark, spare word 7 = the index of the second one,
//     which lies behind the nCells first records and holds slots 6..11 (null-padded).  A lane in such a cell tests the
//     first record in one round and the second in the next, carrying (dTmin, next, best) across -- the same twelve tests
//     in the same order with the same strict "<", so bit-identical to the walk over the CSR slots -- and both stay LDS
//     tests; a cell with more than 12 slots keeps the header record.
constexpr int kNullNbr = INT32_MIN + 5;
constexpr int kBigCellMark = INT32_MIN + 6;
constexpr int kTwoRecMark = INT32_MIN + 9;

// BOX RECORDS (MeshView::boxRec, 128 bytes = 16 doubles per cell; built by cpf_mesh.cpp when EVERY cell of the mesh is an
// axis-aligned box: six planes whose normals are exactly +-e_x, +-e_y, +-e_z, one of each -- blockMesh cases such as the
// TJunction tutorial).  Canonical slot k = 2 * axis + (normal component == -1):
//   doubles 0..5   the plane offsets d_k
//   bytes  48..71  the six neighbour codes (int32), bytes 72..75 the ORDER CODE: bits 3k..3k+2 = the slot's place in the
//                  walk's own slot order (HostTables), bits 18+2k, 19+2k = sign bits of the normal's two zero components
//   doubles 10..12 U
// What the six-face test becomes, bit for bit (the dropped terms of the reference's dot products are exact zeros, which
// change at most the sign of a zero result -- and no comparison below sees the sign of a zero):
//   den_k = n_a * Pd_a = +-Pd_a exactly,   fd_k = fl(d_k - n_a * P0_a)  (one rounding, as the innermost live fma of plane_dist).
// A face can be accepted (ConvexQuery.cu:86-95: fd < tol, tol < dT <= 1, smallest dT, ties to the lower slot) only if
// fd and den have equal signs; with den > 0 -- the face of the pair the particle moves AWAY from -- that needs fd > 0: the
// particle outside its cell by a rounding (never beyond 1e-13: fd < tol).  Hence per axis only the face the particle moves
// TOWARDS is tested (den = -|Pd_a|): three candidates per visit instead of six, no normal ever fetched, one LDS round trip
// for the whole record instead of three.  The rest -- a lane with fd > 0 on any face that is not the one it came in through,
// two axes with exactly equal dT (the ORIGINAL slot order decides, not the canonical one), a displacement that is not
// finite (0 * inf = NaN poisons every denominator of the reference form) -- sends the WAVE through trace_box_slow, which
// evaluates the reference's predicate on all six faces and breaks ties by original slot.  Parity: tests/test_gpu_box.py,
// tools/fuzz_parity.py box (structured clouds that sit on faces, edges and diagonals).
__device__ __forceinline__ double4 box_wall_plane(const double4* rec4, int k) {
    const unsigned code = reinterpret_cast<const unsigned*>(rec4)[18];
    const int axis = k >> 1;
    const double one = (k & 1) ? -1.0 : 1.0;
    const double z1 = ((code >> (18 + 2 * k)) & 1u) ? -0.0 : 0.0, z2 = ((code >> (19 + 2 * k)) & 1u) ? -0.0 : 0.0;
    double4 p;
    p.x = axis == 0 ? one : z1;
    p.y = axis == 1 ? one : (axis == 0 ? z1 : z2);
    p.z = axis == 2 ? one : z2;
    p.w = reinterpret_cast<const double*>(rec4)[k];
    return p;
}
// the reference's predicate on all six faces of a box record, ties to the lower ORIGINAL slot (rare path of trace_box)
template <bool GROUPS>
__device__ __forceinline__ void trace_box_slow(const D3& P0, const D3& Pd, const double4* rec4, int token, double& dTmin, int& next, int& best) {
    const double* rd = reinterpret_cast<const double*>(rec4);
    const int* ri = reinterpret_cast<const int*>(rec4);
    const unsigned code = (unsigned)ri[18];
    // (what the zero components of the normals contribute in the reference form: +-0, or NaN next to an infinity or a NaN)
    const double nanD = Pd.x * 0.0 + Pd.y * 0.0 + Pd.z * 0.0, nanP = P0.x * 0.0 + P0.y * 0.0 + P0.z * 0.0;
    int ordBest = 8;
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
        const int a = k >> 1;
        const double pa = a == 0 ? P0.x : (a == 1 ? P0.y : P0.z), da = a == 0 ? Pd.x : (a == 1 ? Pd.y : Pd.z);
        const double w = rd[k];
        const int nb = ri[12 + k];
        const double fd = ((k & 1) ? w + pa : w - pa) + nanP, den = ((k & 1) ? -da : da) + nanD;
        const int ord = (int)((code >> (3 * k)) & 7u);
        double dT = fd / den;
        if (__builtin_isinf(dT)) dT = -1.0;
        if (nb == token) continue;
        if (GROUPS && is_group(nb) && !(den < 0.0)) continue;       // face groups: outward crossings only (cpf_accept.h)
        if (fd < kTol && dT > kTol && dT <= 1.0 && (dT < dTmin || (dT == dTmin && ord < ordBest))) { dTmin = dT; next = nb; best = k; ordBest = ord; }
    }
}
// GROUPS (a mesh of boxes with face groups -- 2:1-refined boxes, the castellated kind: a box with a split face keeps one slot for
// it, neighbour code = the group's): a group slot is only ever left with den < 0, i.e. through the face the particle moves
// TOWARDS -- the three candidates cover it as they are; away from it (den > 0) it is never accepted, so it does not count
// among the "outside a face" lanes either (a lane that came INTO the big cell through one of the group's pieces sits on that
// face with a token that is not the group's code)
template <bool ZERO_SKIP, bool GROUPS = false>
__device__ __forceinline__ int trace_box(D3& S, const D3& E, int cur, const double4* rec4, int token, int& outSlot) {
    const D3 P0 = S;
    const D3 Pd = {E.x - P0.x, E.y - P0.y, E.z - P0.z};
    const double2* rd = reinterpret_cast<const double2*>(rec4);
    const double2 w01 = rd[0], w23 = rd[1], w45 = rd[2];
    const int4 nA = reinterpret_cast<const int4*>(rec4)[3];
    const int2 nB = reinterpret_cast<const int2*>(rec4)[8];
    const double f0 = w01.x - P0.x, f1 = w01.y + P0.x, f2 = w23.x - P0.y, f3 = w23.y + P0.y, f4 = w45.x - P0.z, f5 = w45.y + P0.z;
    int next = cur, best = -1;
    double dTmin = 2.0;
    // lanes the three-candidate form does not cover (see above); voted on once, after the candidates
#define CPF_BOX_ODD(F, NB) (ballot64(F > 0.0) & __builtin_amdgcn_uicmp((unsigned)NB, (unsigned)token, 33 /* ne */) & (GROUPS ? ballot64(!is_group(NB)) : ~0ull))
    const unsigned long long odd = CPF_BOX_ODD(f0, nA.x) | CPF_BOX_ODD(f1, nA.y) | CPF_BOX_ODD(f2, nA.z) | CPF_BOX_ODD(f3, nA.w) |
                                   CPF_BOX_ODD(f4, nB.x) | CPF_BOX_ODD(f5, nB.y) |
                                   ballot64(!(fabs(Pd.x) + fabs(Pd.y) + fabs(Pd.z) < __builtin_inf()));
#undef CPF_BOX_ODD
    bool tie = false;
#define CPF_BOX_AXIS(A, D, FD0, FD1, NB0, NB1)                                                                     \
    if (!ZERO_SKIP || ballot64(D != 0.0) != 0ull) {                                                                \
        const bool pos = D > 0.0;                                                                                  \
        const double fdt = pos ? FD1 : FD0;                                                                        \
        const int nbt = pos ? NB1 : NB0;                                                                           \
        const bool c1 = fabs(fdt) <= fabs(D), c3 = fdt < kTol, c4 = nbt != token;                                  \
        if ((ballot64(c1) & ballot64(c3) & __builtin_amdgcn_uicmp((unsigned)nbt, (unsigned)token, 33)) != 0ull) {  \
            if (c1 && c3 && c4) {                                                                                  \
                const double dT = fdt / -fabs(D);                                                                  \
                const bool ok = dT > kTol;                                                                         \
                tie |= ok && dT == dTmin;                                                                          \
                if (ok && dT < dTmin) { dTmin = dT; next = nbt; best = 2 * A + (pos ? 1 : 0); }                    \
            }                                                                                                      \
        }                                                                                                          \
    }
    CPF_BOX_AXIS(0, Pd.x, f0, f1, nA.x, nA.y)
    CPF_BOX_AXIS(1, Pd.y, f2, f3, nA.z, nA.w)
    CPF_BOX_AXIS(2, Pd.z, f4, f5, nB.x, nB.y)
#undef CPF_BOX_AXIS
    if ((odd | ballot64(tie)) != 0ull) {
        next = cur; best = -1; dTmin = 2.0;
        trace_box_slow<GROUPS>(P0, Pd, rec4, token, dTmin, next, best);
    }
    if (best >= 0) {
        S = axpy(dTmin, Pd, P0);
        outSlot = best;
    }
    return next;
}

// One cell of the walk in the reference's own form: traceIntet (query/ConvexQuery.cu:32-131) on the CSR slots [s0, s0 + nf) of a
// polyhedral cell.  Exit through the face slot with the smallest admissible dT in (tol, 1]; the slot we came in through
// (nbr == token) is skipped.  Returns the next cell (== cur: segment ends here; < 0: boundary code) and advances S to the exit
// point; outSlot is returned relative to s0.  A group code may come back as `next`: the caller resolves it (resolve_group), as
// after the six-slot tests.
// THE REFERENCE'S FORM -- divide, inf -> -1, token skip, group rule, accept -- is written out in this loop, in trace_in_cell
// below and in trace_box_slow above (there with the tie-break on original slot order).  One helper for the three was tried
// in several spellings: through it the staged kernels of cpf_kernels.hip (trace_in_cell), two LOOKUP 2 streaming kernels (this
// loop: more instructions) and four LOOKUP 11 ones (trace_box_slow: one more VGPR) compile to other code than before, and
// the generated code of the kernels is held fixed -- docs/experiments.md, "the walk's accept predicate".
__device__ __forceinline__ int trace_csr(D3& S, const D3& E, int cur, const double4* __restrict__ planes, const int32_t* __restrict__ nbr,
                                         int s0, int nf, int token, int& outSlot) {
    const D3 P0 = S;
    const D3 Pd = {E.x - P0.x, E.y - P0.y, E.z - P0.z};
    int next = cur, best = -1;
    double dTmin = 1.1;
    for (int s = 0; s < nf; ++s) {
        const double4 pl = planes[s0 + s];
        const int nb = nbr[s0 + s];
        const double fd = plane_dist(pl, P0), den = dot3(pl, Pd);    // (Cf - P0).n  (<= 0 inside)
        double dT = fd / den;
        if (__builtin_isinf(dT)) dT = -1.0;                          // segment parallel to the face
        if (nb == token) continue;
        if (is_group(nb) && !(den < 0.0)) continue;                  // face groups: outward crossings only (cpf_accept.h)
        if (fd < kTol && dT > kTol && dT <= 1.0 && dT < dTmin) { dTmin = dT; next = nb; best = s; }
    }
    if (best >= 0) {
        S = axpy(dTmin, Pd, P0);
        outSlot = best;
    }
    return next;
}
// trace_csr on cell `cur` of the CSR tables, with the group resolved, outSlot absolute and the exit point kept up to date
// inside the loop
__device__ __forceinline__ int trace_in_cell(D3& S, const D3& E, int cur, const MeshView& m, int token,
                                             int& outSlot) {
    const D3 P0 = S;
    const D3 Pd = {E.x - P0.x, E.y - P0.y, E.z - P0.z};
    int next = cur, best = -1;
    double dTmin = 1.1;
    const int s0 = m.cellOff[cur], s1 = m.cellOff[cur + 1];
    for (int s = s0; s < s1; ++s) {
        const double4 pl = m.planes[s];
        const double fd = plane_dist(pl, P0);           // (Cf - P0).n  (<= 0 inside)
        const double den = dot3(pl, Pd);
        double dT = fd / den;
        if (__builtin_isinf(dT)) dT = -1.0;             // segment parallel to the face
        const int nb = m.nbr[s];
        if (nb == token) continue;
        if (is_group(nb) && !(den < 0.0)) continue;     // face groups: outward crossings only (cpf_accept.h)
        if (fd < kTol && dT > kTol && dT <= 1.0 && dT < dTmin) {
            dTmin = dT;
            next = nb;
            S = axpy(dT, Pd, P0);
            best = s;
        }
    }
    if (best >= 0) {
        if (is_group(next)) next = resolve_group(next, S, m.cellOff, m.planes, m.groupOff, m.groupNbr);
        outSlot = best;
    }
    return next;
}

// ------------------------------------------------------------------------------------------------
// "VertexVelocity" advect mode (cuda/particles.cu:244-313, 428-437): the velocity at P is the barycentric interpolation of
// VERTEX velocities in a tet of the particle's cell -- the tet whose smallest barycentric weight of P is largest (the product
// tracks cells, and the interpolant is continuous across the tets of a cell), then weighed exactly like the reference
// (w_X = det(tet with X := P) * (1 / det(tet))).  Shared by the staged advect and the fused cycle: same bits.
//
// CONE LOCATE (round 6; VertexField::cone != nullptr).  Evaluating all tetsPerCell tets costs 12 x 5 determinants per particle
// and cycle: 7.8 x the cell-constant cycle on pitzDaily (BENCH: config.vertex_velocity).  When the cell's tets are a FAN about one
// apex -- the cell centre, src/initCuda.H:99-105 -- that covers every direction exactly once (checked on the host at
// cpf_set_tets: shared apex, determinants of one sign, solid angles adding up to 4 pi, bounded condition), the tets' interiors
// are disjoint.  So if ONE tet holds P with every weight above a margin far beyond the determinants' rounding errors, every
// other tet of the cell has a negative weight in exact arithmetic -- a computed minimum of at most a rounding error -- and the
// arg-max of the full evaluation is that tet: its weights, computed with the very same expressions, ARE the full evaluation's
// result, bit for bit.  The candidate comes from a cheap approximate test (P - apex in the tet's cone: three dot products with
// precomputed rows, 9 FMAs per tet); how good that guess is affects only the speed.  A particle within the margin of a tet's
// face, edge or the apex, or outside its cell by a rounding, takes the full evaluation as before.
// cone: one 256-byte RECORD per tet, everything the cone locate needs of it behind one address -- [0..8] the rows of the
// inverse of [B-A C-A D-A] (approximate: the guess), [9] 1 / det4(A, B, C, D) (exact, computed by the same expressions on the
// device), [10..18] B, C, D, [19..30] the velocities of A, B, C, D (rewritten by cpf_set_vertex_velocity), [31] spare; apex: the
// cells' shared vertex A, one double4 per cell.  A particle's advect is two dependent fetches -- the rows of its cell's tets,
// then the rest of ONE record -- where the index-chasing form (tet -> vertex ids -> positions -> velocities) was five.
struct VertexField { const double* pos; const int32_t* tets; const double* vel; int tetsPerCell; const double* cone; const double4* apex; };
constexpr double kVertexMargin = 1e-8;          // on barycentric weights (O(1)); the host admits meshes whose weights carry errors < 1e-10
constexpr int kConeDoubles = 32;                // doubles per tet record (VertexField::cone)
__device__ __forceinline__ double det4(const D3& A, const D3& B, const D3& C, const D3& D) {
    const D3 a = {B.x - A.x, B.y - A.y, B.z - A.z}, b = {C.x - A.x, C.y - A.y, C.z - A.z}, d = {D.x - A.x, D.y - A.y, D.z - A.z};
    const D3 c = {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y};
    return d.x * c.x + d.y * c.y + d.z * c.z;
}
// ONE tet of the cone locate: the reference's weights of P in tet `t` (record f.cone[t], apex A) and, if every weight clears the
// margin, the interpolated velocity -- exactly what the evaluation of all tets returns then (see above)
__device__ __forceinline__ bool vertex_velocity_in_tet(const VertexField& f, const D3& Pp, const D3& A, int64_t t, D3& v) {
    const double2* R = reinterpret_cast<const double2*>(f.cone + kConeDoubles * t);
    const double2 q4 = R[4], q5 = R[5], q6 = R[6], q7 = R[7], q8 = R[8], q9 = R[9];
    const double2 q10 = R[10], q11 = R[11], q12 = R[12], q13 = R[13], q14 = R[14], q15 = R[15];
    const double inv = q4.y;                                                     // 1. / det4(A, B, C, D), computed on the device
    const D3 B = {q5.x, q5.y, q6.x}, C = {q6.y, q7.x, q7.y}, D = {q8.x, q8.y, q9.x};
    const double a = det4(Pp, B, C, D) * inv, b = det4(A, Pp, C, D) * inv;
    const double cc = det4(A, B, Pp, D) * inv, d = det4(A, B, C, Pp) * inv;
    if (!(fmin(fmin(a, b), fmin(cc, d)) > kVertexMargin)) return false;
    // P is well inside this tet: no other tet of the fan can win; its vertex velocities ride in the record
    const D3 vA = {q9.y, q10.x, q10.y}, vB = {q11.x, q11.y, q12.x}, vC = {q12.y, q13.x, q13.y}, vD = {q14.x, q14.y, q15.x};
    v = {((a * vA.x + b * vB.x) + cc * vC.x) + d * vD.x, ((a * vA.y + b * vB.y) + cc * vC.y) + d * vD.y,
         ((a * vA.z + b * vB.z) + cc * vC.z) + d * vD.z};
    return true;
}
__device__ __forceinline__ bool vertex_velocity(const VertexField& f, const D3& Pp, int c, D3& v) {
    auto ld = [](const double* a, int k) { return D3{a[3 * (int64_t)k], a[3 * (int64_t)k + 1], a[3 * (int64_t)k + 2]}; };
    int best = -1;
    double bestMin = 0.0, w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    if (f.cone != nullptr) {
        const int64_t t0 = (int64_t)c * f.tetsPerCell;
        int cand = 0;
        // the candidate: the tet in whose cone about the apex P lies best (per-lane reads of the records' first 72 bytes; the
        // streaming kernel stages them in LDS once per cell instead: cpf_stream.hip, cycle_begin)
        const double4 ap = f.apex[c];
        const D3 A = {ap.x, ap.y, ap.z};
        const D3 r = {Pp.x - A.x, Pp.y - A.y, Pp.z - A.z};
        double candMin = -1e300;
#pragma unroll 4
        for (int k = 0; k < f.tetsPerCell; ++k) {
            const double2* g = reinterpret_cast<const double2*>(f.cone + kConeDoubles * (t0 + k));
            const double2 g01 = g[0], g23 = g[1], g45 = g[2], g67 = g[3], g89 = g[4];
            const double cb = fma(g23.x, r.z, fma(g01.y, r.y, g01.x * r.x)), cc = fma(g45.y, r.z, fma(g45.x, r.y, g23.y * r.x));
            const double cd = fma(g89.x, r.z, fma(g67.y, r.y, g67.x * r.x));
            const double m = fmin(cb, fmin(cc, cd));
            if (m > candMin) { candMin = m; cand = k; }
        }
        if (vertex_velocity_in_tet(f, Pp, A, t0 + cand, v)) return true;
    }
    const bool full = best < 0;                                   // no cone tables, or the candidate is not clear of its tet's boundary
    for (int k = 0; full && k < f.tetsPerCell; ++k) {
        const int32_t* ix = f.tets + 4 * ((int64_t)c * f.tetsPerCell + k);
        const D3 A = ld(f.pos, ix[0]), B = ld(f.pos, ix[1]), C = ld(f.pos, ix[2]), D = ld(f.pos, ix[3]);
        const double den = det4(A, B, C, D);
        if (den == 0.0) continue;                                 // a bad tet (particles.cu:275-278) cannot hold P
        const double a = det4(Pp, B, C, D) * (1. / den), b = det4(A, Pp, C, D) * (1. / den);
        const double cc = det4(A, B, Pp, D) * (1. / den), d = det4(A, B, C, Pp) * (1. / den);
        const double m = fmin(fmin(a, b), fmin(cc, d));
        if (best < 0 || m > bestMin) { best = k; bestMin = m; w0 = a; w1 = b; w2 = cc; w3 = d; }
    }
    if (best < 0) return false;
    const int32_t* ix = f.tets + 4 * ((int64_t)c * f.tetsPerCell + best);
    const D3 vA = ld(f.vel, ix[0]), vB = ld(f.vel, ix[1]), vC = ld(f.vel, ix[2]), vD = ld(f.vel, ix[3]);
    v = {((w0 * vA.x + w1 * vB.x) + w2 * vC.x) + w3 * vD.x, ((w0 * vA.y + w1 * vB.y) + w2 * vC.y) + w3 * vD.y,
         ((w0 * vA.z + w1 * vB.z) + w2 * vC.z) + w3 * vD.z};
    return true;
}

// step-kernel variants (cpf_set_option "step_variant"); all give bit-identical results
enum { kVariantAuto = -1, kVariantGeneric = 0, kVariantFixed = 1, kVariantFixedScalar = 2, kVariantCoop = 3, kVariantStream = 4, kVariantAhead = 5 };

// Where a walk gets its mesh data from.  Every tracer runs the same arithmetic in the same order.
template <int VARIANT>
struct GlobalTracer {
    const MeshView& m;
    __device__ __forceinline__ int trace(D3& S, const D3& E, int cur, int token, int& outSlot) const {
        if (VARIANT == kVariantGeneric) return trace_in_cell(S, E, cur, m, token, outSlot);
        if (VARIANT == kVariantFixedScalar) {
            // particles are kept sorted by cell, so most waves sit in ONE cell for their first visit:
            // fetch that cell's planes once per wave through the scalar cache instead of 64 times
            const int ucur = __builtin_amdgcn_readfirstlane(cur);
            if (ballot64(cur != ucur) == 0ull)
                return trace_fixed<6, false>(S, E, cur, m.planes + 6 * (int64_t)ucur, m.nbr + 6 * (int64_t)ucur, token,
                                      outSlot, 6 * ucur);
        }
        return trace_fixed<6, false>(S, E, cur, m.planes + 6 * (int64_t)cur, m.nbr + 6 * (int64_t)cur, token, outSlot,
                              6 * cur);
    }
    __device__ __forceinline__ double4 velocity(int cur) const { return m.U[cur]; }
};

// philox4x32 (Philox4x32-R, R = CPF_PHILOX_ROUNDS = 7): cpf_philox.h, shared with the recycling kernels and the host
// Three N(0,1) deviates for (particle gid, step) from ONE Philox4x32-7 block (parity with the reference's cuRAND stream is
// statistical by contract, SURVEY.md 8c, so the arithmetic is free): Box-Muller evaluated with the fp32 hardware
// transcendentals (v_log_f32, v_sqrt_f32, v_sin_f32 / v_cos_f32, whose argument is in revolutions: no 2*pi, no range
// reduction) -- words 0,1 give two deviates (one log, one sqrt), words 2,3 the third.  The radius uniform uses ALL 32
// bits of its word, u = (w + 0.5) * 2^-32: log2 u = log2(mantissa) + (exponent - 32) of x = float(w) + 0.5, so the tail
// reaches sqrt(2 * 33 * ln 2) = 6.76 sigma (round 2's 23-bit uniforms stopped at 5.77) and the result keeps its relative
// precision near u = 1; the angle uniform is 23-bit, ((w >> 9) + 0.5) * 2^-23.  The fp64 version this replaces (two
// log, two sqrt, sincospi + cospi in double) was a third of the Brownian kernel's time and cost it its occupancy; the
// kick itself, disp += sigma * xi, stays an fp64 fma.  oracle/cellwalk.c (cw_normal3_words) states the same transform
// with libm; what still differs from curand_normal_double is listed there.
__device__ __forceinline__ float log2_radius_uniform(uint32_t w) {
    const float x = (float)w + 0.5f;
    return __builtin_amdgcn_logf(__builtin_amdgcn_frexp_mantf(x)) + (float)(__builtin_amdgcn_frexp_expf(x) - 32);
}
__device__ __forceinline__ D3 normal3(uint64_t gid, uint32_t step, uint32_t seed) {
#ifdef CPF_AB_NO_RNG       // A/B builds only (tools/build_ab.sh): what the kick costs besides its deviates
    return {0.3 + (double)(gid & 1), -0.2, 0.1 * (double)(step & 1)};
#endif
    uint32_t c[4] = {(uint32_t)gid, (uint32_t)(gid >> 32), step, 0u};
    philox4x32(c, seed, 0x43504631u);
    const float s = 1.0f / 8388608.0f;                                    // 2^-23
    const float u1 = ((float)(c[1] >> 9) + 0.5f) * s, u3 = ((float)(c[3] >> 9) + 0.5f) * s;
    const float k = -1.3862943611198906f;                                 // -2 ln 2: -2 ln u = k * log2 u
    const float r0 = __builtin_amdgcn_sqrtf(k * log2_radius_uniform(c[0]));
    const float r1 = __builtin_amdgcn_sqrtf(k * log2_radius_uniform(c[2]));
    return {(double)(r0 * __builtin_amdgcn_cosf(u1)), (double)(r0 * __builtin_amdgcn_sinf(u1)),
            (double)(r1 * __builtin_amdgcn_cosf(u3))};
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

struct StepStats { unsigned steps, hops, refl, lost; };

// block-level counter reduction: 4 global atomics per block, sharded over kCounterSlots slots
__device__ __forceinline__ void flush_stats(StepStats st, unsigned long long* __restrict__ counters, unsigned* sCnt) {
    if (counters == nullptr) return;             // statistics switched off (cpf_set_option "stats" 0)
    if (threadIdx.x < 4) sCnt[threadIdx.x] = 0;
    __syncthreads();
    st.steps = wave_sum(st.steps); st.hops = wave_sum(st.hops); st.refl = wave_sum(st.refl); st.lost = wave_sum(st.lost);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&sCnt[0], st.steps); atomicAdd(&sCnt[1], st.hops);
        atomicAdd(&sCnt[2], st.refl); atomicAdd(&sCnt[3], st.lost);
    }
    __syncthreads();
    if (threadIdx.x < 4 && sCnt[threadIdx.x])
        atomicAdd(&counters[(blockIdx.x & (kCounterSlots - 1)) * 4 + threadIdx.x], (unsigned long long)sCnt[threadIdx.x]);
}

}  // namespace cpf
