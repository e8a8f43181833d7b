// WHICH FACE A VISIT LEAVES THROUGH: the acceptance rule of the cell walk as pure arithmetic -- plain C++, no HIP builtins, so
// that the host compiler can build it too (tests/test_accept_predicate_host.py states the reference's rule in numpy and compares).
// The rule is traceIntet's (query/ConvexQuery.cu:32-131): with fd = (Cf - P0).n and den = (E - P0).n, dT = fd / den, an
// infinite dT replaced by -1 (:89), a face is ADMISSIBLE iff fd < tol and tol < dT <= 1, the face the particle came in
// through (neighbour == token) is skipped, the admissible face with the smallest dT wins and ties go to the lower slot (the
// callers' strict "<" in slot order).  face_accept is the pruned form of it that every LDS face test of the step kernels runs.
// In cpf_walk.h, trace_fixed and trace_box's three-candidate form are different predicates -- a sign-bit test, one face per
// axis -- and keep their own statements and exactness arguments; trace_in_cell, trace_csr and trace_box_slow state the rule in
// the reference's own form, division first, each in its loop (see trace_csr for why they do not share one helper).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define CPF_HD __host__ __device__ __attribute__((always_inline))
#else
#define CPF_HD
#endif

namespace cpf {

constexpr double kTol = 1e-13;     // query/ConvexQuery.cu:42

// FACE GROUPS (cpf_mesh.cpp): the coplanar faces of a cell -- the pieces of a face split by a 2:1 refinement next door --
// share ONE slot, whose neighbour code names the group.  Two additions to the reference's rule, only where a slot is a
// group (no reference semantics exist for such cells, src/initCuda.H:64: hexes only; stated independently in
// oracle/cellwalk.c):
//   1. OUTWARD CROSSINGS ONLY (den < 0).  A particle that came in through one piece sits on the group's plane, a rounding
//      error outside it (fd = +4e-16), moving inward: the reference's acceptance test takes that for an exit at
//      dT ~ 2e-13 > tol, and the token cannot skip the slot (it names the piece's cell, not the group).  A convex cell
//      is left against the face's inward normal, so den < 0 loses no real exit.  Applied by face_accept below (c2) and by the reference-form loops.
//   2. the cell entered is chosen at the exit point X: the piece whose CELL holds X best (cpf_walk.h, resolve_group).
CPF_HD inline bool is_group(int nb) { return nb < -(1 << 30); }

// The pruned form: the division is only executed for a face that can still be accepted, and the running minimum is part of
// the test.  The pre-filter is EXACT, not approximate:
//   c1  with fd and den of equal sign, fl(fd/den) <= 1  <=>  |fd| <= |den| (1 is representable and rounding is monotone;
//       |fd| > |den| gives a quotient >= 1 + 2^-52); den == 0 / NaN fall out of this and every later comparison exactly like
//       the isinf -> -1 substitution of ConvexQuery.cu:89;
//   c2  only prunes divisions (a face the lane moves away from): "den < 0 or fd >= 0" holds whenever the exact condition
//       "equal sign bits" can still lead to an accepted face, and whatever else slips through -- zeros, opposite signs -- has a
//       quotient <= 0 or NaN and fails dT > tol below, exactly as in the reference.  GROUPS: a face-group slot is only left
//       with den < 0 (rule 1 above), which takes the "fd >= 0" alternative away from it;
//   c3, c4  the reference's fd < tol and its entry-face skip.
// dTmin starts above 1 (candidates have dT <= 1), so dT < dTmin is also the reference's dT <= 1 for the first face accepted.
template <bool GROUPS>
CPF_HD inline void face_accept(double den, double fd, int bs, int token, int s, double& dTmin, int& next, int& best) {
    // (c2 in "|" and "&", not "||" and "&&": three compares and two mask operations, whatever GROUPS is -- the short-circuit form
    // leaves the compiler a branch per operand to fold, and whether it does depends on what else it sees around the call)
    const bool c1 = fabs(fd) <= fabs(den), c2 = (den < 0.0) | ((fd >= 0.0) & !(GROUPS && is_group(bs)));
    const bool c3 = fd < kTol, c4 = bs != token;
    if (c1 && c2 && c3 && c4) {
        const double dT = fd / den;
        if (dT > kTol && dT < dTmin) { dTmin = dT; next = bs; best = s; }
    }
}

// THE CHAIN FORM (GROUPS == false only): what the hand-written face block of the flat walk's body without z executes
// (cpf_walk.h, face_accept_flat_asm), stated in plain C++ so that the host can compare it with face_accept<false> above
// (tests/test_flat_face_predicate_host.py).  Three conditions narrow the set of lanes one after the other: c4, c3, and in place
// of c1 and c2 ONE comparison of the two bit patterns as unsigned 64-bit integers,
//   c12  bits(fd) <= bits(den).
// The order of IEEE doubles of one sign is the order of their magnitudes' bit patterns, and a set sign bit is the integer's top
// bit.  So, for fd not a NaN (c3 has seen to that):
//   * equal sign bits: c12 <=> |fd| <= |den| = c1, for finite and infinite den alike (a NaN den has the largest patterns of its
//     sign: c12 holds, c1 does not -- and the quotient is NaN);
//   * fd negative, den positive: the top bit decides, c12 fails.  Nothing is lost: the quotient is negative, zero or NaN;
//   * fd positive (or +0), den negative (or -0): c12 HOLDS whatever the magnitudes -- the one case that c1 and c2 prune and c12
//     lets through to the division.  Its quotient is negative, a zero or NaN as well.
// What is accepted is the same: a lane is accepted only with dT = fl(fd / den) > tol > 0, and an IEEE quotient is positive only
// if neither operand is a NaN or a zero and the sign bits are EQUAL (the sign of a quotient is the exclusive-or of its operands'
// signs, exactly, whatever it rounds to).  So dT > tol implies equal signs on non-zero operands -- where c12 is c1, and where c2
// holds (both negative: den < 0; both positive: fd > 0) -- and every lane on which c12 and (c1 and c2) differ has unequal signs, a
// zero or a NaN among its operands and fails dT > tol either way.  dTmin, next and best change for the same lanes, to the same
// values.  (Which lanes reach the division for nothing: a particle on or outside a plane, 0 <= fd < tol, moving further out --
// the face it came in through, which c4 has skipped, or a start a rounding error outside its cell.)
CPF_HD inline bool bits_le(double a, double b) {
    unsigned long long ia, ib;
    __builtin_memcpy(&ia, &a, 8);
    __builtin_memcpy(&ib, &b, 8);
    return ia <= ib;
}
CPF_HD inline void face_accept_chain(double den, double fd, int bs, int token, int s, double& dTmin, int& next, int& best) {
    if (!(bs != token)) return;                        // c4
    if (!(fd < kTol)) return;                          // c3
    if (!bits_le(fd, den)) return;                     // c12
    const double dT = fd / den;
    if (!(dT > kTol)) return;
    if (!(dT < dTmin)) return;
    dTmin = dT; next = bs; best = s;
}

}  // namespace cpf
