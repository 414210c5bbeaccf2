// quotient_plan.h -- which route the AIR quotient takes (quotient.hip) and, in valid-trace mode, on which points each class of
// constraints is evaluated: a pure function of the shape and the options.  Plain C++17 (no HIP, no context): quotient.hip walks the
// plan, tests/quotient_plan_dump.cpp prints it.  This file is the one place that knows the degree bounds.
#pragma once
#include <cstdint>

#include "triton_hip.h"   // TVM_AIR_CLASS_*

namespace tvm {
// ---- the bound ---------------------------------------------------------------------------------------------------------------------
// Valid-trace mode (TVM_OPTION_AIR_VALID_TRACE; off by default).  Every column is a polynomial with at most m = interpolant_len
// coefficients (trace length N + trace randomizers h), and the AIR is degree-lowered to 4, so a constraint of degree d in the columns
// is a polynomial of degree <= d (m - 1).  The consistency and transition quotients divide by X^N - 1 (the transition one times
// X - w^-1): at most d (m - 1) + 2 - N coefficients.  An initial / terminal quotient (zerofier of degree 1) of a constraint of degree
// d' has fewer than d' (m - 1) + 1.  The constraints are generated in four classes by these lengths (air_gen.h: TVM_AIR_PART_CLASS);
// class d holds the consistency / transition constraints of degree d with the initial / terminal ones of degree d - 1:
//   TVM_AIR_CLASS_HALF     d = 4  (parts 1-5, 87 % of the work)   about 3N + 4h coefficients
//   TVM_AIR_CLASS_THREE    d = 3  (parts 6, 7)                     about 2N + 3h
//   TVM_AIR_CLASS_QUARTER  d = 2  (parts 8, 9, a quarter of the multiplications)   about N + 2h
//   TVM_AIR_CLASS_FULL     the FOUR initial / terminal quotients of degree 4: d' = 4 alone, about 4N + 4h
// A class whose quotient has at most `whole` N + `extra` coefficients is determined by its values on `whole` cosets of the trace
// domain (N points each) plus `extra` more points.  On a VALID trace -- the constraints vanish on the trace domain, so the quotients
// ARE polynomials -- evaluating on those points, interpolating and evaluating on the quotient domain gives exactly the field
// elements of the row-by-row evaluation, at a fraction of the cost; on an invalid trace the row-by-row values are those of a rational
// function and differ (either way the unmodified verifier rejects: it recomputes the quotient at the out-of-domain point).
inline bool boundary_quotient_fits(std::uint64_t d, std::uint64_t m, std::uint64_t N, std::uint64_t whole, std::uint64_t extra) {
    return d * (m - 1) + 1 <= whole * N + extra;
}
inline bool fits(std::uint64_t d, std::uint64_t m, std::uint64_t N, std::uint64_t whole, std::uint64_t extra) {
    return d * (m - 1) + 2 <= (whole + 1) * N + extra && boundary_quotient_fits(d - 1, m, N, whole, extra);
}

// tvm_air_class_cosets: how many cosets of the trace domain determine each class (out[bit of the class]; 0: the bound does not hold)
inline void air_class_cosets(std::uint64_t m, std::uint64_t N, std::uint32_t out[4]) {
    out[0] = 0;   // (needed on every point)
    out[1] = fits(4, m, N, 4, 0) ? 4 : 0;
    out[2] = fits(2, m, N, 2, 0) ? 2 : 0;
    out[3] = fits(3, m, N, 3, 0) ? 3 : 0;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------
constexpr std::uint64_t QUOTIENT_ROW_BLOCK = 16;   // context.h: TVM_RB (quotient.hip asserts that they agree)
struct QuotientShape {
    std::uint64_t N, Q;                    // the lengths of the trace domain and of the quotient domain
    std::uint64_t m;                       // the larger interpolant length of the two tables; 0: one of them is not known
    std::uint64_t n1, n2, pitch, X, rows;  // the tables' layout (context.h: TabLayout) and the length of the domain they are defined over
    bool valid_trace;                      // TVM_OPTION_AIR_VALID_TRACE
    bool parts_fork;                       // air.hip: air_parts_fork(Q) -- the quotient domain is short enough for the parts to run side by side
    bool remainder_option;                 // TVM_OPTION_AIR_REMAINDER_COSET
    std::uint64_t remainder_min_rows;      // TVM_OPTION_AIR_REMAINDER_MIN_ROWS (a context starts with 2^18)
};
enum class QuotientRoute {
    row_by_row,       // every constraint on every point of the quotient domain
    whole_cosets,     // each class on the whole cosets that determine it, ONE evaluation of their sum on the quotient domain, class 0 added row by row
    remainder_coset,  // the same with one coset fewer per class, plus one block T of another coset (quotient.hip: remainder_coset_coefficients)
};
// One evaluation step of a class-wise route.
struct QuotientStep {
    std::uint32_t class_mask;   // TVM_AIR_CLASS_*: the classes evaluated together
    std::uint32_t stride;       // != 0: ONE launch on the sub-domain of every stride-th point of the quotient domain; 0: coset by coset
    std::uint32_t n_cosets;     // the cosets of the trace domain the step evaluates on; stride == 0: cosets[0 .. n_cosets) of the quotient domain
    std::uint32_t cosets[4];
    std::uint32_t t_coset;      // remainder route: T = block 0 (n1 rows) of this coset
};
struct QuotientPlan {
    QuotientRoute route = QuotientRoute::row_by_row;
    int n_steps = 0;
    QuotientStep steps[4] = {};
    std::uint64_t n_coeffs = 0;   // class-wise routes: the coefficients of the classes' sum -- Q / 2 (whole cosets), 4N, or 4N + n1 with class 0
};
// `with_class_0`: the caller wants COEFFICIENTS (tvm_all_quotients_coefficients), class 0 among them -- possible on the remainder route
// only, where class 0 goes the way of the others (the cosets 0, 2, 4, 6 and T in coset 1: the even cosets are used up, the tables hold
// all eight); the codeword routes add class 0 row by row after their one evaluation on the quotient domain.
inline QuotientPlan quotient_plan(const QuotientShape& s, bool with_class_0 = false) {
    QuotientPlan p;
    const std::uint64_t N = s.N, m = s.m, half = s.Q / 2, quarter = s.Q / 4, M = s.n1;
    // The half class on the half domain and the quarter class on the quarter domain, both a whole number (>= 2) of cosets that the tables
    // hold; a quotient domain short enough for the parts to fork is evaluated row by row (kernels.h: air_parts_fork).  (The half-domain
    // conditions imply the quarter-domain ones for N >= 4: from 4(m - 1) + 2 <= half + N and m >= N follows half >= 4N, hence quarter >= 2N,
    // 2(m - 1) + 2 <= quarter + N and m <= quarter -- tests/test_quotient_plan.py sweeps it.  A class-wise route always has its quarter class.)
    const bool split = s.valid_trace && !s.parts_fork && m && half >= 2 * N && half % N == 0 && quarter >= 2 * N && quarter % N == 0 &&
                       fits(4, m, N, half / N, 0) && fits(2, m, N, quarter / N, 0) && s.rows % half == 0;
    if (!split) return p;
    // The three-coset class: cosets 0, 2, 4 of a quotient domain of 8N points, each ONE coset of the tables, in whole row blocks.
    const bool three = half == 4 * N && fits(3, m, N, 3, 0) && s.X == 2 * (half / N) && s.pitch % QUOTIENT_ROW_BLOCK == 0;
    // One coset fewer per class, plus the block T: when every class's quotient has at most M = n1 coefficients beyond its whole
    // blocks of N -- and the trace is long enough that the dropped cosets (about 1.9 ms of AIR work at 2^18 rows, a quarter of that
    // at 2^16) outweigh the latency of the three short evaluations on T (about 0.1 ms each, whatever N).
    const bool remainder = three && s.remainder_option && N >= s.remainder_min_rows && M % QUOTIENT_ROW_BLOCK == 0 &&
                           boundary_quotient_fits(4, m, N, 4, M) &&   // class 0 (the coefficient form only)
                           fits(4, m, N, 3, M) && fits(3, m, N, 2, M) && fits(2, m, N, 1, M);
    if (remainder) {
        p.route = QuotientRoute::remainder_coset;
        p.n_coeffs = with_class_0 ? 4 * N + M : 4 * N;
        if (with_class_0) p.steps[p.n_steps++] = {TVM_AIR_CLASS_FULL, 0, 4, {0, 2, 4, 6}, 1};
        p.steps[p.n_steps++] = {TVM_AIR_CLASS_HALF, 0, 3, {0, 2, 4}, 6};
        p.steps[p.n_steps++] = {TVM_AIR_CLASS_THREE, 0, 2, {0, 2}, 6};
        p.steps[p.n_steps++] = {TVM_AIR_CLASS_QUARTER, 0, 1, {0}, 6};
        return p;
    }
    p.route = QuotientRoute::whole_cosets;
    p.n_coeffs = half;
    p.steps[p.n_steps++] = {(std::uint32_t)(TVM_AIR_CLASS_HALF | (three ? 0 : TVM_AIR_CLASS_THREE)), 2, (std::uint32_t)(half / N), {}, 0};
    p.steps[p.n_steps++] = {TVM_AIR_CLASS_QUARTER, 4, (std::uint32_t)(quarter / N), {}, 0};
    if (three) p.steps[p.n_steps++] = {TVM_AIR_CLASS_THREE, 0, 3, {0, 2, 4}, 0};
    return p;
}
}  // namespace tvm
