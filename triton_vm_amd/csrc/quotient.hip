// quotient.hip -- the AIR quotient above the AIR kernels (air.hip): tvm_all_quotients_combined / _coefficients and, piecewise for a
// multi-GPU host, tvm_air_class_cosets / tvm_air_class_values / tvm_coset_values_to_coefficients.  Which route a call takes, and where
// valid-trace mode evaluates each class of constraints, is decided in quotient_plan.h (with the degree bounds); this unit walks that plan.
#include "kernels.h"
#include "quotient_plan.h"

using namespace tvm;
static_assert(QUOTIENT_ROW_BLOCK == TVM_RB, "quotient_plan.h counts in the row blocks of context.h");

namespace tvm {
// coeffs[i * N + t] (+)= sum_j w[4 i + j] * q_j[t]  (i, j < n <= 4; t < N; XFE vectors q_j, base-field weights): the polynomial
// sum_i X^(iN) A_i from its restrictions Q_j = sum_i c_j^i A_i to n cosets (w = the inverse Vandermonde matrix); added to coeffs, or
// (accumulate = 0) stored -- the first summand of an array that is then never cleared
struct CosetCombineWeights {
    u64 w[16];
};
struct CosetCombinePointers {
    const u64* q[4];
};
__global__ void k_coset_combine(CosetCombinePointers p, int n, u64 N, CosetCombineWeights m, u64* __restrict__ coeffs, int accumulate) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    xfe v[4];
    for (int j = 0; j < n; j++) v[j] = xfe_make(p.q[j][3 * t], p.q[j][3 * t + 1], p.q[j][3 * t + 2]);
    for (int i = 0; i < n; i++) {
        u64* o = coeffs + 3 * ((u64)i * N + t);
        xfe acc = accumulate ? xfe_make(o[0], o[1], o[2]) : xfe_zero();
        for (int j = 0; j < n; j++) acc = xfe_add(acc, xfe_mul_bfe(v[j], m.w[4 * i + j]));
        o[0] = acc.c0, o[1] = acc.c1, o[2] = acc.c2;
    }
}
// The same for n = 3, added to coeffs: coeffs[i + N * r] += sum_k w[3 * r + k] * q[k][i].  The whole-coset route's three-coset class keeps
// it -- 7 us a launch against 10 us for k_coset_combine on the 65 536 elements of a 2^16-row trace (profiles/quotient_unit_bench_ab.txt):
// the general kernel holds its vectors in an array indexed by n (112 B of scratch per lane).
struct ThreeCosetWeights {
    u64 w[9];
};
__global__ void k_three_coset_combine(const u64* __restrict__ q0, const u64* __restrict__ q1, const u64* __restrict__ q2, u64 n,
                                      ThreeCosetWeights m, u64* __restrict__ coeffs) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const xfe a = xfe_make(q0[3 * i], q0[3 * i + 1], q0[3 * i + 2]), b = xfe_make(q1[3 * i], q1[3 * i + 1], q1[3 * i + 2]),
              c = xfe_make(q2[3 * i], q2[3 * i + 1], q2[3 * i + 2]);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const xfe v = xfe_add(xfe_add(xfe_mul_bfe(a, m.w[3 * r]), xfe_mul_bfe(b, m.w[3 * r + 1])), xfe_mul_bfe(c, m.w[3 * r + 2]));
        u64* p = coeffs + 3 * (i + n * r);
        p[0] = bfe_add(p[0], v.c0);
        p[1] = bfe_add(p[1], v.c1);
        p[2] = bfe_add(p[2], v.c2);
    }
}
// The inverse of the n x n Vandermonde matrix of cs[0 .. n-1] (n <= 4) into w (w[4 i + j], zero elsewhere): row i holds the coefficients
// of x^i in the Lagrange basis polynomials L_j(x) = prod_{l != j} (x - c_l) / (c_j - c_l).  false if two of the c_j are equal.
static bool coset_combine_weights(const u64* cs, uint32_t n, CosetCombineWeights& w) {
    for (int i = 0; i < 16; i++) w.w[i] = 0;
    for (uint32_t j = 0; j < n; j++) {
        u64 poly[4] = {TVM_ONE, 0, 0, 0};   // running product prod (x - c_l), low coefficient first
        u64 denom = TVM_ONE;
        int deg = 0;
        for (uint32_t l = 0; l < n; l++) {
            if (l == j) continue;
            if (cs[l] == cs[j]) return false;
            for (int e = deg + 1; e >= 1; e--) poly[e] = bfe_sub(poly[e - 1], bfe_mul(poly[e], cs[l]));
            poly[0] = bfe_neg(bfe_mul(poly[0], cs[l]));
            deg++;
            denom = bfe_mul(denom, bfe_sub(cs[j], cs[l]));
        }
        const u64 dinv = bfe_inv(denom);
        for (uint32_t i = 0; i < n; i++) w.w[4 * i + j] = bfe_mul(poly[i], dinv);
    }
    return true;
}
// The remainder set (remainder_coset_coefficients): partial[g][i] = sum_{r < R} d^(gR + r) sum_j lambda_j q_j[i + (gR + r) M]
// for g < G, i < M -- the polynomial sum_j lambda_j q_j of G R M coefficients modulo X^M - d, as G partial sums (k_remainder_scatter
// adds them up)
struct RemainderFold {
    const u64* q[4];
    u64 lambda[4];
    int n;
};
__global__ void k_remainder_fold(RemainderFold f, u64 M, u64 G, u64 R, u64 d, u64* __restrict__ partial) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G * M) return;
    const u64 i = e % M, g = e / M;
    u64 s = bfe_pow(d, g * R);
    xfe acc = xfe_zero();
    for (u64 r = 0; r < R; r++) {
        const u64 row = 3 * (i + (g * R + r) * M);
        xfe v = xfe_zero();
        for (int j = 0; j < f.n; j++) v = xfe_add(v, xfe_mul_bfe(xfe_make(f.q[j][row], f.q[j][row + 1], f.q[j][row + 2]), f.lambda[j]));
        acc = xfe_add(acc, xfe_mul_bfe(v, s));
        s = bfe_mul(s, d);
    }
    partial[3 * e] = acc.c0, partial[3 * e + 1] = acc.c1, partial[3 * e + 2] = acc.c2;
}
// b = p[i] - sum_g partial[g][i] (the interpolant of q - R on the remainder set, i < M);  coeffs[i + k N] += v[k] * b, k < n_v
struct RemainderScatter {
    u64 v[5];
    int n_v;
};
__global__ void k_remainder_scatter(const u64* __restrict__ p, const u64* __restrict__ partial, u64 G, u64 M, u64 N, RemainderScatter w,
                                    u64* __restrict__ coeffs) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    xfe b = xfe_make(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
    for (u64 g = 0; g < G; g++) {
        const u64* x = partial + 3 * (g * M + i);
        b = xfe_sub(b, xfe_make(x[0], x[1], x[2]));
    }
    for (int k = 0; k < w.n_v; k++) {
        u64* o = coeffs + 3 * (i + (u64)k * N);
        const xfe r = xfe_add(xfe_make(o[0], o[1], o[2]), xfe_mul_bfe(b, w.v[k]));
        o[0] = r.c0, o[1] = r.c1, o[2] = r.c2;
    }
}
// Coset k of a pair of tables made by tvm_lde_table over one domain, as tables of their own: the layout is coset-major (context.h), so
// the coset's rows -- its successor block included -- are the storage rows from k * pitch on, whole row blocks when pitch % TVM_RB == 0.
struct TableCoset {
    const u64 *main, *aux;
    TabLayout layout;   // X = 1
};
static TableCoset table_coset(const tvm_table* mt, const tvm_table* at, u64 k) {
    const u64 first_row = k * mt->layout.pitch;
    TableCoset t{mt->data + tvm_tab_idx(first_row, 0, (u64)mt->W), at->data + tvm_tab_idx(first_row, 0, (u64)at->W), mt->layout};
    t.layout.X = 1;
    t.layout.log_x = 0;
    return t;
}
// A step's classes coset by coset (the cosets of the quotient domain ARE those of the tables: the plan asks for X == layout.X):
// P = sum_i X^(iN) A_i with A_i of degree < N.  On the coset gamma_j <w_N>, X^N is the constant c_j = gamma_j^N, so the interpolant of
// P's values there is Q_j = sum_i c_j^i A_i.  vals: [N] XFE, the values on one coset at a time; q: [n_cosets][N] XFE, the Q_j;
// -> the c_j, the Q_j and the inverse Vandermonde matrix of the c_j for k_coset_combine.
struct CosetInterpolants {
    u64 cs[4];
    CosetCombinePointers ptrs;
    CosetCombineWeights w;
};
static int class_on_cosets(tvm_ctx* c, const tvm_table* mt, const tvm_table* at, tvm_domain td, tvm_domain qd, const QuotientStep& step,
                           const u64* d_ch, const u64* d_w, u64* vals, u64* q, CosetInterpolants& on) {
    const u64 N = td.length, g_n = bfe_pow(qd.generator, qd.length / N);
    for (uint32_t j = 0; j < 4; j++) on.ptrs.q[j] = nullptr;
    for (uint32_t j = 0; j < step.n_cosets; j++) {
        const u64 k = step.cosets[j];
        const tvm_domain dom = {bfe_mul(qd.offset, bfe_pow(qd.generator, k)), g_n, N};
        const TableCoset t = table_coset(mt, at, k);
        on.cs[j] = bfe_pow(dom.offset, N);
        TVM_TRY(all_quotients_combined(c, t.main, t.layout, (u64)mt->W, t.aux, (u64)at->W, N, td.generator, dom.offset, dom.generator, N, d_ch,
                                       d_w, vals, (int)step.class_mask, 0));
        TVM_TRY(tvm_interpolate(c, 3, vals, dom, q + 3 * N * j));
        on.ptrs.q[j] = q + 3 * N * j;
    }
    if (!coset_combine_weights(on.cs, step.n_cosets, on.w)) return set_error(c, TVM_ERR_INVALID_ARGUMENT, "quotients: two cosets with the same X^N");
    return TVM_OK;
}
// The remainder route: one coset fewer per class.  A class's quotient q has fewer than nN + s coefficients, s <= M = n1 (the rows of one
// block of the tables).  With S the n cosets gamma_k <w_N> (X^N = c_k there) and V(X) = prod_{k in S} (X^N - c_k),
//   q = R + V B,  deg R < nN,  deg B < s:
// R is the interpolant of q's values on S -- n N-point interpolations Q_k, combined by the inverse Vandermonde matrix of the c_k
// (k_coset_combine, as tvm_coset_values_to_coefficients).  B comes from q on ONE BLOCK T of another coset: its n1 storage rows are the
// points tau w_M^i, i < M (tau = gamma_T w_N^0, w_M = w_N^n2, a coset of the order-M subgroup) and their successors are the next block
// (context.h), so the AIR evaluates them like a coset of their own (air_quotients_on_block).  On T, X^N is the constant c'' = gamma_T^N
// and V the constant beta = prod (c'' - c_k); R restricted to gamma_T <w_N> is sum_k L_k(c'') Q_k (L_k the Lagrange basis in the c_k),
// which modulo X^M - tau^M is the interpolant of R on T (k_remainder_fold).  So B = (interpolant of q on T - that fold) / beta, and V B
// adds v_i / beta times it at the coefficients i N + (0 .. M-1) (k_remainder_scatter).  On a valid trace B's coefficients s .. M-1 are zero.
// With class 0 among the plan's steps (the caller wants COEFFICIENTS) this is half the rows of the row-by-row evaluation on the quotient
// domain, and no codeword of 8N points on the way.
// coeffs: [plan.n_coeffs] XFE -- 4N (classes 1, 3, 2), or 4N + M with class 0; every element is written
static int remainder_coset_coefficients(tvm_ctx* c, const tvm_table* mt, const tvm_table* at, tvm_domain td, tvm_domain qd, const u64* d_ch,
                                        const u64* d_w, const QuotientPlan& plan, u64* coeffs) {
    const u64 N = td.length, M = mt->layout.n1, n2 = mt->layout.n2;
    const u64 G = n2 < 64 ? n2 : 64, R = n2 / G;   // the fold: G partial sums of R chunks of M coefficients
    const u64 n_q = plan.steps[0].n_cosets;        // (the first step has the most cosets)
    PoolBlock block(c, (size_t)3 * (N + n_q * N + 2 * M + G * M) * sizeof(u64));   // released on every exit path
    u64* vals = (u64*)block.p;     // [N] XFE: a class on one coset
    if (!vals) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "quotient scratch");
    u64* q = vals + 3 * N;         // [n_q][N] XFE: its interpolants Q_k
    u64* q_t = q + 3 * n_q * N;    // [M] XFE: a class on T, then ...
    u64* p_t = q_t + 3 * M;        // ... its interpolant there
    u64* partial = p_t + 3 * M;    // [G][M] XFE
    const u64 g_m = bfe_pow(bfe_pow(qd.generator, qd.length / N), n2);
    for (int s = 0; s < plan.n_steps; s++) {
        const QuotientStep& step = plan.steps[s];
        const uint32_t n = step.n_cosets;
        const u64 gamma_t = bfe_mul(qd.offset, bfe_pow(qd.generator, step.t_coset)), c_t = bfe_pow(gamma_t, N), d_t = bfe_pow(gamma_t, M);
        CosetInterpolants on;
        TVM_TRY(class_on_cosets(c, mt, at, td, qd, step, d_ch, d_w, vals, q, on));
        // (+)= R: the first class stores its n blocks and the rest of the array is cleared -- no pass over all of it beforehand
        TVM_LAUNCH(k_coset_combine, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, on.ptrs, (int)n, N, on.w, coeffs, s ? 1 : 0);
        if (!s) TVM_HIP_CHECK(c, hipMemsetAsync(coeffs + 3 * n * N, 0, (size_t)3 * (plan.n_coeffs - n * N) * sizeof(u64), c->stream));
        // R on T, modulo X^M - tau^M: the Lagrange weights L_j(c'') = sum_i c''^i w[4 i + j]
        RemainderFold f;
        f.n = (int)n;
        for (uint32_t j = 0; j < 4; j++) f.q[j] = on.ptrs.q[j], f.lambda[j] = 0;
        for (uint32_t j = 0; j < n; j++) {
            u64 ci = TVM_ONE;
            for (uint32_t i = 0; i < n; i++, ci = bfe_mul(ci, c_t)) f.lambda[j] = bfe_add(f.lambda[j], bfe_mul(ci, on.w.w[4 * i + j]));
        }
        TVM_LAUNCH(k_remainder_fold, dim3((unsigned)((G * M + 255) / 256)), dim3(256), 0, c->stream, f, M, G, R, d_t, partial);
        // q on T, its interpolant there
        const TableCoset t = table_coset(mt, at, step.t_coset);
        TVM_TRY(air_quotients_on_block(c, t.main, (u64)mt->W, t.aux, (u64)at->W, M, N, td.generator, gamma_t, g_m, d_ch, d_w, q_t, (int)step.class_mask));
        TVM_TRY(tvm_interpolate(c, 3, q_t, tvm_domain{gamma_t, g_m, M}, p_t));
        // V = prod (Y - c_k) in Y = X^N, its coefficients divided by beta = V(c'')
        RemainderScatter v;
        v.n_v = (int)n + 1;
        u64 beta = TVM_ONE;
        for (int i = 0; i < 5; i++) v.v[i] = 0;
        v.v[0] = TVM_ONE;
        for (uint32_t j = 0; j < n; j++) {
            for (int e = (int)j + 1; e >= 1; e--) v.v[e] = bfe_sub(v.v[e - 1], bfe_mul(v.v[e], on.cs[j]));
            v.v[0] = bfe_neg(bfe_mul(v.v[0], on.cs[j]));
            beta = bfe_mul(beta, bfe_sub(c_t, on.cs[j]));
        }
        const u64 beta_inv = bfe_inv(beta);
        for (int i = 0; i < v.n_v; i++) v.v[i] = bfe_mul(v.v[i], beta_inv);
        TVM_LAUNCH(k_remainder_scatter, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->stream, p_t, partial, G, M, N, v, coeffs);
        TVM_HIP_CHECK(c, hipGetLastError());
    }
    return TVM_OK;
}
// The codeword of a class-wise route: the coefficients of the classes' sum, evaluated on the quotient domain, class 0 added row by row.
// Whole cosets: the sub-domain steps evaluate their classes in ONE launch on every stride-th point of the quotient domain (the half class
// on the half domain -- it comes first, and its interpolant is the sum the others are added to -- the quarter class on the quarter
// domain); the three-coset class goes coset by coset (k_three_coset_combine).
static int quotients_by_class(tvm_ctx* c, const tvm_table* mt, const tvm_table* at, tvm_domain td, tvm_domain qd, const u64* d_ch,
                              const u64* d_w, const QuotientPlan& plan, u64* d_out) {
    const u64 N = td.length;
    const bool remainder = plan.route == QuotientRoute::remainder_coset;
    u64 n_xfe = 0;   // the coefficients; whole cosets: per step its values (one coset's at a time), then their interpolants
    if (remainder) n_xfe = plan.n_coeffs;
    for (int s = 0; s < plan.n_steps && !remainder; s++) n_xfe += ((plan.steps[s].stride ? plan.steps[s].n_cosets : 1) + plan.steps[s].n_cosets) * N;
    PoolBlock block(c, (size_t)3 * n_xfe * sizeof(u64));   // released on every exit path
    u64 *next = (u64*)block.p, *coeffs = remainder ? next : nullptr;
    if (!next) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "quotient scratch");
    if (remainder) TVM_TRY(remainder_coset_coefficients(c, mt, at, td, qd, d_ch, d_w, plan, coeffs));
    for (int s = 0; s < plan.n_steps && !remainder; s++) {   // whole cosets
        const QuotientStep& step = plan.steps[s];
        const u64 len = step.n_cosets * N;
        u64* vals = next;
        u64* q = vals + 3 * (step.stride ? len : N);
        next = q + 3 * len;
        if (step.stride) {
            const tvm_domain dom = {qd.offset, bfe_pow(qd.generator, step.stride), len};
            TVM_TRY(all_quotients_combined(c, mt->data, mt->layout, (u64)mt->W, at->data, (u64)at->W, N, td.generator, dom.offset, dom.generator,
                                           len, d_ch, d_w, vals, (int)step.class_mask, 0));
            TVM_TRY(tvm_interpolate(c, 3, vals, dom, q));
            if (!coeffs) coeffs = q;
            else TVM_TRY(tvm_xfe_add_assign(c, coeffs, q, len));
        } else {
            CosetInterpolants on;
            TVM_TRY(class_on_cosets(c, mt, at, td, qd, step, d_ch, d_w, vals, q, on));
            ThreeCosetWeights w3;   // (the plan's one step of this kind is the three-coset class)
            for (int r = 0; r < 3; r++)
                for (int k = 0; k < 3; k++) w3.w[3 * r + k] = on.w.w[4 * r + k];
            TVM_LAUNCH(k_three_coset_combine, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, on.ptrs.q[0], on.ptrs.q[1], on.ptrs.q[2],
                       N, w3, coeffs);
            TVM_HIP_CHECK(c, hipGetLastError());
        }
    }
    TVM_TRY(tvm_evaluate(c, 3, coeffs, plan.n_coeffs, qd, d_out));
    return all_quotients_combined(c, mt->data, mt->layout, (u64)mt->W, at->data, (u64)at->W, N, td.generator, qd.offset, qd.generator, qd.length,
                                  d_ch, d_w, d_out, TVM_AIR_CLASS_FULL, 1);
}
}  // namespace tvm
// what tvm_all_quotients_combined and tvm_all_quotients_coefficients share: the checks of their arguments, the shape their plan is made
// for, and the staging of the challenges and weights (once per call, before the first AIR launch: context.h, the scratch-slot rule)
static int quotient_arguments(tvm_ctx* c, const tvm_table* mt, const tvm_table* at, tvm_domain td, tvm_domain qd, const uint64_t* h_challenges,
                              const uint64_t* h_weights, const uint64_t* d_out) {
    if (!c || !mt || !at || !h_challenges || !h_weights || !d_out || !valid_domain(td) || !valid_domain(qd))
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "all_quotients_combined arguments");
    if (mt->fk != 1 || mt->n_cols != TVM_NUM_MAIN_COLUMNS || at->fk != 3 || at->n_cols != TVM_NUM_AUX_COLUMNS ||
        mt->rows != at->rows || qd.length > mt->rows || !mt->has_successor_blocks || !at->has_successor_blocks ||
        mt->layout.X != at->layout.X || mt->layout.n1 != at->layout.n1 || mt->layout.n2 != at->layout.n2 || mt->layout.pitch != at->layout.pitch)
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "all_quotients_combined: tables must be 379 BFE / 91 XFE columns wide, made by tvm_lde_table over one domain");
    return TVM_OK;
}
static u64 larger_interpolant(const tvm_table* mt, const tvm_table* at) {   // 0: one of the two is not known
    if (!mt->interpolant_len || !at->interpolant_len) return 0;
    return mt->interpolant_len > at->interpolant_len ? mt->interpolant_len : at->interpolant_len;
}
static QuotientShape quotient_shape(const tvm_ctx* c, const tvm_table* mt, const tvm_table* at, tvm_domain td, tvm_domain qd) {
    const TabLayout& l = mt->layout;   // (quotient_arguments: the two tables have one layout)
    return {td.length, qd.length, larger_interpolant(mt, at), l.n1, l.n2, l.pitch, l.X, mt->rows, c->air_valid_trace, air_parts_fork(c, qd.length),
            c->air_remainder_coset, c->air_remainder_min_rows};
}
// `staged`: the two arrays are host arrays and go through the slot; else they are device arrays and are used where they lie
static int stage_quotient_inputs(tvm_ctx* c, const uint64_t* challenges, const uint64_t* weights, bool staged, const u64** d_ch, const u64** d_w) {
    *d_ch = challenges;
    *d_w = weights;
    if (!staged) return TVM_OK;
    u64* slot = (u64*)scratch(c, Scratch::QuotientInputs, (size_t)3 * (TVM_NUM_CHALLENGES + TVM_NUM_QUOTIENT_WEIGHTS) * sizeof(u64));
    if (!slot) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "challenge staging");
    TVM_TRY(h2d_small(c, slot, challenges, 3 * TVM_NUM_CHALLENGES * sizeof(u64)));
    TVM_TRY(h2d_small(c, slot + 3 * TVM_NUM_CHALLENGES, weights, 3 * TVM_NUM_QUOTIENT_WEIGHTS * sizeof(u64)));
    *d_ch = slot;
    *d_w = slot + 3 * TVM_NUM_CHALLENGES;
    return TVM_OK;
}
// the bodies of the two entry points and of their _device_args twins
static int quotients_combined(tvm_ctx* c, const tvm_table* mt, const tvm_table* at, tvm_domain td, tvm_domain qd, const uint64_t* challenges,
                              const uint64_t* weights, bool staged, uint64_t* d_out) {
    TVM_TRY(quotient_arguments(c, mt, at, td, qd, challenges, weights, d_out));
    const u64 *d_ch = nullptr, *d_w = nullptr;
    TVM_TRY(stage_quotient_inputs(c, challenges, weights, staged, &d_ch, &d_w));
    const QuotientPlan plan = quotient_plan(quotient_shape(c, mt, at, td, qd));
    if (plan.route == QuotientRoute::row_by_row)
        return all_quotients_combined(c, mt->data, mt->layout, (u64)mt->W, at->data, (u64)at->W, td.length, td.generator, qd.offset,
                                      qd.generator, qd.length, d_ch, d_w, d_out);
    return quotients_by_class(c, mt, at, td, qd, d_ch, d_w, plan, d_out);
}
static int quotients_coefficients(tvm_ctx* c, const tvm_table* mt, const tvm_table* at, tvm_domain td, tvm_domain qd, const uint64_t* challenges,
                                  const uint64_t* weights, bool staged, uint64_t* d_coeffs, uint64_t capacity, uint64_t* n_coeffs) {
    if (!n_coeffs) return set_error(c, TVM_ERR_INVALID_ARGUMENT, "all_quotients_coefficients arguments");
    *n_coeffs = 0;
    TVM_TRY(quotient_arguments(c, mt, at, td, qd, challenges, weights, d_coeffs));
    const QuotientPlan plan = quotient_plan(quotient_shape(c, mt, at, td, qd), true);
    if (plan.route != QuotientRoute::remainder_coset) return TVM_NOT_APPLICABLE;
    if (capacity < plan.n_coeffs) return set_error(c, TVM_ERR_INVALID_ARGUMENT, "all_quotients_coefficients: capacity below 4 N + n1 elements");
    const u64 *d_ch = nullptr, *d_w = nullptr;
    TVM_TRY(stage_quotient_inputs(c, challenges, weights, staged, &d_ch, &d_w));
    TVM_TRY(remainder_coset_coefficients(c, mt, at, td, qd, d_ch, d_w, plan, d_coeffs));
    *n_coeffs = plan.n_coeffs;
    return TVM_OK;
}
extern "C" {
int32_t tvm_all_quotients_combined(tvm_ctx* c, const tvm_table* mt, const tvm_table* at, tvm_domain td, tvm_domain qd,
                                   const uint64_t* h_challenges, const uint64_t* h_weights, uint64_t* d_out) {
    return quotients_combined(c, mt, at, td, qd, h_challenges, h_weights, true, d_out);
}
int32_t tvm_all_quotients_combined_device_args(tvm_ctx* c, const tvm_table* mt, const tvm_table* at, tvm_domain td, tvm_domain qd,
                                               const uint64_t* d_challenges, const uint64_t* d_weights, uint64_t* d_out) {
    return quotients_combined(c, mt, at, td, qd, d_challenges, d_weights, false, d_out);
}
// The combined quotient in COEFFICIENT form, for a prover that goes on to the segments (tvm_quotient_segments_from_coefficients): no
// codeword of the quotient domain is made and taken apart again.  Only on the remainder route; elsewhere the status is
// TVM_NOT_APPLICABLE, nothing is written and the caller takes tvm_all_quotients_combined.
int32_t tvm_all_quotients_coefficients(tvm_ctx* c, const tvm_table* mt, const tvm_table* at, tvm_domain td, tvm_domain qd,
                                       const uint64_t* h_challenges, const uint64_t* h_weights, uint64_t* d_coeffs, uint64_t capacity,
                                       uint64_t* n_coeffs) {
    return quotients_coefficients(c, mt, at, td, qd, h_challenges, h_weights, true, d_coeffs, capacity, n_coeffs);
}
int32_t tvm_all_quotients_coefficients_device_args(tvm_ctx* c, const tvm_table* mt, const tvm_table* at, tvm_domain td, tvm_domain qd,
                                                   const uint64_t* d_challenges, const uint64_t* d_weights, uint64_t* d_coeffs,
                                                   uint64_t capacity, uint64_t* n_coeffs) {
    return quotients_coefficients(c, mt, at, td, qd, d_challenges, d_weights, false, d_coeffs, capacity, n_coeffs);
}
// ---- the valid-trace AIR piecewise: what tvm_all_quotients_combined does in one call on one device, as the pieces a multi-GPU
// host distributes over its ranks (triton_vm_amd/host/sharded_host.cpp).  A class's quotient polynomial has fewer than n * N
// coefficients (n = tvm_air_class_cosets), so its values on ANY n cosets of the trace domain determine it.
int32_t tvm_air_class_cosets(const tvm_table* mt, const tvm_table* at, tvm_domain td, uint32_t out[4]) {
    if (!mt || !at || !out || !valid_domain(td)) return TVM_ERR_INVALID_ARGUMENT;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (const u64 m = larger_interpolant(mt, at)) air_class_cosets(m, td.length, out);
    return TVM_OK;
}

int32_t tvm_air_class_values(tvm_ctx* c, const tvm_table* mt, const tvm_table* at, tvm_domain td, tvm_domain table_dom, uint32_t coset,
                             uint32_t class_mask, const uint64_t* h_challenges, const uint64_t* h_weights, uint64_t* d_out) {
    if (!c || !mt || !at || !h_challenges || !h_weights || !d_out || !valid_domain(td) || !valid_domain(table_dom) || !class_mask || class_mask > 15)
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "air_class_values arguments");
    const u64 N = td.length;
    if (mt->fk != 1 || mt->n_cols != TVM_NUM_MAIN_COLUMNS || at->fk != 3 || at->n_cols != TVM_NUM_AUX_COLUMNS || mt->rows != at->rows ||
        mt->rows != table_dom.length || table_dom.length % N || coset >= table_dom.length / N || !mt->has_successor_blocks ||
        !at->has_successor_blocks || mt->layout.X != table_dom.length / N || at->layout.X != mt->layout.X || mt->layout.pitch != at->layout.pitch ||
        mt->layout.pitch % TVM_RB)
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "air_class_values: tables made by tvm_lde_table over table_domain, one coset of them");
    const u64 *d_ch = nullptr, *d_w = nullptr;
    TVM_TRY(stage_quotient_inputs(c, h_challenges, h_weights, true, &d_ch, &d_w));
    const u64 gamma = bfe_mul(table_dom.offset, bfe_pow(table_dom.generator, coset));
    const TableCoset t = table_coset(mt, at, coset);
    return all_quotients_combined(c, t.main, t.layout, (u64)mt->W, t.aux, (u64)at->W, N, td.generator, gamma,
                                  bfe_pow(table_dom.generator, table_dom.length / N), N, d_ch, d_w, d_out, (int)class_mask, 0);
}
// The n interpolations Q_j of class_on_cosets on values the caller has, on any n <= 4 cosets h_offsets[j] <w_N>, and the same combination.
int32_t tvm_coset_values_to_coefficients(tvm_ctx* c, tvm_domain td, uint32_t n_cosets, const uint64_t* h_offsets,
                                         const uint64_t* const* d_values, uint64_t* d_coeffs) {
    if (!c || !valid_domain(td) || !n_cosets || n_cosets > 4 || !h_offsets || !d_values || !d_coeffs)
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "coset_values_to_coefficients arguments");
    const u64 N = td.length;
    u64 cs[4];
    for (uint32_t j = 0; j < n_cosets; j++) cs[j] = bfe_pow(h_offsets[j], N);
    CosetCombineWeights w;
    if (!coset_combine_weights(cs, n_cosets, w))
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "coset_values_to_coefficients: two cosets with the same X^N");
    PoolBlock block(c, (size_t)n_cosets * 3 * N * sizeof(u64));
    u64* q = (u64*)block.p;
    if (!q) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "coset interpolants");
    CosetCombinePointers ptrs;
    for (uint32_t j = 0; j < 4; j++) ptrs.q[j] = nullptr;
    for (uint32_t j = 0; j < n_cosets; j++) {
        if (!d_values[j]) return set_error(c, TVM_ERR_INVALID_ARGUMENT, "coset_values_to_coefficients: null values");
        const tvm_domain dom = {h_offsets[j], td.generator, N};
        TVM_TRY(tvm_interpolate(c, 3, d_values[j], dom, q + (u64)j * 3 * N));
        ptrs.q[j] = q + (u64)j * 3 * N;
    }
    TVM_LAUNCH(k_coset_combine, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, ptrs, (int)n_cosets, N, w, d_coeffs, 1);
    TVM_HIP_CHECK(c, hipGetLastError());
    return TVM_OK;
}
}  // extern "C"
