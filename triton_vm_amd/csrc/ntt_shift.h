// ntt_shift.h -- transforms of 2, 4, 8 and 16 points whose twiddles are powers of two.
//
// In F_p, p = 2^64 - 2^32 + 1, two is a 192nd root of unity (2^96 = -1), and the 2^k-th roots of unity the reference's
// domains are built from (BFieldElement::primitive_root_of_unity, twenty-first; the generator of every ArithmeticDomain,
// /root/reference/triton-vm/src/arithmetic_domain.rs:99-108) are powers of two up to order 64:
//     w_4 = 2^48,  w_8 = 2^120 = -2^24,  w_16 = 2^156 = -2^60,  w_32 = 2^78,  w_64 = 2^39.
// A multiplication by 2^s is a 96-bit shift and one folding step with the shape of p -- 9 to 12 VALU instructions against
// the 16 of a general Montgomery multiplication, on the Montgomery word directly ((a R) 2^s = (a 2^s) R) -- and the sign of
// 2^(96 + s) = -2^s is absorbed by exchanging the butterfly's addition and subtraction.  The lowest four layers of every
// decimation-in-time transform (the highest four of a decimation-in-frequency one) are 16-point transforms of this kind.
#pragma once
#include "field.h"

namespace tvm {

// x * 2^S mod p for ANY 64-bit word x, 0 <= S < 96, canonical result: every branch works on the limbs of x and ends in a
// canonicalising step, none needs x < p (S = 0 reduces x and nothing else; the butterflies do not call it for a twiddle of 1).
// With y = x << (S % 32) as three 32-bit limbs y2:y1:y0 and phi = 2^32 (phi^2 = phi - 1, phi^3 = -1):
//   S < 32:        y0 + y1 phi + y2 phi^2          = (y1:y0) + y2 (2^32 - 1)
//   32 <= S < 64:  y0 phi + y1 phi^2 + y2 phi^3    = (y0 + y1) 2^32 - (y1 + y2)
//   64 <= S < 96:  y0 phi^2 + y1 phi^3 + y2 phi^4  = y0 (2^32 - 1) - (y2:y1)
template <int S>
TVM_HD u64 bfe_mul_pow2(u64 x) {
    static_assert(S >= 0 && S < 96, "exponent out of range");
    constexpr int R = S % 32, Q = S / 32;
    if constexpr (S == 0) return bfe_canon(x);
    const u32 x0 = (u32)x, x1 = (u32)(x >> 32);
    const u32 y0 = x0 << R;
    const u32 y1 = R ? ((x1 << R) | (x0 >> (32 - R))) : x1;
    const u32 y2 = R ? (x1 >> (32 - R)) : 0u;
    if constexpr (Q == 0) {
        const u64 lo = ((u64)y1 << 32) | y0;
        u64 t = lo + (u64)y2 * TVM_EPS;       // y2 < 2^31: the product fits; the sum may wrap once
        if (t < lo) t += TVM_EPS;             // 2^64 = 2^32 - 1; no second wrap: t < 2^63 after the first
        return t >= TVM_P ? t - TVM_P : t;
    } else if constexpr (Q == 1) {
        const u64 h = (u64)y0 + y1;           // 33 bits
        const u64 a = (h << 32) + ((h >> 32) ? TVM_EPS : 0);   // (h mod 2^32) 2^32 + [carry] 2^64, canonical either way
        const u64 b = (u64)y1 + y2;           // < 2^33
        return bfe_sub(a, b);
    } else {
        const u64 a = (u64)y0 * TVM_EPS;      // <= (2^32 - 1)^2 < p
        const u64 b = ((u64)y2 << 32) | y1;   // < 2^63
        return bfe_sub(a, b);
    }
}

// bit reversal of a K-bit index, usable in constant expressions
TVM_HD constexpr int brev_k(int e, int k) {
    int r = 0;
    for (int i = 0; i < k; i++) r |= ((e >> i) & 1) << (k - 1 - i);
    return r;
}

// log2 of the primitive 2^K-th root of unity the domains use (K <= 4), forward and inverse
TVM_HD constexpr int pow2_root_log(int K, bool inverse) { return ((inverse ? 36 : 156) << (4 - K)) % 192; }
template <int K, bool INVERSE>
struct Pow2Root {
    static constexpr int value = pow2_root_log(K, INVERSE);
};
// log2 of the twiddle of the butterflies with index M in layer T of the 2^K-point transform at the points 2^SHIFT w^j (below)
TVM_HD constexpr int pow2_twiddle_log(int K, bool inverse, int T, int M, int shift) {
    return ((pow2_root_log(K, inverse) * M + shift % 192 + 192) * (((1 << K) / 2) >> T)) % 192;
}

// ---------------------------------------------------------------- lazy sums: the canonicality plan
// The LDE row kernels (ntt.hip) let words of a butterfly group leave the canonical range [0, p) where nothing reads them as
// canonical: a sum with ONE canonical operand is then bfe_add_folded (5 VALU instructions) instead of bfe_add (6 and a scalar
// one).  Which sums may be, for a given group, is decided here at compile time.  The facts (field.h, above):
//   (1) bfe_add(a, b): both canonical -> canonical.
//   (2) bfe_add_folded(a, b): one of them canonical, the other any 64-bit word -> a 64-bit representative of a + b.
//   (3) bfe_sub(a, b): b canonical, a any word -> a representative of a - b, canonical when a is.
//   (4) bfe_mul_pow2<S>(x), bfe_mul(x, w) with w < p: any word x -> canonical (x w < p 2^64 is all bfe_montyred asks).
// A decimation-in-time butterfly is (u, hi) -> (u + v, u - v) with v = 2^E hi, canonical by (4), or v = hi where the twiddle is
// 1; a decimation-in-frequency one is (u, v) -> (u + v, 2^E (u - v)), the difference v - u where the twiddle carries the sign.
// The SUBTRAHEND of every butterfly is therefore either canonical by construction or has to be, and with it the sum of the
// same butterfly always has its one canonical operand: a sum may be folded exactly when nobody needs its RESULT canonical.
// The plan walks the schedule of Ntt2kStep backwards from the outputs that are owed canonical and collects the needs:
//   * a sum whose result is needed is bfe_add, and needs both operands (1);
//   * a difference whose result is needed needs its minuend (3), unless a shift multiplication follows it (4);
//   * a subtrahend is needed unless it has just been multiplied by a power of two other than 1.
// What is left at the inputs is `need_in`; the caller states which inputs are canonical, and `ok` is the result of an
// independent forward walk that checks every precondition (1)-(3) with the chosen instructions and that every owed output
// comes out canonical.  ntt_pow2_points static_asserts it, so a caller cannot ask for a form whose words are not what the
// next reader expects.  Residues are never affected: every instruction above is exact mod p.
struct CanonPlan {
    unsigned fold[4];     // bit e of fold[T]: the sum of layer T's butterfly on elements (e, e + 2^T) is bfe_add_folded
    unsigned need_in;     // inputs that have to be canonical
    unsigned out_canon;   // outputs that are canonical when the inputs `in_canon` are
    int folded;           // number of folded sums (of K 2^(K-1))
    bool ok;              // every precondition holds and every owed output is canonical
};
TVM_HD constexpr CanonPlan canon_plan(int K, bool dit, bool inverse, int shift, unsigned in_canon, unsigned owed) {
    CanonPlan P = {{0, 0, 0, 0}, 0, 0, 0, true};
    const int R = 1 << K;
    unsigned need = owed & ((1u << R) - 1);
    for (int tt = K - 1; tt >= 0; tt--) {   // backwards: the last layer first
        const int T = dit ? tt : K - 1 - tt, h = 1 << T;
        for (int M = 0; M < h; M++)
            for (int q = 0; q < R / (2 * h); q++) {
                const int e = q * 2 * h + M, E = pow2_twiddle_log(K, inverse, T, M, shift);
                const bool tw = E % 96 != 0, neg = E >= 96;
                const bool n_lo = (need >> e) & 1, n_hi = (need >> (e + h)) & 1;
                bool need_u = false, need_v = false, fold = false;
                if (dit) {   // lo, hi = u + v, u - v (neg: exchanged), v = 2^E hi
                    const bool n_sum = neg ? n_hi : n_lo, n_diff = neg ? n_lo : n_hi;
                    fold = !n_sum;
                    need_u = n_sum || n_diff;
                    need_v = !tw;
                } else {     // lo = u + v, hi = 2^E (u - v) (neg: v - u)
                    fold = !n_lo;
                    const bool need_min = n_lo || (!tw && n_hi);
                    need_u = neg ? true : need_min;
                    need_v = neg ? need_min : true;
                }
                if (fold) P.fold[T] |= 1u << e, P.folded++;
                need = (need & ~((1u << e) | (1u << (e + h)))) | ((unsigned)need_u << e) | ((unsigned)need_v << (e + h));
            }
    }
    P.need_in = need;
    // forwards: the preconditions of the instructions chosen above, from what the caller says about the inputs
    unsigned c = in_canon & ((1u << R) - 1);
    for (int tt = 0; tt < K; tt++) {
        const int T = dit ? tt : K - 1 - tt, h = 1 << T;
        for (int M = 0; M < h; M++)
            for (int q = 0; q < R / (2 * h); q++) {
                const int e = q * 2 * h + M, E = pow2_twiddle_log(K, inverse, T, M, shift);
                const bool tw = E % 96 != 0, neg = E >= 96, fold = (P.fold[T] >> e) & 1;
                const bool cu = (c >> e) & 1, ch = (c >> (e + h)) & 1;
                bool c_lo = false, c_hi = false;
                if (dit) {
                    const bool cv = tw || ch;
                    if (!cv) P.ok = false;                          // (3) the subtrahend
                    if (fold ? !(cu || cv) : !(cu && cv)) P.ok = false;   // (2) / (1)
                    const bool c_sum = !fold, c_diff = cu;
                    c_lo = neg ? c_diff : c_sum, c_hi = neg ? c_sum : c_diff;
                } else {
                    const bool c_sub = neg ? cu : ch, c_min = neg ? ch : cu;
                    if (!c_sub) P.ok = false;
                    if (fold ? !(cu || ch) : !(cu && ch)) P.ok = false;
                    c_lo = !fold, c_hi = tw || c_min;
                }
                c = (c & ~((1u << e) | (1u << (e + h)))) | ((unsigned)c_lo << e) | ((unsigned)c_hi << (e + h));
            }
    }
    P.out_canon = c;
    if (owed & ((1u << R) - 1) & ~c) P.ok = false;
    return P;
}
// TVM_LDE_LAZY_SUMS 1: the LDE row kernels of 256 .. 1024 points take the lazy forms; 0: every word canonical, bfe_add everywhere.
// Measured, not adopted: a folded sum saves one VALU instruction, one scalar one and one pair of wait states --
// pass 2 issues 2.4 % fewer VALU instructions, passes 1 and 3 1.3 % -- and every launch shape of the three kernels is faster in
// the trace, but over whole proofs the slower runs with it overlap the faster ones without (profiles/lde_lazy_sums_*).
#ifndef TVM_LDE_LAZY_SUMS
#define TVM_LDE_LAZY_SUMS 0
#endif

// u + 2^E v and u - 2^E v for E mod 192 (the sign of E >= 96 exchanges the two); FOLD: the sum is bfe_add_folded
template <int E, bool FOLD = false>
TVM_HD void bfe_butterfly_pow2(u64& lo, u64& hi) {
    constexpr int EE = ((E % 192) + 192) % 192;
    const u64 u = lo;
    u64 v = hi;
    if constexpr (EE % 96 != 0) v = bfe_mul_pow2<EE % 96>(hi);
    if constexpr (EE < 96) {
        lo = FOLD ? bfe_add_folded(u, v) : bfe_add(u, v);
        hi = bfe_sub(u, v);
    } else {
        lo = bfe_sub(u, v);
        hi = FOLD ? bfe_add_folded(u, v) : bfe_add(u, v);
    }
}
// (u + v, (u - v) 2^E)
template <int E, bool FOLD = false>
TVM_HD void bfe_butterfly_dif_pow2(u64& lo, u64& hi) {
    constexpr int EE = ((E % 192) + 192) % 192;
    const u64 u = lo, v = hi;
    lo = FOLD ? bfe_add_folded(u, v) : bfe_add(u, v);
    const u64 d = EE < 96 ? bfe_sub(u, v) : bfe_sub(v, u);
    if constexpr (EE % 96 != 0) hi = bfe_mul_pow2<EE % 96>(d);
    else hi = d;
}

// In-register transform of 2^K points with the domain's 2^K-th root (INVERSE: its inverse), element e at x[e * STRIDE].
// DIT: bit-reversed order in, natural order out; DIF: natural order in, bit-reversed order out -- the conventions of
// lds_ntt_group (ntt.hip), of which these are the twiddle-free lowest / highest layers.
// SHIFT (decimation in time only): the transform at the points 2^SHIFT w^j instead of w^j, which is the plain transform of the
// inputs c_a 2^(SHIFT a), a = brev(e) the coefficient index at element e.  Layer T joins two transforms of h = 2^T points each
// in the variable y = x^(R / 2h); its twiddle at the shifted points is (2^SHIFT w^M')^(R / 2h) -- the plain twiddle times
// 2^(SHIFT (R/2 >> T)), still a power of two: the same instructions with other shift counts.
// OWED < 0: every word stays canonical (bfe_add in every butterfly).  OWED >= 0, the lazy form: the mask of outputs the caller
// is owed canonical, IN the mask of inputs it hands over canonical; the sums follow canon_plan.
template <int K, bool DIT, bool INVERSE, int SHIFT, int OWED, unsigned IN>
struct CanonPlanOf {
    static constexpr CanonPlan value = canon_plan(K, DIT, INVERSE, SHIFT, IN, OWED < 0 ? ~0u : (unsigned)OWED);
};
template <int K, bool DIT, bool INVERSE, int T, int M, int Qi, int SHIFT = 0, int OWED = -1, unsigned IN = ~0u>
struct Ntt2kStep {
    template <typename X>
    TVM_HD static void run(X& x) {
        constexpr int R = 1 << K, h = 1 << T;
        static_assert(SHIFT == 0 || DIT, "input shift: decimation in time only");
        if constexpr (Qi < R / (2 * h)) {
            constexpr int e = Qi * 2 * h + M;
            constexpr int E = pow2_twiddle_log(K, INVERSE, T, M, SHIFT);
            constexpr bool FOLD = OWED >= 0 && ((CanonPlanOf<K, DIT, INVERSE, SHIFT, OWED, IN>::value.fold[T] >> e) & 1);
            if constexpr (DIT) bfe_butterfly_pow2<E, FOLD>(x[e], x[e + h]);
            else bfe_butterfly_dif_pow2<E, FOLD>(x[e], x[e + h]);
            Ntt2kStep<K, DIT, INVERSE, T, M, Qi + 1, SHIFT, OWED, IN>::run(x);
        } else if constexpr (M + 1 < h) {
            Ntt2kStep<K, DIT, INVERSE, T, M + 1, 0, SHIFT, OWED, IN>::run(x);
        } else if constexpr (DIT ? (T + 1 < K) : (T > 0)) {
            Ntt2kStep<K, DIT, INVERSE, DIT ? T + 1 : T - 1, 0, 0, SHIFT, OWED, IN>::run(x);
        }
    }
};
template <int K, bool DIT, bool INVERSE, int OWED = -1, unsigned IN = ~0u>
TVM_HD void ntt_pow2_points(u64 (&x)[1 << K]) {
    static_assert(OWED < 0 || CanonPlanOf<K, DIT, INVERSE, 0, OWED, IN>::value.ok, "lazy sums: a precondition of the plan does not hold");
    if constexpr (K > 0) Ntt2kStep<K, DIT, INVERSE, DIT ? 0 : K - 1, 0, 0, 0, OWED, IN>::run(x);
}
// bit-reversed order in, natural order out: out[j] = sum_a x[brev(a)] (2^SHIFT w^j)^a, w the domains' 2^K-th root
template <int K, int SHIFT, int OWED = -1, unsigned IN = ~0u>
TVM_HD void ntt_pow2_points_shifted(u64 (&x)[1 << K]) {
    static_assert(OWED < 0 || CanonPlanOf<K, true, false, SHIFT, OWED, IN>::value.ok, "lazy sums: a precondition of the plan does not hold");
    if constexpr (K > 0) Ntt2kStep<K, true, false, 0, 0, 0, SHIFT, OWED, IN>::run(x);
}

}  // namespace tvm
