// ntt_mfma.h -- the 16-point transform with power-of-two twiddles (ntt_shift.h: ntt_pow2_points<4, ...>) on the matrix cores.
//
// The domains' 16th root of unity is 2^156 (its inverse 2^36), so every entry of the 16 x 16 transform matrix is
//     w^(jk) = 2^(12 m mod 192) = +-2^(8q + r),   q in 0 .. 11,  r in {0, 4},   the sign negative for exponents >= 96 (2^96 = -1),
// and the map is linear: it applies to Montgomery words as they are, and to ANY 64-bit representative of a residue.  With the
// inputs in bytes, x_k = sum_b 2^(8b) x_kb,
//     y_j = sum_{d = 0 .. 11} 2^(8d) D_jd,     D_jd = sum_k +-2^(r_jk) x_{k,b}  over the one b per k with b + q_jk = d (mod 12),
// the sign flipping once more where b + q_jk >= 12.  Each D_jd has at most 16 terms of magnitude <= 16 * 255: |D_jd| < 2^16.
//
// One transform is spread over FOUR lanes, sixteen transforms per wavefront -- the arrangement of the Tip5 MDS layer (tip5.h): lane
// l = (n = l % 16, g = l / 16) holds four points of transform n; the B operand of v_mfma_i32_16x16x64_i8 is "the low halves of the
// four words this lane holds", then "the high halves", as they lie in the registers; the byte shifts and signs are in the CONSTANT A
// operands, one per digit position d and half h (the wrap sign makes the operand of (d, high) differ from that of (d - 4, low), so
// there are 24 of them, 4 VGPRs each); lane (n, g) receives rows 4g .. 4g+3 of column n: all twelve digit sums of four outputs of its
// own transform.  No cross-lane instruction.  24 MFMAs per sixteen transforms.
// The i8 operands are signed: bytes travel as x - 128 (one XOR per 32-bit half), and the accumulator input of (d, row) carries the
// correction 128 * sum(entries of that row of the two operands of d) and a bias B_d >= 2^16 that keeps every sum positive.  The biases are
// chosen so that sum_d 2^(8d) B_d is a multiple of 2^96 + 1 = p (2^32 + 1): they vanish mod p and nothing has to be subtracted.
//
// MEASURED SLOWER than the shift form (tools/ubench/dft16_mfma.hip): the 24 matrix instructions alone take 84 % of the
// time of the 32 shift butterflies they would replace, and the recombination does not hide under them.  No kernel of the LDE uses
// this; tvm_dft16_selfcheck (capi.hip) and the microbenchmark do.
//
// Which point a lane holds in which register, and which output a row is, is the LAYOUT (Dft16Layout): the generator below takes it
// and the root's exponent (156 forward, 36 inverse) and makes the operands; one generator serves both directions.
#pragma once
#include "field.h"
#include "mfma_i8.h"
#include "ntt_mfma_table.h"   // the generator of the constant operands (plain C++)
#include "ntt_shift.h"

namespace tvm {

// Twelve digit sums T_d = D_d + B_d per word -> sum_d 2^(8d) T_d mod p, for the four words of a lane.
//   0 < T_d < 2^16 + 2^16 + 2^9 (|D_d| <= 16 * 16 * 255 = 65280 < 2^16 <= B_d <= 2^16 + 256), so the pairs E_k = T_2k + 2^8 T_(2k+1)
//   (< 2^26) are one v_lshl_add_u32 each, and P_i = E_2i + 2^16 E_(2i+1) (< 2^43) one v_mad_u64_u32 each by a 2^16 the compiler
//   cannot see through (tip5_mfma_recombine): the value is P_0 + phi P_1 + phi^2 P_2 with phi = 2^32, phi^2 = phi - 1, phi^3 = -1.
//   P_2 = l2 + phi h2 (h2 < 2^11):   phi^2 P_2 = phi l2 - (l2 + h2).
//   Q = P_1 + l2 = ql + phi qh (qh < 2^12):  phi Q = phi ql + EPS qh.
//   t = EPS qh + P_0 (< 2^45: one v_mad_u64_u32);  s = t + phi ql (carry k);  u = l2 + h2 (< 2^33);  the value is s + 2^64 k - u,
//   which is never negative as an integer (qh >= 1: EPS qh >= l2; qh = 0: ql = Q >= l2; and P_0 >= 2^8 T_1 > h2) and below
//   2^64 + 2^45:  r = s - u (borrow b), k' = k and not b.
//   CANONICAL tail: z = r + EPS;  result = (k' or z carries) ? z : r  -- k' set means r < 2^45, so r + EPS is the canonical value;
//   k' clear means the value is r < 2^64 and one subtraction of p (the addition of EPS modulo 2^64) makes it canonical exactly when
//   r >= p, i.e. when z carries.
//   FOLDED tail: result = k' ? r + EPS : r, some 64-bit representative -- for words that next meet bfe_mul (residue-correct on any
//   64-bit inputs: tip5.h) or another transform on the matrix cores (bytes of any representative), never bfe_add / bfe_sub or a store.
// Plain C++ on 32-bit halves (carries from 32-bit compares: the 64-bit compare forms run at a fraction of the rate).
template <bool CANONICAL>
TVM_D void dft16_mfma_recombine(const tvm_v4i (&T)[DFT16_MFMA_DIGITS], u64 (&x)[4]) {
    u32 w16 = 1u << 16;
#ifdef TVM_FIELD_ASM
    asm("" : "+s"(w16));
#endif
#pragma unroll
    for (int v = 0; v < 4; v++) {
        u32 e[6];
#pragma unroll
        for (int k = 0; k < 6; k++) e[k] = (u32)T[2 * k][v] + ((u32)T[2 * k + 1][v] << 8);
        const u64 p0 = (u64)e[1] * w16 + e[0], p1 = (u64)e[3] * w16 + e[2], p2 = (u64)e[5] * w16 + e[4];
        const u32 l2 = (u32)p2, h2 = (u32)(p2 >> 32);
        const u64 q = p1 + l2;
        const u64 t = (u64)(u32)(q >> 32) * 0xFFFFFFFFu + p0;
        const u32 tl = (u32)t, th = (u32)(t >> 32);
        const u32 sh = th + (u32)q;
        const bool k = sh < th;
        // r = (sh : tl) - (l2 + h2), as two 32-bit subtractions of l2 and of h2 with their borrows collected
        const u32 r0a = tl - l2;
        const u32 b0 = tl < l2;
        const u32 r0 = r0a - h2;
        const u32 b1 = r0a < h2;
        const u32 bb = b0 + b1;             // 0 .. 2
        const u32 rh = sh - bb;
        const bool brw = sh < bb;
        const bool kk = k != brw;           // k and not borrow (a borrow without k cannot happen: the value is not negative)
        if constexpr (CANONICAL) {
            const u32 z0 = r0 + 0xFFFFFFFFu;
            const u32 c0 = r0 != 0;         // r0 + (2^32 - 1) carries unless r0 == 0
            const u32 z1 = rh + c0;
            const bool c1 = z1 < c0;
            const bool take = kk | c1;
            x[v] = take ? (((u64)z1 << 32) | z0) : (((u64)rh << 32) | r0);
        } else {
            const u32 m = kk ? 0xFFFFFFFFu : 0u;
            const u32 z0 = r0 + m;
            const u32 c0 = z0 < m;
            x[v] = ((u64)(rh + c0) << 32) | z0;
        }
    }
}

// Where the constant operands come from.  Dft16OperandsAt: from a table in memory (LDS or constant memory), fetched digit by digit.
struct Dft16OperandsAt {
    const Dft16MfmaTable* t;
    int lane;
    TVM_D tvm_v4i a(int d, int h) const {
        const u32* p = t->a[d][h][lane];
        tvm_v4i r;
#pragma unroll
        for (int i = 0; i < 4; i++) r[i] = (int)p[i];
        return r;
    }
    TVM_D tvm_v4i c(int d) const {
        const int* p = t->c[d] + 4 * (lane >> 4);
        tvm_v4i r;
#pragma unroll
        for (int i = 0; i < 4; i++) r[i] = p[i];
        return r;
    }
};
// Dft16OperandsHeld: all 24 A operands resident in registers (96 VGPRs: for kernels at two wavefronts per SIMD); the accumulator
// inputs still come from the table.
struct Dft16OperandsHeld {
    tvm_v4i ops[DFT16_MFMA_DIGITS][2];
    const Dft16MfmaTable* t;
    int lane;
    TVM_D void load(const Dft16MfmaTable* table, int lane_) {
        t = table;
        lane = lane_;
        const Dft16OperandsAt at{table, lane_};
#pragma unroll
        for (int d = 0; d < DFT16_MFMA_DIGITS; d++) {
            ops[d][0] = at.a(d, 0);
            ops[d][1] = at.a(d, 1);
        }
    }
    TVM_D tvm_v4i a(int d, int h) const { return ops[d][h]; }
    TVM_D tvm_v4i c(int d) const { return Dft16OperandsAt{t, lane}.c(d); }
};

// The transform of the sixteen groups of a wavefront: x[t] = the point in_point[4g + t] of transform n on entry (any 64-bit
// representative), the output out_point[4g + t] on return (CANONICAL: canonical words; otherwise folded representatives).  Every lane
// of the wavefront must take part.
template <bool CANONICAL, class Operands>
TVM_D void dft16_mfma(u64 (&x)[4], const Operands& m) {
    const u32 pad = 0x80808080u;  // bytes travel lowered by 128
    tvm_v4i lo, hi;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        lo[t] = (int)((u32)x[t] ^ pad);
        hi[t] = (int)((u32)(x[t] >> 32) ^ pad);
    }
    tvm_v4i T[DFT16_MFMA_DIGITS];
#pragma unroll
    for (int d = 0; d < DFT16_MFMA_DIGITS; d++) T[d] = TVM_MFMA_I8(m.a(d, 0), lo, m.c(d));
#pragma unroll
    for (int d = 0; d < DFT16_MFMA_DIGITS; d++) T[d] = TVM_MFMA_I8(m.a(d, 1), hi, T[d]);
    dft16_mfma_recombine<CANONICAL>(T, x);
}

}  // namespace tvm
