// ntt_mfma_table.h -- the constant operands of the 16-point transform on the matrix cores (ntt_mfma.h), as a constexpr generator
// from the root's exponent and the lane layout.  Plain C++ (no device code, nothing else of the project): tests/dft16_table_dump.cpp
// expands it on the host.
#pragma once
#include <cstdint>

namespace tvm {

#define DFT16_MFMA_DIGITS 12
#define DFT16_MFMA_BIAS_LOG 16

// in_point[4g + t]: the (natural) index of the point lane (n, g) holds in x[t]; out_point[4g + v]: the (natural) index of the output
// lane (n, g) receives in x[v]
struct Dft16Layout {
    int in_point[16], out_point[16];
};
// decimation in time as ntt_pow2_points<4, true, .> has it: element e = 4g + t of the group is point brev(e), output e is output e
constexpr int dft16_brev4(int e) { return ((e & 1) << 3) | ((e & 2) << 1) | ((e & 4) >> 1) | ((e & 8) >> 3); }
constexpr Dft16Layout dft16_layout_dit() {
    Dft16Layout l{};
    for (int e = 0; e < 16; e++) {
        l.in_point[e] = dft16_brev4(e);
        l.out_point[e] = e;
    }
    return l;
}

// a[d][h][lane][t]: the A operand of digit position d against the low (h = 0) / high (h = 1) halves, register t of lane
// (i = lane % 16, g = lane / 16): row i, the four bytes of point in_point[4g + t].  c[d][r]: the accumulator input of row r.
struct Dft16MfmaTable {
    uint32_t a[DFT16_MFMA_DIGITS][2][64][4];
    int c[DFT16_MFMA_DIGITS][16];
};
struct Dft16Bias {
    int b[DFT16_MFMA_DIGITS];
};
// B_d = 2^16 + e_d with sum_d 2^(8d) B_d = m (2^96 + 1) for the smallest m that leaves every e_d >= 0: e_d < 256 for d < 11, e_11 <= 256
constexpr Dft16Bias dft16_bias() {
    typedef unsigned __int128 u128;
    u128 base = 0;
    for (int d = 0; d < DFT16_MFMA_DIGITS; d++) base += (u128)1 << (8 * d + DFT16_MFMA_BIAS_LOG);
    const u128 M = ((u128)1 << 96) + 1;
    const u128 delta = (base + M - 1) / M * M - base;   // < 2^96 + 1
    Dft16Bias r{};
    for (int d = 0; d < DFT16_MFMA_DIGITS; d++)
        r.b[d] = (1 << DFT16_MFMA_BIAS_LOG) + (int)(d < DFT16_MFMA_DIGITS - 1 ? (delta >> (8 * d)) & 0xFF : delta >> (8 * d));
    return r;
}
constexpr Dft16MfmaTable dft16_make_mfma_table(int root_exponent, Dft16Layout lay) {
    Dft16MfmaTable t{};
    int row_sum[DFT16_MFMA_DIGITS][16] = {};
    for (int i = 0; i < 16; i++)
        for (int g = 0; g < 4; g++)
            for (int tt = 0; tt < 4; tt++) {
                const int j = lay.out_point[i], k = lay.in_point[4 * g + tt];
                const int E = (root_exponent * j * k) % 192;
                const bool neg = E >= 96;
                const int q = (E % 96) / 8, r = (E % 96) % 8;   // r is 0 or 4: E is a multiple of 12
                for (int b = 0; b < 8; b++) {
                    const int pos = b + q, d = pos % DFT16_MFMA_DIGITS;
                    const int coef = (neg != (pos >= DFT16_MFMA_DIGITS)) ? -(1 << r) : (1 << r);
                    t.a[d][b / 4][16 * g + i][tt] |= (uint32_t)(coef & 0xFF) << (8 * (b % 4));
                    row_sum[d][i] += coef;
                }
            }
    const Dft16Bias bias = dft16_bias();
    for (int d = 0; d < DFT16_MFMA_DIGITS; d++)
        for (int i = 0; i < 16; i++) t.c[d][i] = 128 * row_sum[d][i] + bias.b[d];   // every product was taken with the byte lowered by 128
    return t;
}

}  // namespace tvm
