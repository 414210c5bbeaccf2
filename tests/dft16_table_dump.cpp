// dft16_table_dump.cpp -- csrc/ntt_mfma_table.h expanded on the host (g++, nothing else of the project): for the root exponent
// given, the layout, the biases, the accumulator inputs and every non-zero byte of the 24 constant operands, one per line.
// tests/test_dft16_mfma.py rebuilds the 16 x 16 matrix of field elements from them.
#include <cstdio>
#include <cstdlib>

#include "ntt_mfma_table.h"

using namespace tvm;

static constexpr Dft16MfmaTable forward = dft16_make_mfma_table(156, dft16_layout_dit());
static constexpr Dft16MfmaTable inverse = dft16_make_mfma_table(36, dft16_layout_dit());

int main(int argc, char** argv) {
    const int root = argc > 1 ? std::atoi(argv[1]) : 156;
    if (root != 156 && root != 36) return 2;
    const Dft16MfmaTable& t = root == 156 ? forward : inverse;
    const Dft16Layout lay = dft16_layout_dit();
    const Dft16Bias bias = dft16_bias();
    for (int e = 0; e < 16; e++) std::printf("layout %d %d %d\n", e, lay.in_point[e], lay.out_point[e]);
    for (int d = 0; d < DFT16_MFMA_DIGITS; d++) std::printf("bias %d %d\n", d, bias.b[d]);
    for (int d = 0; d < DFT16_MFMA_DIGITS; d++)
        for (int i = 0; i < 16; i++) std::printf("c %d %d %d\n", d, i, t.c[d][i]);
    // a <digit> <half> <row i> <group g> <register t> <byte> <signed entry>
    for (int d = 0; d < DFT16_MFMA_DIGITS; d++)
        for (int h = 0; h < 2; h++)
            for (int lane = 0; lane < 64; lane++)
                for (int tt = 0; tt < 4; tt++)
                    for (int bb = 0; bb < 4; bb++) {
                        const int entry = (signed char)((t.a[d][h][lane][tt] >> (8 * bb)) & 0xFF);
                        if (entry) std::printf("a %d %d %d %d %d %d %d\n", d, h, lane % 16, lane / 16, tt, bb, entry);
                    }
    return 0;
}
