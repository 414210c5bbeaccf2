// mfma_i8.h -- v_mfma_i32_16x16x64_i8 as tip5.h (the MDS layer) and ntt_mfma.h (the 16-point transforms with power-of-two
// twiddles) use it, and the model of it that the CPU emulation runs.
#pragma once
#include "platform.h"

#ifdef TVM_EMU
struct tvm_v4i {
    int v[4];
    int& operator[](int i) { return v[i]; }
    const int& operator[](int i) const { return v[i]; }
};
// v_mfma_i32_16x16x64_i8 as its users rely on it: lane (i = l % 16, q = l / 16) supplies 16 signed bytes of row i
// of A and of column i of B for the same sixteen k-indices (which sixteen is irrelevant to a sum over k), and
// receives D[4q + v][i] = C + sum_k A[4q + v][k] B[k][i] in element v.  The GPU parity tests of tvm_hash_rows
// (tests/test_kernels_hash.py) and of tvm_dft16_selfcheck (tests/test_dft16_mfma.py) run the same kernels on the hardware: they
// fail if it differs from this model.
static inline tvm_v4i emu_mfma_i32_16x16x64_i8(tvm_v4i a, tvm_v4i b, tvm_v4i c) {
    struct { tvm_v4i a, b; } mine = {a, b}, all[64];
    emu_wave_gather(&mine, sizeof(mine), all);
    const int lane = emu::lane_id(), col = lane & 15, q = lane >> 4;
    tvm_v4i d = c;
    for (int v = 0; v < 4; v++)
        for (int kq = 0; kq < 4; kq++) {
            const signed char* pa = (const signed char*)&all[16 * kq + 4 * q + v].a;
            const signed char* pb = (const signed char*)&all[16 * kq + col].b;
            for (int k = 0; k < 16; k++) d[v] += (int)pa[k] * (int)pb[k];
        }
    return d;
}
#define TVM_MFMA_I8(a, b, c) emu_mfma_i32_16x16x64_i8((a), (b), (c))
#else
typedef int tvm_v4i __attribute__((ext_vector_type(4)));
#define TVM_MFMA_I8(a, b, c) __builtin_amdgcn_mfma_i32_16x16x64_i8((a), (b), (c), 0, 0, 0)
#endif
