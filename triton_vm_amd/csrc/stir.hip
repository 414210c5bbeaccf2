// stir.hip -- the device side of the STIR prover (/root/reference/triton-vm/src/low_degree_test/stir.rs:885-993).
//
// Per round the reference (all on the CPU, polynomial arithmetic from twenty-first):
//   StirMerkleTree::new      stack 4 codeword entries taken at distance n/4 into one leaf, hash_varlen, Merkle tree
//                            (stir.rs:1380-1419)                                          -> tvm_stir_merkle_tree
//   fold_polynomial          chunks of 4 coefficients evaluated at the folding randomness (stir.rs:1132-1147)
//                                                                                         -> tvm_fold_polynomial
//   next_round_domain.evaluate, out-of-domain evaluations                                 -> tvm_evaluate, tvm_evaluate_at_points
//   quotient = (folded - Ans) / Zerofier,  next = quotient * (sum_i r^i X^i)   (stir.rs:945-966, Polynomial
//   interpolate / zerofier / division / multiplication: O(n k) on the CPU)                -> tvm_stir_next_polynomial
// The last step never forms Zerofier or the product as polynomials: on a coset that avoids the quotient set it
// evaluates folded, Ans, Zerofier (as a product of linear factors) and the degree-correction series pointwise,
// divides and multiplies pointwise and interpolates once.  The division is exact (folded - Ans vanishes on the
// quotient set) and deg(next) = deg(folded) < |coset|, so the interpolant IS the reference's polynomial.
#include "kernels.h"
#include "stir_kernels.h"
#include "tip5.h"

namespace tvm {

// leaf i = Tip5::hash_varlen(cw[i], cw[i + d], ..., cw[i + (sh-1) d]) with d = n / sh, XFEs flattened c0,c1,c2: the matrix-core
// form of the permutation (tip5.h), four lanes per leaf, sixteen leaves per wavefront, as the table rows are hashed
// (hash.hip: k_hash_rows_mfma).  Lane (n, g) absorbs the words g, g + 4 (and g + 8 for g < 2) of each block of ten.
__global__ void __launch_bounds__(256, 6) k_hash_stacked(const u64* __restrict__ cw, u64 d, int stack_height,
                                                         u64* __restrict__ digests) {
    __shared__ unsigned char lut[256];
    __shared__ int ctab[TIP5_ROUNDS * TIP5_MFMA_POSITIONS * 16];
    const int tid = threadIdx.x;
    for (int i = tid; i < TIP5_ROUNDS * TIP5_MFMA_POSITIONS * 16; i += blockDim.x) ctab[i] = d_tip5_mfma_table.v[i];
    tip5_stage_lut_lowered(lut, tid, blockDim.x);
    const int lane = tid & 63, n = lane & 15, g = lane >> 4;
    u64 i = ((u64)blockIdx.x * 4 + (tid >> 6)) * 16 + n;
    const bool live = i < d;  // every lane of a wavefront takes part in the matrix instructions
    if (!live) i = d - 1;
    const Tip5MfmaOperands a = tip5_mfma_matrix_operands(lane);
    const int W = 3 * stack_height;
    u64 st[4] = {0, 0, 0, 0};
    const int n_perms = W / TIP5_RATE + 1;
    for (int perm = 0; perm < n_perms; perm++) {
#pragma unroll
        for (int t3 = 0; t3 < 3; t3++) {
            const int q = g + 4 * t3;  // word of the state, overwritten if it is in the rate part
            const int wi = perm * TIP5_RATE + q;
            if (q < TIP5_RATE) st[t3] = wi < W ? cw[(i + (u64)(wi / 3) * d) * 3 + wi % 3] : (wi == W ? TVM_ONE : 0);  // padding: 1, 0s
        }
        tip5_permute_mfma(st, a, g, lut, ctab);
    }
    if (live) {
        digests[i * 5 + g] = st[0];
        if (g == 0) digests[i * 5 + 4] = st[1];
    }
}

// the bodies: stir_kernels.h (shared with the device-argument forms of stir_rounds.hip)
__global__ void k_fold_polynomial(const u64* __restrict__ poly, u64 n, int ff, u64 r0, u64 r1, u64 r2, u64 n_out,
                                  u64* __restrict__ out) {
    fold_polynomial_item(poly, n, ff, xfe_make(r0, r1, r2), n_out, out);
}
__global__ void __launch_bounds__(256) k_stir_quotient(StirQuotientArgs a) { stir_quotient_item(a); }
__global__ void __launch_bounds__(256) k_xfe_interpolate(const u64* __restrict__ points, const u64* __restrict__ values, int k,
                                                         u64* __restrict__ out, int* __restrict__ status) {
    xfe_interpolate_workgroup(points, values, k, out, status);
}
int xfe_interpolate(tvm_ctx* c, const u64* d_points, const u64* d_values, int k, u64* d_out, int* d_status) {
    TVM_LAUNCH(k_xfe_interpolate, dim3(1), dim3(256), 0, c->stream, d_points, d_values, k, d_out, d_status);
    TVM_HIP_CHECK(c, hipGetLastError());
    return TVM_OK;
}

int stir_hash_stacked(tvm_ctx* c, const u64* cw, u64 n, int stack_height, u64* digests) {
    const u64 d = n / (u64)stack_height;
    TVM_LAUNCH(k_hash_stacked, dim3((unsigned)((d + 63) / 64)), dim3(256), 0, c->stream, cw, d, stack_height, digests);
    TVM_HIP_CHECK(c, hipGetLastError());
    return TVM_OK;
}
int stir_fold_polynomial(tvm_ctx* c, const u64* poly, u64 n, int ff, const u64* h_r, u64* out) {
    const u64 n_out = (n + ff - 1) / ff;
    if (!n_out) return TVM_OK;
    TVM_LAUNCH(k_fold_polynomial, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, c->stream, poly, n, ff, h_r[0], h_r[1],
               h_r[2], n_out, out);
    TVM_HIP_CHECK(c, hipGetLastError());
    return TVM_OK;
}
int stir_quotient(tvm_ctx* c, u64* vals, u64 n, u64 offset, u64 gen, const u64* d_points, const u64* d_answer,
                  const u64* d_answer_values, u32 k, u32 kb, const u64* h_r) {
    StirQuotientArgs a;
    a.vals = vals;
    a.n = n;
    a.offset = offset;
    a.gen = gen;
    a.points = d_points;
    a.answer = d_answer;
    a.answer_values = d_answer_values;
    a.k = k;
    a.kb = kb;
    a.r0 = h_r[0];
    a.r1 = h_r[1];
    a.r2 = h_r[2];
    TVM_LAUNCH(k_stir_quotient, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, a);
    TVM_HIP_CHECK(c, hipGetLastError());
    return TVM_OK;
}

}  // namespace tvm
