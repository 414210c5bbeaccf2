// verify_kernels.h -- the bodies of the verifier's per-query kernels, shared by the one-proof entry points (verify.hip,
// verify_ldt.hip) and the many-proof ones (verify_batch.hip): a body takes its arguments as a struct and the work-item's or
// workgroup's place in ITS proof, so that the batched kernels differ from the single ones only in where the struct comes from.
#pragma once
#include "kernels.h"

namespace tvm {

TVM_D xfe vl_ld(const u64* p) { return xfe_make(p[0], p[1], p[2]); }
TVM_D void vl_st(u64* p, xfe v) { p[0] = v.c0, p[1] = v.c1, p[2] = v.c2; }

// ---------------------------------------------------------------------------------------------- DEEP values of the revealed rows
struct VerifyArgs {
    const u64* main_rows;   // [q][n_main]
    const u64* aux_rows;    // [q][n_aux][3]
    const u64* quot_rows;   // [q][5][3]
    const u64* row_idx;     // [q]
    const u64* w_ma;        // [n_main + n_aux][3]
    const u64* small;       // weights_quot[5][3], weights_deep[4][3], ood points[4][3], ood values[4][3]
    u64 offset, gen;        // low-degree-test domain
    int n_main, n_aux;
    u64* out;               // [q][3]
};

#define VF_BLOCK 256
// one workgroup of VF_BLOCK work-items for row j of `a`
TVM_D void verifier_deep_values_row(const VerifyArgs& a, u64 j) {
    __shared__ u64 smem[3 * VF_BLOCK];
    const int tid = threadIdx.x;
    const u64* mrow = a.main_rows + j * (u64)a.n_main;
    const u64* arow = a.aux_rows + j * (u64)a.n_aux * 3;
    // linearly_sum_main_and_aux_row (stark.rs:1765-1787)
    xfe acc = xfe_zero();
    for (int c = tid; c < a.n_main; c += VF_BLOCK) acc = xfe_add(acc, xfe_mul_bfe(vl_ld(a.w_ma + 3 * c), mrow[c]));
    for (int c = tid; c < a.n_aux; c += VF_BLOCK) acc = xfe_add(acc, xfe_mul(vl_ld(a.w_ma + 3 * (a.n_main + c)), vl_ld(arow + 3 * c)));
    // sum over the workgroup
    smem[tid] = acc.c0, smem[VF_BLOCK + tid] = acc.c1, smem[2 * VF_BLOCK + tid] = acc.c2;
    __syncthreads();
    for (int s = VF_BLOCK >> 1; s > 0; s >>= 1) {
        if (tid < s)
            for (int k = 0; k < 3; k++) smem[k * VF_BLOCK + tid] = bfe_add(smem[k * VF_BLOCK + tid], smem[k * VF_BLOCK + tid + s]);
        __syncthreads();
    }
    if (tid) return;
    const xfe ma = xfe_make(smem[0], smem[VF_BLOCK], smem[2 * VF_BLOCK]);
    const u64* wq = a.small;
    const u64* wd = a.small + 15;
    const u64* pts = a.small + 27;
    const u64* vals = a.small + 39;
    const u64* q = a.quot_rows + j * 15;
    // quotient segments: P uses segments 0..3, R segments 1..4 (stark.rs:1700-1717)
    xfe shared = xfe_zero();
    for (int k = 1; k < 4; k++) shared = xfe_add(shared, xfe_mul(vl_ld(q + 3 * k), vl_ld(wq + 3 * k)));
    const xfe for_p = xfe_add(xfe_mul(vl_ld(wq), vl_ld(q)), shared);
    const xfe for_r = xfe_add(xfe_mul(vl_ld(wq + 12), vl_ld(q + 12)), shared);
    // deep_update (stark.rs:2096-2103): (value - ood value) / (domain point - ood point)
    const u64 x = bfe_mul(a.offset, bfe_pow(a.gen, a.row_idx[j]));
    const xfe elems[4] = {ma, ma, for_p, for_r};
    xfe total = xfe_zero();
#pragma unroll   // (elems[k] with a loop counter would put the array into scratch memory)
    for (int k = 0; k < 4; k++) {
        const xfe num = xfe_sub(elems[k], vl_ld(vals + 3 * k));
        const xfe den = xfe_bfe_minus(x, vl_ld(pts + 3 * k));
        total = xfe_add(total, xfe_mul(vl_ld(wd + 3 * k), xfe_mul(num, xfe_inv(den))));
    }
    u64* o = a.out + 3 * j;
    o[0] = total.c0, o[1] = total.c1, o[2] = total.c2;
}

// ---------------------------------------------------------------------------------------------- FRI collinearity folds
// One work-item per query walks the rounds (fri.rs:520-560): the line through (x_a, a) and (x_b, b), b the revealed leaf at the
// index half a domain away, evaluated at the round's folding challenge; the round's domain is the square of the previous one.
struct FriFoldArgs {
    const u64 *idx, *a, *b, *challenges;   // [q], [q][3], [n_rounds][q][3], [n_rounds][3]
    u64 offset, gen, len, q;
    u32 n_rounds;
    u64* out;                              // [q][3]
};
TVM_D void verifier_fri_fold_query(const FriFoldArgs& g, u64 j) {
    xfe a = vl_ld(g.a + 3 * j);
    u64 offset = g.offset, gen = g.gen, len = g.len;
    const u64 i = g.idx[j];
    for (u32 r = 0; r < g.n_rounds; r++) {
        const u64 ia = i & (len - 1), ib = (ia + (len >> 1)) & (len - 1);
        const u64 xa = bfe_mul(offset, bfe_pow(gen, ia)), xb = bfe_mul(offset, bfe_pow(gen, ib));
        const xfe b = vl_ld(g.b + 3 * ((u64)r * g.q + j));
        const xfe slope = xfe_mul_bfe(xfe_sub(b, a), bfe_inv(bfe_sub(xb, xa)));
        a = xfe_add(a, xfe_mul(slope, xfe_sub_bfe(vl_ld(g.challenges + 3 * r), xa)));
        offset = bfe_sqr(offset), gen = bfe_sqr(gen), len >>= 1;
    }
    vl_st(g.out + 3 * j, a);
}

// ---------------------------------------------------------------------------------------------- STIR in-domain answers
// One workgroup per query.  The query's coset is x_j = root * kth_root^j, j < ff.  In a subsequent round (k > 0) the revealed values
// are first taken through the previous round's quotient and degree correction (stir.rs:1270-1340):
//     (value_j - Ans(x_j)) / Z(x_j) * sum_{e' <= k} (rc x_j)^e',   Z = prod_i (X - quotient_set[i]),
// the k-term sums and products split over the work-items and reduced through LDS; then the polynomial of degree < ff through the
// coset is evaluated at the folding randomness (fast_coset_interpolate(..).evaluate(..), stir.rs:1259-1268).
#define SA_BLOCK 256
#define SA_MAX_FF 16
struct StirAnswerArgs {
    const u64 *values, *roots;   // [q][ff][3], [q]
    const u64* small;            // folding randomness [3], degree-correction randomness [3]
    const u64 *qset, *ans;       // [k][3] each
    u64 kth_root;
    u32 k, ff;
    u64* out;                    // [q][3]
};
// one workgroup of SA_BLOCK work-items for query `query` of `g`
TVM_D void verifier_stir_answer_query(const StirAnswerArgs& g, u64 query) {
    __shared__ u64 sum[3 * SA_BLOCK], prod[3 * SA_BLOCK];
    __shared__ u64 ans_at[3 * SA_MAX_FF], z_at[3 * SA_MAX_FF], ev[3 * SA_MAX_FF], xs[SA_MAX_FF];
    __shared__ u64 dinv[SA_MAX_FF * SA_MAX_FF];   // 1 / (x_i - x_{i-l}) at [i * ff + l]: the denominators of the divided differences
    const int tid = threadIdx.x, ff = (int)g.ff;
    u64 x = g.roots[query];
    for (int j = 0; j < ff; j++, x = bfe_mul(x, g.kth_root)) {
        if (!tid) xs[j] = x;
        if (!g.k) continue;
        const u64 step = bfe_pow(x, SA_BLOCK);
        u64 xp = bfe_pow(x, (u64)tid);
        xfe s = xfe_zero(), p = xfe_one();
        for (u32 i = tid; i < g.k; i += SA_BLOCK, xp = bfe_mul(xp, step)) {
            s = xfe_add(s, xfe_mul_bfe(vl_ld(g.ans + 3 * (u64)i), xp));
            p = xfe_mul(p, xfe_bfe_minus(x, vl_ld(g.qset + 3 * (u64)i)));
        }
        sum[tid] = s.c0, sum[SA_BLOCK + tid] = s.c1, sum[2 * SA_BLOCK + tid] = s.c2;
        prod[tid] = p.c0, prod[SA_BLOCK + tid] = p.c1, prod[2 * SA_BLOCK + tid] = p.c2;
        __syncthreads();
        for (int h = SA_BLOCK >> 1; h > 0; h >>= 1) {
            if (tid < h) {
                const xfe a = xfe_mul(xfe_make(prod[tid], prod[SA_BLOCK + tid], prod[2 * SA_BLOCK + tid]),
                                      xfe_make(prod[tid + h], prod[SA_BLOCK + tid + h], prod[2 * SA_BLOCK + tid + h]));
                prod[tid] = a.c0, prod[SA_BLOCK + tid] = a.c1, prod[2 * SA_BLOCK + tid] = a.c2;
                for (int c = 0; c < 3; c++) sum[c * SA_BLOCK + tid] = bfe_add(sum[c * SA_BLOCK + tid], sum[c * SA_BLOCK + tid + h]);
            }
            __syncthreads();
        }
        if (!tid)
            for (int c = 0; c < 3; c++) ans_at[3 * j + c] = sum[c * SA_BLOCK], z_at[3 * j + c] = prod[c * SA_BLOCK];
        __syncthreads();
    }
    __syncthreads();
    // the ff (ff - 1) / 2 inversions of the divided differences, one per work-item, beside the ff quotients below
    if (tid < ff * ff && tid % ff >= 1 && tid / ff >= tid % ff) dinv[tid] = bfe_inv(bfe_sub(xs[tid / ff], xs[tid / ff - tid % ff]));
    if (tid < ff) {
        xfe v = vl_ld(g.values + 3 * (query * (u64)ff + (u64)tid));
        if (g.k) {
            const xfe quotient = xfe_mul(xfe_sub(v, vl_ld(ans_at + 3 * tid)), xfe_inv(vl_ld(z_at + 3 * tid)));
            const xfe common = xfe_mul_bfe(vl_ld(g.small + 3), xs[tid]);
            const u64 e = (u64)g.k + 1;
            xfe factor;
            if (xfe_eq(common, xfe_one())) factor = xfe_lift(bfe_from_u64(e));  // the geometric sum of e ones
            else factor = xfe_mul(xfe_sub(xfe_one(), xfe_pow(common, e)), xfe_inv(xfe_sub(xfe_one(), common)));
            v = xfe_mul(factor, quotient);
        }
        vl_st(ev + 3 * tid, v);
    }
    __syncthreads();
    if (tid) return;
    // Newton's divided differences over the coset, evaluated at the folding randomness
    // (in place in LDS: a register array indexed by a loop over ff would live in scratch)
    for (int l = 1; l < ff; l++)
        for (int i = ff - 1; i >= l; i--)
            vl_st(ev + 3 * i, xfe_mul_bfe(xfe_sub(vl_ld(ev + 3 * i), vl_ld(ev + 3 * (i - 1))), dinv[i * ff + l]));
    const xfe r = vl_ld(g.small);
    xfe acc = vl_ld(ev + 3 * (ff - 1));
    for (int i = ff - 2; i >= 0; i--) acc = xfe_add(xfe_mul(acc, xfe_sub_bfe(r, xs[i])), vl_ld(ev + 3 * i));
    vl_st(g.out + 3 * query, acc);
}

}  // namespace tvm
