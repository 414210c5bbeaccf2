// proof_middle.hip -- the middle of a proof with the transcript on the device: from the quotient's Merkle root to the DEEP codeword,
// queued on the stream with no host decision in between.
//
// A translation unit of its own, entry points included (as proof_tail.hip: nothing is added to the code objects of poly.hip, hash.hip,
// proof_tail.hip or stir.hip).
//
// Replaces, on the host's side of the reference's hot path:
//   ProofStream::enqueue(MerkleRoot(quotient root)), sample_scalars(1), the four out-of-domain points   stark.rs:444-456     -> k_middle_points
//   the six out-of-domain ProofItems into the sponge, sample_scalars(3)                                 stark.rs:478-505     -> k_middle_weights
//   the weight vectors (powers of the three scalars) and the two segment combination values             stark.rs:507-543     -> k_weight_vectors
//   Prover::deep_codeword with the points, values and weights where the kernels above left them         stark.rs:545-625     -> k_deep_dev
// These are latency kernels: one wavefront each for the first two.  What they buy is the host round trips between the evaluation
// kernels of poly.hip, which already take their small operands from device memory.
#include <cstring>
#include <vector>

#include "air_eval.h"   // AirAcc: the weighted terms of a DEEP point summed unreduced
#include "context.h"
#include "kernels.h"
#include "tail_kernels.h"
#include "tip5.h"

namespace tvm {

TVM_D xfe pm_ld(const u64* p) { return xfe_make(p[0], p[1], p[2]); }
TVM_D void pm_st(u64* p, xfe v) { p[0] = v.c0; p[1] = v.c1; p[2] = v.c2; }

// ---------------------------------------------------------------------------------------------- the out-of-domain point
// One wavefront, the lane convention of k_sponge_tail (tail_kernels.h).  Where a tree is given, ProofItem::MerkleRoot(nodes[1]) is
// absorbed first ([0, root] padded with 1, 0, 0, 0: one block, as k_sponge_root_and_sample) and the root handed out; a null tree
// means the state already holds it.  Then sample_scalars(1) = alpha, and lane 0 forms the four points
//     alpha, alpha * omega (the next row), alpha^4, (zeta alpha)^4 (the two points of the quotient segments).
struct MiddlePointsArgs {
    u64* state;          // [16], in and out
    const u64* nodes;    // the quotient tree [2 L][5], or null
    u64 omega, zeta;     // the trace domain's generator; Stark::ZETA
    u64* root;           // [5]: nodes[1], or zeros
    u64* points;         // [4][3]
};
__global__ void __launch_bounds__(64) k_middle_points(MiddlePointsArgs g) {
    __shared__ unsigned char lut[256];
    __shared__ u64 alpha_s[3];
    tip5_stage_lut(lut, threadIdx.x, blockDim.x);
    const int lane = (int)threadIdx.x, pos = lane & 15;
    u64 x = g.state[pos];
    if (g.nodes) {
        if (pos == 0) x = 0;                       // the discriminant of ProofItem::MerkleRoot
        else if (pos <= 5) x = g.nodes[5 + pos - 1];
        else if (pos == 6) x = TVM_ONE;            // padding: 1, then zeros
        else if (pos < TIP5_RATE) x = 0;
        x = tip5_permute_lanes(x, pos, lane, lut);
    }
    if (lane < 5) g.root[lane] = g.nodes ? g.nodes[5 + lane] : 0;
    x = sponge_sample_scalars_lanes(x, pos, lane, lut, 1, alpha_s);
    __syncthreads();
    if (lane < 16) g.state[pos] = x;
    if (lane == 0) {
        const xfe a = pm_ld(alpha_s);
        pm_st(g.points, a);
        pm_st(g.points + 3, xfe_mul_bfe(a, g.omega));
        pm_st(g.points + 6, xfe_sqr(xfe_sqr(a)));
        pm_st(g.points + 9, xfe_sqr(xfe_sqr(xfe_mul_bfe(a, g.zeta))));
    }
}

// ---------------------------------------------------------------------------------------------- the combination weights
// One wavefront.  The six out-of-domain items are absorbed straight from the arrays the evaluation kernels wrote, in the order of
// ProofSteps::prove -- main row, aux row, main next row, aux next row, the segments 0..3 at alpha^4, the segments 1..4 at (zeta alpha)^4
// --: these variants are statically sized, so an item's encoding is [discriminant, its words] (encode_item, proof_item.rs:96-150).
// The two segment items are strided picks out of the [5][2] evaluations and pass through LDS.  Then sample_scalars(3) = w0, w1, w2.
struct MiddleWeightsArgs {
    u64* state;                      // [16], in and out
    const u64 *main_rows, *aux_rows; // [2][n_main][3], [2][n_aux][3]: the rows at alpha and at alpha * omega
    u32 n_main, n_aux;
    const u64* segments;             // [5][2][3]: the segment polynomials at alpha^4 and (zeta alpha)^4
    u64* scalars;                    // [3][3]: w0, w1, w2
};
__global__ void __launch_bounds__(64) k_middle_weights(MiddleWeightsArgs g) {
    __shared__ unsigned char lut[256];
    __shared__ u64 picks[24];   // the two segment items' words
    tip5_stage_lut(lut, threadIdx.x, blockDim.x);
    const int lane = (int)threadIdx.x, pos = lane & 15;
    if (lane < 24) {
        const int item = lane / 12, k = lane % 12 / 3 + item, comp = lane % 3;
        picks[lane] = g.segments[3 * (2 * k + item) + comp];
    }
    __syncthreads();
    u64 x = g.state[pos];
    const u64 main_row = bfe_from_u64(2), aux_row = bfe_from_u64(3), quotient_segments = bfe_from_u64(4);   // the discriminants
    const u64 wm = 3 * (u64)g.n_main, wa = 3 * (u64)g.n_aux;
    x = sponge_absorb_lanes(x, pos, lane, lut, main_row, 0, 0, 0, 1, g.main_rows, wm);
    x = sponge_absorb_lanes(x, pos, lane, lut, aux_row, 0, 0, 0, 1, g.aux_rows, wa);
    x = sponge_absorb_lanes(x, pos, lane, lut, main_row, 0, 0, 0, 1, g.main_rows + wm, wm);
    x = sponge_absorb_lanes(x, pos, lane, lut, aux_row, 0, 0, 0, 1, g.aux_rows + wa, wa);
    x = sponge_absorb_lanes(x, pos, lane, lut, quotient_segments, 0, 0, 0, 1, picks, 12);
    x = sponge_absorb_lanes(x, pos, lane, lut, quotient_segments, 0, 0, 0, 1, picks + 12, 12);
    x = sponge_sample_scalars_lanes(x, pos, lane, lut, 3, g.scalars);
    if (lane < 16) g.state[pos] = x;
}
// The weight vectors from the three scalars, a kernel of its own (log depth: work-item i raises w0 to the i-th power):
//     w_columns = w0^0 .. w0^(n_columns - 1)
//     wp = (w1^0 .. w1^3, 0),  wr = (0, w1^1 .. w1^4),  wd = w2^0 .. w2^3
//     p_value = sum_{k < 4} w1^k seg[k](alpha^4),  r_value = sum_{1 <= k < 5} w1^k seg[k]((zeta alpha)^4)
// All field words are canonical, so the powers are the words of the host's xfe_powers whatever the order of the multiplications.
struct WeightVectorsArgs {
    const u64* scalars;              // [3][3]: w0, w1, w2
    const u64* segments;             // [5][2][3]
    u32 n_columns;
    u64 *w_columns, *wp, *wr, *wd;   // [n_columns][3], [5][3], [5][3], [4][3]
    u64* pr_values;                  // [2][3]: p_value, r_value
};
__global__ void __launch_bounds__(64) k_weight_vectors(WeightVectorsArgs g) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < g.n_columns) pm_st(g.w_columns + 3 * (u64)i, xfe_pow(pm_ld(g.scalars), (u64)i));
    if (i) return;
    const xfe w1 = pm_ld(g.scalars + 3), w2 = pm_ld(g.scalars + 6);
    xfe w = xfe_one(), p_value = xfe_zero(), r_value = xfe_zero();
    for (int k = 0; k < 5; k++) {
        pm_st(g.wp + 3 * k, k < 4 ? w : xfe_zero());
        pm_st(g.wr + 3 * k, k > 0 ? w : xfe_zero());
        if (k < 4) p_value = xfe_add(p_value, xfe_mul(w, pm_ld(g.segments + 3 * (2 * k))));
        if (k > 0) r_value = xfe_add(r_value, xfe_mul(w, pm_ld(g.segments + 3 * (2 * k + 1))));
        w = xfe_mul(w, w1);
    }
    pm_st(g.pr_values, p_value);
    pm_st(g.pr_values + 3, r_value);
    w = xfe_one();
    for (int k = 0; k < 4; k++) {
        pm_st(g.wd + 3 * k, w);
        w = xfe_mul(w, w2);
    }
}

// ---------------------------------------------------------------------------------------------- DEEP
// k_deep / k_deep_short (poly.hip) over the same work-items, with the n_comp (point, value, weight) triples read from device memory
// at kernel entry: the addresses are uniform and the arrays are only read, so the loads are scalar and the operands sit where the
// kernel arguments of k_deep sit.  The bodies are restated here and not shared through a header: k_deep is issue-bound, and calling
// its body as a function of a header -- the argument struct by reference or by value -- changed its registers in poly.hip's code
// object (profiles/device_middle_kernel_static_properties.txt; the bodies of today: profiles/ood_deep_kernel_static_properties.txt).
#define TVM_DEEP_MAX 4
#define TVM_DEEP_POINTS 4
struct DeepDeviceArgs {
    const u64* cw[TVM_DEEP_MAX];
    const u64 *points, *values, *weights;   // n_comp XFE each
    int n_comp;
    u64 offset, gen, n;
    u64* out;
};
struct DeepOperands {
    xfe point[TVM_DEEP_MAX], value[TVM_DEEP_MAX], weight[TVM_DEEP_MAX];
};
TVM_D DeepOperands deep_operands(const DeepDeviceArgs& a) {
    DeepOperands o;
#pragma unroll
    for (int k = 0; k < TVM_DEEP_MAX; k++) {
        const bool live = k < a.n_comp;
        o.point[k] = live ? pm_ld(a.points + 3 * k) : xfe_zero();
        o.value[k] = live ? pm_ld(a.values + 3 * k) : xfe_zero();
        o.weight[k] = live ? pm_ld(a.weights + 3 * k) : xfe_zero();
    }
    return o;
}
// The denominators x - p = (x - p0, -p1, -p2) inverted through the base field (poly.hip: FixedTail and its functions, restated
// here with the kernel body): adjugate and norm with the point's two upper coefficients fixed.
struct PmFixedTail {
    u64 a1, a2, e, f, g;   // e = (a1 - a2) a1, f = (a1 - a2) a2, g = a1^2
};
TVM_D u64 pm_uniform_u64(u64 v) { return ((u64)(u32)tvm_uniform((int)(u32)(v >> 32)) << 32) | (u32)tvm_uniform((int)(u32)v); }
TVM_D PmFixedTail pm_fixed_tail(u64 a1, u64 a2) {
    PmFixedTail d;
    d.a1 = a1, d.a2 = a2;
    const u64 d12 = bfe_sub(a1, a2);
    bfe_mul3(d12, a1, d12, a2, a1, a1, d.e, d.f, d.g);
    d.e = pm_uniform_u64(d.e), d.f = pm_uniform_u64(d.f), d.g = pm_uniform_u64(d.g);
    return d;
}
TVM_D xfe pm_tail_adjugate(u64 a0, const PmFixedTail& d) {
    const u64 s = bfe_add(a0, d.a2);
    u64 ss, t1, t2;
    bfe_mul3(s, s, d.a1, s, s, d.a2, ss, t1, t2);
    u64 k0, k1, k2;
    bfe_sub3(ss, d.e, d.f, t1, d.g, t2, k0, k1, k2);
    return xfe_make(k0, k1, k2);
}
TVM_D u64 pm_tail_norm(u64 a0, const PmFixedTail& d, xfe adj) {
    u64 m0, m1, m2;
    bfe_mul3(a0, adj.c0, d.a2, adj.c1, d.a1, adj.c2, m0, m1, m2);
    return bfe_sub(bfe_sub(m0, m1), m2);
}
// Four points per work-item, a quarter of the domain apart, one base-field inversion for the norms of their 4 n_comp denominators
// (see k_deep; a zero denominator zeroes every term of the work-item's four points there and here).
__global__ void __launch_bounds__(256) k_deep_dev(DeepDeviceArgs a) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 quarter = a.n / TVM_DEEP_POINTS;
    if (i >= quarter) return;
    const DeepOperands o = deep_operands(a);
    const u64 w = bfe_pow(a.gen, quarter);
    u64 x[TVM_DEEP_POINTS];
    x[0] = bfe_mul(a.offset, bfe_pow(a.gen, i));
#pragma unroll
    for (int j = 1; j < TVM_DEEP_POINTS; j++) x[j] = bfe_mul(x[j - 1], w);
    PmFixedTail pt[TVM_DEEP_MAX];
#pragma unroll
    for (int k = 0; k < TVM_DEEP_MAX; k++) pt[k] = pm_fixed_tail(bfe_neg(o.point[k].c1), bfe_neg(o.point[k].c2));
    u64 pre[TVM_DEEP_POINTS][TVM_DEEP_MAX];
    u64 run = TVM_ONE;
#pragma unroll
    for (int j = 0; j < TVM_DEEP_POINTS; j++) {
#pragma unroll
        for (int k = 0; k < TVM_DEEP_MAX; k++) {
            pre[j][k] = run;
            if (k < a.n_comp) {
                const u64 a0 = bfe_sub(x[j], o.point[k].c0);
                run = bfe_mul(run, pm_tail_norm(a0, pt[k], pm_tail_adjugate(a0, pt[k])));
            }
        }
    }
    u64 inv = bfe_inv(run);
#pragma unroll
    for (int j = TVM_DEEP_POINTS - 1; j >= 0; j--) {
        AirAcc acc = air_acc_zero();
        const u64 row = i + (u64)j * quarter;
#pragma unroll
        for (int k = TVM_DEEP_MAX - 1; k >= 0; k--) {
            if (k < a.n_comp) {
                const u64 a0 = bfe_sub(x[j], o.point[k].c0);
                const xfe adj = pm_tail_adjugate(a0, pt[k]);
                u64 ninv;
                bfe_mul2(inv, pre[j][k], inv, pm_tail_norm(a0, pt[k], adj), ninv, inv);
                const xfe num = xfe_sub(pm_ld(a.cw[k] + 3 * row), o.value[k]);
                air_acc_x(acc, o.weight[k], xfe_mul(num, xfe_mul_bfe(adj, ninv)));
            }
        }
        pm_st(a.out + 3 * row, air_acc_value(acc));
    }
}
// a domain shorter than four points: one point per work-item
__global__ void k_deep_short_dev(DeepDeviceArgs a) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const DeepOperands o = deep_operands(a);
    const u64 x = bfe_mul(a.offset, bfe_pow(a.gen, i));
    xfe acc = xfe_zero();
#pragma unroll
    for (int k = 0; k < TVM_DEEP_MAX; k++) {
        if (k < a.n_comp) {
            const xfe num = xfe_sub(pm_ld(a.cw[k] + 3 * i), o.value[k]);
            acc = xfe_add(acc, xfe_mul(xfe_mul(num, xfe_inv(xfe_bfe_minus(x, o.point[k]))), o.weight[k]));
        }
    }
    pm_st(a.out + 3 * i, acc);
}

namespace {
int weight_vectors_launch(tvm_ctx* c, const u64* d_scalars, const u64* d_segments, u32 n_columns, u64* d_w, u64* d_wp, u64* d_wr, u64* d_wd,
                          u64* d_pr_values) {
    WeightVectorsArgs g = {d_scalars, d_segments, n_columns, d_w, d_wp, d_wr, d_wd, d_pr_values};
    TVM_LAUNCH(k_weight_vectors, dim3((n_columns + 63) / 64 ? (n_columns + 63) / 64 : 1), dim3(64), 0, c->stream, g);
    TVM_HIP_CHECK(c, hipGetLastError());
    return TVM_OK;
}
int deep_sum_device_args(tvm_ctx* c, int n_comp, const u64* const* d_cw, const u64* d_points, const u64* d_values, const u64* d_weights,
                         u64 offset, u64 gen, u64 n, u64* d_out) {
    DeepDeviceArgs a = {};
    for (int k = 0; k < n_comp; k++) a.cw[k] = d_cw[k];
    a.points = d_points, a.values = d_values, a.weights = d_weights;
    a.n_comp = n_comp, a.offset = offset, a.gen = gen, a.n = n, a.out = d_out;
    if (n % TVM_DEEP_POINTS) TVM_LAUNCH(k_deep_short_dev, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, a);
    else TVM_LAUNCH(k_deep_dev, dim3((unsigned)((n / TVM_DEEP_POINTS + 255) / 256)), dim3(256), 0, c->stream, a);
    TVM_HIP_CHECK(c, hipGetLastError());
    return TVM_OK;
}

// tvm_weighted_sum_of_columns of both tables and their sum, with the weights on the device: the two sums over the rows are added
// before the one inverse transform (it is linear, and the field words are canonical: the same words as two transforms and an
// addition), then each table's randomizers contribute.  d_poly: 2 n XFE.
int weighted_sum_of_both_tables(tvm_ctx* c, const u64* main_trace, u64 n_main, const u64* main_rnd, const u64* aux_trace, u64 n_aux,
                                const u64* aux_rnd, u64 n, u64 h, u64 trace_gen, const u64* d_w, u64* d_poly) {
    TVM_TRY(weighted_row_sum(c, 1, main_trace, n, n_main, d_w, 0, d_poly));
    TVM_TRY(weighted_row_sum(c, 3, aux_trace, n, n_aux, d_w + 3 * n_main, 1, d_poly));
    TVM_HIP_CHECK(c, hipMemsetAsync(d_poly + 3 * n, 0, 3 * n * sizeof(u64), c->stream));
    if (n > 1)
        TVM_TRY(ntt_columns(c, d_poly, n, 3, 0, d_poly, 3, 0, 1, 0, 3, n, bfe_inv(trace_gen), TVM_ONE, TVM_ONE, bfe_inv(bfe_from_u64(n))));
    TVM_TRY(randomizer_contribution(c, 1, main_rnd, n, n_main, h, d_w, d_poly));
    return randomizer_contribution(c, 3, aux_rnd, n, n_aux, h, d_w + 3 * n_main, d_poly);
}
}  // namespace

}  // namespace tvm

extern "C" {
using namespace tvm;

int32_t tvm_deep_codeword_device_args(tvm_ctx* c, uint32_t n_comp, const uint64_t* const* d_cw, tvm_domain dom, const uint64_t* d_points,
                                      const uint64_t* d_values, const uint64_t* d_weights, uint64_t* d_out) {
    if (!c || !d_cw || !d_points || !d_values || !d_weights || !d_out || !valid_domain(dom))
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "deep_codeword_device_args arguments");
    if (n_comp < 1 || n_comp > TVM_DEEP_MAX) return set_error(c, TVM_ERR_INVALID_ARGUMENT, "deep: 1..4 components");
    for (uint32_t k = 0; k < n_comp; k++)
        if (!d_cw[k]) return set_error(c, TVM_ERR_INVALID_ARGUMENT, "deep_codeword_device_args: null codeword");
    return deep_sum_device_args(c, (int)n_comp, d_cw, d_points, d_values, d_weights, dom.offset, dom.generator, dom.length, d_out);
}

int32_t tvm_combination_weight_vectors(tvm_ctx* c, const uint64_t* h_scalars, const uint64_t* h_segments, uint32_t n_columns,
                                       uint64_t* h_w_columns, uint64_t* h_wp, uint64_t* h_wr, uint64_t* h_wd, uint64_t* h_pr_values) {
    if (!c || !h_scalars || !h_segments || !n_columns || n_columns > (1u << 20) || !h_w_columns || !h_wp || !h_wr || !h_wd || !h_pr_values)
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_combination_weight_vectors arguments");
    // one block: scalars | segments || w_columns | wp | wr | wd | p_value, r_value   (the part behind || comes back in one copy)
    const size_t w_back = 3 * (size_t)n_columns + 15 + 15 + 12 + 6;
    PoolBlock block(c, (9 + 30 + w_back) * sizeof(u64));
    u64* d = (u64*)block.p;
    if (!d) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "tvm_combination_weight_vectors staging");
    u64 *d_w = d + 39, *d_wp = d_w + 3 * (size_t)n_columns, *d_wr = d_wp + 15, *d_wd = d_wr + 15, *d_pr = d_wd + 12;
    std::vector<u64> back(w_back);
    int rc = h2d_small(c, d, h_scalars, 9 * sizeof(u64));
    if (rc == TVM_OK) rc = h2d_small(c, d + 9, h_segments, 30 * sizeof(u64));
    if (rc == TVM_OK) rc = weight_vectors_launch(c, d, d + 9, n_columns, d_w, d_wp, d_wr, d_wd, d_pr);
    if (rc == TVM_OK && hipMemcpyAsync(back.data(), d_w, w_back * sizeof(u64), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = set_error(c, TVM_ERR_DEVICE, "tvm_combination_weight_vectors download");
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == TVM_OK) rc = set_error(c, TVM_ERR_DEVICE, "tvm_combination_weight_vectors");
    if (rc != TVM_OK) return rc;
    const u64* b = back.data();
    std::memcpy(h_w_columns, b, 3 * (size_t)n_columns * sizeof(u64)), b += 3 * (size_t)n_columns;
    std::memcpy(h_wp, b, 15 * sizeof(u64)), b += 15;
    std::memcpy(h_wr, b, 15 * sizeof(u64)), b += 15;
    std::memcpy(h_wd, b, 12 * sizeof(u64)), b += 12;
    std::memcpy(h_pr_values, b, 6 * sizeof(u64));
    return TVM_OK;
}

uint64_t tvm_out_of_domain_to_deep_block_words(uint64_t n_main_cols, uint64_t n_aux_cols) { return TVM_MIDDLE_BLOCK_WORDS(n_main_cols, n_aux_cols); }

// tvm_out_of_domain_to_deep and its _device_state twin: one body.  The sponge state comes from the host (h_state, staged) or lies on the
// device (d_state_io: copied into the block device to device, and the state after the combination weights copied back the same way).
static int out_of_domain_to_deep(tvm_ctx* c, const uint64_t* d_main_trace, uint64_t n_main, const uint64_t* d_main_rnd,
                                 const uint64_t* d_aux_trace, uint64_t n_aux, const uint64_t* d_aux_rnd, uint64_t n, uint64_t h,
                                 tvm_domain td, const uint64_t* d_polys, uint64_t poly_len, const tvm_table* segments,
                                 const uint64_t* d_quotient_nodes, tvm_domain sd, uint64_t zeta, const uint64_t* h_state, uint64_t* d_state_io,
                                 uint64_t* d_combination, uint64_t* h_block, uint64_t block_capacity) {
    if (!c || !d_main_trace || !d_aux_trace || (h && (!d_main_rnd || !d_aux_rnd)) || !n_main || !n_aux || n_main + n_aux > (1u << 20) ||
        !valid_domain(td) || td.length != n || h > n || !d_polys || !poly_len || !segments || segments->fk != 3 || segments->n_cols != 5 ||
        !valid_domain(sd) || sd.length > segments->rows || zeta >= TVM_P || (!h_state && !d_state_io) || !d_combination || !h_block ||
        block_capacity < TVM_MIDDLE_BLOCK_WORDS(n_main, n_aux))
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_out_of_domain_to_deep arguments");
    if (td.offset != TVM_ONE) return set_error(c, TVM_ERR_UNSUPPORTED, "trace domain offset must be 1");
    const u64 n_ma = n_main + n_aux, w_block = TVM_MIDDLE_BLOCK_WORDS(n_main, n_aux), S = sd.length;
    // one slot: the block that goes back to the host | w_ma | wp | wr | wd
    u64* d = (u64*)scratch(c, Scratch::MiddleBlock, (w_block + 3 * n_ma + 15 + 15 + 12) * sizeof(u64));
    // the combination polynomial (2 n XFE), its codeword and the two segment combinations on the short domain
    PoolBlock pool(c, (6 * n + 9 * S) * sizeof(u64));
    if (!d || !pool.p) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "tvm_out_of_domain_to_deep staging");
    u64 *d_root = d + TVM_MIDDLE_ROOT, *d_points = d + TVM_MIDDLE_POINTS, *d_main_rows = d + TVM_MIDDLE_MAIN_ROWS,
        *d_aux_rows = d + TVM_MIDDLE_AUX_ROWS(n_main), *d_seg = d + TVM_MIDDLE_SEGMENTS(n_main, n_aux), *d_values = d + TVM_MIDDLE_VALUES(n_main, n_aux),
        *d_scalars = d + TVM_MIDDLE_WEIGHTS(n_main, n_aux), *d_state = d + TVM_MIDDLE_STATE(n_main, n_aux);
    u64 *d_w_ma = d + w_block, *d_wp = d_w_ma + 3 * n_ma, *d_wr = d_wp + 15, *d_wd = d_wr + 15;
    u64 *comb = (u64*)pool.p, *mac = comb + 6 * n, *cw_p = mac + 3 * S, *cw_r = cw_p + 3 * S;

    // From here on work is queued that reads the caller's arrays and writes the block: every way out synchronises the stream first.
    auto leave = [&](int rc) {
        if (hipStreamSynchronize(c->stream) != hipSuccess && rc == TVM_OK) rc = set_error(c, TVM_ERR_DEVICE, "tvm_out_of_domain_to_deep");
        return rc;
    };
    auto queue = [&]() -> int {
        if (d_state_io) TVM_HIP_CHECK(c, hipMemcpyAsync(d_state, d_state_io, 16 * sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
        else TVM_TRY(h2d_small(c, d_state, h_state, 16 * sizeof(u64)));
        // 12 (the root into the sponge), 13: the out-of-domain point, rows and segment values
        MiddlePointsArgs mp = {d_state, d_quotient_nodes, td.generator, zeta, d_root, d_points};
        TVM_LAUNCH(k_middle_points, dim3(1), dim3(64), 0, c->stream, mp);
        TVM_TRY(out_of_domain_rows(c, 1, d_main_trace, n, n_main, d_main_rnd, h, td.generator, d_points, 2, d_main_rows));
        TVM_TRY(out_of_domain_rows(c, 3, d_aux_trace, n, n_aux, d_aux_rnd, h, td.generator, d_points, 2, d_aux_rows));
        for (int k = 0; k < 5; k++) TVM_TRY(poly_eval(c, d_polys + (u64)k * poly_len * 3, poly_len, d_points + 6, 2, d_seg + 6 * k));
        // 14: the six items into the sponge, the weights
        MiddleWeightsArgs mw = {d_state, d_main_rows, d_aux_rows, (u32)n_main, (u32)n_aux, d_seg, d_scalars};
        TVM_LAUNCH(k_middle_weights, dim3(1), dim3(64), 0, c->stream, mw);
        TVM_TRY(weight_vectors_launch(c, d_scalars, d_seg, (u32)n_ma, d_w_ma, d_wp, d_wr, d_wd, d_values + 6));
        // 15: the linear combinations and their values at the out-of-domain points
        TVM_TRY(weighted_sum_of_both_tables(c, d_main_trace, n_main, d_main_rnd, d_aux_trace, n_aux, d_aux_rnd, n, h, td.generator, d_w_ma, comb));
        TVM_TRY(tvm_evaluate(c, 3, comb, n + h, sd, mac));
        TVM_TRY(table_lincomb(c, segments->data, segments->layout, 3, 5, segments->rows / S, d_wp, cw_p));
        TVM_TRY(table_lincomb(c, segments->data, segments->layout, 3, 5, segments->rows / S, d_wr, cw_r));
        TVM_TRY(poly_eval(c, comb, n + h, d_points, 2, d_values));
        // 16: DEEP
        const u64* cws[4] = {mac, mac, cw_p, cw_r};
        TVM_TRY(deep_sum_device_args(c, 4, cws, d_points, d_values, d_wd, sd.offset, sd.generator, S, d_combination));
        if (d_state_io) TVM_HIP_CHECK(c, hipMemcpyAsync(d_state_io, d_state, 16 * sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
        TVM_HIP_CHECK(c, hipMemcpyAsync(h_block, d, w_block * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        return TVM_OK;
    };
    return leave(queue());
}
int32_t tvm_out_of_domain_to_deep(tvm_ctx* c, const uint64_t* d_main_trace, uint64_t n_main, const uint64_t* d_main_rnd,
                                  const uint64_t* d_aux_trace, uint64_t n_aux, const uint64_t* d_aux_rnd, uint64_t n, uint64_t h,
                                  tvm_domain td, const uint64_t* d_polys, uint64_t poly_len, const tvm_table* segments,
                                  const uint64_t* d_quotient_nodes, tvm_domain sd, uint64_t zeta, const uint64_t* h_state,
                                  uint64_t* d_combination, uint64_t* h_block, uint64_t block_capacity) {
    return out_of_domain_to_deep(c, d_main_trace, n_main, d_main_rnd, d_aux_trace, n_aux, d_aux_rnd, n, h, td, d_polys, poly_len, segments,
                                 d_quotient_nodes, sd, zeta, h_state, nullptr, d_combination, h_block, block_capacity);
}
int32_t tvm_out_of_domain_to_deep_device_state(tvm_ctx* c, const uint64_t* d_main_trace, uint64_t n_main, const uint64_t* d_main_rnd,
                                               const uint64_t* d_aux_trace, uint64_t n_aux, const uint64_t* d_aux_rnd, uint64_t n, uint64_t h,
                                               tvm_domain td, const uint64_t* d_polys, uint64_t poly_len, const tvm_table* segments,
                                               const uint64_t* d_quotient_nodes, tvm_domain sd, uint64_t zeta, uint64_t* d_state,
                                               uint64_t* d_combination, uint64_t* h_block, uint64_t block_capacity) {
    return out_of_domain_to_deep(c, d_main_trace, n_main, d_main_rnd, d_aux_trace, n_aux, d_aux_rnd, n, h, td, d_polys, poly_len, segments,
                                 d_quotient_nodes, sd, zeta, nullptr, d_state, d_combination, h_block, block_capacity);
}
}  // extern "C"
