// stir_rounds.hip -- Stir::prove with the transcript on the device: every round of the STIR prover queued on the stream with no host
// decision in between.
//
// A translation unit of its own, entry points included (as proof_tail.hip: nothing is added to the code objects of hash.hip, stir.hip
// or capi.hip).
//
// Replaces, on the host's side of the reference's hot path (stir.rs:885-993):
//   ProofStream::enqueue(MerkleRoot / StirOutOfDomainValues / Polynomial) into the sponge, sample_scalars, sample_indices
//                                                        proof_stream.rs:40-104                        -> k_stir_sponge
//   queried_indices.map(|i| i % folded_len).unique(), the quotient set and its answers   stir.rs:929-950 -> k_stir_query_set
//   the folding / degree-correction randomness and the size of the quotient set handed from the host to the kernels of stir.hip
//                                                        -> k_fold_polynomial_dev, k_xfe_interpolate_dev, k_stir_quotient_dev
//   StirMerkleTree::inclusion_proof of every answered tree                               stir.rs:1421-1440
//                                                        -> k_authentication_structures, k_tail_gather (proof_tail.hip)
// These are latency kernels of one wavefront or one workgroup; what they buy is the host round trips between them.
#include <cstring>
#include <vector>

#include "context.h"
#include "kernels.h"
#include "stir_kernels.h"
#include "tail_kernels.h"
#include "tip5.h"

namespace tvm {

// ---------------------------------------------------------------------------------------------- the sponge of a STIR proof
// One wavefront (tail_kernels.h).  The stages run in this order, each one only if its argument asks for it -- between two device steps
// of Stir::prove the transcript is one such sequence:
//   absorb ProofItem::MerkleRoot(root)                          encoding [0, the 5 words]
//   absorb ProofItem::StirOutOfDomainValues(values)             encoding [6, 1 + 3n, n, the 3n words], also for n = 0
//   absorb ProofItem::Polynomial(polynomial)                    tail_kernels.h
//   sample_scalars(n_scalars) -> scalars
//   sample_indices(mask + 1, n_indices) -> indices
//   n_single times sample_scalars(1) -> singles [n_single][3]   (each a squeeze of its own: not sample_scalars(n_single))
struct StirSpongeArgs {
    u64* state;                 // [16], in and out
    const u64* root;            // null, or 5 words; they are copied to root_out
    u64* root_out;
    const u64* values;          // absorb_values: n_values XFE
    u32 absorb_values, n_values;
    const u64* polynomial;      // null, or n_coefficients XFE
    u32 n_coefficients;
    u32 n_scalars;
    u64* scalars;
    u32 n_indices;
    u64 mask;
    u64* indices;
    u32 n_single;
    u64* singles;
};
__global__ void __launch_bounds__(64) k_stir_sponge(StirSpongeArgs g) {
    __shared__ unsigned char lut[256];
    __shared__ u64 rate[TIP5_RATE];
    tip5_stage_lut(lut, threadIdx.x, blockDim.x);
    const int lane = (int)threadIdx.x, pos = lane & 15;
    u64 x = g.state[pos];
    if (g.root) {
        if (lane < 5) g.root_out[lane] = g.root[lane];
        x = sponge_absorb_lanes(x, pos, lane, lut, 0, 0, 0, 0, 1, g.root, 5);   // ProofItem::MerkleRoot: discriminant 0
    }
    if (g.absorb_values)   // ProofItem::StirOutOfDomainValues (proof_item.rs: the seventh variant), a Vec<XFieldElement> behind its length
        x = sponge_absorb_lanes(x, pos, lane, lut, bfe_from_u64(6), bfe_from_u64(1 + 3 * (u64)g.n_values), bfe_from_u64(g.n_values), 0, 3, g.values,
                                3 * (u64)g.n_values);
    if (g.polynomial) x = sponge_absorb_polynomial_lanes(x, pos, lane, lut, 5, g.polynomial, g.n_coefficients);
    x = sponge_sample_scalars_lanes(x, pos, lane, lut, g.n_scalars, g.scalars);
    x = sponge_sample_indices_lanes(x, pos, lane, lut, rate, g.n_indices, g.mask, g.indices);
    for (u32 s = 0; s < g.n_single; s++) x = sponge_sample_scalars_lanes(x, pos, lane, lut, 1, g.singles + 3 * s);
    if (lane < 16) g.state[pos] = x;
}

// ---------------------------------------------------------------------------------------------- the queried set of a round
// One workgroup, one sampled index per work-item (n_raw <= TVM_TAIL_MAX_INDICES <= blockDim.x).  folded[i] = raw[i] mod folded_len; an
// index stays if no EARLIER entry has its value -- Itertools::unique keeps first occurrences in their order, and that order is the order
// of the stacked leaves in the StirResponse item --, and one prefix sum over the flags gives every survivor its place.  Out: the list,
// its length u, and -- for a full round -- the quotient set (folded_domain.value(i) lifted to the extension field for the u indices,
// then the out-of-domain points), its answers (the folded polynomial's values on the folded domain at the indices, then the
// out-of-domain values) and its size k = u + n_ood.
struct StirQuerySetArgs {
    const u64* raw;
    u32 n_raw, n_ood;
    u64 folded_mask;                       // folded_domain.length - 1
    u64 offset, gen;                       // of the folded domain
    const u64 *ood_points, *ood_values;    // [n_ood][3]
    const u64* on_folded_domain;           // [folded_domain.length][3]; null: the final round, no quotient set
    u64 *unique, *counts;                  // [n_raw]; [2] = (u, k)
    u64 *set, *answers;                    // [n_raw + n_ood][3]
};
__global__ void __launch_bounds__(TVM_TAIL_MAX_INDICES) k_stir_query_set(StirQuerySetArgs g) {
    __shared__ u64 folded[TVM_TAIL_MAX_INDICES];
    __shared__ u32 wave_sums[TVM_TAIL_MAX_INDICES / 64];
    const u32 tid = threadIdx.x;
    const bool live = tid < g.n_raw;
    const u64 mine = live ? g.raw[tid] & g.folded_mask : 0;
    folded[tid] = mine;
    __syncthreads();
    bool first = live;
    for (u32 j = 0; j < tid && first; j++) first = folded[j] != mine;   // (every lane reads the same word: a broadcast)
    u32 u;
    const u32 at = as_block_scan(first ? 1u : 0u, wave_sums, u);
    if (first) {
        g.unique[at - 1] = mine;
        if (g.on_folded_domain) {
            u64* p = g.set + 3 * (u64)(at - 1);
            p[0] = bfe_mul(g.offset, bfe_pow(g.gen, mine)), p[1] = 0, p[2] = 0;
            for (int w = 0; w < 3; w++) g.answers[3 * (u64)(at - 1) + w] = g.on_folded_domain[3 * mine + w];
        }
    }
    if (g.on_folded_domain)
        for (u32 e = tid; e < 3 * g.n_ood; e += blockDim.x) g.set[3 * (u64)u + e] = g.ood_points[e], g.answers[3 * (u64)u + e] = g.ood_values[e];
    if (tid == 0) g.counts[0] = u, g.counts[1] = u + (g.on_folded_domain ? g.n_ood : 0);
}

// ---------------------------------------------------------------------------------------------- device-argument forms of stir.hip
// the same work-items (stir_kernels.h); the randomness is three words of device memory, counts = (u, k) as k_stir_query_set writes them
__global__ void k_fold_polynomial_dev(const u64* __restrict__ poly, u64 n, int ff, const u64* __restrict__ r, u64 n_out, u64* __restrict__ out) {
    fold_polynomial_item(poly, n, ff, xfe_make(r[0], r[1], r[2]), n_out, out);
}
__global__ void __launch_bounds__(256) k_xfe_interpolate_dev(const u64* __restrict__ points, const u64* __restrict__ values,
                                                             const u64* __restrict__ counts, u64* __restrict__ out, int* __restrict__ status) {
    xfe_interpolate_workgroup(points, values, (int)counts[1], out, status);
}
__global__ void __launch_bounds__(256) k_stir_quotient_dev(StirQuotientArgs a, const u64* __restrict__ counts, const u64* __restrict__ r) {
    a.kb = (u32)counts[0], a.k = (u32)counts[1];
    a.r0 = r[0], a.r1 = r[1], a.r2 = r[2];
    stir_quotient_item(a);
}

namespace {
u64 pow2_at_least(u64 n, u64 p) {
    while (p < n) p <<= 1;
    return p;
}
// the instance as the rounds see it: tree t (t = 0 .. R) is over the domain of length L >> t, answered at queries[t] sampled indices
struct StirShape {
    u32 R = 0;
    u64 ff = 0, L = 0, n_ood_all = 0, n_queries_all = 0, n_final = 0;
    std::vector<u64> queries, ood;   // [R + 1], [R]
    u64 length(u32 t) const { return L >> t; }
    u64 n_leaves(u32 t) const { return length(t) / ff; }
    u64 n_scalar_words() const { return 3 * (2 * (u64)R + 1 + n_ood_all); }
};
// 0: fine; otherwise the status to return
int stir_shape(tvm_domain dom, uint32_t ff, uint32_t n_rounds, const uint64_t* round_queries, uint64_t final_queries, StirShape& s) {
    if (!is_pow2(dom.length) || dom.length > (1ull << 32) || dom.generator >= TVM_P || dom.offset >= TVM_P || !is_pow2(ff) || ff < 2 || ff > 16 ||
        n_rounds >= 32 || (n_rounds && !round_queries) || (dom.length >> n_rounds) < ff)
        return TVM_ERR_INVALID_ARGUMENT;
    s.R = n_rounds, s.ff = ff, s.L = dom.length;
    u64 n_coeffs = dom.length;
    for (u32 r = 0; r <= n_rounds; r++) {
        const u64 q = r < n_rounds ? round_queries[2 * r] : final_queries, ood = r < n_rounds ? round_queries[2 * r + 1] : 0;
        if (!q || q > TVM_VERIFIER_MAX_QUERIES || ood > TVM_VERIFIER_MAX_QUERIES) return TVM_ERR_INVALID_ARGUMENT;
        // k_stir_query_set takes one workgroup's indices; a full round's quotient set goes through k_xfe_interpolate (the final round
        // has no quotient set: only the first limit holds for it)
        if (q > TVM_TAIL_MAX_INDICES || (r < n_rounds && q + ood > 256)) return TVM_NOT_APPLICABLE;
        s.queries.push_back(q), s.n_queries_all += q;
        if (r < n_rounds) s.ood.push_back(ood), s.n_ood_all += ood;
        n_coeffs = (n_coeffs + ff - 1) / ff;
    }
    s.n_final = n_coeffs;
    return TVM_OK;
}
u64 stir_payload_bound(const StirShape& s) {
    u64 words = 0;
    for (u32 t = 0; t <= s.R; t++) words += 3 * s.ff * std::min(s.queries[t], s.n_leaves(t)) + 5 * auth_capacity(s.n_leaves(t), s.queries[t]);
    return words;
}
}  // namespace
}  // namespace tvm

extern "C" {
using namespace tvm;

uint64_t tvm_stir_prove_rounds_payload_bound(tvm_domain domain, uint32_t folding_factor, uint32_t n_rounds, const uint64_t* round_queries,
                                             uint64_t final_queries) {
    StirShape s;
    return stir_shape(domain, folding_factor, n_rounds, round_queries, final_queries, s) == TVM_OK ? stir_payload_bound(s) : 0;
}

int32_t tvm_stir_prove_rounds(tvm_ctx* c, const uint64_t* h_state, const uint64_t* d_codeword, tvm_domain dom, uint32_t folding_factor,
                              uint32_t n_rounds, const uint64_t* round_queries, uint64_t final_queries, uint64_t final_degree,
                              uint64_t* h_state_out, uint64_t* h_roots, uint64_t* h_scalars, uint64_t* h_ood_values, uint64_t* h_indices,
                              uint64_t* h_unique, uint64_t* h_unique_counts, uint64_t* h_final_polynomial, uint64_t* h_directory,
                              uint64_t* h_payload, uint64_t payload_capacity, uint64_t* payload_words) {
    if (!c || !h_state || !d_codeword || !h_state_out || !h_roots || !h_scalars || !h_indices || !h_unique || !h_unique_counts ||
        !h_final_polynomial || !h_directory || !payload_words || (payload_capacity && !h_payload))
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_stir_prove_rounds arguments");
    StirShape s;
    const int shape = stir_shape(dom, folding_factor, n_rounds, round_queries, final_queries, s);
    if (shape == TVM_NOT_APPLICABLE) return TVM_NOT_APPLICABLE;
    if (shape != TVM_OK || final_degree >= s.n_final || (s.n_ood_all && !h_ood_values))
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_stir_prove_rounds: the instance");
    const u32 R = s.R, n_trees = R + 1, n_segments = 2 * n_trees;
    const u64 ff = s.ff, bound = stir_payload_bound(s);
    u64 most = 0, auth_stride = 0, k_max_all = 0;
    for (u32 t = 0; t < n_trees; t++) {
        most = std::max(most, s.queries[t]), auth_stride = std::max(auth_stride, auth_capacity(s.n_leaves(t), s.queries[t]));
        if (t < R) k_max_all += s.queries[t] + s.ood[t];
    }

    // one block:  job and segment descriptors || the fixed-size part || quotient sets, answers, answer polynomials | index lists | payloads
    // the fixed-size part (it comes back in the first copy):
    //   sponge | roots | scalars in transcript order | out-of-domain values | sampled indices | indices without repeats | (u, k) per tree |
    //   final polynomial | interpolation status | lengths of the authentication structures | directory
    const size_t w_jobs = (size_t)n_trees * sizeof(AuthJob) / sizeof(u64), w_segments = (size_t)n_segments * sizeof(TailSegment) / sizeof(u64);
    const size_t o_roots = 16, o_scalars = o_roots + 5 * (size_t)n_trees, o_oodv = o_scalars + s.n_scalar_words(), o_raw = o_oodv + 3 * s.n_ood_all,
                 o_unique = o_raw + s.n_queries_all, o_counts = o_unique + s.n_queries_all, o_final = o_counts + 2 * (size_t)n_trees,
                 o_status = o_final + 3 * s.n_final, o_auth_counts = o_status + 1, o_directory = o_auth_counts + n_trees,
                 w_fixed = o_directory + 2 * (size_t)n_segments;
    const size_t w_sets = 9 * k_max_all, w_small = w_jobs + w_segments + w_fixed + w_sets;
    PoolBlock block(c, (w_small + (size_t)n_trees * auth_stride + bound + 1) * sizeof(u64));
    u64* d = (u64*)block.p;
    if (!d) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "tvm_stir_prove_rounds staging");
    u64 *d_fixed = d + w_jobs + w_segments, *d_state = d_fixed, *d_sets = d_fixed + w_fixed, *d_auth = d + w_small,
        *d_payload = d_auth + (size_t)n_trees * auth_stride;
    // what lives as long as the call: the trees (all of them are answered at the end), the codewords under them, the polynomials
    std::vector<PoolBlock*> owned;
    struct Owned {
        std::vector<PoolBlock*>& v;
        ~Owned() { for (PoolBlock* b : v) delete b; }
    } release{owned};
    auto alloc = [&](u64 words) -> u64* {
        owned.push_back(new PoolBlock(c, (size_t)std::max<u64>(words, 1) * sizeof(u64)));
        return (u64*)owned.back()->p;
    };
    // the work domain's values and the answer polynomial's (tvm_stir_next_polynomial): the first round's are the longest
    const u64 work_max = R ? pow2_at_least((s.L + ff - 1) / ff, 1) : 1;
    u64 *d_vals = alloc(3 * work_max), *d_ans_values = alloc(3 * work_max);
    if (!d_vals || !d_ans_values) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "tvm_stir_prove_rounds scratch");

    // From here on work is queued that reads or writes the blocks and the locals below: every way out synchronises the stream first
    std::vector<u64> host(w_jobs + w_segments + 1), fixed(w_fixed);
    auto leave = [&](int rc) {
        if (hipStreamSynchronize(c->stream) != hipSuccess && rc == TVM_OK) rc = set_error(c, TVM_ERR_DEVICE, "tvm_stir_prove_rounds");
        return rc;
    };
    auto launched = [&](const char* what) { return hipGetLastError() == hipSuccess ? TVM_OK : set_error(c, TVM_ERR_DEVICE, what); };
#define STIR_STEP(expr)                            \
    do {                                           \
        const int rc_ = (expr);                    \
        if (rc_ != TVM_OK) return leave(rc_);      \
    } while (0)
    if (hipMemsetAsync(d_fixed, 0, (w_fixed + w_sets) * sizeof(u64), c->stream) != hipSuccess)   // the status, the padding of the answer polynomials
        return leave(set_error(c, TVM_ERR_DEVICE, "tvm_stir_prove_rounds memset"));
    STIR_STEP(h2d_small(c, d_state, h_state, 16 * sizeof(u64)));

    AuthJob* jobs = (AuthJob*)host.data();
    TailSegment* segments = (TailSegment*)(host.data() + w_jobs);
    auto sponge = [&](const StirSpongeArgs& g) {
        TVM_LAUNCH(k_stir_sponge, dim3(1), dim3(64), 0, c->stream, g);
        return launched("stir sponge launch");
    };
    std::vector<u64> at_queries(n_trees, 0);   // where tree t's sampled indices (and those without repeats) start in their arrays
    for (u32 t = 1; t < n_trees; t++) at_queries[t] = at_queries[t - 1] + s.queries[t - 1];
    // tree t over `cw` (domain of length(t)): its root into the sponge, then n_scalars scalars; the response is planned for the end
    auto commit = [&](u32 t, const u64* cw, u32 n_scalars, u64* d_scalars) {
        const u64 n_leaves = s.n_leaves(t);
        u64* nodes = alloc(10 * n_leaves);
        if (!nodes) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "tvm_stir_prove_rounds tree");
        TVM_TRY(tvm_stir_merkle_tree(c, cw, s.length(t), (uint32_t)ff, nodes));
        StirSpongeArgs g = {};
        g.state = d_state, g.root = nodes + 5, g.root_out = d_fixed + o_roots + 5 * (size_t)t, g.n_scalars = n_scalars, g.scalars = d_scalars;
        TVM_TRY(sponge(g));
        const u64 *d_list = d_fixed + o_unique + at_queries[t], *d_u = d_fixed + o_counts + 2 * (size_t)t;
        jobs[t] = AuthJob{d_list, n_leaves, 0, d_auth + (size_t)t * auth_stride, nullptr, nullptr, s.queries[t], d_u};
        segments[2 * t] = TailSegment{cw, n_leaves - 1, 0, 0, t, d_list, d_u, n_leaves, (u32)ff};   // StirMerkleTree: entries n_leaves apart
        segments[2 * t + 1] = TailSegment{nodes, 0, 0, 1, t, nullptr, nullptr, 0, 0};
        return (int)TVM_OK;
    };
    auto fold = [&](const u64* poly, u64 n_coeffs, const u64* d_r, u64* out) {
        const u64 n_out = (n_coeffs + ff - 1) / ff;
        TVM_LAUNCH(k_fold_polynomial_dev, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, c->stream, poly, n_coeffs, (int)ff, d_r, n_out, out);
        return launched("stir fold launch");
    };
    auto query_set = [&](StirQuerySetArgs g, u32 t) {
        g.raw = d_fixed + o_raw + at_queries[t], g.n_raw = (u32)s.queries[t], g.unique = d_fixed + o_unique + at_queries[t];
        g.counts = d_fixed + o_counts + 2 * (size_t)t;
        TVM_LAUNCH(k_stir_query_set, dim3(1), dim3((unsigned)pow2_at_least(s.queries[t], 64)), 0, c->stream, g);
        return launched("stir query set launch");
    };

    tvm_domain domain = dom;
    u64* d_scalar = d_fixed + o_scalars;   // the next word of the scalars
    STIR_STEP(commit(0, d_codeword, 1, d_scalar));   // ... and the first folding randomness
    u64* poly = alloc(3 * s.L);
    if (!poly) return leave(set_error(c, TVM_ERR_OUT_OF_MEMORY, "tvm_stir_prove_rounds polynomial"));
    STIR_STEP(tvm_interpolate(c, 3, d_codeword, domain, poly));
    u64 n_coeffs = s.L, at_ood = 0, at_sets = 0;
    for (u32 r = 0; r < R; r++) {
        const u64 n_in = s.queries[r], n_ood = s.ood[r], k_max = n_in + n_ood, n_folded = (n_coeffs + ff - 1) / ff;
        const u64 *d_fold_r = d_scalar, *d_ood_points = d_scalar + 3;
        u64 *d_degree_correction = d_scalar + 3 + 3 * n_ood, *d_ood_values = d_fixed + o_oodv + 3 * at_ood;
        u64 *d_set = d_sets + at_sets, *d_answers = d_set + 3 * k_max, *d_answer_poly = d_answers + 3 * k_max;
        // stir.rs:1149-1155: the next round's domain; stir.rs:929: the folded domain
        const tvm_domain next = {bfe_mul(bfe_mul(domain.offset, domain.offset), domain.offset), bfe_mul(domain.generator, domain.generator), domain.length / 2};
        const tvm_domain folded_domain = {bfe_pow(domain.offset, ff), bfe_pow(domain.generator, ff), domain.length / ff};
        // (the folded polynomial and its values on the folded domain live for this round only: back to the pool, whose reuse is stream-ordered)
        PoolBlock folded_block(c, 3 * (size_t)n_folded * sizeof(u64)), on_folded_block(c, 3 * (size_t)folded_domain.length * sizeof(u64));
        u64 *folded = (u64*)folded_block.p, *next_cw = alloc(3 * next.length), *on_folded = (u64*)on_folded_block.p;
        if (!folded || !next_cw || !on_folded) return leave(set_error(c, TVM_ERR_OUT_OF_MEMORY, "tvm_stir_prove_rounds round"));
        STIR_STEP(fold(poly, n_coeffs, d_fold_r, folded));
        STIR_STEP(tvm_evaluate(c, 3, folded, n_folded, next, next_cw));
        STIR_STEP(commit(r + 1, next_cw, (u32)n_ood, (u64*)d_ood_points));   // launch one: the root, the out-of-domain points
        if (n_ood) STIR_STEP(poly_eval(c, folded, n_folded, d_ood_points, (int)n_ood, d_ood_values));
        StirSpongeArgs g = {};   // launch two: the values, the indices, the degree-correction and the next folding randomness
        g.state = d_state, g.absorb_values = 1, g.values = d_ood_values, g.n_values = (u32)n_ood;
        g.n_indices = (u32)n_in, g.mask = domain.length - 1, g.indices = d_fixed + o_raw + at_queries[r];
        g.n_single = 2, g.singles = d_degree_correction;
        STIR_STEP(sponge(g));
        STIR_STEP(tvm_evaluate(c, 3, folded, n_folded, folded_domain, on_folded));
        StirQuerySetArgs q = {};
        q.n_ood = (u32)n_ood, q.folded_mask = folded_domain.length - 1, q.offset = folded_domain.offset, q.gen = folded_domain.generator;
        q.ood_points = d_ood_points, q.ood_values = d_ood_values, q.on_folded_domain = on_folded, q.set = d_set, q.answers = d_answers;
        STIR_STEP(query_set(q, r));
        const u64* d_counts = d_fixed + o_counts + 2 * (size_t)r;
        TVM_LAUNCH(k_xfe_interpolate_dev, dim3(1), dim3(256), 0, c->stream, (const u64*)d_set, (const u64*)d_answers, d_counts, d_answer_poly,
                   (int*)(d_fixed + o_status));
        STIR_STEP(launched("stir interpolation launch"));
        // the witness polynomial of the next round (tvm_stir_next_polynomial, capi.hip), with k and the randomness on the device: the
        // answer polynomial is zero-padded to k_max coefficients, and whether it is transformed or evaluated by Horner's rule is decided
        // on k_max -- the arithmetic is exact, the words are the same either way
        const u64 M = pow2_at_least(n_folded, 1);
        const tvm_domain work = {bfe_mul(folded_domain.offset, bfe_from_u64(7)), bfe_pow(bfe_from_u64(7), (TVM_P - 1) / M), M};
        STIR_STEP(tvm_evaluate(c, 3, folded, n_folded, work, d_vals));
        const bool transform = k_max >= 32 && k_max <= M;
        if (transform) STIR_STEP(tvm_evaluate(c, 3, d_answer_poly, k_max, work, d_ans_values));
        StirQuotientArgs a = {};
        a.vals = d_vals, a.n = M, a.offset = work.offset, a.gen = work.generator, a.points = d_set, a.answer = d_answer_poly;
        a.answer_values = transform ? d_ans_values : nullptr;
        TVM_LAUNCH(k_stir_quotient_dev, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->stream, a, d_counts, (const u64*)d_degree_correction);
        STIR_STEP(launched("stir quotient launch"));
        u64* next_poly = alloc(3 * M);
        if (!next_poly) return leave(set_error(c, TVM_ERR_OUT_OF_MEMORY, "tvm_stir_prove_rounds polynomial"));
        STIR_STEP(tvm_interpolate(c, 3, d_vals, work, next_poly));
        poly = next_poly, n_coeffs = n_folded, domain = next;
        d_scalar = d_degree_correction + 3, at_ood += n_ood, at_sets += 9 * k_max;
    }
    {   // the final round has no quotienting (stir.rs:975-992)
        u64* d_final = d_fixed + o_final;
        STIR_STEP(fold(poly, n_coeffs, d_scalar, d_final));
        StirSpongeArgs g = {};
        g.state = d_state, g.polynomial = d_final, g.n_coefficients = (u32)s.n_final;
        g.n_indices = (u32)final_queries, g.mask = domain.length - 1, g.indices = d_fixed + o_raw + at_queries[R];
        STIR_STEP(sponge(g));
        StirQuerySetArgs q = {};
        q.folded_mask = domain.length / ff - 1;
        STIR_STEP(query_set(q, R));
    }
    // StirMerkleTree::inclusion_proof for all R + 1 trees: the stacked leaves at the indices without repeats and the authentication
    // structures, in proof-item order (leaves, structure per tree)
    STIR_STEP(h2d_small(c, d, host.data(), (w_jobs + w_segments) * sizeof(u64)));   // (`host` is a local: every way out synchronises)
    STIR_STEP(authentication_structures_launch(c, (const AuthJob*)d, n_trees, most, d_fixed + o_auth_counts));
    TailGatherArgs tg = {};
    tg.segments = (const TailSegment*)(d + w_jobs), tg.auth_idx = d_auth, tg.auth_counts = d_fixed + o_auth_counts, tg.auth_stride = auth_stride;
    tg.out = d_payload, tg.directory = d_fixed + o_directory;
    STIR_STEP(tail_gather_launch(c, tg, n_segments));
#undef STIR_STEP

    // first round trip: what has a fixed size
    int rc = TVM_OK;
    if (hipMemcpyAsync(fixed.data(), d_fixed, w_fixed * sizeof(u64), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = set_error(c, TVM_ERR_DEVICE, "tvm_stir_prove_rounds download");
    if ((rc = leave(rc)) != TVM_OK) return rc;
    if (fixed[o_status]) return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_stir_prove_rounds: STIR quotient set has repeated points");
    const u64* directory = fixed.data() + o_directory;
    const u64 total = directory[2 * (n_segments - 1)] + directory[2 * (n_segments - 1) + 1];
    if (total > bound) return set_error(c, TVM_ERR_DEVICE, "tvm_stir_prove_rounds: payloads longer than their bound");
    *payload_words = total;
    if (total > payload_capacity) return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_stir_prove_rounds: payload capacity");
    std::memcpy(h_state_out, fixed.data(), 16 * sizeof(u64));
    std::memcpy(h_roots, fixed.data() + o_roots, 5 * (size_t)n_trees * sizeof(u64));
    std::memcpy(h_scalars, fixed.data() + o_scalars, s.n_scalar_words() * sizeof(u64));
    if (s.n_ood_all) std::memcpy(h_ood_values, fixed.data() + o_oodv, 3 * s.n_ood_all * sizeof(u64));
    std::memcpy(h_indices, fixed.data() + o_raw, s.n_queries_all * sizeof(u64));
    std::memcpy(h_unique, fixed.data() + o_unique, s.n_queries_all * sizeof(u64));
    for (u32 t = 0; t < n_trees; t++) h_unique_counts[t] = fixed[o_counts + 2 * (size_t)t];
    std::memcpy(h_final_polynomial, fixed.data() + o_final, 3 * s.n_final * sizeof(u64));
    std::memcpy(h_directory, directory, 2 * (size_t)n_segments * sizeof(u64));
    // second round trip: exactly the words the proof holds
    if (total && hipMemcpyAsync(h_payload, d_payload, total * sizeof(u64), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = set_error(c, TVM_ERR_DEVICE, "tvm_stir_prove_rounds payload download");
    return leave(rc);
}
}  // extern "C"
