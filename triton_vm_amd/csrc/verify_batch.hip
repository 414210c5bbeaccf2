// verify_batch.hip -- the verifier's device work for MANY proofs per launch (tvmh_verify_batch, host/verify_batch.cpp).
//
// A verification is a chain of latency kernels (verify.hip, verify_ldt.hip): a few hundred work-items each, one launch and one
// stream synchronisation per entry point.  The device work of a proof is microseconds, the round trips are milliseconds, and no
// device result ever reaches the Fiat-Shamir sponge -- so a host that verifies many proofs walks all transcripts first and then
// runs each stage ONCE for all of them.  The entry points here are the stages that assume one domain, one set of challenges or one
// set of weights per launch in their one-proof form; each takes "groups" (a proof, or a STIR round of a proof) with their own:
//   tvm_verifier_fri_folds_batch      one work-item per (group, check), groups found through a prefix table of check counts
//   tvm_verifier_fri_last_rounds      one workgroup per group: the last codeword's Merkle root and its interpolant at one point
//   tvm_xfe_interpolate_batch         one workgroup per group: stir_kernels.h's one-workgroup interpolation with a grid dimension
//   tvm_verifier_stir_answers_batch   one workgroup per (group, query)
//   tvm_verifier_deep_values_batch    one workgroup per (group, row)
// (tvm_verifier_row_digests and tvm_verifier_merkle_roots take rows and trees from anywhere already.)  The per-query bodies are
// those of the one-proof kernels (verify_kernels.h): a batched kernel only looks its argument struct up in a descriptor table.
// One staging block, one launch and one synchronisation per call; a malformed group is a per-group flag (1), a group beyond a
// kernel's bound is flagged TVM_NOT_APPLICABLE, and nothing is written for either.
#include <cstring>
#include <vector>

#include "context.h"
#include "kernels.h"
#include "stir_kernels.h"
#include "tip5.h"
#include "verify_kernels.h"

namespace tvm {

// the group of global item t: the largest g with prefix[g] <= t (prefix[0] = 0, prefix[n_groups] = the number of items > t;
// groups without items have prefix[g] == prefix[g + 1] and are never the answer)
TVM_D u32 vb_group_of(const u64* __restrict__ prefix, u32 n_groups, u64 t) {
    u32 lo = 0, hi = n_groups;
    while (hi - lo > 1) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (prefix[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------------------------- FRI folds
// descriptor: offset, generator, length, n_rounds, base -- the group's words from `data + base`: idx [q], a [q][3],
// b [n_rounds][q][3], challenges [n_rounds][3].  out: [all checks][3] in group order.
#define FB_DESC 5
__global__ void __launch_bounds__(256) k_verifier_fri_folds_batch(const u64* __restrict__ desc, const u64* __restrict__ prefix, u32 n_groups,
                                                                  const u64* __restrict__ data, u64* __restrict__ out) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= prefix[n_groups]) return;
    const u32 grp = vb_group_of(prefix, n_groups, t);   // (a group boundary may fall anywhere inside a wavefront)
    const u64* d = desc + FB_DESC * (u64)grp;
    FriFoldArgs g;
    g.offset = d[0], g.gen = d[1], g.len = d[2], g.n_rounds = (u32)d[3], g.q = prefix[grp + 1] - prefix[grp];
    g.idx = data + d[4], g.a = g.idx + g.q, g.b = g.a + 3 * g.q, g.challenges = g.b + 3 * g.q * g.n_rounds;
    g.out = out + 3 * prefix[grp];
    verifier_fri_fold_query(g, t - prefix[grp]);
}

// ---------------------------------------------------------------------------------------------- FRI last rounds
// One workgroup per group.  (a) The Merkle tree over the last codeword (leaves Digest::from(xfe), fri.rs:343-347): the levels
// in the group's node array [2 L][5] in global memory, sixteen lanes per pair as in k_verifier_merkle_roots, the levels
// separated by workgroup barriers.  (b) The interpolant over the L-th roots of unity (offset one: ArithmeticDomain::of_length)
// at the point x, as a barycentric sum:  P(x) = (x^L - 1) / L * sum_i y_i w^i / (x - w^i);  P(x) = y_i where x = w^i.  The
// same field element as interpolating and evaluating the coefficients, since the interpolant is unique.
// descriptor: L, w, codeword base (words), node base (nodes of 5 words)
#define LR_BLOCK 1024
#define LR_DESC 4
__global__ void __launch_bounds__(LR_BLOCK) k_verifier_fri_last_rounds(const u64* __restrict__ desc, const u64* __restrict__ data,
                                                                       const u64* __restrict__ points, u64* __restrict__ nodes_all,
                                                                       u64* __restrict__ out) {
    __shared__ unsigned char lut[256];
    __shared__ u64 red[3 * LR_BLOCK];
    __shared__ u64 hit;   // i + 1 where x = w^i
    tip5_stage_lut(lut, threadIdx.x, blockDim.x);
    const u64* d = desc + LR_DESC * (u64)blockIdx.x;
    const u64 L = d[0], w = d[1];
    const u64* cw = data + d[2];
    u64* nodes = nodes_all + 5 * d[3];
    const u32 tid = threadIdx.x;
    if (!tid) hit = 0;
    for (u64 i = tid; i < L; i += LR_BLOCK) {
        u64* leaf = nodes + 5 * (L + i);
        leaf[0] = cw[3 * i], leaf[1] = cw[3 * i + 1], leaf[2] = cw[3 * i + 2], leaf[3] = 0, leaf[4] = 0;
    }
    __syncthreads();
    const int pos = (int)(tid & 15), lane = (int)(tid & 63);
    for (u64 m = L >> 1; m >= 1; m >>= 1) {   // the parents m .. 2 m - 1
        for (u64 r = 0; r < m; r += LR_BLOCK / 16) {
            // (a wavefront without a pair sits the round out; one with fewer than four clamps the rest: every lane joins the rotations)
            if (r + ((tid & ~63u) >> 4) < m) {
                u64 i = r + (tid >> 4);
                const bool live = i < m;
                if (!live) i = m - 1;
                u64 v = TVM_ONE;  // fixed-length domain: capacity all ones (tip-0005.md:82)
                if (pos < 10) v = nodes[5 * (2 * (m + i)) + pos];   // the children 2 p, 2 p + 1 lie side by side
                v = tip5_permute_lanes(v, pos, lane, lut);
                if (live && pos < 5) nodes[5 * (m + i) + pos] = v;
            }
        }
        __syncthreads();  // the same workgroup wrote the children of the next level: workgroup-scope visibility suffices
    }
    const xfe x = vl_ld(points + 3 * (u64)blockIdx.x);
    xfe acc = xfe_zero();
    const u64 step = bfe_pow(w, LR_BLOCK);
    u64 wi = bfe_pow(w, (u64)tid);
    for (u64 i = tid; i < L; i += LR_BLOCK, wi = bfe_mul(wi, step)) {
        const xfe den = xfe_sub_bfe(x, wi);
        if (xfe_eq(den, xfe_zero())) hit = i + 1;   // at most one i: the w^i are pairwise distinct
        else acc = xfe_add(acc, xfe_mul(xfe_mul_bfe(vl_ld(cw + 3 * i), wi), xfe_inv(den)));
    }
    red[tid] = acc.c0, red[LR_BLOCK + tid] = acc.c1, red[2 * LR_BLOCK + tid] = acc.c2;
    __syncthreads();
    for (u32 s = LR_BLOCK >> 1; s > 0; s >>= 1) {
        if (tid < s)
            for (int k = 0; k < 3; k++) red[k * LR_BLOCK + tid] = bfe_add(red[k * LR_BLOCK + tid], red[k * LR_BLOCK + tid + s]);
        __syncthreads();
    }
    u64* o = out + 8 * (u64)blockIdx.x;   // root [5], value [3]
    if (tid < 5) o[tid] = nodes[5 + tid];
    if (tid) return;
    xfe value;
    if (hit) value = vl_ld(cw + 3 * (hit - 1));
    else {
        const xfe zerofier = xfe_sub_bfe(xfe_pow(x, L), TVM_ONE);
        value = xfe_mul(xfe_mul_bfe(zerofier, bfe_inv(bfe_from_u64(L))), xfe_make(red[0], red[LR_BLOCK], red[2 * LR_BLOCK]));
    }
    vl_st(o + 5, value);
}

// ---------------------------------------------------------------------------------------------- interpolation
// descriptor: k, base -- points [k][3] then values [k][3] from `data + base`, the coefficients [k][3] to `out + base / 2`
#define IB_DESC 2
__global__ void __launch_bounds__(256) k_xfe_interpolate_batch(const u64* __restrict__ desc, const u64* __restrict__ data,
                                                               u64* __restrict__ out, int* __restrict__ status) {
    const u64* d = desc + IB_DESC * (u64)blockIdx.x;
    const int k = (int)d[0];
    xfe_interpolate_workgroup(data + d[1], data + d[1] + 3 * (u64)k, k, out + d[1] / 2, status + blockIdx.x);
}

// ---------------------------------------------------------------------------------------------- STIR in-domain answers
// descriptor: folding factor, k, kth_root, base -- from `data + base`: folding randomness [3], degree-correction randomness [3],
// quotient set [k][3], answer polynomial [k][3], coset roots [q], values [q][ff][3].  out: [all queries][3] in group order.
#define AB_DESC 4
__global__ void __launch_bounds__(SA_BLOCK) k_verifier_stir_answers_batch(const u64* __restrict__ desc, const u64* __restrict__ prefix,
                                                                          u32 n_groups, const u64* __restrict__ data, u64* __restrict__ out) {
    const u64 t = blockIdx.x;
    const u32 grp = vb_group_of(prefix, n_groups, t);
    const u64* d = desc + AB_DESC * (u64)grp;
    StirAnswerArgs g;
    g.ff = (u32)d[0], g.k = (u32)d[1], g.kth_root = d[2];
    g.small = data + d[3], g.qset = g.small + 6, g.ans = g.qset + 3 * (u64)g.k, g.roots = g.ans + 3 * (u64)g.k;
    g.values = g.roots + (prefix[grp + 1] - prefix[grp]);
    g.out = out + 3 * prefix[grp];
    verifier_stir_answer_query(g, t - prefix[grp]);
}

// ---------------------------------------------------------------------------------------------- DEEP values
// descriptor: the LDT domain's offset and generator, base -- from `data + base`: the weights of the main and auxiliary columns
// [470][3], then the 51 small words of VerifyArgs, the row indices [q], main rows [q][379], auxiliary rows [q][91][3], quotient
// segment rows [q][5][3].  out: [all rows][3] in group order.
#define DB_DESC 3
__global__ void __launch_bounds__(VF_BLOCK) k_verifier_deep_values_batch(const u64* __restrict__ desc, const u64* __restrict__ prefix,
                                                                         u32 n_groups, const u64* __restrict__ data, u64* __restrict__ out) {
    const u64 t = blockIdx.x;
    const u32 grp = vb_group_of(prefix, n_groups, t);
    const u64* d = desc + DB_DESC * (u64)grp;
    const u64 q = prefix[grp + 1] - prefix[grp];
    VerifyArgs a;
    a.offset = d[0], a.gen = d[1], a.n_main = TVM_NUM_MAIN_COLUMNS, a.n_aux = TVM_NUM_AUX_COLUMNS;
    a.w_ma = data + d[2], a.small = a.w_ma + 3 * (TVM_NUM_MAIN_COLUMNS + TVM_NUM_AUX_COLUMNS), a.row_idx = a.small + 51;
    a.main_rows = a.row_idx + q, a.aux_rows = a.main_rows + q * TVM_NUM_MAIN_COLUMNS, a.quot_rows = a.aux_rows + q * 3 * TVM_NUM_AUX_COLUMNS;
    a.out = out + 3 * prefix[grp];
    verifier_deep_values_row(a, t - prefix[grp]);
}

namespace {
// One staging block: [host words | room for `out_words` results (| `work_words` of scratch)].  up(): the host words to the device;
// down(): the results back and the call's ONE synchronisation.  `host` lives until down() returns.
struct Staged {
    tvm_ctx* c;
    const char* what;
    std::vector<u64> host;
    PoolBlock block;
    u64 *d = nullptr, *d_out = nullptr, *d_work = nullptr;
    Staged(tvm_ctx* c_, const char* what_) : c(c_), what(what_), block(c_) {}
    size_t put(const u64* words, size_t n) {   // -> the word offset
        const size_t at = host.size();
        host.insert(host.end(), words, words + n);
        return at;
    }
    int up(size_t out_words, size_t work_words = 0) {
        d = (u64*)block.alloc((host.size() + out_words + work_words + 1) * sizeof(u64));
        if (!d) return set_error(c, TVM_ERR_OUT_OF_MEMORY, what);
        d_out = d + host.size(), d_work = d_out + out_words;
        if (hipMemcpyAsync(d, host.data(), host.size() * sizeof(u64), hipMemcpyHostToDevice, c->stream) != hipSuccess) {
            (void)hipStreamSynchronize(c->stream);
            return set_error(c, TVM_ERR_DEVICE, what);
        }
        return TVM_OK;
    }
    int down(std::vector<u64>& results, size_t out_words) {
        int rc = TVM_OK;
        results.resize(out_words);
        if (hipGetLastError() != hipSuccess) rc = set_error(c, TVM_ERR_DEVICE, what);
        if (rc == TVM_OK && out_words &&
            hipMemcpyAsync(results.data(), d_out, out_words * sizeof(u64), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            rc = set_error(c, TVM_ERR_DEVICE, what);
        if (hipStreamSynchronize(c->stream) != hipSuccess && rc == TVM_OK) rc = set_error(c, TVM_ERR_DEVICE, what);
        return rc;
    }
};
bool canonical(const u64* w, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (w[i] >= TVM_P) return false;
    return true;
}
const u64 VB_MAX_ITEMS = 1ull << 30;   // work-items or workgroups of one launch
}  // namespace

}  // namespace tvm

extern "C" {
using namespace tvm;

int32_t tvm_verifier_fri_folds_batch(tvm_ctx* c, uint32_t n_groups, const tvm_domain* first_domains, const uint32_t* n_rounds,
                                     const uint64_t* n_checks, const uint64_t* const* h_challenges, const uint64_t* const* h_indices,
                                     const uint64_t* const* h_a_leaves, const uint64_t* const* h_b_leaves, uint64_t* const* h_out,
                                     uint32_t* h_flags) {
    if (!c || !n_groups || !first_domains || !n_rounds || !n_checks || !h_challenges || !h_indices || !h_a_leaves || !h_b_leaves || !h_out || !h_flags)
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_verifier_fri_folds_batch arguments");
    Staged s(c, "tvm_verifier_fri_folds_batch");
    std::vector<u64> prefix(n_groups + 1, 0), desc((size_t)FB_DESC * n_groups, 0);
    for (uint32_t g = 0; g < n_groups; g++) {   // the conditions of tvm_verifier_fri_folds, per group
        const tvm_domain dom = first_domains[g];
        const u64 q = n_checks[g];
        const uint32_t r = n_rounds[g];
        bool ok = q && q <= TVM_VERIFIER_MAX_QUERIES && h_indices[g] && h_a_leaves[g] && h_out[g] && (!r || (h_challenges[g] && h_b_leaves[g])) &&
                  is_pow2(dom.length) && dom.generator < TVM_P && dom.offset < TVM_P && r <= 63 && (!r || (dom.length >> (r - 1)) >= 2);
        for (u64 j = 0; ok && j < q; j++) ok = h_indices[g][j] < dom.length;
        h_flags[g] = ok ? 0 : 1;
        prefix[g + 1] = prefix[g] + (ok ? q : 0);
    }
    const u64 total = prefix[n_groups];
    if (total > VB_MAX_ITEMS) return set_error(c, TVM_ERR_UNSUPPORTED, "tvm_verifier_fri_folds_batch: more than 2^30 checks in one call");
    if (!total) return TVM_OK;
    size_t words = prefix.size() + desc.size();
    for (uint32_t g = 0; g < n_groups; g++)
        if (!h_flags[g]) words += (size_t)n_checks[g] * (4 + 3 * (size_t)n_rounds[g]) + 3 * (size_t)n_rounds[g];
    s.host.reserve(words);
    s.host.resize(prefix.size() + desc.size());
    for (uint32_t g = 0; g < n_groups; g++) {
        if (h_flags[g]) continue;
        const size_t q = (size_t)n_checks[g], r = n_rounds[g];
        u64* d = &desc[(size_t)FB_DESC * g];
        d[0] = first_domains[g].offset, d[1] = first_domains[g].generator, d[2] = first_domains[g].length, d[3] = r;
        d[4] = s.put(h_indices[g], q);
        s.put(h_a_leaves[g], 3 * q);
        if (r) s.put(h_b_leaves[g], 3 * q * r), s.put(h_challenges[g], 3 * r);
    }
    std::memcpy(s.host.data(), prefix.data(), prefix.size() * sizeof(u64));
    std::memcpy(s.host.data() + prefix.size(), desc.data(), desc.size() * sizeof(u64));
    TVM_TRY(s.up(3 * (size_t)total));
    const u64 *d_in = s.d, *d_desc = s.d + prefix.size();   // (named: the emulation's launch captures its arguments by value)
    u64* d_out = s.d_out;
    TVM_LAUNCH(k_verifier_fri_folds_batch, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, d_desc, d_in, n_groups, d_in, d_out);
    std::vector<u64> out;
    TVM_TRY(s.down(out, 3 * (size_t)total));
    for (uint32_t g = 0; g < n_groups; g++)
        if (!h_flags[g]) std::memcpy(h_out[g], &out[3 * prefix[g]], 3 * (size_t)n_checks[g] * sizeof(u64));
    return TVM_OK;
}

int32_t tvm_verifier_fri_last_rounds(tvm_ctx* c, uint32_t n_groups, const uint64_t* lengths, const uint64_t* const* h_codewords,
                                     const uint64_t* h_points, uint64_t* h_roots, uint64_t* h_values, uint32_t* h_flags) {
    if (!c || !n_groups || !lengths || !h_codewords || !h_points || !h_roots || !h_values || !h_flags)
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_verifier_fri_last_rounds arguments");
    Staged s(c, "tvm_verifier_fri_last_rounds");
    std::vector<uint32_t> live;
    std::vector<u64> desc, points;
    u64 n_nodes = 0;
    for (uint32_t g = 0; g < n_groups; g++) {
        const u64 L = lengths[g];
        if (!is_pow2(L) || !h_codewords[g] || (L <= TVM_VERIFIER_MAX_LAST_CODEWORD && !canonical(h_codewords[g], 3 * (size_t)L)) ||
            !canonical(h_points + 3 * (size_t)g, 3))
            h_flags[g] = 1;
        else if (L > TVM_VERIFIER_MAX_LAST_CODEWORD) h_flags[g] = TVM_NOT_APPLICABLE;
        else h_flags[g] = 0, live.push_back(g);
        if (h_flags[g]) continue;
        const u64 w = bfe_pow(bfe_from_u64(7), (TVM_P - 1) / L);   // BFieldElement::primitive_root_of_unity(L)
        const u64 words[LR_DESC] = {L, w, 0, n_nodes};
        desc.insert(desc.end(), words, words + LR_DESC);
        points.insert(points.end(), h_points + 3 * (size_t)g, h_points + 3 * (size_t)g + 3);
        n_nodes += 2 * L;
    }
    if (live.empty()) return TVM_OK;
    if (n_nodes > VB_MAX_ITEMS) return set_error(c, TVM_ERR_UNSUPPORTED, "tvm_verifier_fri_last_rounds: more than 2^29 codeword elements in one call");
    s.host = desc;
    const size_t points_at = s.put(points.data(), points.size());
    for (size_t i = 0; i < live.size(); i++) s.host[LR_DESC * i + 2] = s.put(h_codewords[live[i]], 3 * (size_t)lengths[live[i]]);
    TVM_TRY(s.up(8 * live.size(), 5 * (size_t)n_nodes));
    const u64 *d_in = s.d, *d_points = s.d + points_at;
    u64 *d_nodes = s.d_work, *d_out = s.d_out;
    TVM_LAUNCH(k_verifier_fri_last_rounds, dim3((unsigned)live.size()), dim3(LR_BLOCK), 0, c->stream, d_in, d_in, d_points, d_nodes, d_out);
    std::vector<u64> out;
    TVM_TRY(s.down(out, 8 * live.size()));
    for (size_t i = 0; i < live.size(); i++) {
        std::memcpy(h_roots + 5 * (size_t)live[i], &out[8 * i], 5 * sizeof(u64));
        std::memcpy(h_values + 3 * (size_t)live[i], &out[8 * i + 5], 3 * sizeof(u64));
    }
    return TVM_OK;
}

int32_t tvm_xfe_interpolate_batch(tvm_ctx* c, uint32_t n_groups, const uint32_t* k, const uint64_t* const* h_points,
                                  const uint64_t* const* h_values, uint64_t* const* h_out_coeffs, uint32_t* h_flags) {
    if (!c || !n_groups || !k || !h_points || !h_values || !h_out_coeffs || !h_flags)
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_xfe_interpolate_batch arguments");
    Staged s(c, "tvm_xfe_interpolate_batch");
    std::vector<uint32_t> live;
    for (uint32_t g = 0; g < n_groups; g++) {
        if (k[g] && (!h_points[g] || !h_values[g] || !h_out_coeffs[g])) h_flags[g] = 1;
        else if (k[g] > 256) h_flags[g] = TVM_NOT_APPLICABLE;   // the limit of the one-workgroup interpolation
        else if (k[g] && !(canonical(h_points[g], 3 * (size_t)k[g]) && canonical(h_values[g], 3 * (size_t)k[g]))) h_flags[g] = 1;
        else {
            h_flags[g] = 0;
            if (k[g]) live.push_back(g);
        }
    }
    if (live.empty()) return TVM_OK;
    // descriptors (an even number of words) | per group: points, values
    s.host.assign((size_t)IB_DESC * live.size(), 0);
    for (size_t i = 0; i < live.size(); i++) {
        const uint32_t g = live[i];
        s.host[IB_DESC * i] = k[g];
        s.host[IB_DESC * i + 1] = s.put(h_points[g], 3 * (size_t)k[g]);
        s.put(h_values[g], 3 * (size_t)k[g]);
    }
    // results: coefficients at half the group's base (every group's base is even and its input twice its output), then the status words
    const size_t coeff_words = s.host.size() / 2 + 1, status_words = (live.size() + 1) / 2;
    TVM_TRY(s.up(coeff_words + status_words));
    int* d_status = (int*)(s.d_out + coeff_words);
    if (hipMemsetAsync(d_status, 0, status_words * sizeof(u64), c->stream) != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        return set_error(c, TVM_ERR_DEVICE, "tvm_xfe_interpolate_batch");
    }
    const u64* d_in = s.d;
    u64* d_out = s.d_out;
    TVM_LAUNCH(k_xfe_interpolate_batch, dim3((unsigned)live.size()), dim3(256), 0, c->stream, d_in, d_in, d_out, d_status);
    std::vector<u64> out;
    TVM_TRY(s.down(out, coeff_words + status_words));
    const int* status = (const int*)(out.data() + coeff_words);
    for (size_t i = 0; i < live.size(); i++) {
        const uint32_t g = live[i];
        if (status[i]) h_flags[g] = 1;   // a repeated point
        else std::memcpy(h_out_coeffs[g], &out[s.host[IB_DESC * i + 1] / 2], 3 * (size_t)k[g] * sizeof(u64));
    }
    return TVM_OK;
}

int32_t tvm_verifier_stir_answers_batch(tvm_ctx* c, uint32_t n_groups, const uint32_t* folding_factors, const uint64_t* kth_roots,
                                        const uint64_t* h_folding_randomness, const uint32_t* k, const uint64_t* const* h_quotient_sets,
                                        const uint64_t* const* h_answer_polynomials, const uint64_t* h_degree_correction_randomness,
                                        const uint64_t* n_queries, const uint64_t* const* h_values, const uint64_t* const* h_coset_roots,
                                        uint64_t* const* h_out, uint32_t* h_flags) {
    if (!c || !n_groups || !folding_factors || !kth_roots || !h_folding_randomness || !k || !h_quotient_sets || !h_answer_polynomials ||
        !h_degree_correction_randomness || !n_queries || !h_values || !h_coset_roots || !h_out || !h_flags)
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_verifier_stir_answers_batch arguments");
    Staged s(c, "tvm_verifier_stir_answers_batch");
    std::vector<u64> prefix(n_groups + 1, 0), desc((size_t)AB_DESC * n_groups, 0);
    for (uint32_t g = 0; g < n_groups; g++) {   // the conditions of tvm_verifier_stir_answers, per group
        const u64 q = n_queries[g];
        const uint32_t ff = folding_factors[g];
        bool ok = q && q <= TVM_VERIFIER_MAX_QUERIES && h_values[g] && h_coset_roots[g] && h_out[g] && kth_roots[g] < TVM_P && ff >= 1 &&
                  ff <= SA_MAX_FF && k[g] <= TVM_VERIFIER_MAX_QUOTIENT_SET && (!k[g] || (h_quotient_sets[g] && h_answer_polynomials[g]));
        u64 w = TVM_ONE;  // the coset's points must be pairwise distinct, and none of them zero
        for (uint32_t j = 1; ok && j < ff; j++) ok = (w = bfe_mul(w, kth_roots[g])) != TVM_ONE;
        for (u64 j = 0; ok && j < q; j++) ok = h_coset_roots[g][j] && h_coset_roots[g][j] < TVM_P;
        h_flags[g] = ok ? 0 : 1;
        prefix[g + 1] = prefix[g] + (ok ? q : 0);
    }
    const u64 total = prefix[n_groups];
    if (total > VB_MAX_ITEMS) return set_error(c, TVM_ERR_UNSUPPORTED, "tvm_verifier_stir_answers_batch: more than 2^30 queries in one call");
    if (!total) return TVM_OK;
    size_t words = prefix.size() + desc.size();
    for (uint32_t g = 0; g < n_groups; g++)
        if (!h_flags[g]) words += 6 + 6 * (size_t)k[g] + (size_t)n_queries[g] * (1 + 3 * (size_t)folding_factors[g]);
    s.host.reserve(words);
    s.host.resize(prefix.size() + desc.size());
    const u64 zeros[3] = {0, 0, 0};
    for (uint32_t g = 0; g < n_groups; g++) {
        if (h_flags[g]) continue;
        const size_t q = (size_t)n_queries[g], ff = folding_factors[g], kk = k[g];
        u64* d = &desc[(size_t)AB_DESC * g];
        d[0] = ff, d[1] = kk, d[2] = kth_roots[g];
        d[3] = s.put(h_folding_randomness + 3 * (size_t)g, 3);
        s.put(kk ? h_degree_correction_randomness + 3 * (size_t)g : zeros, 3);
        if (kk) s.put(h_quotient_sets[g], 3 * kk), s.put(h_answer_polynomials[g], 3 * kk);
        s.put(h_coset_roots[g], q);
        s.put(h_values[g], 3 * q * ff);
    }
    std::memcpy(s.host.data(), prefix.data(), prefix.size() * sizeof(u64));
    std::memcpy(s.host.data() + prefix.size(), desc.data(), desc.size() * sizeof(u64));
    TVM_TRY(s.up(3 * (size_t)total));
    const u64 *d_in = s.d, *d_desc = s.d + prefix.size();
    u64* d_out = s.d_out;
    TVM_LAUNCH(k_verifier_stir_answers_batch, dim3((unsigned)total), dim3(SA_BLOCK), 0, c->stream, d_desc, d_in, n_groups, d_in, d_out);
    std::vector<u64> out;
    TVM_TRY(s.down(out, 3 * (size_t)total));
    for (uint32_t g = 0; g < n_groups; g++)
        if (!h_flags[g]) std::memcpy(h_out[g], &out[3 * prefix[g]], 3 * (size_t)n_queries[g] * sizeof(u64));
    return TVM_OK;
}

int32_t tvm_verifier_deep_values_batch(tvm_ctx* c, uint32_t n_groups, const tvm_domain* ldt_domains, const uint64_t* const* h_weights_main_aux,
                                       const uint64_t* h_weights_quot, const uint64_t* h_weights_deep, const uint64_t* h_ood_points,
                                       const uint64_t* h_ood_values, const uint64_t* n_rows, const uint64_t* const* h_main_rows,
                                       const uint64_t* const* h_aux_rows, const uint64_t* const* h_quot_rows,
                                       const uint64_t* const* h_row_indices, uint64_t* const* h_out, uint32_t* h_flags) {
    if (!c || !n_groups || !ldt_domains || !h_weights_main_aux || !h_weights_quot || !h_weights_deep || !h_ood_points || !h_ood_values || !n_rows ||
        !h_main_rows || !h_aux_rows || !h_quot_rows || !h_row_indices || !h_out || !h_flags)
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_verifier_deep_values_batch arguments");
    Staged s(c, "tvm_verifier_deep_values_batch");
    std::vector<u64> prefix(n_groups + 1, 0), desc((size_t)DB_DESC * n_groups, 0);
    for (uint32_t g = 0; g < n_groups; g++) {   // the conditions of tvm_verifier_deep_values, per group
        const u64 q = n_rows[g];
        bool ok = q && q <= TVM_VERIFIER_MAX_QUERIES && h_weights_main_aux[g] && h_main_rows[g] && h_aux_rows[g] && h_quot_rows[g] &&
                  h_row_indices[g] && h_out[g] && valid_domain(ldt_domains[g]);
        for (u64 j = 0; ok && j < q; j++) ok = h_row_indices[g][j] < ldt_domains[g].length;
        h_flags[g] = ok ? 0 : 1;
        prefix[g + 1] = prefix[g] + (ok ? q : 0);
    }
    const u64 total = prefix[n_groups];
    if (total > VB_MAX_ITEMS) return set_error(c, TVM_ERR_UNSUPPORTED, "tvm_verifier_deep_values_batch: more than 2^30 rows in one call");
    if (!total) return TVM_OK;
    // (reserved at its final size: a staging array that grows by doubling copies itself and faults its pages in again each time)
    s.host.reserve(prefix.size() + desc.size() + (size_t)n_groups * (3 * (TVM_NUM_MAIN_COLUMNS + TVM_NUM_AUX_COLUMNS) + 51) +
                   (size_t)total * (1 + TVM_NUM_MAIN_COLUMNS + 3 * TVM_NUM_AUX_COLUMNS + 15));
    s.host.resize(prefix.size() + desc.size());
    for (uint32_t g = 0; g < n_groups; g++) {
        if (h_flags[g]) continue;
        const size_t q = (size_t)n_rows[g];
        u64* d = &desc[(size_t)DB_DESC * g];
        d[0] = ldt_domains[g].offset, d[1] = ldt_domains[g].generator;
        d[2] = s.put(h_weights_main_aux[g], 3 * (TVM_NUM_MAIN_COLUMNS + TVM_NUM_AUX_COLUMNS));
        s.put(h_weights_quot + 15 * (size_t)g, 15), s.put(h_weights_deep + 12 * (size_t)g, 12);
        s.put(h_ood_points + 12 * (size_t)g, 12), s.put(h_ood_values + 12 * (size_t)g, 12);
        s.put(h_row_indices[g], q);
        s.put(h_main_rows[g], q * TVM_NUM_MAIN_COLUMNS), s.put(h_aux_rows[g], q * 3 * TVM_NUM_AUX_COLUMNS), s.put(h_quot_rows[g], q * 15);
    }
    std::memcpy(s.host.data(), prefix.data(), prefix.size() * sizeof(u64));
    std::memcpy(s.host.data() + prefix.size(), desc.data(), desc.size() * sizeof(u64));
    TVM_TRY(s.up(3 * (size_t)total));
    const u64 *d_in = s.d, *d_desc = s.d + prefix.size();
    u64* d_out = s.d_out;
    TVM_LAUNCH(k_verifier_deep_values_batch, dim3((unsigned)total), dim3(VF_BLOCK), 0, c->stream, d_desc, d_in, n_groups, d_in, d_out);
    std::vector<u64> out;
    TVM_TRY(s.down(out, 3 * (size_t)total));
    for (uint32_t g = 0; g < n_groups; g++)
        if (!h_flags[g]) std::memcpy(h_out[g], &out[3 * prefix[g]], 3 * (size_t)n_rows[g] * sizeof(u64));
    return TVM_OK;
}
}  // extern "C"
