// verify_ldt.hip -- the verifier's batch work outside the revealed rows: Merkle inclusion for all trees of a proof, the FRI
// collinearity folds, the in-domain answers of a STIR round.  (verify.hip has the work over the revealed rows.)
//
// A translation unit of its own, entry points included: nothing is added to the code objects of hash.hip, verify.hip or capi.hip
// (merkle_subtrees.hip records what a kernel added to hash.hip cost the row hashing).
//
// Replaces, in Verifier::verify (/root/reference/triton-vm/src/stark.rs:1388-1763) and the low-degree tests it calls:
//   MerkleTreeInclusionProof::verify [twenty-first] for the three row openings (stark.rs:1592-1672), every FRI round
//   (fri.rs:430-560) and every STIR round (stir.rs:1157-1226)                                  -> tvm_verifier_merkle_roots
//   the collinearity checks of all FRI rounds, Polynomial::get_colinear_y (fri.rs:520-560)     -> tvm_verifier_fri_folds
//   initial_in_domain_answers / subsequent_in_domain_answers (stir.rs:1259-1340)               -> tvm_verifier_stir_answers
// These are latency kernels: a few hundred queries, dependent tree levels.  What a verification costs is the number of dependent
// launches and stream synchronisations, so each entry point is ONE launch and ONE synchronisation however many trees, rounds or
// queries it is given.  The decisions (root comparison, agreement with the last codeword) stay with the caller.
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "context.h"
#include "kernels.h"
#include "tip5.h"
#include "verify_kernels.h"

namespace tvm {

// ---------------------------------------------------------------------------------------------- partial Merkle trees
// One workgroup per tree.  The plan -- which node is a revealed leaf, which comes from the authentication structure, which is the
// hash of a pair below -- depends on the public indices only and is made on the host (plan_job); the device only hashes.  A node is a
// "slot": slots below n_init are the job's given digests (deduplicated leaves, then the authentication structure) in `init`, the
// others are computed nodes in `work`.  An op is (left slot, right slot, slot of the parent); the ops of a level are independent, the
// levels are separated by workgroup barriers.  Sixteen lanes per pair (tip5_permute_lanes), 64 pairs per round of the workgroup.
#define MR_BLOCK 1024
#define MR_JOB_WORDS 8   // init_base, n_init, work_base, op_base, level_base, n_levels, root_slot, malformed
__global__ void __launch_bounds__(MR_BLOCK) k_verifier_merkle_roots(const u32* __restrict__ jobs, const u32* __restrict__ level_end,
                                                                    const u32* __restrict__ ops, const u64* __restrict__ init,
                                                                    u64* __restrict__ work, u64* __restrict__ roots) {
    __shared__ unsigned char lut[256];
    tip5_stage_lut(lut, threadIdx.x, blockDim.x);
    const u32* job = jobs + MR_JOB_WORDS * (u64)blockIdx.x;
    const u32 n_init = job[1], n_levels = job[5], root = job[6];
    const u64* ini = init + 5 * (u64)job[0];
    u64* wrk = work + 5 * (u64)job[2];
    const u32* op = ops + 3 * (u64)job[3];
    const u32* ends = level_end + job[4];
    const int pos = (int)(threadIdx.x & 15), lane = (int)(threadIdx.x & 63);
    u32 begin = 0;
    for (u32 l = 0; l < n_levels; l++) {
        const u32 end = ends[l];
        for (u32 r = begin; r < end; r += MR_BLOCK / 16) {
            // (a wavefront without a pair sits the round out; one with fewer than four clamps the rest: every lane joins the rotations)
            if (r + ((threadIdx.x & ~63u) >> 4) < end) {
                u32 i = r + (threadIdx.x >> 4);
                const bool live = i < end;
                if (!live) i = end - 1;
                u64 x = TVM_ONE;  // fixed-length domain: capacity all ones (tip-0005.md:82)
                if (pos < 10) {
                    const u32 s = op[3 * (u64)i + (pos >= 5 ? 1 : 0)];
                    const u64* src = s < n_init ? ini + 5 * (u64)s : wrk + 5 * (u64)(s - n_init);
                    x = src[pos >= 5 ? pos - 5 : pos];
                }
                x = tip5_permute_lanes(x, pos, lane, lut);
                if (live && pos < 5) wrk[5 * (u64)(op[3 * (u64)i + 2] - n_init) + pos] = x;
            }
        }
        begin = end;
        __syncthreads();  // the same workgroup wrote the children of the next level: workgroup-scope visibility suffices
    }
    if (threadIdx.x < 5) {
        u64 v = 0;
        if (!job[7]) v = root < n_init ? ini[5 * (u64)root + threadIdx.x] : wrk[5 * (u64)(root - n_init) + threadIdx.x];
        roots[5 * (u64)blockIdx.x + threadIdx.x] = v;
    }
}

namespace {
struct MerklePlan {
    std::vector<u64> init;                 // [slots][5]
    std::vector<u32> jobs, level_end, ops; // [n_jobs][MR_JOB_WORDS], level ends per job, [n_ops][3]
    u64 work_slots = 0;
};

// [twenty-first MerkleTreeInclusionProof::verify, restated as a plan]  false: the job is malformed (what it added is taken back).
bool plan_job(u64 n_leaves, const u64* idx, u64 q, const u64* leaves, u64 n_auth, const u64* auth, MerklePlan& P, u32* job) {
    const size_t init0 = P.init.size(), ops0 = P.ops.size(), levels0 = P.level_end.size();
    auto fail = [&]() {
        P.init.resize(init0), P.ops.resize(ops0), P.level_end.resize(levels0);
        return false;
    };
    if (!q) return fail();
    std::vector<std::pair<u64, u64>> order(q);  // (leaf index, position in the query list)
    for (u64 i = 0; i < q; i++) {
        if (idx[i] >= n_leaves) return fail();
        order[i] = {idx[i], i};
    }
    std::sort(order.begin(), order.end());
    std::vector<std::pair<u64, u32>> level;  // (heap index, slot), ascending
    for (u64 i = 0; i < q; i++) {
        const u64* d = leaves + 5 * order[i].second;
        if (i && order[i].first == order[i - 1].first) {  // a repeated index must repeat its digest
            if (std::memcmp(d, leaves + 5 * order[i - 1].second, 5 * sizeof(u64))) return fail();
            continue;
        }
        level.push_back({n_leaves + order[i].first, (u32)level.size()});
        P.init.insert(P.init.end(), d, d + 5);
    }
    const u32 n_init = (u32)(level.size() + n_auth);
    P.init.insert(P.init.end(), auth, auth + 5 * n_auth);
    // the authentication structure is in descending heap order: level by level from the leaves, descending inside a level
    u64 auth_used = 0;
    u32 next_slot = n_init, n_levels = 0, op_count = 0;
    std::vector<std::pair<u64, u32>> parents;
    while (level[0].first > 1) {
        const size_t m = level.size();
        u64 needed = 0;
        for (size_t i = 0; i < m; i++) {
            const u64 k = level[i].first;
            const bool sibling_known = (k & 1) ? (i > 0 && level[i - 1].first == k - 1) : (i + 1 < m && level[i + 1].first == k + 1);
            if (!sibling_known) needed++;
        }
        if (auth_used + needed > n_auth) return fail();  // a missing sibling
        parents.clear();
        u64 rank = 0;  // among this level's needed siblings in ASCENDING order; its place in the structure counts from the other end
        for (size_t i = 0; i < m; i++) {
            const u64 k = level[i].first;
            u32 left, right;
            if (!(k & 1) && i + 1 < m && level[i + 1].first == k + 1) {
                left = level[i].second, right = level[i + 1].second;
                i++;
            } else {
                const u32 sibling = (u32)(n_init - n_auth + auth_used + (needed - 1 - rank));
                rank++;
                if (k & 1) left = sibling, right = level[i].second;
                else left = level[i].second, right = sibling;
            }
            P.ops.push_back(left), P.ops.push_back(right), P.ops.push_back(next_slot);
            parents.push_back({k >> 1, next_slot++});
            op_count++;
        }
        auth_used += needed;
        P.level_end.push_back(op_count);
        n_levels++;
        level.swap(parents);
    }
    if (auth_used != n_auth) return fail();  // superfluous nodes
    job[1] = n_init, job[5] = n_levels, job[6] = level[0].second, job[7] = 0;
    P.work_slots += next_slot - n_init;
    return true;
}
}  // namespace

// ---------------------------------------------------------------------------------------------- FRI folds, STIR answers
// The bodies, their argument structs and block sizes: verify_kernels.h (shared with verify_batch.hip).
__global__ void __launch_bounds__(256) k_verifier_fri_folds(FriFoldArgs g) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= g.q) return;
    verifier_fri_fold_query(g, j);
}
__global__ void __launch_bounds__(SA_BLOCK) k_verifier_stir_answers(StirAnswerArgs g) { verifier_stir_answer_query(g, blockIdx.x); }

}  // namespace tvm

extern "C" {
using namespace tvm;

int32_t tvm_verifier_merkle_roots(tvm_ctx* c, uint32_t n_jobs, const uint64_t* n_leaves, const uint64_t* n_indices,
                                  const uint64_t* const* h_indices, const uint64_t* const* h_leaf_digests, const uint64_t* n_auth,
                                  const uint64_t* const* h_auth, uint64_t* h_roots, uint32_t* h_flags) {
    if (!c || !n_jobs || !n_leaves || !n_indices || !h_indices || !h_leaf_digests || !n_auth || !h_auth || !h_roots || !h_flags)
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_verifier_merkle_roots arguments");
    if (n_jobs > TVM_VERIFIER_MAX_TREES) return set_error(c, TVM_ERR_UNSUPPORTED, "tvm_verifier_merkle_roots: too many trees");
    for (uint32_t j = 0; j < n_jobs; j++) {
        if (!is_pow2(n_leaves[j]) || (n_indices[j] && (!h_indices[j] || !h_leaf_digests[j])) || (n_auth[j] && !h_auth[j]))
            return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_verifier_merkle_roots: tree size not a power of two, or a null job");
        if (n_leaves[j] > TVM_VERIFIER_MAX_LEAVES || n_indices[j] > TVM_VERIFIER_MAX_QUERIES || n_auth[j] > 64 * TVM_VERIFIER_MAX_QUERIES)
            return set_error(c, TVM_ERR_UNSUPPORTED, "tvm_verifier_merkle_roots: beyond 2^40 leaves, 2^16 indices or 2^22 nodes per tree");
    }
    MerklePlan P;
    P.jobs.assign((size_t)n_jobs * MR_JOB_WORDS, 0);
    for (uint32_t j = 0; j < n_jobs; j++) {
        u32* job = P.jobs.data() + (size_t)j * MR_JOB_WORDS;
        const u64 init_base = P.init.size() / 5, work_base = P.work_slots, op_base = P.ops.size() / 3, level_base = P.level_end.size();
        if ((init_base | work_base | op_base | level_base) >> 31)
            return set_error(c, TVM_ERR_UNSUPPORTED, "tvm_verifier_merkle_roots: more than 2^31 nodes in one call");
        job[0] = (u32)init_base, job[2] = (u32)work_base, job[3] = (u32)op_base, job[4] = (u32)level_base;
        h_flags[j] = plan_job(n_leaves[j], h_indices[j], n_indices[j], h_leaf_digests[j], n_auth[j], h_auth[j], P, job) ? 0 : 1;
        if (h_flags[j]) job[1] = job[5] = job[6] = 0, job[7] = 1;
    }
    // one staging block: given digests | job descriptors | level ends | ops (32-bit words, padded to whole 64-bit words)
    const size_t w_init = P.init.size(), w_jobs = P.jobs.size() / 2, w_levels = (P.level_end.size() + 1) / 2, w_ops = (P.ops.size() + 1) / 2;
    std::vector<u64> host(w_init + w_jobs + w_levels + w_ops + 1, 0);
    if (w_init) std::memcpy(host.data(), P.init.data(), w_init * sizeof(u64));
    std::memcpy(host.data() + w_init, P.jobs.data(), P.jobs.size() * sizeof(u32));
    if (!P.level_end.empty()) std::memcpy(host.data() + w_init + w_jobs, P.level_end.data(), P.level_end.size() * sizeof(u32));
    if (!P.ops.empty()) std::memcpy(host.data() + w_init + w_jobs + w_levels, P.ops.data(), P.ops.size() * sizeof(u32));
    PoolBlock staged(c, host.size() * sizeof(u64)), work(c, (size_t)(5 * P.work_slots + 1) * sizeof(u64)), out(c, (size_t)5 * n_jobs * sizeof(u64));
    if (!staged.p || !work.p || !out.p) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "tvm_verifier_merkle_roots staging");
    u64 *d = (u64*)staged.p, *d_work = (u64*)work.p, *d_roots = (u64*)out.p;
    const u32 *d_jobs = (const u32*)(d + w_init), *d_levels = (const u32*)(d + w_init + w_jobs), *d_ops = (const u32*)(d + w_init + w_jobs + w_levels);
    int rc = TVM_OK;
    if (hipMemcpyAsync(d, host.data(), host.size() * sizeof(u64), hipMemcpyHostToDevice, c->stream) != hipSuccess)
        rc = set_error(c, TVM_ERR_DEVICE, "merkle roots upload");
    if (rc == TVM_OK) {
        TVM_LAUNCH(k_verifier_merkle_roots, dim3(n_jobs), dim3(MR_BLOCK), 0, c->stream, d_jobs, d_levels, d_ops, (const u64*)d, d_work, d_roots);
        if (hipGetLastError() != hipSuccess) rc = set_error(c, TVM_ERR_DEVICE, "merkle roots launch");
    }
    if (rc == TVM_OK && hipMemcpyAsync(h_roots, d_roots, (size_t)5 * n_jobs * sizeof(u64), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = set_error(c, TVM_ERR_DEVICE, "merkle roots download");
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == TVM_OK) rc = set_error(c, TVM_ERR_DEVICE, "merkle roots");  // `host` is a local
    return rc;
}

int32_t tvm_verifier_fri_folds(tvm_ctx* c, tvm_domain first_domain, uint32_t n_rounds, const uint64_t* h_challenges,
                               const uint64_t* h_indices, uint64_t n_checks, const uint64_t* h_a_leaves, const uint64_t* h_b_leaves,
                               uint64_t* h_out) {
    if (!c || !n_checks || !h_indices || !h_a_leaves || !h_out || (n_rounds && (!h_challenges || !h_b_leaves)) ||
        !is_pow2(first_domain.length) || first_domain.generator >= TVM_P || first_domain.offset >= TVM_P || n_rounds > 63 ||
        (n_rounds && (first_domain.length >> (n_rounds - 1)) < 2))
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_verifier_fri_folds arguments");
    if (n_checks > TVM_VERIFIER_MAX_QUERIES) return set_error(c, TVM_ERR_UNSUPPORTED, "tvm_verifier_fri_folds: more than 2^16 queries");
    for (u64 j = 0; j < n_checks; j++)
        if (h_indices[j] >= first_domain.length) return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_verifier_fri_folds: index out of range");
    const size_t q = (size_t)n_checks, w_b = 3 * q * n_rounds, total = q + 3 * q + w_b + 3 * (size_t)n_rounds;
    std::vector<u64> host(total + 1);
    u64* p = host.data();
    std::memcpy(p, h_indices, q * 8); p += q;
    std::memcpy(p, h_a_leaves, 3 * q * 8); p += 3 * q;
    if (n_rounds) std::memcpy(p, h_b_leaves, w_b * 8), std::memcpy(p + w_b, h_challenges, 3 * (size_t)n_rounds * 8);
    PoolBlock block(c, (total + 1 + 3 * q) * sizeof(u64));
    u64* d = (u64*)block.p;
    if (!d) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "tvm_verifier_fri_folds staging");
    int rc = TVM_OK;
    if (hipMemcpyAsync(d, host.data(), total * sizeof(u64), hipMemcpyHostToDevice, c->stream) != hipSuccess)
        rc = set_error(c, TVM_ERR_DEVICE, "fri folds upload");
    FriFoldArgs g;
    g.idx = d, g.a = d + q, g.b = d + 4 * q, g.challenges = d + 4 * q + w_b, g.out = d + total + 1;
    g.offset = first_domain.offset, g.gen = first_domain.generator, g.len = first_domain.length, g.q = n_checks, g.n_rounds = n_rounds;
    if (rc == TVM_OK) {
        TVM_LAUNCH(k_verifier_fri_folds, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, c->stream, g);
        if (hipGetLastError() != hipSuccess) rc = set_error(c, TVM_ERR_DEVICE, "fri folds launch");
    }
    if (rc == TVM_OK && hipMemcpyAsync(h_out, g.out, 3 * q * sizeof(u64), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = set_error(c, TVM_ERR_DEVICE, "fri folds download");
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == TVM_OK) rc = set_error(c, TVM_ERR_DEVICE, "fri folds");
    return rc;
}

int32_t tvm_verifier_stir_answers(tvm_ctx* c, uint32_t folding_factor, uint64_t n_queries, const uint64_t* h_values,
                                  const uint64_t* h_coset_roots, uint64_t kth_root, const uint64_t* h_folding_randomness,
                                  uint32_t k, const uint64_t* h_quotient_set, const uint64_t* h_answer_polynomial,
                                  const uint64_t* h_degree_correction_randomness, uint64_t* h_out) {
    if (!c || !n_queries || !h_values || !h_coset_roots || !h_folding_randomness || !h_out || kth_root >= TVM_P ||
        (k && (!h_quotient_set || !h_answer_polynomial || !h_degree_correction_randomness)))
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_verifier_stir_answers arguments");
    if (folding_factor < 1 || folding_factor > SA_MAX_FF || n_queries > TVM_VERIFIER_MAX_QUERIES || k > TVM_VERIFIER_MAX_QUOTIENT_SET)
        return set_error(c, TVM_ERR_UNSUPPORTED, "tvm_verifier_stir_answers: folding factor above 16, more than 2^16 queries or 2^20 quotient points");
    u64 w = TVM_ONE;  // the coset's points must be pairwise distinct, and none of them zero
    for (uint32_t j = 1; j < folding_factor; j++)
        if ((w = bfe_mul(w, kth_root)) == TVM_ONE) return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_verifier_stir_answers: kth_root of too small an order");
    for (u64 j = 0; j < n_queries; j++)
        if (!h_coset_roots[j] || h_coset_roots[j] >= TVM_P) return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_verifier_stir_answers: coset root");
    const size_t q = (size_t)n_queries, ff = folding_factor, total = 3 * q * ff + q + 6 + 6 * (size_t)k;
    std::vector<u64> host(total, 0);
    u64* p = host.data();
    std::memcpy(p, h_values, 3 * q * ff * 8); p += 3 * q * ff;
    std::memcpy(p, h_coset_roots, q * 8); p += q;
    std::memcpy(p, h_folding_randomness, 24);
    if (k) std::memcpy(p + 3, h_degree_correction_randomness, 24), std::memcpy(p + 6, h_quotient_set, 24 * (size_t)k),
        std::memcpy(p + 6 + 3 * (size_t)k, h_answer_polynomial, 24 * (size_t)k);
    PoolBlock block(c, (total + 3 * q) * sizeof(u64));
    u64* d = (u64*)block.p;
    if (!d) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "tvm_verifier_stir_answers staging");
    int rc = TVM_OK;
    if (hipMemcpyAsync(d, host.data(), total * sizeof(u64), hipMemcpyHostToDevice, c->stream) != hipSuccess)
        rc = set_error(c, TVM_ERR_DEVICE, "stir answers upload");
    StirAnswerArgs g;
    g.values = d, g.roots = d + 3 * q * ff, g.small = g.roots + q, g.qset = g.small + 6, g.ans = g.qset + 3 * (size_t)k;
    g.kth_root = kth_root, g.k = k, g.ff = folding_factor, g.out = d + total;
    if (rc == TVM_OK) {
        TVM_LAUNCH(k_verifier_stir_answers, dim3((unsigned)q), dim3(SA_BLOCK), 0, c->stream, g);
        if (hipGetLastError() != hipSuccess) rc = set_error(c, TVM_ERR_DEVICE, "stir answers launch");
    }
    if (rc == TVM_OK && hipMemcpyAsync(h_out, g.out, 3 * q * sizeof(u64), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = set_error(c, TVM_ERR_DEVICE, "stir answers download");
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == TVM_OK) rc = set_error(c, TVM_ERR_DEVICE, "stir answers");
    return rc;
}
}  // extern "C"
