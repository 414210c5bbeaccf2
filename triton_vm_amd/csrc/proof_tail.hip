// proof_tail.hip -- the tail of a FRI proof with the transcript on the device: everything after the commit phase of Fri::prove
// and the trace openings of Prover::prove, queued on the stream with no host decision in between.
//
// A translation unit of its own, entry points included (as verify_ldt.hip: nothing is added to the code objects of hash.hip or capi.hip).
//
// Replaces, on the host's side of the reference's hot path:
//   ProofStream::enqueue(Polynomial) into the sponge, sample_indices           /root/reference/triton-vm/src/low_degree_test/fri.rs:265-293,
//                                                                               proof_stream.rs:54-59, 86-104     -> k_sponge_tail
//   MerkleTree::authentication_structure [twenty-first] for every round's tree and the three trace trees
//                                                     fri.rs:295-319, stark.rs:672-716             -> k_authentication_structures
//   the leaves, authentication nodes and opened rows those items hold                               -> k_tail_gather
// These are latency kernels: a few hundred indices, a few dozen dependent steps.  What they buy is the host round trips between them.
#include <algorithm>
#include <cstring>
#include <vector>

#include "context.h"
#include "kernels.h"
#include "tail_kernels.h"
#include "tip5.h"

namespace tvm {

// ---------------------------------------------------------------------------------------------- the sponge
// One wavefront; lanes 0..15 hold the sponge state, the other lanes follow along so that every lane joins the rotations of
// tip5_permute_lanes (as k_sponge_root_and_sample, hash.hip).  An item is a ProofItem that holds a Polynomial<XFieldElement> over a
// device array (ProofItem::Polynomial, FRI's last polynomial: of the items behind the commit phase the only one that
// ProofItem::include_in_fiat_shamir_heuristic admits, proof_item.rs:96-150 -- the last codeword, the responses and the openings go
// into the proof, not into the sponge); its encoding (BFieldCodec: triton_host.cpp, encode_item) is
//     [discriminant, 2 + 3n, 1 + 3n, n, the 3n words]     n: the coefficients once the trailing zeros are dropped
// padded with 1, 0, ... to whole blocks of the rate and absorbed in overwrite mode, each item on its own (proof_stream.rs:40-59).
struct SpongeTailArgs {
    u64* state;                       // [16], in and out
    const u64* polynomial;            // null: no item (tvm_sponge_sample_indices); else n_coefficients XFE
    u32 n_coefficients, discriminant;
    u32 n_indices;
    u64 mask;                         // upper_bound - 1 (a power of two)
    u64* indices;                     // [n_indices]
};
__global__ void __launch_bounds__(64) k_sponge_tail(SpongeTailArgs g) {
    __shared__ unsigned char lut[256];
    __shared__ u64 rate[TIP5_RATE];
    tip5_stage_lut(lut, threadIdx.x, blockDim.x);
    const int lane = (int)threadIdx.x, pos = lane & 15;
    u64 x = g.state[pos];
    if (g.polynomial) x = sponge_absorb_polynomial_lanes(x, pos, lane, lut, g.discriminant, g.polynomial, g.n_coefficients);
    x = sponge_sample_indices_lanes(x, pos, lane, lut, rate, g.n_indices, g.mask, g.indices);
    if (lane < 16) g.state[pos] = x;
}

// ---------------------------------------------------------------------------------------------- authentication structures
// One workgroup per tree, one leaf index per work-item.  The path nodes of a level are kept as a sorted, duplicate-free list in LDS:
// a node's sibling is needed unless it is a path node itself -- then it is the node's neighbour in the list --, and the parents of
// the list are the next level's list.  Both compactions of a level (the needed siblings, in descending order behind those of the
// levels below; the parents without repeats) come from ONE workgroup prefix sum over two packed 16-bit counters; no atomics.
// Deeper levels have the larger heap indices, so this order is the descending heap order of MerkleTree::authentication_structure
// (auth_node_indices, triton_host.cpp).
__global__ void __launch_bounds__(TVM_TAIL_MAX_INDICES) k_authentication_structures(const AuthJob* __restrict__ jobs, u64* __restrict__ counts) {
    __shared__ u64 key[TVM_TAIL_MAX_INDICES];
    __shared__ u32 wave_sums[TVM_TAIL_MAX_INDICES / 64];
    const AuthJob job = jobs[blockIdx.x];
    const u32 tid = threadIdx.x, nt = blockDim.x;   // nt: a power of two, at least n_idx
    const u64 n_idx = job.n_idx_device ? *job.n_idx_device : job.n_idx;
    key[tid] = tid < n_idx ? ((job.idx[tid] + job.add) & (job.n_leaves - 1)) + job.n_leaves : ~0ull;
    __syncthreads();
    for (u32 size = 2; size <= nt; size <<= 1)   // bitonic sort, ascending; the padding sorts to the end
        for (u32 j = size >> 1; j; j >>= 1) {
            const u32 partner = tid ^ j;
            if (partner > tid) {
                const u64 a = key[tid], b = key[partner];
                if ((a > b) == !(tid & size)) key[tid] = b, key[partner] = a;
            }
            __syncthreads();
        }
    u32 total, m;
    {   // without repeats
        const u64 x = key[tid];
        const bool first = tid < n_idx && (tid == 0 || key[tid - 1] != x);
        const u32 at = as_block_scan(first ? 1u : 0u, wave_sums, total);
        if (first) key[at - 1] = x;
        m = total;
        __syncthreads();
    }
    u64 n_out = 0;
    for (u64 width = job.n_leaves; width > 1; width >>= 1) {   // key[0..m): the path nodes of the level of `width` nodes
        const bool live = tid < m;
        const u64 x = live ? key[tid] : 0, sibling = x ^ 1;
        bool need = false, first = false;
        if (live) {
            need = (x & 1) ? !(tid > 0 && key[tid - 1] == sibling) : !(tid + 1 < m && key[tid + 1] == sibling);
            first = tid == 0 || (key[tid - 1] >> 1) != (x >> 1);
        }
        const u32 at = as_block_scan((need ? 1u : 0u) | (first ? 1u << 16 : 0u), wave_sums, total);   // (counts <= 1024: no carry)
        const u32 n_need = total & 0xFFFFu;
        if (need) job.out_idx[n_out + (n_need - (at & 0xFFFFu))] = sibling;   // this level's siblings in descending order
        if (first) key[(at >> 16) - 1] = x >> 1;
        n_out += n_need;
        m = total >> 16;
        __syncthreads();
    }
    if (tid == 0) counts[blockIdx.x] = n_out;
    if (job.nodes)   // (this workgroup wrote out_idx, and the barrier above carries a fence: workgroup-scope visibility suffices)
        for (u64 e = tid; e < 5 * n_out; e += nt) job.out_nodes[e] = job.nodes[5 * job.out_idx[e / 5] + e % 5];
}

// ---------------------------------------------------------------------------------------------- the payloads
// The payloads of the proof items behind the sampling, packed in proof-item order.  gridDim.y = the number of payloads ("segments"),
// gridDim.x workgroups share a segment's words.  A segment's offset is the sum of the lengths before it, and those of the
// authentication structures are only known on the device (counts of k_authentication_structures).
TVM_D u64 tg_words(const TailGatherArgs& g, const TailSegment& s) {
    return s.kind == 0 ? 3 * (u64)(s.stack ? s.stack : 1) * (s.count ? *s.count : g.n_checks) : s.kind == 1 ? 5 * g.auth_counts[s.which] : (u64)g.W[s.which] * g.n_checks;
}
__global__ void __launch_bounds__(256) k_tail_gather(TailGatherArgs g) {
    __shared__ u64 offset_s;
    const u32 seg = blockIdx.y;
    if (threadIdx.x == 0) {
        u64 offset = 0;
        for (u32 s = 0; s < seg; s++) offset += tg_words(g, g.segments[s]);
        offset_s = offset;
    }
    __syncthreads();
    const TailSegment s = g.segments[seg];
    const u64 words = tg_words(g, s);
    u64* out = g.out + offset_s;
    if (blockIdx.x == 0 && threadIdx.x == 0) g.directory[2 * seg] = offset_s, g.directory[2 * seg + 1] = words;
    for (u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x; e < words; e += (u64)gridDim.x * blockDim.x) {
        if (s.kind == 0) {   // element e / 3 = element `rest` of the stack at index `at`
            const u64 stack = s.stack ? s.stack : 1, at = e / (3 * stack), rest = e / 3 % stack;
            out[e] = s.src[3 * ((((s.idx ? s.idx : g.a)[at] + s.add) & s.mask) + rest * s.stride) + e % 3];
        } else if (s.kind == 1) {
            out[e] = s.src[5 * g.auth_idx[s.which * g.auth_stride + e / 5] + e % 5];
        } else {   // reveal_rows (k_gather_rows, hash.hip): domain row -> storage row of the row-block-major table
            const u64 W = g.W[s.which];
            const u64 row = g.layout[s.which].storage_row(g.a[e / W] * g.row_stride[s.which]);
            out[e] = s.src[tvm_tab_idx(row, e % W, W)];
        }
    }
}

namespace {
u32 pow2_ceil(u64 n) {
    u32 p = 64;
    while (p < n) p <<= 1;
    return p;
}
u64 responses(u32 n_rounds) { return n_rounds ? n_rounds + 1u : 1u; }
}  // namespace

int authentication_structures_launch(tvm_ctx* c, const AuthJob* d_jobs, u32 n_jobs, u64 most_indices, u64* d_counts) {
    TVM_LAUNCH(k_authentication_structures, dim3(n_jobs), dim3(pow2_ceil(most_indices)), 0, c->stream, d_jobs, d_counts);
    return hipGetLastError() == hipSuccess ? TVM_OK : set_error(c, TVM_ERR_DEVICE, "authentication structures launch");
}
int tail_gather_launch(tvm_ctx* c, const TailGatherArgs& g, u32 n_segments) {
    TVM_LAUNCH(k_tail_gather, dim3(16, n_segments), dim3(256), 0, c->stream, g);
    return hipGetLastError() == hipSuccess ? TVM_OK : set_error(c, TVM_ERR_DEVICE, "tail gather launch");
}

}  // namespace tvm

extern "C" {
using namespace tvm;

int32_t tvm_sponge_sample_indices(tvm_ctx* c, const uint64_t* h_state, uint64_t upper_bound, uint64_t n, uint64_t* h_indices_out,
                                  uint64_t* h_state_out) {
    if (!c || !h_state || !h_state_out || (n && !h_indices_out) || !is_pow2(upper_bound) || upper_bound > (1ull << 32) || n > TVM_VERIFIER_MAX_QUERIES)
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_sponge_sample_indices arguments");
    PoolBlock block(c, (16 + n + 1) * sizeof(u64));
    u64* d = (u64*)block.p;
    if (!d) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "tvm_sponge_sample_indices staging");
    TVM_TRY(h2d_small(c, d, h_state, 16 * sizeof(u64)));
    SpongeTailArgs g = {};
    g.state = d, g.indices = d + 16, g.n_indices = (u32)n, g.mask = upper_bound - 1;
    TVM_LAUNCH(k_sponge_tail, dim3(1), dim3(64), 0, c->stream, g);
    int rc = hipGetLastError() == hipSuccess ? TVM_OK : set_error(c, TVM_ERR_DEVICE, "sponge tail launch");
    if (rc == TVM_OK && (hipMemcpyAsync(h_state_out, d, 16 * sizeof(u64), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                         (n && hipMemcpyAsync(h_indices_out, d + 16, n * sizeof(u64), hipMemcpyDeviceToHost, c->stream) != hipSuccess)))
        rc = set_error(c, TVM_ERR_DEVICE, "sponge tail download");
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == TVM_OK) rc = set_error(c, TVM_ERR_DEVICE, "sponge tail");
    return rc;
}

int32_t tvm_authentication_structures(tvm_ctx* c, uint32_t n_trees, const uint64_t* n_leaves, const uint64_t* const* h_indices,
                                      const uint64_t* n_indices, const uint64_t* const* d_nodes, uint64_t* const* h_node_indices_out,
                                      uint64_t* const* h_nodes_out, uint64_t* n_out) {
    if (!c || !n_trees || !n_leaves || !h_indices || !n_indices || !h_node_indices_out || !n_out)
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_authentication_structures arguments");
    if (n_trees > TVM_VERIFIER_MAX_TREES) return set_error(c, TVM_ERR_UNSUPPORTED, "tvm_authentication_structures: too many trees");
    u64 n_idx_all = 0, n_out_all = 0, n_nodes_all = 0, most = 0;
    for (uint32_t j = 0; j < n_trees; j++) {
        if (!is_pow2(n_leaves[j]) || (n_indices[j] && !h_indices[j]))
            return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_authentication_structures: tree size not a power of two, or a null job");
        if (n_leaves[j] > TVM_VERIFIER_MAX_LEAVES) return set_error(c, TVM_ERR_UNSUPPORTED, "tvm_authentication_structures: beyond 2^40 leaves");
        if (n_indices[j] > TVM_TAIL_MAX_INDICES) return TVM_NOT_APPLICABLE;
        const u64 cap = auth_capacity(n_leaves[j], n_indices[j]);
        const bool gather = d_nodes && d_nodes[j];
        if (cap && (!h_node_indices_out[j] || (gather && (!h_nodes_out || !h_nodes_out[j]))))
            return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_authentication_structures: null output");
        for (u64 i = 0; i < n_indices[j]; i++)
            if (h_indices[j][i] >= n_leaves[j]) return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_authentication_structures: index out of range");
        n_idx_all += n_indices[j], n_out_all += cap, n_nodes_all += gather ? 5 * cap : 0;
        most = std::max<u64>(most, n_indices[j]);
    }
    // one block: job descriptors | leaf indices || counts | index lists | digests   (the part behind || comes back in one copy)
    const size_t w_jobs = (size_t)n_trees * sizeof(AuthJob) / sizeof(u64), w_in = w_jobs + n_idx_all, w_back = n_trees + n_out_all + n_nodes_all;
    PoolBlock block(c, (w_in + w_back + 1) * sizeof(u64));
    u64* d = (u64*)block.p;
    if (!d) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "tvm_authentication_structures staging");
    u64 *d_counts = d + w_in, *d_out_idx = d_counts + n_trees, *d_out_nodes = d_out_idx + n_out_all;
    std::vector<u64> host(w_in + 1), back(w_back + 1);
    AuthJob* jobs = (AuthJob*)host.data();
    u64 at_idx = w_jobs, at_out = 0, at_nodes = 0;
    for (uint32_t j = 0; j < n_trees; j++) {
        const u64 cap = auth_capacity(n_leaves[j], n_indices[j]);
        const bool gather = d_nodes && d_nodes[j];
        jobs[j] = AuthJob{d + at_idx, n_leaves[j], 0, d_out_idx + at_out, gather ? d_nodes[j] : nullptr, d_out_nodes + at_nodes, n_indices[j]};
        if (n_indices[j]) std::memcpy(host.data() + at_idx, h_indices[j], n_indices[j] * sizeof(u64));
        at_idx += n_indices[j], at_out += cap, at_nodes += gather ? 5 * cap : 0;
    }
    int rc = TVM_OK;
    if (hipMemcpyAsync(d, host.data(), w_in * sizeof(u64), hipMemcpyHostToDevice, c->stream) != hipSuccess)
        rc = set_error(c, TVM_ERR_DEVICE, "authentication structures upload");
    if (rc == TVM_OK) {
        rc = authentication_structures_launch(c, (const AuthJob*)d, n_trees, most, d_counts);
    }
    if (rc == TVM_OK && hipMemcpyAsync(back.data(), d_counts, w_back * sizeof(u64), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = set_error(c, TVM_ERR_DEVICE, "authentication structures download");
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == TVM_OK) rc = set_error(c, TVM_ERR_DEVICE, "authentication structures");  // `host` is a local
    if (rc != TVM_OK) return rc;
    at_out = at_nodes = 0;
    for (uint32_t j = 0; j < n_trees; j++) {
        const u64 cap = auth_capacity(n_leaves[j], n_indices[j]), n = back[j];
        const bool gather = d_nodes && d_nodes[j];
        if (n > cap) return set_error(c, TVM_ERR_DEVICE, "authentication structures: a list longer than its bound");
        n_out[j] = n;
        if (n) std::memcpy(h_node_indices_out[j], back.data() + n_trees + at_out, n * sizeof(u64));
        if (n && gather) std::memcpy(h_nodes_out[j], back.data() + n_trees + n_out_all + at_nodes, 5 * n * sizeof(u64));
        at_out += cap, at_nodes += gather ? 5 * cap : 0;
    }
    return TVM_OK;
}

uint64_t tvm_fri_query_and_open_payload_bound(tvm_domain domain, uint32_t n_rounds, uint64_t n_checks, const tvm_table* const* tables) {
    if (!is_pow2(domain.length) || n_rounds >= 64 || !tables) return 0;
    u64 words = 0;
    for (u64 k = 0; k < responses(n_rounds); k++) {
        const u64 n = domain.length >> (k ? k - 1 : 0);
        words += 3 * n_checks + 5 * auth_capacity(n, n_checks);
    }
    for (int t = 0; t < 3; t++) words += (tables[t] ? (u64)tables[t]->W : 0) * n_checks + 5 * auth_capacity(domain.length, n_checks);
    return words;
}

int32_t tvm_fri_query_and_open(tvm_ctx* c, const uint64_t* h_state, const uint64_t* d_cw, tvm_domain dom, uint32_t n_rounds,
                               const uint64_t* const* d_codewords, const uint64_t* const* d_nodes, uint64_t n_checks,
                               const tvm_table* const* tables, const uint64_t* const* d_table_nodes, uint64_t ldt_length,
                               uint64_t* h_state_out, uint64_t* h_indices_out, uint64_t* h_last_codeword, uint64_t* h_last_polynomial,
                               uint64_t* h_directory, uint64_t* h_payload, uint64_t payload_capacity, uint64_t* payload_words) {
    if (!c || !h_state || !d_cw || !d_nodes || !tables || !d_table_nodes || !h_state_out || !h_indices_out || !h_last_codeword ||
        !h_last_polynomial || !h_directory || !payload_words || (payload_capacity && !h_payload) || (n_rounds && !d_codewords) ||
        !is_pow2(dom.length) || dom.length > (1ull << 32) || dom.generator >= TVM_P || dom.offset >= TVM_P || n_rounds >= 64 ||
        (dom.length >> n_rounds) < 1 || !n_checks || ldt_length != dom.length)
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_fri_query_and_open arguments");
    for (uint32_t r = 0; r <= n_rounds; r++)
        if (!d_nodes[r] || (r < n_rounds && !d_codewords[r])) return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_fri_query_and_open: null buffer");
    for (int t = 0; t < 3; t++)
        if (!tables[t] || !d_table_nodes[t] || ldt_length > tables[t]->rows) return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_fri_query_and_open: tables");
    if (n_checks > TVM_TAIL_MAX_INDICES) return TVM_NOT_APPLICABLE;

    const u32 n_lists = (u32)responses(n_rounds), n_segments = TVM_TAIL_ITEMS(n_rounds);
    const u64 n_last = dom.length >> n_rounds, auth_stride = auth_capacity(dom.length, n_checks);
    const u64 bound = tvm_fri_query_and_open_payload_bound(dom, n_rounds, n_checks, tables);
    // one block: job and segment descriptors || sponge | counts | directory | a indices | last polynomial || index lists | payloads
    // (the part between the bars comes back in the first copy)
    const size_t w_jobs = (size_t)n_lists * sizeof(AuthJob) / sizeof(u64), w_segments = (size_t)n_segments * sizeof(TailSegment) / sizeof(u64);
    const size_t w_fixed = 16 + n_lists + 2 * (size_t)n_segments + n_checks + 3 * n_last;
    PoolBlock block(c, (w_jobs + w_segments + w_fixed + (size_t)n_lists * auth_stride + bound + 1) * sizeof(u64));
    u64* d = (u64*)block.p;
    if (!d) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "tvm_fri_query_and_open staging");
    u64 *d_fixed = d + w_jobs + w_segments, *d_state = d_fixed, *d_counts = d_state + 16, *d_directory = d_counts + n_lists,
        *d_a = d_directory + 2 * (size_t)n_segments, *d_poly = d_a + n_checks, *d_auth = d_fixed + w_fixed, *d_payload = d_auth + (size_t)n_lists * auth_stride;

    // list k: round 0 at the a indices, then round k - 1 at its b indices; segment pairs (leaves, nodes) in the same order
    std::vector<u64> host(w_jobs + w_segments + 1);
    AuthJob* jobs = (AuthJob*)host.data();
    TailSegment* segments = (TailSegment*)(host.data() + w_jobs);
    const u64* last_cw = d_cw;
    for (u32 k = 0; k < n_lists; k++) {
        const u32 r = k ? k - 1 : 0;
        const u64 n = dom.length >> r, add = k ? n / 2 : 0;
        const u64* cw = r ? d_codewords[r - 1] : d_cw;
        jobs[k] = AuthJob{d_a, n, add, d_auth + (size_t)k * auth_stride, nullptr, nullptr, n_checks};
        segments[2 * k] = TailSegment{cw, n - 1, add, 0, k};
        segments[2 * k + 1] = TailSegment{d_nodes[r], 0, 0, 1, k};
    }
    if (n_rounds) last_cw = d_codewords[n_rounds - 1];
    TailGatherArgs tg = {};
    for (u32 t = 0; t < 3; t++) {
        segments[2 * n_lists + 2 * t] = TailSegment{tables[t]->data, 0, 0, 2, t};
        segments[2 * n_lists + 2 * t + 1] = TailSegment{d_table_nodes[t], 0, 0, 1, 0};   // the trace trees share round 0's list at a
        tg.layout[t] = tables[t]->layout, tg.row_stride[t] = tables[t]->rows / ldt_length, tg.W[t] = (u32)tables[t]->W;
    }
    // From here on work is queued that reads or writes the block and the locals below: every way out synchronises the stream first
    // (as tvm_authentication_structures does).
    std::vector<u64> fixed(w_fixed);
    auto leave = [&](int rc) {
        if (hipStreamSynchronize(c->stream) != hipSuccess && rc == TVM_OK) rc = set_error(c, TVM_ERR_DEVICE, "tvm_fri_query_and_open");
        return rc;
    };
    int rc = h2d_small(c, d, host.data(), (w_jobs + w_segments) * sizeof(u64));   // (`host` is a local)
    if (rc == TVM_OK) rc = h2d_small(c, d_state, h_state, 16 * sizeof(u64));
    // the last polynomial: fri.rs:268-271 interpolates over the domain of the codeword's length with offset 1
    const tvm_domain last_dom = {TVM_ONE, bfe_pow(bfe_from_u64(7), (TVM_P - 1) / n_last), n_last};
    if (rc == TVM_OK) rc = tvm_interpolate(c, 3, last_cw, last_dom, d_poly);
    if (rc != TVM_OK) return leave(rc);
    SpongeTailArgs st = {};
    st.state = d_state, st.n_indices = (u32)n_checks, st.mask = dom.length - 1, st.indices = d_a;
    st.polynomial = d_poly, st.n_coefficients = (u32)n_last, st.discriminant = 5;   // ProofItem::Polynomial (proof_item.rs: the sixth variant)
    TVM_LAUNCH(k_sponge_tail, dim3(1), dim3(64), 0, c->stream, st);
    rc = authentication_structures_launch(c, (const AuthJob*)d, n_lists, n_checks, d_counts);
    tg.segments = (const TailSegment*)(d + w_jobs), tg.a = d_a, tg.auth_idx = d_auth, tg.auth_counts = d_counts;
    tg.n_checks = n_checks, tg.auth_stride = auth_stride, tg.out = d_payload, tg.directory = d_directory;
    if (rc == TVM_OK) rc = tail_gather_launch(c, tg, n_segments);
    if (rc != TVM_OK) return leave(rc);   // (a refused launch of the sponge shows in the next launch's check)

    // first round trip: what has a fixed size
    if (hipMemcpyAsync(fixed.data(), d_fixed, w_fixed * sizeof(u64), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipMemcpyAsync(h_last_codeword, last_cw, 3 * n_last * sizeof(u64), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = set_error(c, TVM_ERR_DEVICE, "tvm_fri_query_and_open download");
    if ((rc = leave(rc)) != TVM_OK) return rc;
    const u64* directory = fixed.data() + 16 + n_lists;
    const u64 total = directory[2 * (n_segments - 1)] + directory[2 * (n_segments - 1) + 1];
    if (total > bound) return set_error(c, TVM_ERR_DEVICE, "tvm_fri_query_and_open: payloads longer than their bound");
    *payload_words = total;
    if (total > payload_capacity) return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_fri_query_and_open: payload capacity");
    std::memcpy(h_state_out, fixed.data(), 16 * sizeof(u64));
    std::memcpy(h_directory, directory, 2 * (size_t)n_segments * sizeof(u64));
    std::memcpy(h_indices_out, directory + 2 * (size_t)n_segments, n_checks * sizeof(u64));
    std::memcpy(h_last_polynomial, directory + 2 * (size_t)n_segments + n_checks, 3 * n_last * sizeof(u64));
    // second round trip: exactly the words the proof holds
    if (hipMemcpyAsync(h_payload, d_payload, total * sizeof(u64), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = set_error(c, TVM_ERR_DEVICE, "tvm_fri_query_and_open payload download");
    return leave(rc);
}
}  // extern "C"
