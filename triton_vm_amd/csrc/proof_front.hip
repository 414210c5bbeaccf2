// proof_front.hip -- the front of a proof with the transcript on the device: from the main table's Merkle root to the quotient
// weights, queued on the stream with no host decision in between.
//
// A translation unit of its own, entry points included (as proof_middle.hip: nothing is added to the code objects of extend.hip,
// quotient.hip, the air_gen units or proof_middle.hip).
//
// Replaces, on the host's side of the reference's hot path:
//   ProofStream::enqueue(MerkleRoot(main root)), sample_scalars(59), Challenges::new            stark.rs:369-377, challenges.rs:85-121  -> k_front_challenges
//   ProofStream::enqueue(MerkleRoot(aux root)), sample_scalars(1)                               stark.rs:389-396                         -> k_front_weights
//   the quotient weights (powers of that scalar)                                                stark.rs:396-401                         -> k_front_weight_powers
// These are latency kernels: one wavefront each for the first two.  What they buy is the two host round trips between the LDEs, the
// trees, the extension and the AIR, whose kernels already take challenges and weights from device memory.
//
// The front's state is a block of TVM_FRONT_BLOCK_WORDS words that the caller owns (include/triton_hip.h: TVM_FRONT_*), not a scratch
// slot: tvm_front_challenges, the extension, tvm_front_quotient_weights, the quotient and the proof's middle queue work on it in turn.
#include "context.h"
#include "tail_kernels.h"
#include "tip5.h"

namespace tvm {

TVM_D xfe pf_ld(const u64* p) { return xfe_make(p[0], p[1], p[2]); }
TVM_D void pf_st(u64* p, xfe v) { p[0] = v.c0; p[1] = v.c1; p[2] = v.c2; }
TVM_D xfe pf_shfl(xfe v, int src) { return xfe_make(__shfl(v.c0, src, 64), __shfl(v.c1, src, 64), __shfl(v.c2, src, 64)); }

// ProofItem::MerkleRoot(nodes[1]) into the sponge: the item's encoding is [0, root] -- the discriminant as the one prefix word, five
// words of body; sponge_absorb_lanes pads it to its one block (as stir_rounds.hip absorbs its roots)
TVM_D u64 front_absorb_root_lanes(u64 x, int pos, int lane, const unsigned char* lut, const u64* nodes) {
    return sponge_absorb_lanes(x, pos, lane, lut, 0, 0, 0, 0, 1, nodes + 5, 5);
}

// EvalArg::compute_terminal(symbols, 1, x) = x^n + sum_i s_i x^(n - 1 - i) over the wavefront (every lane calls; lane 0 has the
// result).  The symbols are split into 64 contiguous chunks of ceil(n / 64) (the last ones shorter or empty); lane l runs Horner from
// zero on its chunk, which makes the map acc -> acc * x^len + P_l of its stretch of the host's loop, and the 64 maps are composed in
// lane order by a shuffle tree (a map is the pair (x^len, P); lane i takes the composition of the lanes behind it every step).
// Applied to the host's initial 1.  All words are canonical: the host's words, whatever the order of the operations.
template <class Symbol>
TVM_D xfe front_terminal_lanes(Symbol symbol, u64 n, xfe x, int lane) {
    const u64 chunk = (n + 63) / 64;
    const u64 lo = (u64)lane * chunk < n ? (u64)lane * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    xfe p = xfe_zero();
    for (u64 i = lo; i < hi; i++) p = xfe_add_bfe(xfe_mul(p, x), symbol(i));
    xfe m = xfe_pow(x, hi - lo);
    for (int d = 1; d < 64; d <<= 1) {
        const xfe m_behind = pf_shfl(m, (lane + d) & 63), p_behind = pf_shfl(p, (lane + d) & 63);
        if (lane + d < 64) {
            p = xfe_add(xfe_mul(p, m_behind), p_behind);
            m = xfe_mul(m, m_behind);
        }
    }
    return xfe_add(m, p);
}

// ---------------------------------------------------------------------------------------------- the challenges
// One wavefront, the lane convention of k_middle_points.  The 59 sampled scalars pass through LDS (the terminals read four of them),
// and all 63 challenges leave from there.
struct FrontChallengesArgs {
    u64* front;          // the block: the state is read at TVM_FRONT_STATE and left there
    const u64* nodes;    // the main table's tree [2 L][5]
    const u64* claim;    // [5 + n_input + n_output]: program digest, public input, public output
    u64 n_input, n_output;
};
__global__ void __launch_bounds__(64) k_front_challenges(FrontChallengesArgs g) {
    __shared__ unsigned char lut[256];
    __shared__ u64 ch[3 * TVM_NUM_CHALLENGES];
    tip5_stage_lut(lut, threadIdx.x, blockDim.x);
    const int lane = (int)threadIdx.x, pos = lane & 15;
    u64* state = g.front + TVM_FRONT_STATE;
    u64 x = front_absorb_root_lanes(state[pos], pos, lane, lut, g.nodes);
    if (lane < 5) g.front[TVM_FRONT_MAIN_ROOT + lane] = g.nodes[5 + lane];
    x = sponge_sample_scalars_lanes(x, pos, lane, lut, TVM_NUM_CHALLENGES - 4, ch);
    __syncthreads();
    if (lane < 16) state[pos] = x;
    // Challenges::new: input at StandardInputIndeterminate (1), output at StandardOutputIndeterminate (2), the lookup table at
    // LookupTablePublicIndeterminate (54), the digest at CompressProgramDigestIndeterminate (0)
    const u64 *digest = g.claim, *input = g.claim + 5, *output = input + g.n_input;
    const xfe t_input = front_terminal_lanes([&](u64 i) { return input[i]; }, g.n_input, pf_ld(ch + 3), lane);
    const xfe t_output = front_terminal_lanes([&](u64 i) { return output[i]; }, g.n_output, pf_ld(ch + 6), lane);
    const xfe t_lookup = front_terminal_lanes([&](u64 i) { return bfe_from_u64(lut[i]); }, 256, pf_ld(ch + 3 * 54), lane);
    const xfe t_digest = front_terminal_lanes([&](u64 i) { return digest[i]; }, 5, pf_ld(ch), lane);
    if (lane == 0) {
        u64* derived = ch + 3 * (TVM_NUM_CHALLENGES - 4);
        pf_st(derived, t_input);
        pf_st(derived + 3, t_output);
        pf_st(derived + 6, t_lookup);
        pf_st(derived + 9, t_digest);
    }
    __syncthreads();
    for (int i = lane; i < 3 * TVM_NUM_CHALLENGES; i += 64) g.front[TVM_FRONT_CHALLENGES + i] = ch[i];
}

// ---------------------------------------------------------------------------------------------- the quotient weights
// One wavefront: the aux root into the state the block holds, sample_scalars(1).
struct FrontWeightsArgs {
    u64* front;
    const u64* nodes;    // the aux table's tree [2 L][5]
};
__global__ void __launch_bounds__(64) k_front_weights(FrontWeightsArgs g) {
    __shared__ unsigned char lut[256];
    tip5_stage_lut(lut, threadIdx.x, blockDim.x);
    const int lane = (int)threadIdx.x, pos = lane & 15;
    u64* state = g.front + TVM_FRONT_STATE;
    u64 x = front_absorb_root_lanes(state[pos], pos, lane, lut, g.nodes);
    if (lane < 5) g.front[TVM_FRONT_AUX_ROOT + lane] = g.nodes[5 + lane];
    x = sponge_sample_scalars_lanes(x, pos, lane, lut, 1, g.front + TVM_FRONT_WEIGHT_SCALAR);
    if (lane < 16) state[pos] = x;
}
// The 604 weights, a kernel of its own (log depth: work-item i raises the scalar to the i-th power, as k_weight_vectors).  The words
// of the host's xfe_powers whatever the order of the multiplications.
__global__ void __launch_bounds__(64) k_front_weight_powers(u64* front) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < TVM_NUM_QUOTIENT_WEIGHTS) pf_st(front + TVM_FRONT_WEIGHTS + 3 * (u64)i, xfe_pow(pf_ld(front + TVM_FRONT_WEIGHT_SCALAR), (u64)i));
}

}  // namespace tvm

extern "C" {
using namespace tvm;

uint64_t tvm_front_block_words(void) { return TVM_FRONT_BLOCK_WORDS; }

int32_t tvm_front_challenges(tvm_ctx* c, const uint64_t* d_main_nodes, const uint64_t* h_state, const uint64_t* h_program_digest,
                             const uint64_t* h_input, uint64_t n_input, const uint64_t* h_output, uint64_t n_output, uint64_t* d_front) {
    if (!c || !d_main_nodes || !h_state || !h_program_digest || (n_input && !h_input) || (n_output && !h_output) || !d_front ||
        n_input > (1ull << 32) || n_output > (1ull << 32))
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_front_challenges arguments");
    u64* d_claim = (u64*)scratch(c, Scratch::FrontClaim, (size_t)(5 + n_input + n_output) * sizeof(u64));
    if (!d_claim) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "tvm_front_challenges staging");
    TVM_TRY(h2d_small(c, d_front + TVM_FRONT_STATE, h_state, 16 * sizeof(u64)));
    TVM_TRY(h2d_small(c, d_claim, h_program_digest, 5 * sizeof(u64)));
    TVM_TRY(h2d_small(c, d_claim + 5, h_input, (size_t)n_input * sizeof(u64)));
    TVM_TRY(h2d_small(c, d_claim + 5 + n_input, h_output, (size_t)n_output * sizeof(u64)));
    FrontChallengesArgs g = {d_front, d_main_nodes, d_claim, n_input, n_output};
    TVM_LAUNCH(k_front_challenges, dim3(1), dim3(64), 0, c->stream, g);
    TVM_HIP_CHECK(c, hipGetLastError());
    return TVM_OK;
}

int32_t tvm_front_quotient_weights(tvm_ctx* c, const uint64_t* d_aux_nodes, uint64_t* d_front) {
    if (!c || !d_aux_nodes || !d_front) return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_front_quotient_weights arguments");
    FrontWeightsArgs g = {d_front, d_aux_nodes};
    TVM_LAUNCH(k_front_weights, dim3(1), dim3(64), 0, c->stream, g);
    TVM_LAUNCH(k_front_weight_powers, dim3((TVM_NUM_QUOTIENT_WEIGHTS + 63) / 64), dim3(64), 0, c->stream, d_front);
    TVM_HIP_CHECK(c, hipGetLastError());
    return TVM_OK;
}

int32_t tvm_front_block(tvm_ctx* c, const uint64_t* d_front, uint64_t* h_block, uint64_t n_words, uint32_t wait) {
    if (!c || !d_front || !h_block || !n_words || n_words > TVM_FRONT_BLOCK_WORDS)
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "tvm_front_block arguments");
    TVM_HIP_CHECK(c, hipMemcpyAsync(h_block, d_front, (size_t)n_words * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (wait) TVM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return TVM_OK;
}
}  // extern "C"
