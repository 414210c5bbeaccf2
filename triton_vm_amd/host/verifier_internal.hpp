// verifier_internal.hpp -- what Verifier::verify (verifier.cpp) and tvmh_verify_batch (verify_batch.cpp) share: the proof items and
// the walk over them, the part of Verifier::verify in front of the low-degree test (no device work: both run it as it is), and the
// deferred Merkle inclusion jobs.  Not part of the interface: triton_host.hpp is.
#pragma once
#include <functional>

#include "host_internal.hpp"

namespace triton_vm {
namespace verifier_detail {

[[noreturn]] inline void reject(uint32_t verdict) { throw VerificationFailure(verdict); }
inline u64 from_mont(u64 w) { return mont_mul(w, 1); }
inline u64 bfe_sub(u64 a, u64 b) { return (u64)(((unsigned __int128)(a % P) + P - (b % P)) % P); }
inline Xfe xfe_sub(const Xfe& a, const Xfe& b) { return Xfe{{bfe_sub(a.c[0], b.c[0]), bfe_sub(a.c[1], b.c[1]), bfe_sub(a.c[2], b.c[2])}}; }
inline Xfe xfe_inv(const Xfe& a) {
    Xfe o;
    tvm_host_xfe_inv(a.c, o.c);
    return o;
}
inline Xfe lift(u64 b) { return Xfe{{b, 0, 0}}; }
inline Xfe xfe_at(const u64* w) { return Xfe{{w[0], w[1], w[2]}}; }
inline bool xfe_eq(const Xfe& a, const Xfe& b) { return a.c[0] == b.c[0] && a.c[1] == b.c[1] && a.c[2] == b.c[2]; }
static const Xfe ZERO{{0, 0, 0}};

// proof_item.rs:96-150 in declaration order (= discriminant)
enum { MERKLE_ROOT, LOG2_PADDED_HEIGHT, OOD_MAIN_ROW, OOD_AUX_ROW, OOD_QUOTIENT_SEGMENTS, POLYNOMIAL, STIR_OOD_VALUES, AUTH_STRUCTURE,
       MAIN_ROWS, AUX_ROWS, QUOTIENT_SEGMENT_ELEMENTS, FRI_CODEWORD, FRI_RESPONSE, STIR_RESPONSE, NUM_VARIANTS };
// > 0: statically sized, that many words; < 0: Vec of that many words per element; 0: polynomial or response
static const int64_t PAYLOAD[NUM_VARIANTS] = {5, 1, 379 * 3, 91 * 3, 4 * 3, 0, -3, -5, -379, -273, -15, -3, 0, 0};
static const bool FIAT_SHAMIR[NUM_VARIANTS] = {true, true, true, true, true, true, true, false, false, false, false, false, false, false};

// The verifier's place in a decoded proof and its Fiat-Shamir sponge.  Every failure here is decided on the host.
struct Walk {
    const u64* words;
    std::vector<DecodedItem> items;
    size_t next = 0;
    ProofStream sponge;
    explicit Walk(const u64* words_) : words(words_) {}

    const DecodedItem& dequeue(int variant) {   // ProofStream::dequeue (proof_stream.rs:62-72) + the try_into_* of proof_item.rs
        if (next >= items.size()) reject(VERDICT_PROOF_STREAM_ERROR);   // EmptyQueue
        const DecodedItem& it = items[next++];
        if (it.variant != variant) reject(VERDICT_PROOF_STREAM_ERROR);   // UnexpectedItem
        // the decoder accepts canonical encodings only: the item's words in the proof ARE its encoding
        if (FIAT_SHAMIR[variant]) sponge.alter_fiat_shamir_state_with(std::vector<u64>(words + it.at, words + it.at + it.size));
        return it;
    }
    const u64* payload(const DecodedItem& it) const { return words + it.payload_at; }
    Xfe sample() { return sponge.sample_scalars(1)[0]; }
};

// Verifier::verify from the claim to the out-of-domain sums (stark.rs:1388-1575): the parameters the proof's height implies, the
// three roots, the out-of-domain quotient check, the weights.  No device work.
struct Front {
    StarkParameters p{0};
    bool use_stir = false;
    const u64 *main_root = nullptr, *aux_root = nullptr, *quot_root = nullptr;
    std::vector<Xfe> w_ma, w_q, w_d;   // the weights of the main and auxiliary columns, the quotient segments, the DEEP terms
    Xfe ood_points[4], ood_values[4];  // current row, next row, alpha^4, (zeta alpha)^4 (stark.rs:1722-1745)
};
Front walk_front(const Context& c, Walk& walk, const Claim& claim, unsigned security_level, unsigned log2_expansion, unsigned ldt_choice);

// one deferred MerkleTreeInclusionProof::verify
struct Inclusion {
    u64 n_leaves;
    std::vector<u64> idx, digests, rows;   // digests [q][5], or rows [q][row_words] still to be hashed
    u64 row_words;
    const u64 *auth, *root;
    u64 n_auth;
    uint32_t verdict;
};
// The jobs' row digests (one tvm_verifier_row_digests call per row width), then ONE tvm_verifier_merkle_roots for all of them (at
// most TVM_VERIFIER_MAX_TREES).  -> per job: did it fail (malformed, or another root).  lap(stage) is called after the host
// preparation (Verifier::STAGE_LDT), the digests (STAGE_ROW_DIGESTS) and the roots (STAGE_INCLUSION).
std::vector<char> run_inclusion_jobs(const Context& c, const std::vector<Inclusion*>& jobs, const std::function<void(int)>& lap);

}  // namespace verifier_detail
}  // namespace triton_vm
