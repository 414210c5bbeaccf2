// verifier.cpp -- triton_vm::Verifier: Verifier::verify (/root/reference/triton-vm/src/stark.rs:1388-1763) with Fri::verify
// (fri.rs:368-700) and Stir::verify (stir.rs:995-1340), and the proof decoder it needs (proof_stream.rs:106-113, BFieldCodec).
// Step order and decisions are those of triton_vm_amd/verifier.py; the host keeps the transcript, does the index arithmetic and
// decides, everything per query goes through the C ABI (tvm_verifier_row_digests, tvm_verifier_merkle_roots, tvm_verifier_fri_folds,
// tvm_verifier_stir_answers, tvm_verifier_deep_values).
//
// Merkle inclusion is DEFERRED: a tree's job (indices, leaves, authentication structure, root) is queued where the reference checks it,
// and all queued jobs run in one tvm_verifier_merkle_roots call -- at the end of an accepting run, or as soon as any other check
// fails.  Every queued job precedes that failure in the reference's order, so the verdict reported is the one the reference's order
// gives: the first failing inclusion if there is one, else the failure that stopped the walk.
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <tuple>

#include "host_internal.hpp"
#include "triton_host.hpp"
#include "verifier_internal.hpp"

namespace triton_vm {

const char* verdict_name(uint32_t verdict) {
    switch (verdict) {
        case VERDICT_ACCEPTED: return "Accepted";
        case VERDICT_PROOF_DECODING_ERROR: return "ProofDecodingError";
        case VERDICT_PROOF_STREAM_ERROR: return "ProofStreamError";
        case VERDICT_LOG2_PADDED_HEIGHT_TOO_LARGE: return "Log2PaddedHeightTooLarge";
        case VERDICT_OUT_OF_DOMAIN_QUOTIENT_VALUE_MISMATCH: return "OutOfDomainQuotientValueMismatch";
        case VERDICT_INCORRECT_NUMBER_OF_ROW_INDICES: return "IncorrectNumberOfRowIndices";
        case VERDICT_INCORRECT_NUMBER_OF_MAIN_ROWS: return "IncorrectNumberOfMasterMainTableRows";
        case VERDICT_INCORRECT_NUMBER_OF_AUX_ROWS: return "IncorrectNumberOfMasterAuxTableRows";
        case VERDICT_INCORRECT_NUMBER_OF_QUOTIENT_SEGMENT_ELEMENTS: return "IncorrectNumberOfQuotientSegmentsElements";
        case VERDICT_MAIN_CODEWORD_AUTHENTICATION_FAILURE: return "MainCodewordAuthenticationFailure";
        case VERDICT_AUX_CODEWORD_AUTHENTICATION_FAILURE: return "AuxiliaryCodewordAuthenticationFailure";
        case VERDICT_QUOTIENT_CODEWORD_AUTHENTICATION_FAILURE: return "QuotientCodewordAuthenticationFailure";
        case VERDICT_COMBINATION_CODEWORD_MISMATCH: return "CombinationCodewordMismatch";
        case VERDICT_SUPERFLUOUS_PROOF_ITEMS: return "SuperfluousProofItems";
        case VERDICT_BAD_MERKLE_AUTHENTICATION_PATH: return "BadMerkleAuthenticationPath";
        case VERDICT_INCORRECT_NUMBER_OF_REVEALED_LEAVES: return "IncorrectNumberOfRevealedLeaves";
        case VERDICT_LAST_CODEWORD_MISMATCH: return "LastCodewordMismatch";
        case VERDICT_BAD_MERKLE_ROOT_FOR_LAST_CODEWORD: return "BadMerkleRootForLastCodeword";
        case VERDICT_LAST_ROUND_POLYNOMIAL_HAS_TOO_HIGH_DEGREE: return "LastRoundPolynomialHasTooHighDegree";
        case VERDICT_LAST_ROUND_POLYNOMIAL_EVALUATION_MISMATCH: return "LastRoundPolynomialEvaluationMismatch";
        case VERDICT_INCORRECT_NUMBER_OF_OUT_OF_DOMAIN_VALUES: return "IncorrectNumberOfOutOfDomainValues";
        case VERDICT_REPEATED_INTERPOLATION_POINT: return "repeated point in an interpolation";
        case VERDICT_UNSUPPORTED_PARAMETERS: return "UnsupportedParameters";
    }
    return "unknown verdict";
}

using namespace verifier_detail;   // the items, the walk, the front and the inclusion jobs: verifier_internal.hpp (shared with verify_batch.cpp)
namespace {
constexpr int STAGE_LDT = Verifier::STAGE_LDT, STAGE_INCLUSION = Verifier::STAGE_INCLUSION, STAGE_ROW_DIGESTS = Verifier::STAGE_ROW_DIGESTS;
}  // namespace

// ------------------------------------------------------------------------------------------------ ProofStream::try_from(&Proof)
// As strict as triton_vm_amd/proof_stream.py: every length prefix must agree with what encloses it, a statically sized payload has
// exactly its type's length, a u32 is one, a polynomial has no trailing zero coefficient, nothing follows the last item -- and
// stricter in one point: a word >= p is no BFieldElement and does not decode (the Python decoder reads its residue).  Every read is
// bounds-checked against the item that encloses it.
std::vector<DecodedItem> decode_proof(const u64* words, u64 n) {
    auto bad = []() { reject(VERDICT_PROOF_DECODING_ERROR); };
    std::vector<u64> w(n);
    for (u64 i = 0; i < n; i++) {
        if (words[i] >= P) bad();   // not the word of a BFieldElement: BFieldCodec decodes canonical elements only
        w[i] = from_mont(words[i]);
    }
    if (n < 2 || w[0] != n - 1) bad();
    std::vector<DecodedItem> items;
    u64 pos = 2;
    // Vec<T> of elem-word elements occupying exactly `length` words from `start` (all inside the proof) -> (first payload word, words)
    auto vec = [&](u64 start, u64 length, u64 elem) {
        if (length < 1 || w[start] > (length - 1) / elem || w[start] * elem != length - 1) bad();
        return std::make_pair(start + 1, length - 1);
    };
    for (u64 k = 0, n_items = w[1]; k < n_items; k++) {
        if (pos >= n) bad();
        const u64 size = w[pos++];
        if (size > n - pos || size < 1) bad();
        const u64 start = pos;
        pos += size;
        if (w[start] >= NUM_VARIANTS) bad();
        DecodedItem it;
        it.variant = (int)w[start], it.at = start, it.size = size;
        const int64_t kind = PAYLOAD[it.variant];
        if (kind > 0) {
            if (size - 1 != (u64)kind) bad();
            if (it.variant == LOG2_PADDED_HEIGHT && w[start + 1] >= (1ull << 32)) bad();
            it.payload_at = start + 1, it.payload_words = size - 1;
            items.push_back(std::move(it));
            continue;
        }
        if (size < 2 || w[start + 1] != size - 2) bad();
        const u64 body = start + 2, length = size - 2;
        if (kind < 0) {
            std::tie(it.payload_at, it.payload_words) = vec(body, length, (u64)-kind);
        } else if (it.variant == POLYNOMIAL) {
            if (length < 1 || w[body] != length - 1) bad();
            std::tie(it.payload_at, it.payload_words) = vec(body + 1, length - 1, 3);
            const u64* last = words + it.payload_at + it.payload_words - 3;
            if (it.payload_words && !(last[0] | last[1] | last[2])) bad();   // trailing zeros in the encoding
        } else {   // the struct's fields, last field first: auth_structure, then the leaves
            if (length < 2) bad();
            const u64 auth_len = w[body];
            if (auth_len > length - 2) bad();
            std::tie(it.auth_at, it.auth_words) = vec(body + 1, auth_len, 5);
            const u64 leaves_at = body + 1 + auth_len, leaves_len = w[leaves_at];
            if (2 + auth_len + leaves_len != length || leaves_len > length) bad();
            if (it.variant == FRI_RESPONSE) {
                const auto leaves = vec(leaves_at + 1, leaves_len, 3);
                it.leaves.assign(words + leaves.first, words + leaves.first + leaves.second);
            } else {   // Vec<Vec<XFieldElement>>
                if (leaves_len < 1) bad();
                const u64 end = leaves_at + 1 + leaves_len;
                u64 q = leaves_at + 2;
                for (u64 s = 0, n_stacks = w[leaves_at + 1]; s < n_stacks; s++) {
                    if (q >= end || w[q] > end - q - 1) bad();
                    const auto stack = vec(q + 1, w[q], 3);
                    if (s && stack.second != 3 * it.stack_height) bad();   // stacks of different heights
                    it.stack_height = stack.second / 3;
                    it.leaves.insert(it.leaves.end(), words + stack.first, words + stack.first + stack.second);
                    q += 1 + w[q];
                    it.n_stacks++;
                }
                if (q != end) bad();
            }
        }
        items.push_back(std::move(it));
    }
    if (pos != n) bad();
    return items;
}

// Proof::padded_height (proof.rs:45-59)
u64 proof_padded_height(const u64* words, u64 n) {
    u64 found = 0, log2 = 0;
    for (const DecodedItem& it : decode_proof(words, n))
        if (it.variant == LOG2_PADDED_HEIGHT) found++, log2 = from_mont(words[it.payload_at]);
    if (found != 1 || log2 >= 64) reject(VERDICT_PROOF_DECODING_ERROR);   // NoLog2PaddedHeight / TooManyLog2PaddedHeights
    return 1ull << log2;
}

// ------------------------------------------------------------------------------------------------ Verifier::verify
namespace verifier_detail {
std::vector<char> run_inclusion_jobs(const Context& c, const std::vector<Inclusion*>& inclusions, const std::function<void(int)>& lap) {
    lap(STAGE_LDT);
    std::map<u64, std::vector<size_t>> by_width;
    for (size_t j = 0; j < inclusions.size(); j++)
        if (inclusions[j]->row_words && !inclusions[j]->idx.empty()) by_width[inclusions[j]->row_words].push_back(j);
    for (const auto& group : by_width) {
        std::vector<u64> rows;
        for (size_t j : group.second) rows.insert(rows.end(), inclusions[j]->rows.begin(), inclusions[j]->rows.end());
        std::vector<u64> digests(rows.size() / group.first * 5);
        c.check(tvm_verifier_row_digests(c.raw(), rows.data(), rows.size() / group.first, group.first, digests.data()), "tvm_verifier_row_digests");
        size_t at = 0;
        for (size_t j : group.second) {
            inclusions[j]->digests.assign(digests.begin() + at, digests.begin() + at + 5 * inclusions[j]->idx.size());
            at += 5 * inclusions[j]->idx.size();
        }
    }
    lap(STAGE_ROW_DIGESTS);
    const size_t n = inclusions.size();
    std::vector<u64> n_leaves(n), n_idx(n), n_auth(n), roots(5 * n);
    std::vector<const u64*> idx(n), leaves(n), auth(n);
    std::vector<uint32_t> flags(n);
    for (size_t j = 0; j < n; j++) {
        const Inclusion& t = *inclusions[j];
        n_leaves[j] = t.n_leaves, n_idx[j] = t.idx.size(), n_auth[j] = t.n_auth;
        idx[j] = t.idx.data(), leaves[j] = t.digests.data(), auth[j] = t.auth;
    }
    c.check(tvm_verifier_merkle_roots(c.raw(), (uint32_t)n, n_leaves.data(), n_idx.data(), idx.data(), leaves.data(), n_auth.data(),
                                      auth.data(), roots.data(), flags.data()), "tvm_verifier_merkle_roots");
    lap(STAGE_INCLUSION);
    std::vector<char> failed(n);
    for (size_t j = 0; j < n; j++) failed[j] = flags[j] || std::memcmp(&roots[5 * j], inclusions[j]->root, 5 * sizeof(u64));
    return failed;
}
}  // namespace verifier_detail

namespace {
struct Run : Walk {
    const Context& c;
    std::vector<Inclusion> inclusions;
    double* ms;
    std::chrono::steady_clock::time_point mark = std::chrono::steady_clock::now();
    Run(const Context& c_, const u64* words_, double* ms_) : Walk(words_), c(c_), ms(ms_) {}

    void lap(int stage) {
        const auto now = std::chrono::steady_clock::now();
        ms[stage] += std::chrono::duration<double, std::milli>(now - mark).count();
        mark = now;
    }
    // all queued inclusion jobs: the row digests (one call per row width), then ONE tvm_verifier_merkle_roots
    void flush() {
        if (inclusions.empty()) return;
        std::vector<Inclusion> jobs;
        jobs.swap(inclusions);   // (a failing job leaves nothing queued: flush() runs again when the failure passes verify()'s handler)
        std::vector<Inclusion*> refs;
        for (Inclusion& t : jobs) refs.push_back(&t);
        const std::vector<char> failed = run_inclusion_jobs(c, refs, [this](int stage) { lap(stage); });
        for (size_t j = 0; j < jobs.size(); j++)
            if (failed[j]) reject(jobs[j].verdict);
    }
};

struct LdtResult {
    std::vector<u64> indices, revealed;   // first-round indices, the first codeword there [n][3]
};

// Fri::verify (fri.rs:368-700)
LdtResult fri_verify(Run& run, const StarkParameters& p) {
    const Context& c = run.c;
    const u64 checks = p.num_collinearity_checks;
    const unsigned num_rounds = p.fri_rounds;
    std::vector<ArithmeticDomain> domains{p.ldt};
    std::vector<const u64*> roots;
    std::vector<u64> challenges;
    for (unsigned r = 0; r <= num_rounds; r++) {
        roots.push_back(run.payload(run.dequeue(MERKLE_ROOT)));
        if (r < num_rounds) {
            const Xfe ch = run.sample();
            challenges.insert(challenges.end(), ch.c, ch.c + 3);
            domains.push_back(domains.back().pow(2));
        }
    }
    const ArithmeticDomain last_domain = domains[num_rounds];
    const DecodedItem& last_codeword = run.dequeue(FRI_CODEWORD);
    const DecodedItem& last_polynomial = run.dequeue(POLYNOMIAL);
    if (last_codeword.payload_words != 3 * last_domain.length) reject(VERDICT_LAST_CODEWORD_MISMATCH);
    LdtResult out;
    out.indices = run.sponge.sample_indices(p.ldt.length, checks);
    auto receive = [&](unsigned r, const std::vector<u64>& indices) -> const std::vector<u64>& {
        const DecodedItem& response = run.dequeue(FRI_RESPONSE);
        if (response.leaves.size() != 3 * checks) reject(VERDICT_INCORRECT_NUMBER_OF_REVEALED_LEAVES);
        Inclusion t{domains[r].length, indices, {}, {}, 0, run.words + response.auth_at, roots[r], response.auth_words / 5, VERDICT_BAD_MERKLE_AUTHENTICATION_PATH};
        t.digests.assign(5 * checks, 0);   // Digest::from(XFieldElement): the three coefficients, two zeros
        for (u64 j = 0; j < checks; j++) std::memcpy(&t.digests[5 * j], &response.leaves[3 * j], 3 * sizeof(u64));
        run.inclusions.push_back(std::move(t));
        return response.leaves;
    };
    out.revealed = receive(0, out.indices);
    std::vector<u64> b_leaves;
    for (unsigned r = 0; r < num_rounds; r++) {
        const u64 len = domains[r].length;
        std::vector<u64> ib(checks);
        for (u64 j = 0; j < checks; j++) ib[j] = (out.indices[j] + len / 2) % len;
        const std::vector<u64>& leaves = receive(r, ib);
        b_leaves.insert(b_leaves.end(), leaves.begin(), leaves.end());
    }
    std::vector<u64> folded(3 * checks);
    c.check(tvm_verifier_fri_folds(c.raw(), p.ldt.c(), num_rounds, challenges.data(), out.indices.data(), checks, out.revealed.data(),
                                   b_leaves.data(), folded.data()), "tvm_verifier_fri_folds");
    // the last round: commitment, agreement with the folded values, low degree (fri.rs:560-640)
    const u64 last_len = last_domain.length;
    const std::vector<u64> codeword(run.payload(last_codeword), run.payload(last_codeword) + 3 * last_len);
    const DeviceBuffer d_codeword = upload(c, codeword);
    {
        const DeviceBuffer nodes(c, 10 * last_len);
        c.check(tvm_codeword_merkle_tree(c.raw(), d_codeword.ptr(), last_len, nodes.ptr()), "tvm_codeword_merkle_tree");
        const std::vector<u64> root = merkle_root(c, nodes);
        if (std::memcmp(root.data(), roots[num_rounds], 5 * sizeof(u64))) reject(VERDICT_BAD_MERKLE_ROOT_FOR_LAST_CODEWORD);
    }
    for (u64 j = 0; j < checks; j++)
        if (std::memcmp(&codeword[3 * (out.indices[j] % last_len)], &folded[3 * j], 3 * sizeof(u64))) reject(VERDICT_LAST_CODEWORD_MISMATCH);
    const u64 max_degree = ((p.ldt.length >> p.log2_expansion) - 1) >> num_rounds;
    if (last_polynomial.payload_words / 3 > max_degree + 1) reject(VERDICT_LAST_ROUND_POLYNOMIAL_HAS_TOO_HIGH_DEGREE);
    const Xfe x = run.sample();
    const DeviceBuffer interpolant = ArithmeticDomain::of_length(last_len).interpolate(c, d_codeword.ptr(), 3);
    Xfe at_x, claimed = ZERO;
    c.check(tvm_evaluate_at_points(c.raw(), interpolant.ptr(), last_len, x.c, 1, at_x.c), "tvm_evaluate_at_points");
    if (last_polynomial.payload_words) tvm_host_xfe_poly_eval(run.payload(last_polynomial), last_polynomial.payload_words / 3, x.c, 1, 0, claimed.c);
    if (!xfe_eq(claimed, at_x)) reject(VERDICT_LAST_ROUND_POLYNOMIAL_EVALUATION_MISMATCH);
    return out;
}

// Stir::verify (stir.rs:995-1340)
LdtResult stir_verify(Run& run, const Stir& stir) {
    const Context& c = run.c;
    const u64 ff = stir.folding_factor;
    struct Queries {
        std::vector<u64> indices, values, roots;   // values [q][ff][3]; the coset's first point per query
        std::vector<Xfe> points;                    // the query's point of the folded domain
        u64 kth_root;
    };
    struct Previous {
        std::vector<Xfe> quotient_set, quotient_answers;
        Xfe degree_correction_randomness;
    };
    // extract_inclusion_proof + authenticated_queries (stir.rs:1157-1226)
    auto queries = [&](const ArithmeticDomain& domain, u64 num_queries, const u64* root) {
        Queries q;
        q.indices = run.sponge.sample_indices(domain.length, num_queries);
        const DecodedItem& response = run.dequeue(STIR_RESPONSE);
        const u64 folded_len = domain.length / ff;
        std::vector<u64> folded;   // .map(|i| i % len).unique(): first occurrences, in order
        std::map<u64, u64> place;
        for (u64 i : q.indices)
            if (place.emplace(i % folded_len, folded.size()).second) folded.push_back(i % folded_len);
        if (response.stack_height != ff || response.n_stacks != folded.size()) reject(VERDICT_INCORRECT_NUMBER_OF_REVEALED_LEAVES);
        run.inclusions.push_back(Inclusion{folded_len, folded, {}, response.leaves, 3 * ff, run.words + response.auth_at, root,
                                           response.auth_words / 5, VERDICT_BAD_MERKLE_AUTHENTICATION_PATH});
        const ArithmeticDomain folded_domain = domain.pow(ff);
        q.kth_root = mont_pow(domain.generator, folded_len);
        for (u64 i : q.indices) {
            const u64 f = i % folded_len;
            q.points.push_back(lift(folded_domain.value(f)));
            q.roots.push_back(domain.value(f));
            const u64* v = &response.leaves[3 * ff * place[f]];
            q.values.insert(q.values.end(), v, v + 3 * ff);
        }
        return q;
    };
    auto partial_codeword = [&](const ArithmeticDomain& domain, const Queries& q) {
        std::vector<u64> out;
        for (size_t j = 0; j < q.indices.size(); j++) {
            const u64* v = &q.values[3 * (ff * j + q.indices[j] / (domain.length / ff))];
            out.insert(out.end(), v, v + 3);
        }
        return out;
    };
    // initial_in_domain_answers / subsequent_in_domain_answers (stir.rs:1259-1340), on the device
    auto in_domain_answers = [&](const Queries& q, const Xfe& folding_randomness, const Previous* previous) {
        std::vector<Xfe> out(q.indices.size());
        if (out.empty()) return out;
        std::vector<Xfe> answer_poly;
        const uint32_t k = previous ? (uint32_t)previous->quotient_set.size() : 0;
        if (k) {
            answer_poly.resize(k);
            const int32_t status = tvm_xfe_interpolate(c.raw(), previous->quotient_set[0].c, previous->quotient_answers[0].c, k, answer_poly[0].c);
            if (status == TVM_ERR_INVALID_ARGUMENT) reject(VERDICT_REPEATED_INTERPOLATION_POINT);   // the only way valid arguments are refused
            c.check(status, "tvm_xfe_interpolate");   // out of memory, a device failure: an error status, not a verdict
        }
        c.check(tvm_verifier_stir_answers(c.raw(), (uint32_t)ff, q.indices.size(), q.values.data(), q.roots.data(), q.kth_root,
                                          folding_randomness.c, k, k ? previous->quotient_set[0].c : nullptr, k ? answer_poly[0].c : nullptr,
                                          k ? previous->degree_correction_randomness.c : nullptr, out[0].c), "tvm_verifier_stir_answers");
        return out;
    };

    ArithmeticDomain domain = stir.initial_domain;
    const u64* previous_root = run.payload(run.dequeue(MERKLE_ROOT));
    Previous previous;
    bool have_previous = false, have_first = false;
    LdtResult out;
    for (const auto& round : stir.round_queries) {
        const Xfe folding_randomness = run.sample();
        const u64* current_root = run.payload(run.dequeue(MERKLE_ROOT));
        const std::vector<Xfe> ood_queries = run.sponge.sample_scalars(round.second);
        const DecodedItem& ood = run.dequeue(STIR_OOD_VALUES);
        if (ood.payload_words != 3 * round.second) reject(VERDICT_INCORRECT_NUMBER_OF_OUT_OF_DOMAIN_VALUES);
        const Queries q = queries(domain, round.first, previous_root);
        if (!have_first) out.indices = q.indices, out.revealed = partial_codeword(domain, q), have_first = true;
        const std::vector<Xfe> answers = in_domain_answers(q, folding_randomness, have_previous ? &previous : nullptr);
        Previous next;   // queried indices repeat; interpolation points must not
        std::map<std::array<u64, 3>, bool> seen;
        auto add = [&](const Xfe& point, const Xfe& answer) {
            if (seen.emplace(std::array<u64, 3>{point.c[0], point.c[1], point.c[2]}, true).second)
                next.quotient_set.push_back(point), next.quotient_answers.push_back(answer);
        };
        for (size_t j = 0; j < answers.size(); j++) add(q.points[j], answers[j]);
        for (u64 j = 0; j < round.second; j++) add(ood_queries[j], xfe_at(run.payload(ood) + 3 * j));
        next.degree_correction_randomness = run.sample();
        previous = std::move(next), have_previous = true;
        const ArithmeticDomain squared = domain.pow(2);   // stir.rs:1149-1155
        domain = squared.with_offset(mont_mul(squared.offset, domain.offset));
        previous_root = current_root;
    }
    const Xfe folding_randomness = run.sample();
    const DecodedItem& final_polynomial = run.dequeue(POLYNOMIAL);
    const u64 n_final = final_polynomial.payload_words / 3;
    if ((n_final ? n_final - 1 : 0) > stir.final_degree) reject(VERDICT_LAST_ROUND_POLYNOMIAL_HAS_TOO_HIGH_DEGREE);
    const Queries q = queries(domain, stir.final_num_in_domain_queries, previous_root);
    if (!have_first) out.indices = q.indices, out.revealed = partial_codeword(domain, q);
    std::vector<Xfe> want(q.points.size(), ZERO);
    if (n_final && !want.empty()) tvm_host_xfe_poly_eval(run.payload(final_polynomial), n_final, q.points[0].c, q.points.size(), 0, want[0].c);
    const std::vector<Xfe> got = in_domain_answers(q, folding_randomness, have_previous ? &previous : nullptr);
    for (size_t j = 0; j < got.size(); j++)
        if (!xfe_eq(got[j], want[j])) reject(VERDICT_LAST_ROUND_POLYNOMIAL_EVALUATION_MISMATCH);
    return out;
}
}  // namespace

namespace verifier_detail {
Front walk_front(const Context& c, Walk& walk, const Claim& claim, unsigned security_level, unsigned log2_expansion, unsigned ldt_choice) {
    Front f;
    walk.sponge.alter_fiat_shamir_state_with(claim.encode());
    const u64 log2_padded_height = from_mont(*walk.payload(walk.dequeue(LOG2_PADDED_HEIGHT)));
    if (log2_padded_height >= 32) reject(VERDICT_LOG2_PADDED_HEIGHT_TOO_LARGE);
    f.use_stir = ldt_choice == 2 ? log2_padded_height >= 16 : ldt_choice == 1;   // Stark::ldt (stark.rs:1944-1951)
    StarkParameters& p = f.p;
    try {
        p = stark_parameters((unsigned)log2_padded_height, security_level, log2_expansion, f.use_stir);
    } catch (const Error&) {   // a height this host derives no parameters for (a domain beyond 2^32 points)
        reject(VERDICT_UNSUPPORTED_PARAMETERS);
    }

    // Fiat-Shamir 1 (stark.rs:1418-1437)
    f.main_root = walk.payload(walk.dequeue(MERKLE_ROOT));
    const std::vector<Xfe> challenges = derive_challenges(walk.sponge.sample_scalars(NUM_SAMPLED_CHALLENGES), claim);
    f.aux_root = walk.payload(walk.dequeue(MERKLE_ROOT));
    const std::vector<Xfe> quotient_weights = xfe_powers(walk.sample(), 0, TVM_NUM_QUOTIENT_WEIGHTS);
    f.quot_root = walk.payload(walk.dequeue(MERKLE_ROOT));

    // the out-of-domain rows and the quotient value they imply (stark.rs:1439-1539)
    const Xfe alpha = walk.sample();
    const u64 zeta = to_mont(3);   // Stark::ZETA, stark.rs:1801
    const Xfe alpha_next = xfe_scale(alpha, p.trace.generator), alpha_zeta = xfe_scale(alpha, zeta);
    const Xfe a4 = xfe_powers(alpha, 4, 1)[0], za4 = xfe_powers(alpha_zeta, 4, 1)[0];
    const u64* main_cur = walk.payload(walk.dequeue(OOD_MAIN_ROW));
    const u64* aux_cur = walk.payload(walk.dequeue(OOD_AUX_ROW));
    const u64* main_next = walk.payload(walk.dequeue(OOD_MAIN_ROW));
    const u64* aux_next = walk.payload(walk.dequeue(OOD_AUX_ROW));
    const u64* seg_p = walk.payload(walk.dequeue(OOD_QUOTIENT_SEGMENTS));
    const u64* seg_r = walk.payload(walk.dequeue(OOD_QUOTIENT_SEGMENTS));
    std::vector<Xfe> constraints(TVM_NUM_QUOTIENT_WEIGHTS);
    c.check(tvm_host_air_constraints(main_cur, aux_cur, main_next, aux_next, challenges[0].c, constraints[0].c), "tvm_host_air_constraints");
    const Xfe one = lift(to_mont(1));
    const Xfe consistency_inv = xfe_inv(xfe_sub(xfe_powers(alpha, p.trace.length, 1)[0], one));
    const Xfe except_last = xfe_sub(alpha, lift(mont_pow(p.trace.generator, P - 2)));
    // initial, consistency, transition, terminal (stark.rs:1493-1499)
    const std::pair<unsigned, Xfe> zerofier_inverse[4] = {{81, xfe_inv(xfe_sub(alpha, one))}, {97, consistency_inv},
                                                          {403, xfe_mul(except_last, consistency_inv)}, {23, xfe_inv(except_last)}};
    Xfe ood_quotient = ZERO;
    unsigned k = 0;
    for (const auto& section : zerofier_inverse)
        for (unsigned i = 0; i < section.first; i++, k++)
            ood_quotient = xfe_add(ood_quotient, xfe_mul(quotient_weights[k], xfe_mul(constraints[k], section.second)));
    const std::vector<Xfe> alpha_powers = xfe_powers(alpha, 0, 4), alpha_zeta_powers = xfe_powers(alpha_zeta, 0, 4);
    Xfe derandomized = ZERO;
    for (int i = 0; i < 4; i++) derandomized = xfe_add(derandomized, xfe_mul(alpha_powers[i], xfe_at(seg_p + 3 * i)));
    for (int i = 0; i < 4; i++) derandomized = xfe_add(derandomized, xfe_mul(alpha_zeta_powers[i], xfe_at(seg_r + 3 * i)));
    if (!xfe_eq(ood_quotient, derandomized)) reject(VERDICT_OUT_OF_DOMAIN_QUOTIENT_VALUE_MISMATCH);

    // Fiat-Shamir 2 and the out-of-domain sums (stark.rs:1541-1575)
    const std::vector<Xfe> iw = walk.sponge.sample_scalars(3);
    f.w_ma = xfe_powers(iw[0], 0, NUM_MAIN + NUM_AUX), f.w_q = xfe_powers(iw[1], 0, 5), f.w_d = xfe_powers(iw[2], 0, 4);
    const std::vector<Xfe>&w_ma = f.w_ma, &w_q = f.w_q;
    auto linear_sum = [&](const u64* m, const u64* a) {
        Xfe acc = ZERO;
        for (u64 i = 0; i < NUM_MAIN; i++) acc = xfe_add(acc, xfe_mul(w_ma[i], xfe_at(m + 3 * i)));
        for (u64 i = 0; i < NUM_AUX; i++) acc = xfe_add(acc, xfe_mul(w_ma[NUM_MAIN + i], xfe_at(a + 3 * i)));
        return acc;
    };
    Xfe* ood_values = f.ood_values;
    ood_values[0] = linear_sum(main_cur, aux_cur), ood_values[1] = linear_sum(main_next, aux_next), ood_values[2] = ood_values[3] = ZERO;
    for (int i = 0; i < 4; i++) {
        ood_values[2] = xfe_add(ood_values[2], xfe_mul(xfe_at(seg_p + 3 * i), w_q[i]));
        ood_values[3] = xfe_add(ood_values[3], xfe_mul(xfe_at(seg_r + 3 * i), w_q[i + 1]));
    }
    f.ood_points[0] = alpha, f.ood_points[1] = alpha_next, f.ood_points[2] = a4, f.ood_points[3] = za4;
    return f;
}
}  // namespace verifier_detail

std::vector<u64> Verifier::verify(const Claim& claim, const u64* proof_words, u64 n_words) {
    std::fill(stage_ms, stage_ms + NUM_STAGES, 0.0);
    Run run(c_, proof_words, stage_ms);
    try {
        run.items = decode_proof(proof_words, n_words);
    } catch (const VerificationFailure&) {
        run.lap(STAGE_DECODE);
        throw;
    }
    run.lap(STAGE_DECODE);
    try {
        const Front front = walk_front(c_, run, claim, security_level_, log2_expansion_, ldt_choice_);
        const StarkParameters& p = front.p;
        const u64 checks = p.num_collinearity_checks;
        run.lap(STAGE_TRANSCRIPT_AIR);

        // the low-degree test (stark.rs:1577-1590)
        const LdtResult ldt = front.use_stir ? stir_verify(run, p.stir) : fri_verify(run, p);
        if (ldt.indices.size() != checks || ldt.revealed.size() != 3 * checks) reject(VERDICT_INCORRECT_NUMBER_OF_ROW_INDICES);
        run.lap(STAGE_LDT);

        // the revealed rows against their roots (stark.rs:1592-1672): hashed, and their trees recomputed, with the LDT's trees
        auto rows_of = [&](int variant, u64 width, const u64* root, uint32_t wrong_number, uint32_t wrong_path) {
            const DecodedItem& rows = run.dequeue(variant);
            if (rows.payload_words != checks * width) reject(wrong_number);
            const DecodedItem& auth = run.dequeue(AUTH_STRUCTURE);
            run.inclusions.push_back(Inclusion{p.ldt.length, ldt.indices, {}, std::vector<u64>(run.payload(rows), run.payload(rows) + checks * width),
                                               width, run.payload(auth), root, auth.payload_words / 5, wrong_path});
            return run.payload(rows);
        };
        const u64* main_rows = rows_of(MAIN_ROWS, NUM_MAIN, front.main_root, VERDICT_INCORRECT_NUMBER_OF_MAIN_ROWS, VERDICT_MAIN_CODEWORD_AUTHENTICATION_FAILURE);
        const u64* aux_rows = rows_of(AUX_ROWS, NUM_AUX * 3, front.aux_root, VERDICT_INCORRECT_NUMBER_OF_AUX_ROWS, VERDICT_AUX_CODEWORD_AUTHENTICATION_FAILURE);
        const u64* quot_rows = rows_of(QUOTIENT_SEGMENT_ELEMENTS, 15, front.quot_root, VERDICT_INCORRECT_NUMBER_OF_QUOTIENT_SEGMENT_ELEMENTS,
                                       VERDICT_QUOTIENT_CODEWORD_AUTHENTICATION_FAILURE);
        run.flush();

        // the combination codeword at the revealed rows, on the device (stark.rs:1674-1755)
        std::vector<u64> want(3 * checks);
        c_.check(tvm_verifier_deep_values(c_.raw(), main_rows, aux_rows, quot_rows, ldt.indices.data(), checks, p.ldt.c(), front.w_ma[0].c,
                                          front.w_q[0].c, front.w_d[0].c, front.ood_points[0].c, front.ood_values[0].c, want.data()),
                 "tvm_verifier_deep_values");
        run.lap(STAGE_DEEP_VALUES);
        if (want != ldt.revealed) reject(VERDICT_COMBINATION_CODEWORD_MISMATCH);
        if (run.next != run.items.size()) reject(VERDICT_SUPERFLUOUS_PROOF_ITEMS);
        return ldt.indices;
    } catch (const VerificationFailure&) {
        run.flush();   // an inclusion queued before this failure fails first (see the head of this file)
        throw;
    }
}

}  // namespace triton_vm

extern "C" const char* tvmh_verdict_name(uint32_t verdict) { return triton_vm::verdict_name(verdict); }

extern "C" int32_t tvmh_proof_padded_height(const uint64_t* h_proof, uint64_t proof_words, uint32_t* verdict, uint64_t* padded_height) {
    using namespace triton_vm;
    if ((!h_proof && proof_words) || !verdict || !padded_height) return TVM_ERR_INVALID_ARGUMENT;
    try {
        *padded_height = proof_padded_height(h_proof, proof_words);
        *verdict = VERDICT_ACCEPTED;
    } catch (const VerificationFailure& f) {
        *verdict = f.verdict;
    } catch (const std::exception&) {
        return TVM_ERR_OUT_OF_MEMORY;
    }
    return TVM_OK;
}

extern "C" int32_t tvmh_verify(tvm_ctx* ctx, const uint64_t* h_proof, uint64_t proof_words, const uint64_t* h_program_digest, uint32_t version,
                               const uint64_t* h_public_input, uint64_t n_public_input, const uint64_t* h_public_output,
                               uint64_t n_public_output, uint32_t security_level, uint32_t log2_expansion, uint32_t ldt_choice,
                               uint32_t* verdict, uint64_t* h_indices, uint64_t indices_capacity, uint64_t* n_indices, double* stage_ms,
                               char* error, uint64_t error_capacity) {
    using namespace triton_vm;
    if (error && error_capacity) error[0] = 0;
    return guarded(error, error_capacity, [&] {
        if (!ctx || !verdict || (!h_proof && proof_words) || (n_public_input && !h_public_input) || (n_public_output && !h_public_output))
            throw Error(TVM_ERR_INVALID_ARGUMENT, "tvmh_verify: null context, verdict, proof or claim");
        if (ldt_choice > 2) throw Error(TVM_ERR_INVALID_ARGUMENT, "tvmh_verify: the LDT choice is 0 (FRI), 1 (STIR) or 2 (Stark::ldt's rule)");
        if (!security_level || security_level > 512 || !log2_expansion || log2_expansion > 8)
            throw Error(TVM_ERR_INVALID_ARGUMENT, "tvmh_verify: security level 1..512, log2 expansion 1..8");
        const Context c(ctx);
        Claim claim = make_claim(h_program_digest, h_public_input, n_public_input, h_public_output, n_public_output);
        claim.version = version;
        Verifier verifier(c, security_level, log2_expansion, ldt_choice);
        auto stages = [&]() {
            if (stage_ms) std::memcpy(stage_ms, verifier.stage_ms, sizeof(verifier.stage_ms));
        };
        try {
            const std::vector<u64> indices = verifier.verify(claim, h_proof, proof_words);
            stages();
            if (n_indices) *n_indices = indices.size();
            if (h_indices && indices_capacity >= indices.size()) std::memcpy(h_indices, indices.data(), indices.size() * sizeof(u64));
            *verdict = VERDICT_ACCEPTED;
        } catch (const VerificationFailure& f) {   // a rejection is a verdict, not an error status
            stages();
            if (n_indices) *n_indices = 0;
            *verdict = f.verdict;
            if (error && error_capacity) std::snprintf(error, error_capacity, "%s", verdict_name(f.verdict));
        }
    });
}
