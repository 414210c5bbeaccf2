// verify_batch.cpp -- tvmh_verify_batch: Verifier::verify (verifier.cpp) for many proofs per call, with the device work shared.
//
// The verifier's transcript never depends on a device result: the sponge absorbs proof items only, and what the device computes feeds
// comparisons and -- in STIR -- the next round's interpolation.  So a chunk of jobs is verified in two passes.  First the host walks
// every job's transcript (decode, the front of Verifier::verify as verify() runs it, the low-degree test's items, the revealed rows)
// and only RECORDS what the device has to compute and which comparisons wait for it.  Then the device work of all jobs runs stage by
// stage, one round trip per stage per chunk instead of one per stage per proof:
//   row digests (one tvm_verifier_row_digests per row width), ONE tvm_verifier_merkle_roots, tvm_verifier_fri_folds_batch,
//   tvm_verifier_fri_last_rounds, per STIR round r one tvm_xfe_interpolate_batch and one tvm_verifier_stir_answers_batch over the jobs
//   that have a round r, tvm_verifier_deep_values_batch (csrc/verify_batch.hip), and the jobs are decided.
//
// THE VERDICT.  verify() reports the first failing check in the order of its statements, which is the reference's order (stark.rs:1388-
// 1763, fri.rs:368-700, stir.rs:995-1340) up to the deferred Merkle inclusions (verifier.cpp's head).  Here EVERY device-dependent check
// is deferred, so the rule is explicit: each check site gets an ordinal when the walk reaches it -- the walk visits the sites in verify()'s
// statement order, so the running count is the site's place in that order -- and a job's verdict is its failing check with the LOWEST
// ordinal (Job::fail).  The walk continues past a deferred check and stops at a host-decidable failure (a wrong or missing item, a wrong
// count, a degree bound, the out-of-domain quotient): only such checks guard sizes, so nothing later in the walk or on the device reads
// out of range, and what a failed deferred check leaves behind (a STIR answer polynomial of a repeated point, say) only feeds checks with
// higher ordinals.  A host-decidable failure has a higher ordinal than every check recorded before it, and no check is recorded after it.
#include <array>
#include <chrono>
#include <map>
#include <memory>
#include <string>

#include "host_internal.hpp"
#include "triton_host.hpp"
#include "verifier_internal.hpp"

namespace triton_vm {
using namespace verifier_detail;
namespace {

struct Deferred {   // a comparison that waits for a device result
    uint32_t ordinal, verdict;
};

struct FriWork {   // Fri::verify's device work (fri.rs:520-640)
    ArithmeticDomain first_domain;
    unsigned num_rounds = 0;
    std::vector<u64> challenges, indices, a_leaves, b_leaves, folded;   // [rounds][3], [q], [q][3], [rounds][q][3], [q][3]
    const u64 *codeword = nullptr, *root = nullptr;                     // the last codeword [last_len][3], the root it was committed under
    u64 last_len = 0;
    Xfe x = ZERO, claimed = ZERO, at_x = ZERO;                          // the last polynomial at x: claimed, and interpolated from the codeword
    u64 device_root[5] = {};
    Deferred bad_root{}, mismatch{}, evaluation{};
    bool have_folds = false, have_last = false;                         // how far the walk got
};

struct StirRound {   // one authenticated_queries + in_domain_answers (stir.rs:1157-1340); the last entry is the final round
    u64 ff = 0, kth_root = 0;
    Xfe folding_randomness = ZERO, degree_correction_randomness = ZERO;   // the latter: of the PREVIOUS round, read when there is one
    std::vector<u64> values, roots;                          // [q][ff][3], [q]
    std::vector<Xfe> answers;                                // [q], from the device
    // the quotient set this round leaves to the next: its points, and where each answer comes from -- query j of this round (>= 0) or
    // out-of-domain value -(j + 1)
    std::vector<Xfe> set_points, ood_values;
    std::vector<int64_t> set_source;
    std::vector<Xfe> answer_poly;                            // of the previous round's set, from the device (round >= 1)
    Deferred repeated_point{};
    bool repeated = false;                                   // the device found two equal points in the previous round's set
};

struct Job {
    const tvmh_verify_job* in;
    Claim claim;
    Walk walk;
    Front front;
    uint32_t next_ordinal = 0, verdict = VERDICT_ACCEPTED, verdict_ordinal = 0xFFFFFFFFu;
    std::vector<u64> indices, revealed;   // the low-degree test's first-round indices and the first codeword there [n][3]
    std::vector<Inclusion> inclusions;
    std::vector<uint32_t> inclusion_ordinal;
    bool use_fri = false;
    FriWork fri;
    std::vector<StirRound> stir;
    std::vector<Xfe> stir_want;           // the final polynomial at the final round's points
    Deferred stir_final{};
    bool have_stir_final = false, have_deep = false;
    const u64 *main_rows = nullptr, *aux_rows = nullptr, *quot_rows = nullptr;
    std::vector<u64> deep;                // [n][3]
    Deferred combination{};

    explicit Job(const tvmh_verify_job* in_) : in(in_), walk(in_->h_proof) {}
    uint32_t site() { return next_ordinal++; }   // the ordinal of the check site the walk has reached
    Deferred defer(uint32_t v) { return Deferred{site(), v}; }
    void fail(uint32_t ordinal, uint32_t v) {
        if (ordinal < verdict_ordinal) verdict_ordinal = ordinal, verdict = v;
    }
    void fail(const Deferred& d) { fail(d.ordinal, d.verdict); }
    // a host-decidable check: failing, it is the job's last site and ends the walk
    void require(bool holds, uint32_t v) {
        const uint32_t ordinal = site();
        if (!holds) fail(ordinal, v), reject(v);
    }
    void queue(Inclusion&& t) {
        inclusion_ordinal.push_back(site());
        inclusions.push_back(std::move(t));
    }
};

// (Walk::dequeue throws without a site of its own: the catch in walk_job gives such a failure the next ordinal, the highest so far)

// Fri::verify (fri.rs:368-700): fri_verify of verifier.cpp with the device work recorded
void fri_walk(Job& job) {
    Walk& run = job.walk;
    const StarkParameters& p = job.front.p;
    FriWork& f = job.fri;
    const u64 checks = p.num_collinearity_checks;
    const unsigned num_rounds = f.num_rounds = p.fri_rounds;
    f.first_domain = p.ldt;
    std::vector<ArithmeticDomain> domains{p.ldt};
    std::vector<const u64*> roots;
    for (unsigned r = 0; r <= num_rounds; r++) {
        roots.push_back(run.payload(run.dequeue(MERKLE_ROOT)));
        if (r < num_rounds) {
            const Xfe ch = run.sample();
            f.challenges.insert(f.challenges.end(), ch.c, ch.c + 3);
            domains.push_back(domains.back().pow(2));
        }
    }
    const ArithmeticDomain last_domain = domains[num_rounds];
    const DecodedItem& last_codeword = run.dequeue(FRI_CODEWORD);
    const DecodedItem& last_polynomial = run.dequeue(POLYNOMIAL);
    job.require(last_codeword.payload_words == 3 * last_domain.length, VERDICT_LAST_CODEWORD_MISMATCH);
    job.indices = f.indices = run.sponge.sample_indices(p.ldt.length, checks);
    auto receive = [&](unsigned r, const std::vector<u64>& indices) -> const std::vector<u64>& {
        const DecodedItem& response = run.dequeue(FRI_RESPONSE);
        job.require(response.leaves.size() == 3 * checks, VERDICT_INCORRECT_NUMBER_OF_REVEALED_LEAVES);
        Inclusion t{domains[r].length, indices, {}, {}, 0, run.words + response.auth_at, roots[r], response.auth_words / 5, VERDICT_BAD_MERKLE_AUTHENTICATION_PATH};
        t.digests.assign(5 * checks, 0);   // Digest::from(XFieldElement): the three coefficients, two zeros
        for (u64 j = 0; j < checks; j++) std::memcpy(&t.digests[5 * j], &response.leaves[3 * j], 3 * sizeof(u64));
        job.queue(std::move(t));
        return response.leaves;
    };
    job.revealed = f.a_leaves = receive(0, f.indices);
    for (unsigned r = 0; r < num_rounds; r++) {
        const u64 len = domains[r].length;
        std::vector<u64> ib(checks);
        for (u64 j = 0; j < checks; j++) ib[j] = (f.indices[j] + len / 2) % len;
        const std::vector<u64>& leaves = receive(r, ib);
        f.b_leaves.insert(f.b_leaves.end(), leaves.begin(), leaves.end());
    }
    f.have_folds = true;
    // the last round: commitment, agreement with the folded values, low degree (fri.rs:560-640)
    f.last_len = last_domain.length, f.codeword = run.payload(last_codeword), f.root = roots[num_rounds];
    f.bad_root = job.defer(VERDICT_BAD_MERKLE_ROOT_FOR_LAST_CODEWORD);
    f.mismatch = job.defer(VERDICT_LAST_CODEWORD_MISMATCH);
    const u64 max_degree = ((p.ldt.length >> p.log2_expansion) - 1) >> num_rounds;
    job.require(last_polynomial.payload_words / 3 <= max_degree + 1, VERDICT_LAST_ROUND_POLYNOMIAL_HAS_TOO_HIGH_DEGREE);
    f.x = run.sample();
    f.claimed = ZERO;
    if (last_polynomial.payload_words) tvm_host_xfe_poly_eval(run.payload(last_polynomial), last_polynomial.payload_words / 3, f.x.c, 1, 0, f.claimed.c);
    f.evaluation = job.defer(VERDICT_LAST_ROUND_POLYNOMIAL_EVALUATION_MISMATCH);
    f.have_last = true;
}

// Stir::verify (stir.rs:995-1340): stir_verify of verifier.cpp with the device work recorded
void stir_walk(Job& job) {
    Walk& run = job.walk;
    const Stir& stir = job.front.p.stir;
    const u64 ff = stir.folding_factor;
    bool have_first = false;
    std::vector<Xfe> points;   // of the round being received: the query's point of the folded domain
    // extract_inclusion_proof + authenticated_queries (stir.rs:1157-1226) -> the round with its queries
    auto queries = [&](const ArithmeticDomain& domain, u64 num_queries, const u64* root) {
        StirRound round;
        round.ff = ff;
        const std::vector<u64> indices = run.sponge.sample_indices(domain.length, num_queries);
        const DecodedItem& response = run.dequeue(STIR_RESPONSE);
        const u64 folded_len = domain.length / ff;
        std::vector<u64> folded;   // .map(|i| i % len).unique(): first occurrences, in order
        std::map<u64, u64> place;
        for (u64 i : indices)
            if (place.emplace(i % folded_len, folded.size()).second) folded.push_back(i % folded_len);
        job.require(response.stack_height == ff && response.n_stacks == folded.size(), VERDICT_INCORRECT_NUMBER_OF_REVEALED_LEAVES);
        job.queue(Inclusion{folded_len, folded, {}, response.leaves, 3 * ff, run.words + response.auth_at, root, response.auth_words / 5,
                            VERDICT_BAD_MERKLE_AUTHENTICATION_PATH});
        const ArithmeticDomain folded_domain = domain.pow(ff);
        round.kth_root = mont_pow(domain.generator, folded_len);
        points.clear();
        for (u64 i : indices) {
            const u64 f = i % folded_len;
            points.push_back(lift(folded_domain.value(f)));
            round.roots.push_back(domain.value(f));
            const u64* v = &response.leaves[3 * ff * place[f]];
            round.values.insert(round.values.end(), v, v + 3 * ff);
        }
        if (!have_first) {   // the first codeword at the first round's indices
            job.indices = indices;
            for (size_t j = 0; j < indices.size(); j++) {
                const u64* v = &round.values[3 * (ff * j + indices[j] / folded_len)];
                job.revealed.insert(job.revealed.end(), v, v + 3);
            }
            have_first = true;
        }
        return round;
    };
    // in_domain_answers of a round with a previous one interpolates the previous quotient set first: where a repeated point is found
    auto answers_site = [&](StirRound& round) {
        if (!job.stir.empty() && !round.roots.empty() && !job.stir.back().set_points.empty())
            round.repeated_point = job.defer(VERDICT_REPEATED_INTERPOLATION_POINT);
    };

    ArithmeticDomain domain = stir.initial_domain;
    const u64* previous_root = run.payload(run.dequeue(MERKLE_ROOT));
    Xfe previous_rc = ZERO;
    for (const auto& parameters : stir.round_queries) {
        const Xfe folding_randomness = run.sample();
        const u64* current_root = run.payload(run.dequeue(MERKLE_ROOT));
        const std::vector<Xfe> ood_queries = run.sponge.sample_scalars(parameters.second);
        const DecodedItem& ood = run.dequeue(STIR_OOD_VALUES);
        job.require(ood.payload_words == 3 * parameters.second, VERDICT_INCORRECT_NUMBER_OF_OUT_OF_DOMAIN_VALUES);
        StirRound round = queries(domain, parameters.first, previous_root);
        round.folding_randomness = folding_randomness, round.degree_correction_randomness = previous_rc;
        answers_site(round);
        std::map<std::array<u64, 3>, bool> seen;   // queried indices repeat; interpolation points must not
        auto add = [&](const Xfe& point, int64_t source) {
            if (seen.emplace(std::array<u64, 3>{point.c[0], point.c[1], point.c[2]}, true).second)
                round.set_points.push_back(point), round.set_source.push_back(source);
        };
        for (size_t j = 0; j < points.size(); j++) add(points[j], (int64_t)j);
        for (u64 j = 0; j < parameters.second; j++) {
            round.ood_values.push_back(xfe_at(run.payload(ood) + 3 * j));
            add(ood_queries[j], -(int64_t)(j + 1));
        }
        previous_rc = run.sample();
        job.stir.push_back(std::move(round));
        const ArithmeticDomain squared = domain.pow(2);   // stir.rs:1149-1155
        domain = squared.with_offset(mont_mul(squared.offset, domain.offset));
        previous_root = current_root;
    }
    const Xfe folding_randomness = run.sample();
    const DecodedItem& final_polynomial = run.dequeue(POLYNOMIAL);
    const u64 n_final = final_polynomial.payload_words / 3;
    job.require((n_final ? n_final - 1 : 0) <= stir.final_degree, VERDICT_LAST_ROUND_POLYNOMIAL_HAS_TOO_HIGH_DEGREE);
    StirRound last = queries(domain, stir.final_num_in_domain_queries, previous_root);
    last.folding_randomness = folding_randomness, last.degree_correction_randomness = previous_rc;
    job.stir_want.assign(points.size(), ZERO);
    if (n_final && !points.empty()) tvm_host_xfe_poly_eval(run.payload(final_polynomial), n_final, points[0].c, points.size(), 0, job.stir_want[0].c);
    answers_site(last);
    job.stir.push_back(std::move(last));
    job.stir_final = job.defer(VERDICT_LAST_ROUND_POLYNOMIAL_EVALUATION_MISMATCH);
    job.have_stir_final = true;
}

struct Clock {
    double* ms;   // six stages, or null
    std::chrono::steady_clock::time_point mark = std::chrono::steady_clock::now();
    void lap(int stage) {
        const auto now = std::chrono::steady_clock::now();
        if (ms) ms[stage] += std::chrono::duration<double, std::milli>(now - mark).count();
        mark = now;
    }
};

// the host's pass over one job
void walk_job(const Context& c, Job& job, Clock& clock) {
    const tvmh_verify_job& in = *job.in;
    try {
        try {
            job.walk.items = decode_proof(in.h_proof, in.proof_words);
        } catch (const VerificationFailure&) {
            clock.lap(Verifier::STAGE_DECODE);
            throw;
        }
        clock.lap(Verifier::STAGE_DECODE);
        job.front = walk_front(c, job.walk, job.claim, in.security_level, in.log2_expansion, in.ldt_choice);
        clock.lap(Verifier::STAGE_TRANSCRIPT_AIR);
        const StarkParameters& p = job.front.p;
        const u64 checks = p.num_collinearity_checks;
        // the low-degree test (stark.rs:1577-1590)
        job.use_fri = !job.front.use_stir;
        if (job.use_fri) fri_walk(job);
        else stir_walk(job);
        job.require(job.indices.size() == checks && job.revealed.size() == 3 * checks, VERDICT_INCORRECT_NUMBER_OF_ROW_INDICES);
        // the revealed rows against their roots (stark.rs:1592-1672)
        Walk& run = job.walk;
        auto rows_of = [&](int variant, u64 width, const u64* root, uint32_t wrong_number, uint32_t wrong_path) {
            const DecodedItem& rows = run.dequeue(variant);
            job.require(rows.payload_words == checks * width, wrong_number);
            const DecodedItem& auth = run.dequeue(AUTH_STRUCTURE);
            job.queue(Inclusion{p.ldt.length, job.indices, {}, std::vector<u64>(run.payload(rows), run.payload(rows) + checks * width), width,
                                run.payload(auth), root, auth.payload_words / 5, wrong_path});
            return run.payload(rows);
        };
        job.main_rows = rows_of(MAIN_ROWS, NUM_MAIN, job.front.main_root, VERDICT_INCORRECT_NUMBER_OF_MAIN_ROWS, VERDICT_MAIN_CODEWORD_AUTHENTICATION_FAILURE);
        job.aux_rows = rows_of(AUX_ROWS, NUM_AUX * 3, job.front.aux_root, VERDICT_INCORRECT_NUMBER_OF_AUX_ROWS, VERDICT_AUX_CODEWORD_AUTHENTICATION_FAILURE);
        job.quot_rows = rows_of(QUOTIENT_SEGMENT_ELEMENTS, 15, job.front.quot_root, VERDICT_INCORRECT_NUMBER_OF_QUOTIENT_SEGMENT_ELEMENTS,
                                VERDICT_QUOTIENT_CODEWORD_AUTHENTICATION_FAILURE);
        // the combination codeword at the revealed rows (stark.rs:1674-1755)
        job.combination = job.defer(VERDICT_COMBINATION_CODEWORD_MISMATCH);
        job.have_deep = checks != 0;
        job.require(run.next == run.items.size(), VERDICT_SUPERFLUOUS_PROOF_ITEMS);
    } catch (const VerificationFailure& f) {   // host-decidable: after every site recorded so far (Job::require has taken its own)
        job.fail(job.site(), f.verdict);
    }
    clock.lap(Verifier::STAGE_LDT);
}

template <class T>
std::vector<const u64*> pointers(const std::vector<T*>& of, std::vector<u64> T::*member) {
    std::vector<const u64*> out;
    for (const T* t : of) out.push_back((t->*member).data());
    return out;
}

void fri_on_device(const Context& c, std::vector<Job*>& jobs) {
    std::vector<FriWork*> folds, lasts;
    for (Job* j : jobs) {
        if (j->use_fri && j->fri.have_folds && !j->fri.indices.empty()) folds.push_back(&j->fri);
        if (j->use_fri && j->fri.have_folds) lasts.push_back(&j->fri);   // (the last codeword's checks precede the walk's last host checks)
    }
    if (!folds.empty()) {
        const size_t n = folds.size();
        std::vector<tvm_domain> domains(n);
        std::vector<uint32_t> rounds(n), flags(n);
        std::vector<u64> checks(n);
        std::vector<u64*> out(n);
        for (size_t g = 0; g < n; g++) {
            FriWork& f = *folds[g];
            domains[g] = f.first_domain.c(), rounds[g] = f.num_rounds, checks[g] = f.indices.size();
            f.folded.assign(3 * f.indices.size(), 0);
            out[g] = f.folded.data();
        }
        c.check(tvm_verifier_fri_folds_batch(c.raw(), (uint32_t)n, domains.data(), rounds.data(), checks.data(),
                                             pointers(folds, &FriWork::challenges).data(), pointers(folds, &FriWork::indices).data(),
                                             pointers(folds, &FriWork::a_leaves).data(), pointers(folds, &FriWork::b_leaves).data(), out.data(),
                                             flags.data()), "tvm_verifier_fri_folds_batch");
        for (uint32_t flag : flags)
            if (flag) throw Error(TVM_ERR_DEVICE, "tvm_verifier_fri_folds_batch refused a group the host derived");
    }
    if (lasts.empty()) return;
    const size_t n = lasts.size();
    std::vector<u64> lengths(n), points(3 * n), roots(5 * n), values(3 * n);
    std::vector<const u64*> codewords(n);
    std::vector<uint32_t> flags(n);
    for (size_t g = 0; g < n; g++) {
        lengths[g] = lasts[g]->last_len, codewords[g] = lasts[g]->codeword;
        std::memcpy(&points[3 * g], lasts[g]->x.c, sizeof(Xfe));   // (zero where the walk ended before x was sampled: the value is not read)
    }
    c.check(tvm_verifier_fri_last_rounds(c.raw(), (uint32_t)n, lengths.data(), codewords.data(), points.data(), roots.data(), values.data(),
                                         flags.data()), "tvm_verifier_fri_last_rounds");
    for (size_t g = 0; g < n; g++) {
        FriWork& f = *lasts[g];
        if (flags[g] == TVM_NOT_APPLICABLE) {   // a last codeword beyond the kernel's bound: Verifier::verify's three calls
            const DeviceBuffer d_codeword = upload(c, std::vector<u64>(f.codeword, f.codeword + 3 * f.last_len));
            const DeviceBuffer nodes(c, 10 * f.last_len);
            c.check(tvm_codeword_merkle_tree(c.raw(), d_codeword.ptr(), f.last_len, nodes.ptr()), "tvm_codeword_merkle_tree");
            const std::vector<u64> root = merkle_root(c, nodes);
            std::memcpy(f.device_root, root.data(), sizeof(f.device_root));
            const DeviceBuffer interpolant = ArithmeticDomain::of_length(f.last_len).interpolate(c, d_codeword.ptr(), 3);
            c.check(tvm_evaluate_at_points(c.raw(), interpolant.ptr(), f.last_len, f.x.c, 1, f.at_x.c), "tvm_evaluate_at_points");
        } else if (flags[g]) {
            throw Error(TVM_ERR_DEVICE, "tvm_verifier_fri_last_rounds refused a group the host derived");
        } else {
            std::memcpy(f.device_root, &roots[5 * g], sizeof(f.device_root));
            std::memcpy(f.at_x.c, &values[3 * g], sizeof(Xfe));
        }
    }
}

void stir_on_device(const Context& c, std::vector<Job*>& jobs) {
    size_t max_rounds = 0;
    for (Job* j : jobs)
        if (!j->use_fri) max_rounds = std::max(max_rounds, j->stir.size());
    for (size_t r = 0; r < max_rounds; r++) {
        std::vector<StirRound*> rounds, previous;   // the rounds r that have queries, and the round before each (null: none)
        for (Job* j : jobs)
            if (!j->use_fri && r < j->stir.size() && !j->stir[r].roots.empty())
                rounds.push_back(&j->stir[r]), previous.push_back(r ? &j->stir[r - 1] : nullptr);
        if (rounds.empty()) continue;
        const size_t n = rounds.size();
        // the answer polynomials of the previous rounds' quotient sets
        std::vector<std::vector<Xfe>> set_answers(n);
        std::vector<uint32_t> k(n, 0), flags(n, 0);
        std::vector<const u64*> set_points(n, nullptr), set_values(n, nullptr), polys(n, nullptr);
        std::vector<u64*> poly_out(n, nullptr);
        bool any = false;
        for (size_t g = 0; g < n; g++) {
            if (!previous[g] || previous[g]->set_points.empty()) continue;
            const StirRound& before = *previous[g];
            for (int64_t source : before.set_source) set_answers[g].push_back(source >= 0 ? before.answers[(size_t)source] : before.ood_values[(size_t)(-source - 1)]);
            k[g] = (uint32_t)before.set_points.size();
            rounds[g]->answer_poly.assign(k[g], ZERO);
            set_points[g] = before.set_points[0].c, set_values[g] = set_answers[g][0].c, poly_out[g] = rounds[g]->answer_poly[0].c;
            polys[g] = poly_out[g];
            any = true;
        }
        if (any) {
            c.check(tvm_xfe_interpolate_batch(c.raw(), (uint32_t)n, k.data(), set_points.data(), set_values.data(), poly_out.data(), flags.data()),
                    "tvm_xfe_interpolate_batch");
            for (size_t g = 0; g < n; g++) {
                int32_t status = flags[g] == 1 ? TVM_ERR_INVALID_ARGUMENT : TVM_OK;
                if (flags[g] == TVM_NOT_APPLICABLE)   // more than 256 points: the host's interpolation, as tvm_xfe_interpolate takes it
                    status = tvm_host_xfe_interpolate(set_points[g], set_values[g], k[g], poly_out[g]);
                // a repeated point: the round's flag; its zero polynomial only feeds checks with higher ordinals
                if (status == TVM_ERR_INVALID_ARGUMENT) rounds[g]->answer_poly.assign(k[g], ZERO), rounds[g]->repeated = true;
                else c.check(status, "tvm_host_xfe_interpolate");
            }
        }
        std::vector<uint32_t> ff(n);
        std::vector<u64> kth(n), randomness(3 * n), rc(3 * n, 0), n_queries(n);
        std::vector<u64*> out(n);
        for (size_t g = 0; g < n; g++) {
            StirRound& round = *rounds[g];
            ff[g] = (uint32_t)round.ff, kth[g] = round.kth_root, n_queries[g] = round.roots.size();
            std::memcpy(&randomness[3 * g], round.folding_randomness.c, sizeof(Xfe));
            std::memcpy(&rc[3 * g], round.degree_correction_randomness.c, sizeof(Xfe));
            round.answers.assign(round.roots.size(), ZERO);
            out[g] = round.answers[0].c;
        }
        c.check(tvm_verifier_stir_answers_batch(c.raw(), (uint32_t)n, ff.data(), kth.data(), randomness.data(), k.data(), set_points.data(), polys.data(),
                                                rc.data(), n_queries.data(), pointers(rounds, &StirRound::values).data(),
                                                pointers(rounds, &StirRound::roots).data(), out.data(), flags.data()), "tvm_verifier_stir_answers_batch");
        for (uint32_t flag : flags)
            if (flag) throw Error(TVM_ERR_DEVICE, "tvm_verifier_stir_answers_batch refused a group the host derived");
    }
}

void deep_on_device(const Context& c, std::vector<Job*>& jobs) {
    std::vector<Job*> deep;
    for (Job* j : jobs)
        if (j->have_deep) deep.push_back(j);
    if (deep.empty()) return;
    const size_t n = deep.size();
    std::vector<tvm_domain> domains(n);
    std::vector<u64> w_q(15 * n), w_d(12 * n), points(12 * n), values(12 * n), n_rows(n);
    std::vector<const u64*> w_ma(n), main_rows(n), aux_rows(n), quot_rows(n), row_indices(n);
    std::vector<u64*> out(n);
    std::vector<uint32_t> flags(n);
    for (size_t g = 0; g < n; g++) {
        Job& j = *deep[g];
        const Front& f = j.front;
        domains[g] = f.p.ldt.c(), n_rows[g] = j.indices.size();
        std::memcpy(&w_q[15 * g], f.w_q[0].c, 15 * sizeof(u64)), std::memcpy(&w_d[12 * g], f.w_d[0].c, 12 * sizeof(u64));
        std::memcpy(&points[12 * g], f.ood_points[0].c, 12 * sizeof(u64)), std::memcpy(&values[12 * g], f.ood_values[0].c, 12 * sizeof(u64));
        w_ma[g] = f.w_ma[0].c, main_rows[g] = j.main_rows, aux_rows[g] = j.aux_rows, quot_rows[g] = j.quot_rows, row_indices[g] = j.indices.data();
        j.deep.assign(3 * j.indices.size(), 0);
        out[g] = j.deep.data();
    }
    c.check(tvm_verifier_deep_values_batch(c.raw(), (uint32_t)n, domains.data(), w_ma.data(), w_q.data(), w_d.data(), points.data(), values.data(),
                                           n_rows.data(), main_rows.data(), aux_rows.data(), quot_rows.data(), row_indices.data(), out.data(),
                                           flags.data()), "tvm_verifier_deep_values_batch");
    for (uint32_t flag : flags)
        if (flag) throw Error(TVM_ERR_DEVICE, "tvm_verifier_deep_values_batch refused a group the host derived");
}

// every deferred check of a job against the device's results; the verdict is the failing check with the lowest ordinal
void decide(Job& job, const std::vector<char>& inclusion_failed, size_t first_inclusion) {
    for (size_t t = 0; t < job.inclusions.size(); t++)
        if (inclusion_failed[first_inclusion + t]) job.fail(job.inclusion_ordinal[t], job.inclusions[t].verdict);
    if (job.use_fri && job.fri.have_folds) {
        const FriWork& f = job.fri;
        if (std::memcmp(f.device_root, f.root, sizeof(f.device_root))) job.fail(f.bad_root);
        for (size_t j = 0; j < f.indices.size(); j++)
            if (std::memcmp(&f.codeword[3 * (f.indices[j] % f.last_len)], &f.folded[3 * j], 3 * sizeof(u64))) job.fail(f.mismatch);
        if (f.have_last && !xfe_eq(f.claimed, f.at_x)) job.fail(f.evaluation);
    }
    if (!job.use_fri) {
        for (const StirRound& round : job.stir)
            if (round.repeated) job.fail(round.repeated_point);
        if (job.have_stir_final) {
            const std::vector<Xfe>& got = job.stir.back().answers;
            for (size_t j = 0; j < got.size(); j++)
                if (!xfe_eq(got[j], job.stir_want[j])) job.fail(job.stir_final);
        }
    }
    if (job.have_deep && job.deep != job.revealed) job.fail(job.combination);
}

// A chunk's staged arrays go to the device as ONE pageable copy per stage, and per byte such a copy costs more the larger it is: measured
// (profiles/verify_batch_time.txt's first visit), 16 proofs of 2^16 rows per chunk took 1.1 ms each, 64 took 2.4 ms each -- the loop's time.
const u64 DEFAULT_CHUNK = 16;                 // jobs per chunk (TVMH_OPTION_VERIFY_BATCH_CHUNK = 0)
const u64 MAX_TREES_PER_JOB = 40;             // three row openings and at most 33 low-degree-test rounds (heights below 2^32)
const u64 MAX_CHUNK_PROOF_WORDS = 1ull << 21; // a chunk ends once it holds 16 MiB of proofs

}  // namespace
}  // namespace triton_vm

extern "C" int32_t tvmh_verify_batch(tvm_ctx* ctx, const tvmh_verify_job* jobs, uint64_t n_jobs, uint32_t* verdicts, uint64_t* h_indices,
                                     uint64_t indices_stride, uint64_t* n_indices, double* stage_ms, char* error, uint64_t error_capacity) {
    using namespace triton_vm;
    if (error && error_capacity) error[0] = 0;
    return guarded(error, error_capacity, [&] {
        if (!ctx || (n_jobs && (!jobs || !verdicts)) || (indices_stride && !h_indices))
            throw Error(TVM_ERR_INVALID_ARGUMENT, "tvmh_verify_batch: null context, jobs, verdicts or indices");
        for (u64 i = 0; i < n_jobs; i++) {   // every job's arguments as tvmh_verify takes them, before any work
            const tvmh_verify_job& in = jobs[i];
            const std::string job = "tvmh_verify_batch: job " + std::to_string(i) + ": ";
            if ((!in.h_proof && in.proof_words) || (in.n_public_input && !in.h_public_input) || (in.n_public_output && !in.h_public_output))
                throw Error(TVM_ERR_INVALID_ARGUMENT, job + "null proof or claim with a non-zero length");
            if (in.ldt_choice > 2) throw Error(TVM_ERR_INVALID_ARGUMENT, job + "the LDT choice is 0 (FRI), 1 (STIR) or 2 (Stark::ldt's rule)");
            if (!in.security_level || in.security_level > 512 || !in.log2_expansion || in.log2_expansion > 8)
                throw Error(TVM_ERR_INVALID_ARGUMENT, job + "security level 1..512, log2 expansion 1..8");
        }
        if (stage_ms) std::fill(stage_ms, stage_ms + Verifier::NUM_STAGES, 0.0);
        const Context c(ctx);
        const u64 option = tvmh_get_option(TVMH_OPTION_VERIFY_BATCH_CHUNK), chunk_jobs = option ? option : DEFAULT_CHUNK;
        Clock clock{stage_ms};
        for (u64 first = 0; first < n_jobs;) {
            // the chunk: its jobs walked on the host
            std::vector<std::unique_ptr<Job>> chunk;
            u64 words = 0;
            while (first + chunk.size() < n_jobs && chunk.size() < chunk_jobs &&
                   (chunk.size() + 1) * MAX_TREES_PER_JOB <= TVM_VERIFIER_MAX_TREES && (chunk.empty() || words < MAX_CHUNK_PROOF_WORDS)) {
                const tvmh_verify_job& in = jobs[first + chunk.size()];
                chunk.emplace_back(new Job(&in));
                Job& job = *chunk.back();
                job.claim = make_claim(in.h_program_digest, in.h_public_input, in.n_public_input, in.h_public_output, in.n_public_output);
                job.claim.version = in.version;
                words += in.proof_words;
                walk_job(c, job, clock);
            }
            std::vector<Job*> refs;
            std::vector<Inclusion*> inclusions;
            std::vector<size_t> first_inclusion;
            for (auto& job : chunk) {
                refs.push_back(job.get());
                first_inclusion.push_back(inclusions.size());
                for (Inclusion& t : job->inclusions) inclusions.push_back(&t);
            }
            // the device work, stage by stage
            std::vector<char> inclusion_failed;
            if (!inclusions.empty()) inclusion_failed = run_inclusion_jobs(c, inclusions, [&](int stage) { clock.lap(stage); });
            fri_on_device(c, refs);
            stir_on_device(c, refs);
            clock.lap(Verifier::STAGE_LDT);
            deep_on_device(c, refs);
            clock.lap(Verifier::STAGE_DEEP_VALUES);
            for (size_t i = 0; i < chunk.size(); i++) {
                Job& job = *chunk[i];
                decide(job, inclusion_failed, first_inclusion[i]);
                const bool accepted = job.verdict == VERDICT_ACCEPTED;
                verdicts[first + i] = job.verdict;
                if (n_indices) n_indices[first + i] = accepted ? job.indices.size() : 0;
                if (accepted && indices_stride >= job.indices.size() && !job.indices.empty())
                    std::memcpy(h_indices + (first + i) * indices_stride, job.indices.data(), job.indices.size() * sizeof(u64));
            }
            clock.lap(Verifier::STAGE_LDT);
            first += chunk.size();
        }
    });
}
