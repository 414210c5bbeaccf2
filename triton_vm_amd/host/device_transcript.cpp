// device_transcript.cpp -- the stretches of a proof that run with the Fiat-Shamir sponge on the device, front to back: steps 4-10
// (TVMH_OPTION_DEVICE_FRONT), 12-16 (_MIDDLE), FRI's query phase with the openings of step 19 (_TAIL), the rounds of STIR (_STIR).  Each
// is one call into the library and a replay of its enqueues and samplings on the host's sponge (Replay, host_internal.hpp), which must
// arrive where the device did; each counts the proofs that took it.  ProofSteps::prove and ::fri (triton_host.cpp) decide who is asked.
#include "triton_host.hpp"
#include "host_internal.hpp"

#include <algorithm>
#include <atomic>
#include <memory>

namespace triton_vm {

enum Stretch { TAIL, STIR, MIDDLE, FRONT };
static std::atomic<uint64_t> g_device_proofs[4] = {{0}, {0}, {0}, {0}};   // tvmh_device_{tail,stir,middle,front}_proofs, by Stretch

// TVMH_OPTION_DEVICE_FRONT: steps 4-10 queued without a wait -- main LDE, main tree, the main root into the sponge and the 63 challenges
// (tvm_front_challenges), extend, aux LDE, aux tree, the aux root into the sponge and the 604 quotient weights
// (tvm_front_quotient_weights), the quotient and the segments -- with challenges and weights read where the device left them.  The
// download of the block's head and replay_front are owed afterwards.  false: the call does not apply (no whole trees on one GPU: the
// sharded and coset-wise provers; `extend` without `extend_device`; TVMH_OPTION_CHECK_TRACE, which needs the challenges on the host
// and decides the AIR's mode there) and nothing was queued or enqueued.
bool ProofSteps::device_front(u64 zeta, u64 poly_len, DeviceBuffer& front, tvm_table*& segments, DeviceBuffer& polys) {
    if (!whole() || (extend && !extend_device) || tvmh_get_option(TVMH_OPTION_CHECK_TRACE)) return false;
    front = DeviceBuffer(c, TVM_FRONT_BLOCK_WORDS);
    u64* d = front.ptr();
    mark("main LDE");
    extend_master_table(MAIN);
    mark("main Merkle");
    c.check(tvm_front_challenges(c.raw(), build_whole_tree(MAIN, nullptr), ps.sponge_state(), claim.program_digest, claim.input.data(),
                                 claim.input.size(), claim.output.data(), claim.output.size(), d), "tvm_front_challenges");
    mark("extend");
    if (extend_device) extend_device(d + TVM_FRONT_CHALLENGES);
    mark("aux LDE");
    extend_master_table(AUX);
    mark("aux Merkle");
    c.check(tvm_front_quotient_weights(c.raw(), build_whole_tree(AUX, nullptr), d), "tvm_front_quotient_weights");
    mark("AIR quotients");
    segments = quotient_segments(d + TVM_FRONT_CHALLENGES, d + TVM_FRONT_WEIGHTS, zeta, polys, poly_len);
    return true;
}
void ProofSteps::fetch_front(const u64* d_front, std::vector<u64>& head, bool wait) {
    head.resize(TVM_FRONT_HEAD_WORDS);
    c.check(tvm_front_block(c.raw(), d_front, head.data(), head.size(), wait ? 1 : 0), "tvm_front_block");
}
// The host's side of device_front, once the head of the block is here: the two roots are enqueued from it and both samplings replayed
// on this host's sponge, which must arrive at the same 63 challenges, the same weight scalar and the same state.
void ProofSteps::replay_front(const std::vector<u64>& head) {
    const u64* b = head.data();
    Replay replay{ps};
    ps.enqueue("main root", b + TVM_FRONT_MAIN_ROOT, 5);
    const std::vector<Xfe> challenges = derive_challenges(replay.scalars(NUM_SAMPLED_CHALLENGES, b + TVM_FRONT_CHALLENGES, "the challenges"), claim);
    replay.agree(std::memcmp(challenges[0].c, b + TVM_FRONT_CHALLENGES, 3 * TVM_NUM_CHALLENGES * sizeof(u64)) == 0, "the challenges");   // (the derived four)
    ps.enqueue("aux root", b + TVM_FRONT_AUX_ROOT, 5);
    replay.scalars(1, b + TVM_FRONT_WEIGHT_SCALAR, "the scalar of the quotient weights");
    replay.state(b + TVM_FRONT_STATE, "the state after the quotient weights");
    g_device_proofs[FRONT]++;
}

// TVMH_OPTION_DEVICE_MIDDLE: the quotient root into the sponge and steps 13-16 in one call, the sponge on the device
// (tvm_out_of_domain_to_deep: one stream synchronisation instead of five) -- then the root and the six out-of-domain items are enqueued
// from the block that came back and both samplings are replayed on this host's sponge, which must arrive at the same alpha, the same
// three weights and the same state.  false: the call does not apply (no whole tables and whole quotient tree here: the sharded and
// coset-wise provers) and nothing was enqueued or committed.
bool ProofSteps::device_middle(const tvm_table* segments, const DeviceBuffer& polys, u64 poly_len, const ArithmeticDomain& short_dom, u64 zeta, Xfe& a4,
                               DeviceBuffer& combination, u64* d_front) {
    if (!whole()) return false;
    const u64* tree = build_whole_tree(QUOT, segments);
    mark("out-of-domain rows to DEEP");
    const u64 n_main = main.n_cols(), n_aux = aux.n_cols();
    std::vector<u64> block(TVM_MIDDLE_BLOCK_WORDS(n_main, n_aux));
    combination = DeviceBuffer(c, short_dom.length * 3);
    if (d_front) {   // the front's words come back with this call's synchronisation; the sponge goes from the one to the other on the device
        std::vector<u64> head;
        fetch_front(d_front, head, false);
        const int32_t status = tvm_out_of_domain_to_deep_device_state(c.raw(), main.trace(), n_main, main.randomizers(), aux.trace(), n_aux,
                                                                      aux.randomizers(), p.trace.length, p.h, p.trace.c(), polys.ptr(), poly_len, segments,
                                                                      tree, short_dom.c(), zeta, d_front + TVM_FRONT_STATE, combination.ptr(),
                                                                      block.data(), block.size());
        if (status != TVM_OK) (void)tvm_sync(c.raw());   // (a refusal queues nothing and waits for nothing: `head` is still being written)
        c.check(status, "tvm_out_of_domain_to_deep_device_state");
        replay_front(head);
    } else {
        c.check(tvm_out_of_domain_to_deep(c.raw(), main.trace(), n_main, main.randomizers(), aux.trace(), n_aux, aux.randomizers(), p.trace.length,
                                          p.h, p.trace.c(), polys.ptr(), poly_len, segments, tree, short_dom.c(), zeta, ps.sponge_state(),
                                          combination.ptr(), block.data(), block.size()), "tvm_out_of_domain_to_deep");
    }
    const u64 *b = block.data(), *points = b + TVM_MIDDLE_POINTS, *rows_main = b + TVM_MIDDLE_MAIN_ROWS, *rows_aux = b + TVM_MIDDLE_AUX_ROWS(n_main),
              *seg = b + TVM_MIDDLE_SEGMENTS(n_main, n_aux);
    Replay replay{ps};
    ps.enqueue("quot root", b + TVM_MIDDLE_ROOT, 5);
    replay.scalars(1, points, "the out-of-domain point");
    ps.enqueue("ood main", rows_main, n_main * 3);
    ps.enqueue("ood aux", rows_aux, n_aux * 3);
    ps.enqueue("ood main next", rows_main + n_main * 3, n_main * 3);
    ps.enqueue("ood aux next", rows_aux + n_aux * 3, n_aux * 3);
    u64 quot_p[12], quot_r[12];   // segments 0..3 at alpha^4, 1..4 at (zeta alpha)^4, out of [5][2][3]
    for (int k = 0; k < 4; k++) {
        std::memcpy(quot_p + 3 * k, seg + 3 * (2 * k), 3 * sizeof(u64));
        std::memcpy(quot_r + 3 * k, seg + 3 * (2 * (k + 1) + 1), 3 * sizeof(u64));
    }
    ps.enqueue("ood quot p", quot_p, 12);
    ps.enqueue("ood quot r", quot_r, 12);
    replay.scalars(3, b + TVM_MIDDLE_WEIGHTS(n_main, n_aux), "the combination weights");
    replay.state(b + TVM_MIDDLE_STATE(n_main, n_aux), "the state after the combination weights");
    std::memcpy(a4.c, points + 6, 3 * sizeof(u64));   // step 18 checks it against the revealed points
    g_device_proofs[MIDDLE]++;
    return true;
}

// TVMH_OPTION_DEVICE_TAIL: everything of Fri::prove behind the commit phase (fri.rs:265-319) and the trace openings of step 19 in one
// call, the sponge on the device (tvm_fri_query_and_open) -- then the two enqueues and the sampling are replayed on this host's sponge,
// which must arrive at the same indices and the same state.  false: the call does not apply (no whole tables and trees here, more
// checks than TVM_TAIL_MAX_INDICES) and nothing was enqueued.
bool ProofSteps::fri_device_tail(const std::vector<FriRound>& rounds, std::vector<u64>& a_indices) {
    const WholeTables* t = whole();
    if (!t || !t->table[QUOT] || !t->nodes[MAIN].ptr() || !t->nodes[AUX].ptr() || !t->nodes[QUOT].ptr()) return false;
    const u64* table_nodes[3] = {t->nodes[MAIN].ptr(), t->nodes[AUX].ptr(), t->nodes[QUOT].ptr()};
    const uint32_t n_rounds = (uint32_t)rounds.size() - 1, n_items = TVM_TAIL_ITEMS(n_rounds);
    const u64 n_last = rounds.back().dom.length, q = p.num_collinearity_checks;
    std::vector<const u64*> d_cw, d_nodes;
    for (size_t r = 0; r < rounds.size(); r++) {
        if (r) d_cw.push_back(rounds[r].cw);
        d_nodes.push_back(rounds[r].nodes.ptr());
    }
    u64 state[16], n_payload = 0;
    std::vector<u64> indices(q), last(3 * n_last), last_poly(3 * n_last), directory(2 * (size_t)n_items);
    // (room for the bound -- every list n_checks full paths, some MB at 2^20 rows -- but not filled: only the pages the proof's words reach are touched)
    const u64 capacity = tvm_fri_query_and_open_payload_bound(rounds[0].dom.c(), n_rounds, q, t->table);
    const std::unique_ptr<u64[]> payload(new u64[capacity ? capacity : 1]);
    const int32_t status = tvm_fri_query_and_open(c.raw(), ps.sponge_state(), rounds[0].cw, rounds[0].dom.c(), n_rounds, d_cw.data(), d_nodes.data(), q,
                                                  t->table, table_nodes, p.ldt.length, state, indices.data(), last.data(), last_poly.data(),
                                                  directory.data(), payload.get(), capacity, &n_payload);
    if (status == TVM_NOT_APPLICABLE) return false;
    c.check(status, "tvm_fri_query_and_open");
    Replay replay{ps};
    ps.enqueue("fri last codeword", last.data(), last.size());
    ps.enqueue("fri last polynomial", last_poly.data(), last_poly.size());
    a_indices = replay.indices(p.ldt.length, q, indices.data(), "the FRI query indices");
    replay.state(state, "the FRI query indices");
    auto item = [&](size_t k) { return std::make_pair(payload.get() + directory[2 * k], directory[2 * k + 1]); };
    for (size_t k = 0; 2 * k + 6 < n_items; k++) {   // round 0 at the a indices, then rounds 0 .. n_rounds - 1 at the b indices
        const std::string round = std::to_string(k ? k - 1 : 0);
        ps.enqueue("fri response " + round, item(2 * k).first, item(2 * k).second);
        ps.enqueue("fri auth " + round, item(2 * k + 1).first, item(2 * k + 1).second);
    }
    for (int w = 0; w < 3; w++) {   // kept for step 19
        const size_t k = n_items - 6 + 2 * (size_t)w;
        tail_openings.rows[w].assign(item(k).first, item(k).first + item(k).second);
        tail_openings.auth[w].assign(item(k + 1).first, item(k + 1).first + item(k + 1).second);
    }
    have_tail_openings = true;
    g_device_proofs[TAIL]++;
    return true;
}

// TVMH_OPTION_DEVICE_STIR: the whole of Stir::prove in one call, the sponge on the device (tvm_stir_prove_rounds: two stream
// synchronisations, no host work between the rounds) -- then every enqueue and every sampling is replayed on this host's sponge, which
// must arrive at the same scalars, the same indices and the same state.  false: the call does not apply (a round with more than
// TVM_TAIL_MAX_INDICES in-domain queries, or a full round with more than 256 queries in all) and nothing was enqueued.
bool Stir::prove_on_device(const Context& c, const u64* d_codeword, ProofStream& ps, std::vector<u64>& first_round_indices) const {
    const uint32_t R = (uint32_t)round_queries.size();
    std::vector<u64> pairs, queries;
    u64 n_ood_all = 0, n_queries_all = final_num_in_domain_queries, n_final = initial_domain.length;
    for (const auto& q : round_queries) {
        pairs.push_back(q.first), pairs.push_back(q.second), queries.push_back(q.first);
        n_ood_all += q.second, n_queries_all += q.first;
    }
    queries.push_back(final_num_in_domain_queries);
    for (uint32_t r = 0; r <= R; r++) n_final = (n_final + folding_factor - 1) / folding_factor;
    const u64 capacity = tvm_stir_prove_rounds_payload_bound(initial_domain.c(), (uint32_t)folding_factor, R, pairs.data(), final_num_in_domain_queries);
    u64 state[16], n_payload = 0;
    std::vector<u64> roots(5 * ((size_t)R + 1)), indices(n_queries_all), unique(n_queries_all), unique_counts((size_t)R + 1), final_words(3 * n_final),
        directory(4 * ((size_t)R + 1)), ood_values(3 * n_ood_all + 1);
    std::vector<Xfe> scalars(2 * (size_t)R + 1 + n_ood_all);
    // (room for the bound -- every index distinct, full paths -- but not filled: only the pages the proof's words reach are touched)
    const std::unique_ptr<u64[]> payload(new u64[capacity ? capacity : 1]);
    const int32_t status = tvm_stir_prove_rounds(c.raw(), ps.sponge_state(), d_codeword, initial_domain.c(), (uint32_t)folding_factor, R, pairs.data(),
                                                 final_num_in_domain_queries, final_degree, state, roots.data(), scalars[0].c, ood_values.data(),
                                                 indices.data(), unique.data(), unique_counts.data(), final_words.data(), directory.data(),
                                                 payload.get(), capacity, &n_payload);
    if (status == TVM_NOT_APPLICABLE) return false;
    c.check(status, "tvm_stir_prove_rounds");
    Replay replay{ps};
    // tree t's response: the indices the host samples must be the device's, and their first occurrences mod the folded length its list
    const u64 *scalar = scalars[0].c, *raw = indices.data(), *list = unique.data();
    ArithmeticDomain domain = initial_domain;
    auto respond = [&](uint32_t t) {
        const std::vector<u64> queried = replay.indices(domain.length, queries[t], raw, "the STIR query indices");
        const std::vector<u64> folded = unique_folded(queried, domain.length / folding_factor);
        replay.agree(folded.size() == unique_counts[t] && std::equal(folded.begin(), folded.end(), list), "the STIR query indices without repeats");
        ps.enqueue("stir response leafs", payload.get() + directory[4 * t], directory[4 * t + 1], folding_factor * 3);
        ps.enqueue("stir response auth", payload.get() + directory[4 * t + 2], directory[4 * t + 3]);
        raw += queries[t], list += queries[t];
        return queried;
    };
    ps.enqueue("stir root", roots.data(), 5);
    const u64* values = ood_values.data();
    for (uint32_t r = 0; r < R; r++) {
        const u64 n_ood = round_queries[r].second;
        replay.scalars(1, scalar, "a STIR folding randomness");
        ps.enqueue("stir root", roots.data() + 5 * ((size_t)r + 1), 5);
        replay.scalars(n_ood, scalar + 3, "the STIR out-of-domain points");
        ps.enqueue("stir ood values", n_ood ? values : nullptr, 3 * n_ood);
        const std::vector<u64> queried = respond(r);
        if (r == 0) first_round_indices = queried;
        replay.scalars(1, scalar + 3 * (1 + n_ood), "a STIR degree-correction randomness");
        scalar += 3 * (2 + n_ood), values += 3 * n_ood;
        ArithmeticDomain next = domain.pow(1ull << LOG2_DOMAIN_SHRINKAGE);
        domain = next.with_offset(mont_mul(next.offset, domain.offset));
    }
    replay.scalars(1, scalar, "the final STIR folding randomness");
    ps.enqueue("stir final polynomial", final_words.data(), final_words.size());
    const std::vector<u64> queried = respond(R);
    if (R == 0) first_round_indices = queried;
    replay.state(state, "the state after STIR");
    g_device_proofs[STIR]++;
    return true;
}

}  // namespace triton_vm

// how many proofs (STIR: calls of Stir::prove) of this process took each stretch so far
extern "C" uint64_t tvmh_device_tail_proofs(void) { return triton_vm::g_device_proofs[triton_vm::TAIL].load(); }
extern "C" uint64_t tvmh_device_stir_proofs(void) { return triton_vm::g_device_proofs[triton_vm::STIR].load(); }
extern "C" uint64_t tvmh_device_middle_proofs(void) { return triton_vm::g_device_proofs[triton_vm::MIDDLE].load(); }
extern "C" uint64_t tvmh_device_front_proofs(void) { return triton_vm::g_device_proofs[triton_vm::FRONT].load(); }
