// host_internal.hpp -- what the translation units of the C++ host share (triton_host.cpp, device_transcript.cpp, sharded_host.cpp,
// verifier.cpp): helpers, the steps of one proof (ProofSteps), the frame of an extern "C" entry point.  Not part of the interface:
// triton_host.hpp is.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "triton_host.hpp"

namespace triton_vm {

static const u64 NUM_MAIN = TVM_NUM_MAIN_COLUMNS, NUM_AUX = TVM_NUM_AUX_COLUMNS, NUM_SAMPLED_CHALLENGES = TVM_NUM_CHALLENGES - 4;

u64 bfe_add(u64 a, u64 b);
Xfe xfe_add(const Xfe& a, const Xfe& b);
Xfe xfe_mul(const Xfe& a, const Xfe& b);
Xfe xfe_scale(const Xfe& a, u64 s);
std::vector<Xfe> xfe_powers(const Xfe& x, u64 first, u64 n);
unsigned bit_length(u64 v);
std::vector<u64> merkle_root(const Context& c, const DeviceBuffer& nodes);  // node 1; drains the stream
// [twenty-first MerkleTree::authentication_structure, restated]: heap indices of the nodes a verifier cannot compute itself
std::vector<u64> auth_node_indices(u64 n_leaves, const std::vector<u64>& indices);
std::vector<Xfe> derive_challenges(std::vector<Xfe> sampled, const Claim& claim);  // Challenges::new (challenges.rs:85-121)
std::vector<u64> trace_randomizers_host(const uint8_t table_seed[32], u64 n_cols, u64 h, int fk);
DeviceBuffer upload(const Context& c, const std::vector<u64>& host);
// Stir::prove and Stir::prove_on_device: stir.rs:404-412, and .map(|i| i % len).unique()
static const int LOG2_DOMAIN_SHRINKAGE = 1;
static inline std::vector<u64> unique_folded(const std::vector<u64>& indices, u64 folded_len) {
    std::vector<u64> out;
    for (u64 i : indices)
        if (std::find(out.begin(), out.end(), i % folded_len) == out.end()) out.push_back(i % folded_len);
    return out;
}

// Many gathers with one round trip (tvm_gather_elements_batch): jobs are queued with their index lists, run() fills `out`.
struct GatherBatch {
    struct Job {
        const u64* src;
        uint32_t words;
        std::vector<u64> idx, out;
    };
    std::vector<Job> jobs;
    size_t add(const u64* src, uint32_t words, std::vector<u64> idx) {
        jobs.push_back(Job{src, words, std::move(idx), {}});
        return jobs.size() - 1;
    }
    void run(const Context& c) {
        if (jobs.empty()) return;
        std::vector<const uint64_t*> src, idx;
        std::vector<uint32_t> words;
        std::vector<uint64_t> n;
        std::vector<uint64_t*> out;
        for (Job& j : jobs) {
            j.out.assign(j.idx.size() * j.words, 0);
            src.push_back(j.src);
            words.push_back(j.words);
            idx.push_back(j.idx.data());
            n.push_back(j.idx.size());
            out.push_back(j.out.data());
        }
        c.check(tvm_gather_elements_batch(c.raw(), (uint32_t)jobs.size(), src.data(), words.data(), idx.data(), n.data(), out.data()),
                "tvm_gather_elements_batch");
    }
};

typedef std::vector<u64> Words;

struct TableGuard {
    const Context& c;
    tvm_table* t = nullptr;
    ~TableGuard() { if (t) tvm_table_free(c.raw(), t); }
};

// The host's sponge replaying what the device's did (device_transcript.cpp, ProofSteps::fri): a sampling on `ps`, compared with the
// words the device sampled.  One throw for every site.
struct Replay {
    ProofStream& ps;
    static void agree(bool same, const char* what) {
        if (!same) throw Error(TVM_ERR_DEVICE, std::string("the device's Fiat-Shamir sponge and the host's disagree on ") + what);
    }
    std::vector<Xfe> scalars(u64 n, const u64* device_words, const char* what) {   // (n = 0 compares nothing)
        std::vector<Xfe> mine = ps.sample_scalars(n);
        agree(n == 0 || std::memcmp(mine[0].c, device_words, n * sizeof(Xfe)) == 0, what);
        return mine;
    }
    std::vector<u64> indices(u64 upper_bound, u64 n, const u64* device_indices, const char* what) {
        std::vector<u64> mine = ps.sample_indices(upper_bound, n);
        agree(n == 0 || std::memcmp(mine.data(), device_indices, n * sizeof(u64)) == 0, what);
        return mine;
    }
    void state(const u64 device_state[16], const char* what) { agree(std::memcmp(ps.sponge_state(), device_state, 16 * sizeof(u64)) == 0, what); }
};

// One proof.  prove() is the statement sequence of Prover::prove (stark.rs:331-719) and fri() that of Fri::prove (fri.rs:212-319),
// each written once (triton_host.cpp; the stretches with the sponge on the device: device_transcript.cpp); the virtual steps are the ones that depend on where the data lies -- whole on one GPU
// (Prover, triton_host.cpp) or by cosets over ranks and passes (ShardedRun, sharded_host.cpp).  The hooks of
// triton_vm_amd/prover.py are the model.  A step's default is the single-GPU one where that is a line.
class ProofSteps {
public:
    enum Which { MAIN = 0, AUX = 1, QUOT = 2 };
    ProofSteps(const Context& c_, const StarkParameters& p_, const Claim& claim_, MasterTable& main_, MasterTable& aux_,
               const std::vector<Xfe>& quotient_randomizer_, const std::function<void(const std::vector<Xfe>&)>& extend_,
               const bool& assume_valid_trace_)
        : c(c_), p(p_), claim(claim_), main(main_), aux(aux_), quotient_randomizer(quotient_randomizer_), extend(extend_),
          assume_valid_trace(assume_valid_trace_) {}
    virtual ~ProofSteps() {}
    ProofStream prove();
    // `extend` with the 63 challenges in device memory (TVMH_OPTION_DEVICE_FRONT); a prover that sets `extend` alone keeps the host's front
    std::function<void(const u64*)> extend_device;

protected:
    struct Openings {   // of the three tables, by Which
        Words rows[3], auth[3];
    };
    struct WholeTables {                  // the single-GPU prover's, by Which
        const tvm_table* table[3] = {};   // MAIN, AUX: master(w).table(); QUOT: the segment table -- each as its commit saw it
        DeviceBuffer nodes[3];            // the three whole Merkle trees [2 L][5]
    };
    struct FriRound {
        ArithmeticDomain dom;
        const u64* cw = nullptr;   // the whole codeword; of a distributed round, this rank's elements
        DeviceBuffer nodes;        // the whole tree [2 n][5]; none: the round is distributed, answer_distributed knows its tree
    };
    struct FriQuery {
        size_t round;
        std::vector<u64> indices;
    };
    struct FriAnswer {
        Words leaves, auth;
    };
    const Context& c;
    const StarkParameters& p;
    const Claim& claim;
    MasterTable &main, &aux;
    const std::vector<Xfe>& quotient_randomizer;
    const std::function<void(const std::vector<Xfe>&)>& extend;
    const bool& assume_valid_trace;   // (a reference: a checked proof decides while `extend` runs)
    ProofStream ps;
    MasterTable& master(Which w) { return w == MAIN ? main : aux; }

    virtual void mark(const char* /*stage*/) {}
    // this rank's rows of a domain, and the rows of all ranks in row order (w words per row)
    virtual ArithmeticDomain local(const ArithmeticDomain& d) const { return d; }
    virtual DeviceBuffer gather_rows(DeviceBuffer&& rows, u64 /*n_local*/, uint32_t /*w*/, const char* /*what*/) { return std::move(rows); }
    // 4, 8: low-degree extend a master table; 5, 9, 12: commit to it (QUOT: to the segment table) -> the root
    virtual void extend_master_table(Which w) = 0;
    virtual Words commit(Which w, const tvm_table* segments) = 0;
    // 10: the quotient -> the segment table on this rank's LDT rows (the caller frees it) and the five segment polynomials
    virtual tvm_table* quotient_segments(const std::vector<Xfe>& challenges, const std::vector<Xfe>& weights, u64 zeta, DeviceBuffer& polys,
                                         u64 poly_len) = 0;
    // ... with the challenges and the weights in device memory (TVMH_OPTION_DEVICE_FRONT); only a prover with whole() is asked
    virtual tvm_table* quotient_segments(const u64* /*d_challenges*/, const u64* /*d_weights*/, u64 /*zeta*/, DeviceBuffer& /*polys*/, u64 /*poly_len*/) {
        throw Error(TVM_ERR_UNSUPPORTED, "quotient_segments from device arrays: the single-GPU prover only");
    }
    virtual Words out_of_domain_rows(const MasterTable& mt, const std::vector<Xfe>& points) { return mt.out_of_domain_rows(points); }
    // 15: the weighted sums wp, wr of the segments on this rank's rows of the short domain: rows of the segment table
    virtual void segment_combinations(const tvm_table* segments, const DeviceBuffer& polys, u64 poly_len, const ArithmeticDomain& short_rank,
                                      const Xfe* wp, const Xfe* wr, DeviceBuffer& cw_p, DeviceBuffer& cw_r);
    // 15: the combination of the trace columns (n_comb coefficients, XFE) on this rank's rows of the short domain.  A rank's share of
    // a domain is the general transform's business; the prover that holds the whole domain has a shorter route (WholeSteps)
    virtual DeviceBuffer combination_codeword(const ArithmeticDomain& short_rank, const DeviceBuffer& comb, u64 n_comb) {
        return short_rank.evaluate(c, comb.ptr(), n_comb, 3);
    }
    // FRI: the rounds whose tree is split over the ranks (roots enqueued, challenges sampled, folds done), appended to `rounds`;
    // `dom` moves on to the first round that is not.  -> that round's codeword in row order (after the last round: the last codeword)
    virtual DeviceBuffer fri_distributed_rounds(DeviceBuffer&& codeword, std::vector<FriRound>& /*rounds*/, ArithmeticDomain& /*dom*/) {
        return std::move(codeword);
    }
    virtual std::vector<FriAnswer> answer_distributed(const std::vector<FriQuery>& /*queries*/) { return {}; }
    // 19: the rows of the three tables at `indices` and the authentication structures of the three trees
    virtual Openings open(const tvm_table* segments, const std::vector<u64>& indices) = 0;
    // TVMH_OPTION_DEVICE_FRONT / _MIDDLE / _TAIL: the whole tables and whole trees, where this prover holds them on one GPU (the single-GPU
    // one); null (the sharded and coset-wise provers): those stretches of the proof keep the host's path
    virtual WholeTables* whole() { return nullptr; }
    // commit(w, ..) of a prover with whole(), the root left on the device (no round trip) -> the tree's nodes
    const u64* build_whole_tree(Which w, const tvm_table* segments);

private:
    std::vector<u64> fri(DeviceBuffer&& combination);   // -> the first-round indices
    bool fri_device_tail(const std::vector<FriRound>& rounds, std::vector<u64>& a_indices);
    // 13-16 on this rank's rows of the short domain -> the DEEP codeword; a4: the point alpha^4, which step 18 checks.  host_middle: the
    // host in the loop; device_middle: the quotient root and 13-16 in one device round trip (false: does not apply, nothing was done)
    DeviceBuffer host_middle(const tvm_table* segments, const DeviceBuffer& polys, u64 poly_len, const ArithmeticDomain& short_rank, u64 zeta, Xfe& a4);
    // d_front: the block of a device_front whose download and replay are still owed -- the middle starts from the block's sponge state,
    // and its one synchronisation serves both (the front is replayed before the middle's items are enqueued)
    bool device_middle(const tvm_table* segments, const DeviceBuffer& polys, u64 poly_len, const ArithmeticDomain& short_dom, u64 zeta, Xfe& a4,
                       DeviceBuffer& combination, u64* d_front);
    // 4-10 queued without a wait, the sponge on the device -> the front's block (its download and replay_front are owed), the segment
    // table (the caller frees it) and the segment polynomials; false: does not apply, nothing was queued or enqueued
    bool device_front(u64 zeta, u64 poly_len, DeviceBuffer& front, tvm_table*& segments, DeviceBuffer& polys);
    void fetch_front(const u64* d_front, std::vector<u64>& head, bool wait);
    void replay_front(const std::vector<u64>& head);
    Openings tail_openings;   // the openings of step 19 when fri_device_tail has fetched them
    bool have_tail_openings = false;
};

// ---- what every extern "C" entry point does around its body ------------------------------------------------------------
template <class F>
int32_t guarded(char* error, uint64_t error_capacity, F body) {
    try {
        body();
        return TVM_OK;
    } catch (const Error& e) {
        if (error && error_capacity) std::snprintf(error, error_capacity, "%s", e.what());
        return e.status ? e.status : TVM_ERR_INVALID_ARGUMENT;
    } catch (const std::exception& e) {
        if (error && error_capacity) std::snprintf(error, error_capacity, "%s", e.what());
        return TVM_ERR_DEVICE;
    }
}
inline Claim make_claim(const u64* h_program_digest, const u64* h_public_input, u64 n_public_input, const u64* h_public_output,
                        u64 n_public_output) {
    Claim claim;
    if (h_program_digest) std::memcpy(claim.program_digest, h_program_digest, sizeof(claim.program_digest));
    if (n_public_input) claim.input.assign(h_public_input, h_public_input + n_public_input);
    if (n_public_output) claim.output.assign(h_public_output, h_public_output + n_public_output);
    return claim;
}
inline void copy_proof_out(const Words& proof, u64* h_proof, u64 capacity, u64* proof_words) {
    if (proof_words) *proof_words = proof.size();
    if (h_proof && capacity >= proof.size()) std::memcpy(h_proof, proof.data(), proof.size() * sizeof(u64));
}
// use_stir: 0 = LdtChoice::Fri, 1 = LdtChoice::Stir, 2 = Stark::ldt's rule (STIR from 2^16 padded rows on, stark.rs:1944-1951)
inline bool chooses_stir(uint32_t use_stir, uint32_t log2_padded_height, const char* entry) {
    if (use_stir > 2) throw Error(TVM_ERR_INVALID_ARGUMENT, std::string(entry) + ": use_stir is 0 (FRI), 1 (STIR) or 2 (automatic)");
    return use_stir == 2 ? log2_padded_height >= 16 : use_stir == 1;
}

}  // namespace triton_vm
