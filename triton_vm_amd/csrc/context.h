// context.h -- device context shared by all entry points of libtriton_hip.so (implemented in context.hip).
//
// One context per host thread that proves (the reference's prove() may run concurrently on several
// threads, /root/reference/triton-vm/src/lib.rs:522-532): a context owns one HIP stream, a cache of
// power tables (twiddles, coset scalings) and a growable scratch workspace.  Nothing here
// synchronises with the host unless an entry point has to hand data back.
#pragma once
#include <map>
#include <string>
#include <tuple>

#include "field.h"
#include "triton_hip.h"  // status codes and the public C ABI (include/)

// Device tables are "row-block-major" (DESIGN.md section 2): blocks of TVM_RB = 16 consecutive STORAGE rows,
// column-major inside a block, i.e. element (s, v) of a table with W base-field words per row is at
// ((s / 16) * W + v) * 16 + s % 16.  Sixteen consecutive storage rows of one column form one 128-byte line,
// so a wavefront whose lanes are consecutive storage rows reads any column as four full lines (row hashing,
// AIR evaluation, linear combinations), and the last LDE pass writes full lines.
#define TVM_RB 16
#define TVM_RB_LOG 4
TVM_HD u64 tvm_tab_idx(u64 row, u64 v, u64 W) { return ((row >> TVM_RB_LOG) * W + v) * TVM_RB + (row & (TVM_RB - 1)); }
TVM_HD u64 tvm_tab_words(u64 rows, u64 W) { return ((rows + TVM_RB - 1) / TVM_RB) * TVM_RB * W; }

// Which storage row holds which row of the domain.  A table made by tvm_lde_table over the evaluation domain
// g*<w_L>, L = X*N, N = n1*n2 (the two axes of the transform, csrc/ntt.hip) is stored COSET-MAJOR and, inside a coset of
// the trace domain, in the order the last LDE pass produces it:
//     domain row  i = X*j + k,  j = j1 + n2*j2  (k < X the coset, j1 < n2, j2 < n1)   <->   storage row  k*pitch + j1*n1 + j2.
//   * one transform of the last pass (fixed k, j1; all j2) owns n1 CONSECUTIVE storage rows: it writes full lines whatever the
//     number of transforms a workgroup holds;
//   * the rows of a coset -- of a stride view (every s-th domain row = the cosets k = 0 mod s: the quotient domain inside a
//     longer LDT domain, a rank's or a coset-wise pass's share, the half domain of valid-trace mode) -- are contiguous;
//   * the successor row j + 1 of the AIR (domain row i + X) is storage row + n1; tables the AIR reads carry one more block of
//     n1 rows per coset behind the n2 blocks (`pitch` = (n2 + 1)*n1): block n2 = block 0 shifted by one row, the successors of
//     block n2 - 1.
// Tables in natural row order (the quotient-segment table, the verifier's row packs) are the case X = 1, n2 = 1, n1 = rows.
struct TabLayout {
    u64 X = 1, n1 = 0, n2 = 1, pitch = 0;   // X, n2 and -- unless n2 == 1 -- n1 are powers of two
    int log_x = 0, log_n1 = 0, log_n2 = 0;
    TVM_HD u64 rows() const { return X * n1 * n2; }
    TVM_HD u64 storage_rows() const { return X * pitch; }
    // position r = j1*n1 + j2 inside a coset -> j = j1 + n2*j2
    TVM_HD u64 coset_index(u64 r) const { return n2 == 1 ? r : (r >> log_n1) + ((r & (n1 - 1)) << log_n2); }
    TVM_HD u64 storage_row(u64 i) const {
        const u64 k = i & (X - 1), j = i >> log_x;
        return n2 == 1 ? k * pitch + j : k * pitch + (j & (n2 - 1)) * n1 + (j >> log_n2);
    }
};
inline TabLayout tab_layout_natural(u64 rows) {
    TabLayout l;
    l.n1 = l.pitch = rows;
    return l;
}
// The rows of a stride view in an order that walks storage contiguously: view row index t < rows/stride, in "coset-major"
// order when the stride selects whole cosets, in domain order otherwise.  -> storage row, and the view's domain index of it.
struct TabView {
    TabLayout l;
    u64 stride = 1, n_out = 0;
    bool by_coset = false;   // stride divides X: the view is the cosets k = stride*k', k' < X/stride
    int log_n = 0, log_xv = 0;
    TVM_HD void locate(u64 t, u64& s, u64& out_index) const {
        if (by_coset) {
            const u64 kv = t >> log_n, r = t & ((1ull << log_n) - 1);
            s = kv * stride * l.pitch + r;
            out_index = (l.coset_index(r) << log_xv) + kv;
        } else {
            s = l.storage_row(t * stride);
            out_index = t;
        }
    }
};
inline int tab_ilog2(u64 n) {
    int k = 0;
    while ((1ull << k) < n) k++;
    return k;
}
inline TabView tab_view(const TabLayout& l, u64 stride) {
    TabView v;
    v.l = l;
    v.stride = stride;
    v.n_out = l.rows() / stride;
    // (a single coset too: the table of a rank that owns one coset of the trace domain -- eight ranks at expansion 8 -- is stored
    // in the order of the last LDE pass like any other; walking it in domain order read every word of a row from a line of its own)
    v.by_coset = stride <= l.X && l.X % stride == 0 && l.n2 > 1;
    if (v.by_coset) {
        v.log_n = l.log_n1 + l.log_n2;
        v.log_xv = tab_ilog2(l.X / stride);
    }
    return v;
}

namespace tvm {
// The scratch slots of a context (scratch(), stage_small()): one device block each, grown on demand, kept until tvm_ctx_destroy.
//
// THE RULE.  A slot belongs to the function that asks for it until that function returns -- the kernels it has launched read and
// write the block in stream order, and asking for a slot AGAIN with a larger size frees the old block.  So a function may hold a
// slot across a call only if nothing that call can reach asks for the same slot.  The enumerators are grouped in three layers, and
// calls go downwards only; a function asks for slots of its own layer alone:
//   * entry-point slots: asked for by an extern "C" entry point (or a static helper that only it calls), which may hold them across
//     any call into the layers below.  Entry points do not call entry points that take entry-point slots: the ones that are called
//     from others (tvm_evaluate, tvm_interpolate) take helper and unit slots only.  Entry points that share a slot
//     (GatherIndices / GatherOut, SmallIn / SmallOut, QuotientInputs) never call one another.
//   * helper slots: tvm_evaluate and quotient_segments_of_coefficients (capi.hip), held across calls into the units.
//   * unit slots: asked for inside a kernel unit (ntt.hip, air.hip, poly.hip, pad.hip) by a function that calls no other function
//     that takes a slot -- the bottom; every caller above may rely on their being distinct from its own.
// The cases that decide it:
//   * tvm_all_quotients_combined / _coefficients and tvm_air_class_values (quotient.hip) hold QuotientInputs while air.hip takes ZerofierInverses
//     and AirAccumulators, and (valid-trace mode) while tvm_evaluate / tvm_interpolate take FoldedCoefficients and NttTemp;
//   * tvm_quotient_segments holds QuotientCoefficients and SmallIn across quotient_segments_of_coefficients, which holds SegmentFolded
//     and SegmentValues across ntt_columns (NttTemp); lde_table takes its intermediates from the pool;
//   * tvm_stir_next_polynomial holds StirValues, StirQuotientSet and StirAnswerValues across tvm_evaluate and tvm_interpolate;
//   * tvm_check_constraints holds its first six across air_on_rows (AirAccumulators; the selectors take the place of the zerofier
//     inverses), and takes the last two after the screen's results are on the host.
//   * tvm_evaluate_extended holds CombinationForm and CombinationTable across lde_coefficient_form, lde_table (pool blocks and cached
//     tables only) and table_rows; it calls no entry point, and no entry point calls it.  Slots of its own, not the segment step's
//     SegmentValues: the segment table's intermediates and the combination's differ in size by a factor of five, and a shared slot
//     would be freed and allocated again (a drained stream each time) twice per proof.
// A new unit takes NEW enumerators in the layer it calls from; it shares an existing one only where this comment says why it may.
enum class Scratch : int {
    // ---- unit slots
    NttTemp,                // ntt_columns: the columns between its two passes
    ZerofierInverses,       // air.hip: four factors per row of the quotient domain
    AirAccumulators,        // air.hip: the quotient values in work order, one set per lane
    OodWeights,             // out_of_domain_rows: the barycentric weights, per point and row
    OodSums,                // out_of_domain_rows: numerators and denominator per point
    ReductionPartials,      // out_of_domain_rows, poly_eval: per-workgroup partial sums (the evaluations follow one another on the stream)
    PadPivot,               // pad_main_table: one word
    // ---- helper slots
    FoldedCoefficients,     // tvm_evaluate: more coefficients than points, reduced modulo X^L - offset^L
    SegmentFolded,          // quotient_segments_of_coefficients: the same reduction of the five segment polynomials
    SegmentValues,          // ... and their coefficient form with the randomizers behind it (lde_coefficient_form), or -- the route
                            // through the values -- their values on the M-th roots of unity or (short domains) as planar codewords
    // ---- entry-point slots
    GatherIndices,          // tvm_table_reveal_rows, tvm_gather_elements(_batch): the indices ...
    GatherOut,              // ... and what they select, on its way to the host
    SmallIn,                // a small host array in (points, weights, randomizers): every entry point that stages one
    SmallOut,               // ... and a small result on its way out (rows, values at the points)
    QuotientCoefficients,   // tvm_quotient_segments: the interpolated quotient
    QuotientInputs,         // challenges and quotient weights: both quotient entry points, tvm_air_class_values
    StirValues,             // tvm_stir_next_polynomial: the folded polynomial on the work domain
    StirQuotientSet,        // ... the quotient set and the answer polynomial
    StirAnswerValues,       // ... the answer polynomial on the work domain
    FillChallenges,         // tvm_fill_derived_aux_columns
    ExtendChallenges,       // tvm_extend_aux_table
    FriTranscript,          // tvm_fri_commit_phase: sponge, roots, challenges
    InterpolationStaging,   // tvm_xfe_interpolate: points, values, coefficients, status
    AirCheckInputs,         // tvm_check_constraints: challenges and the screen's weights
    AirCheckSelectors,      // ... four factors per row of a chunk
    AirCheckValues,         // ... the screen's value per row
    AirCheckOffsets,        // ... per-group offsets and the running total
    AirCheckCounts,         // ... per-group counts
    AirCheckListed,         // ... the failing rows
    AirCheckPairIndices,    // ... pinpointing: rows r, r + 1 of a batch of listed rows
    AirCheckPairs,          // ... and their words
    MiddleBlock,            // tvm_out_of_domain_to_deep: the block that goes back to the host and the weight vectors behind it, held
                            // across out_of_domain_rows, poly_eval, ntt_columns (unit slots) and tvm_evaluate (helper and unit slots)
    FrontClaim,             // tvm_front_challenges: the claim's digest, input and output (it calls nothing that takes a slot)
    CombinationForm,        // tvm_evaluate_extended: the polynomial in coefficient form, its upper part behind it as the randomizers
    CombinationTable,       // ... and its values as a table of one column in the order of the last LDE pass
    Count
};
// The kinds of constant table a context caches (cached_table); what the three key words mean is the kind's own business:
//   Powers             (base, count, scale): t[i] = scale * base^i                                             pow_table
//   CosetFactors       (offset, generator, X << 56 | n1 << 28 | n2): lo / hi of the X cosets                   ntt.hip: coset_tables
//   Pass2Twiddles      (trace generator, n1, n2): f of k_lde_pass2_fused                                       ntt.hip: pass2_fused_tables
//   Pass2CosetFactors  (offset, generator, X << 56 | n1 << 28 | n2): hi_pos and u of k_lde_pass2_fused
//   Pass3Halves        (root of the n1-point axis, 2048, 0): the twiddles of k_lde_pass3_halves                ntt.hip: lde_table
//   Pass2ScaleAbsorbed (offset, generator, X << 56 | n1 << 28 | n2): g_abs and d_abs of k_lde_pass2_fused      ntt.hip: pass2_absorbed_tables
enum class TableKind { Powers, CosetFactors, Pass2Twiddles, Pass2CosetFactors, Pass3Halves, Pass2ScaleAbsorbed };
}  // namespace tvm

struct tvm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    std::map<std::tuple<tvm::TableKind, u64, u64, u64>, u64*> tables;   // cached_table: (kind, three words) -> device table
    void* scratch[(int)tvm::Scratch::Count] = {};       // the scratch slots and their capacities
    size_t scratch_bytes[(int)tvm::Scratch::Count] = {};
    // Caching device allocator: every device block handed out by the library (tvm_malloc, table handles)
    // comes from here and returns here; a 2^20-row proof allocates ~45 GiB of tables per prove(), and
    // driver allocations and frees of that size cost hundreds of milliseconds each.  Blocks are reused in stream
    // order (one stream per context), so handing a freed block to the next request needs no host sync.
    std::multimap<size_t, void*> pool_free;             // capacity -> block
    std::map<void*, size_t> pool_live;                  // block -> capacity
    size_t pool_bytes = 0;                              // bytes held from the driver (live + cached)
    size_t pool_limit = 0;                              // tvm_ctx_set_memory_limit: 0 = whatever the device has
    bool air_valid_trace = false;                       // TVM_OPTION_AIR_VALID_TRACE (quotient_plan.h; quotient.hip)
    int lde_chunk_columns = 0;                          // TVM_OPTION_LDE_CHUNK_COLUMNS: 0 = chosen by lde_table (ntt.hip)
    int lde_pass2_tiles = 0;                            // TVM_OPTION_LDE_PASS2_TILES: 1 = the tile kernels instead of k_lde_pass2_fused (A/B)
    bool lde_pass2_scale_absorbed = true;               // TVM_OPTION_LDE_PASS2_SCALE_ABSORBED (ntt.hip: lde_table, k_lde_pass2_fused)
    u64 lde_pass1_workgroups = 0;                      // TVM_OPTION_LDE_PASS1_WORKGROUPS: 0 = one per (column, tile) item (lde_plan.h);
                                                        // tvm_ctx_create starts it at the device's compute-unit count (0 where it reports none)
    bool segments_from_coefficients = true;             // TVM_OPTION_SEGMENTS_FROM_COEFFICIENTS (capi.hip: quotient_segments_of_coefficients)
    bool combination_from_coefficients = true;          // TVM_OPTION_COMBINATION_FROM_COEFFICIENTS (capi.hip: tvm_evaluate_extended)
    u64 merkle_min_workgroups = 4096;                  // TVM_OPTION_MERKLE_MIN_WORKGROUPS (hash.hip: merkle_tree_from_leaves)
    bool merkle_subtrees = true;                        // TVM_OPTION_MERKLE_SUBTREES: narrow levels seven to a launch (k_merkle_subtrees)
    std::string last_error;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    // the side lane (include/triton_hip.h: tvm_side_*): created on first use
    hipStream_t side = nullptr;
    hipEvent_t side_ready = nullptr, side_done[16] = {};
    // the staging ring (h2d_small): pinned host memory that small host arrays (points, weights, challenges, index lists) pass through
    // on their way to the device, so that the copy is asynchronous AND the caller's array is free when the entry point returns
    char* pin = nullptr;
    size_t pin_bytes = 0, pin_head = 0;
    bool pin_unavailable = false;   // hipHostMalloc refused once: the plain path (copy, then wait) from then on
    // the fork lanes (fork_lanes; air.hip: air_run): launches that are independent of one another and too small to fill the
    // chip each -- the parts of the AIR on a short quotient domain -- go out on these streams beside the context's own and meet
    // it again before the next dependent launch.  Created on first use.
    hipStream_t fork[3] = {};
    hipEvent_t fork_ready = nullptr, fork_done[3] = {};
    u64 air_fork_max_workgroups = 256;                  // TVM_OPTION_AIR_FORK_MAX_WORKGROUPS (0 after set_option(…, 0): never fork)
    bool air_remainder_coset = true;                    // TVM_OPTION_AIR_REMAINDER_COSET (quotient_plan.h; quotient.hip)
    u64 air_remainder_min_rows = 1ull << 18;            // TVM_OPTION_AIR_REMAINDER_MIN_ROWS
    u64 air_check_chunk_rows = 1ull << 18;              // TVM_OPTION_AIR_CHECK_CHUNK_ROWS (air_check.hip: tvm_check_constraints)
};

namespace tvm {
// the extension split at the coefficients, for the virtual columns [first_vcol, first_vcol + n_vcols) (a virtual column = one
// base-field component of a column): mode 1 = inverse transforms only, the coefficient form -> coeffs ([n_vcols][n_rows] words);
// mode 2 = forward only, from coeffs, into those columns of the table
struct LdeSplit {
    int mode;
    u64* coeffs;
    int first_vcol, n_vcols;
};
// The driver allocates on the calling thread's CURRENT device, and streams belong to the device that is current when they are created;
// another context (or the application) may have changed it since tvm_ctx_create.  Every path that allocates or creates a stream
// selects the context's device first -- and leaves it selected (only tvm_ctx_memory_info puts the caller's device back).
bool bind_device(tvm_ctx* c);
// The cached table (kind, a, b, d) of `words` words, for the life of the context.  On a miss the block is allocated on the context's
// device and registered, and *is_new tells the caller to launch its fill on c->stream.  nullptr: the device refused.
u64* cached_table(tvm_ctx* c, TableKind kind, u64 a, u64 b, u64 d, u64 words, bool* is_new);
// takes back (and frees) a table registered by a cached_table whose fill will not be launched
void drop_cached_table(tvm_ctx* c, TableKind kind, u64 a, u64 b, u64 d);
// t[i] = scale * base^i, i < count (Montgomery words); cached for the life of the context
const u64* pow_table(tvm_ctx* c, u64 base, u64 count, u64 scale = TVM_ONE);
// scratch slot `slot` of at least `bytes` bytes (grown on demand, contents undefined); see the rule above Scratch
void* scratch(tvm_ctx* c, Scratch slot, size_t bytes);
// a small host array (points, weights) staged into a scratch slot through h2d_small; nullptr on failure
const u64* stage_small(tvm_ctx* c, Scratch slot, const u64* h, size_t words);
int set_error(tvm_ctx* c, int code, const char* what);
// pool: nullptr on device out-of-memory (after the cache has been given back to the driver and the request retried)
void* pool_alloc(tvm_ctx* c, size_t bytes);
void pool_release(tvm_ctx* c, void* p);   // back to the cache (stream-ordered reuse)
void pool_trim(tvm_ctx* c);               // cached blocks back to the driver (synchronises the stream)
// what a pool_alloc could still obtain: the device's free memory plus this context's cached blocks, capped by the context's limit
size_t pool_available(tvm_ctx* c, size_t* device_total);
// Host array -> device, stream-ordered, WITHOUT draining the stream: the bytes are copied into the context's pinned staging ring and
// go from there (the caller's array may be a temporary: it is free on return).  The ring wraps after a stream synchronisation -- once
// in some tens of proofs; arrays above a quarter of the ring take the plain path (copy, then wait).  Before round 6 every such hand-over
// was hipMemcpyAsync + hipStreamSynchronize: some twenty drained streams per proof, a fifth of a proof of a 2^10-row trace.
int h2d_small(tvm_ctx* c, void* d, const void* h, size_t bytes);
// the context's fork lanes (three more streams and their events), created on first use; false if the driver refuses
bool fork_lanes(tvm_ctx* c);
// a pool block that goes back to the cache on every exit path of the function that holds it
struct PoolBlock {
    tvm_ctx* c;
    void* p = nullptr;
    explicit PoolBlock(tvm_ctx* c_) : c(c_) {}
    PoolBlock(tvm_ctx* c_, size_t bytes) : c(c_), p(pool_alloc(c_, bytes)) {}
    void* alloc(size_t bytes) {
        pool_release(c, p);
        return p = pool_alloc(c, bytes);
    }
    ~PoolBlock() { pool_release(c, p); }
    PoolBlock(const PoolBlock&) = delete;
    PoolBlock& operator=(const PoolBlock&) = delete;
};
inline int ilog2(u64 n) {
    int l = 0;
    while ((1ull << l) < n) l++;
    return l;
}
inline bool is_pow2(u64 n) { return n && !(n & (n - 1)); }
}  // namespace tvm

#define TVM_HIP_CHECK(c, expr)                                                              \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return tvm::set_error((c), e_ == hipErrorOutOfMemory ? TVM_ERR_OUT_OF_MEMORY : TVM_ERR_DEVICE, #expr); \
    } while (0)
#define TVM_TRY(expr)                  \
    do {                               \
        int rc_ = (expr);              \
        if (rc_ != TVM_OK) return rc_; \
    } while (0)
