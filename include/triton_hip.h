/*
 * triton_hip.h -- C ABI of libtriton_hip.so, the MI355X (gfx950) backend for the hot path of
 * triton_vm::stark::Prover::prove (/root/reference/triton-vm/src/stark.rs:331-719).
 *
 * The reference has no FFI for this path; these entry points are what a Rust shim
 * (`extern "C"` block) binds in place of the bodies of the cited reference
 * functions.  Everything [twenty-first]-only -- Fiat-Shamir sampling, BFieldCodec, the prover's RNG,
 * authentication structures -- stays on the Rust side and crosses this boundary as plain data.
 *
 * Conventions
 *  - A BFieldElement is one uint64_t holding the Montgomery word a*2^64 mod p, p = 2^64-2^32+1,
 *    exactly BFieldElement::raw_u64() (triton-constraint-builder/src/codegen.rs:28-31,926-944).
 *    An XFieldElement is 3 consecutive words, a Digest 5 words.  field_kind = 1 (BFE) or 3 (XFE).
 *  - Pointers named d_* are DEVICE pointers (hipMalloc / tvm_malloc / a torch tensor's data_ptr);
 *    pointers named h_* are host pointers.  No entry point takes ownership of caller memory.
 *  - Domains are passed as the reference holds them: (offset, generator, length)
 *    (arithmetic_domain.rs:34-47); the library never invents a root of unity for a caller's domain.
 *  - Every function returns a status (0 = ok) mapped 1:1 on the reference's error enums
 *    (triton-vm/src/error.rs:150-186) and never aborts or throws across the boundary.  Device
 *    out-of-memory is TVM_ERR_OUT_OF_MEMORY and leaves the context usable, mirroring the
 *    reference's try_reserve_exact fallback (master_table.rs:268-271).
 *  - Work is enqueued on the context's HIP stream; functions that return host data synchronise
 *    that stream, the others do not.  One context per proving thread (lib.rs:522-532); the calling
 *    thread's current HIP device must be the one the context was created on.
 */
#ifndef TRITON_HIP_H
#define TRITON_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TVM_OK 0
#define TVM_ERR_INVALID_ARGUMENT 1 /* ArithmeticDomainError, TableRowConversionError, length mismatches */
#define TVM_ERR_OUT_OF_MEMORY 2    /* ProvingError::OutOfMemory -- recoverable */
#define TVM_ERR_DEVICE 3           /* HIP runtime failure */
#define TVM_ERR_UNSUPPORTED 4
#define TVM_NOT_APPLICABLE 5       /* not an error: this entry point does not cover these arguments, nothing was written; call the general one */

typedef struct tvm_ctx tvm_ctx;
typedef struct tvm_table tvm_table; /* device-resident low-degree-extended master table */

typedef struct {
    uint64_t offset;    /* Montgomery word */
    uint64_t generator; /* Montgomery word; order == length */
    uint64_t length;    /* power of two */
} tvm_domain;

/* ---- context ------------------------------------------------------------------------------ */
int32_t tvm_abi_version(void);
/* `hip_stream` may be NULL (the context creates its own stream) or an existing hipStream_t. */
int32_t tvm_ctx_create(int32_t device, void* hip_stream, tvm_ctx** out);
void tvm_ctx_destroy(tvm_ctx* ctx);
const char* tvm_last_error(const tvm_ctx* ctx);
const char* tvm_status_string(int32_t status);
int32_t tvm_sync(tvm_ctx* ctx);
/* Device memory comes from a per-context caching allocator (a prove() at 2^20 rows turns over ~45 GiB of
 * tables; the driver's allocator costs hundreds of ms at that size).  tvm_free and tvm_table_free return
 * blocks to the cache for stream-ordered reuse; tvm_ctx_trim gives the cache back to the driver. */
int32_t tvm_malloc(tvm_ctx* ctx, size_t bytes, void** d_ptr);
int32_t tvm_free(tvm_ctx* ctx, void* d_ptr);
int32_t tvm_ctx_trim(tvm_ctx* ctx);
/* Options.  TVM_OPTION_AIR_VALID_TRACE (default 0): the caller guarantees that the master tables come from a valid
 * execution trace -- what Prover::prove is for.  tvm_all_quotients_combined may then use that the constraint quotients
 * are polynomials of known degree: the consistency / transition constraints are evaluated on half of the quotient
 * domain and the codeword completed by interpolation; bit-identical to the row-by-row evaluation on a valid trace,
 * different on an invalid one (where both yield a proof the verifier rejects).  A quotient domain short enough for
 * TVM_OPTION_AIR_FORK_MAX_WORKGROUPS (the parts side by side) disables this split: such a domain is evaluated row by row. */
#define TVM_OPTION_AIR_VALID_TRACE 1
/* Tuning values (per context; they change launch shapes, never results).  TVM_OPTION_LDE_CHUNK_COLUMNS: columns per chunk of
 * tvm_lde_table's three-pass transform, 0 (default) = 96 while the chunk's intermediates fit comfortably, else 32.
 * TVM_OPTION_MERKLE_MIN_WORKGROUPS: tvm_merkle_tree gives a workgroup several groups of parents while at least this many
 * workgroups remain (default 4096; 0 restores it) -- the tests lower it to reach that path with small trees.
 * The library reads NO environment variable: a prover behind triton_vm::prove() must not change kernels on an inherited
 * environment. */
#define TVM_OPTION_LDE_CHUNK_COLUMNS 2
#define TVM_OPTION_MERKLE_MIN_WORKGROUPS 3
/* TVM_OPTION_LDE_PASS2_TILES = 1: tvm_lde_table runs the kernels that the row kernels replaced (A/B, profiles/r05_* and r06_*; the
 * tests use it to reach those kernels at small sizes).  A trace of 2^n rows is transformed as n1 x n2 points, n1 = 2^(n/2) rounded
 * down.  Middle pass (axis n2): never k_lde_pass2_fused -- the tile kernel k_lde_pass2_v3 on 256-, 2048- and 4096-point axes, the
 * generic kernel on 512- and 1024-point ones.  First and last pass (axis n1): the generic kernels instead of the row kernels on 256-
 * and 512-point axes (the last pass: the tile kernel k_lde_pass3_v3 at 256 points) and in the first pass at 2048 points; the last pass
 * at 2048 points runs k_lde_pass3_rows instead of k_lde_pass3_halves.  1024-point axes keep the row kernels of the first and last
 * pass, and axes of at most 128 or of 4096 points run the same kernels with either value (csrc/lde_plan.h decides all of this). */
#define TVM_OPTION_LDE_PASS2_TILES 4
/* TVM_OPTION_LDE_PASS1_WORKGROUPS: workgroups per launch of the first pass's row kernels on 256-, 512- and 1024-point axes
 * (k_lde_pass1_rows<8 | 9 | 10, 16>), at most one per (column, tile) item of the chunk.  With fewer workgroups than items each walks
 * several tiles with the next tile's input in flight under the current one's butterflies.  0 and any value at or above the item
 * count: one tile per workgroup.  A context starts with the compute-unit count of its device (256 on an MI355X: the kernel is 13 %
 * faster at 2^20 rows than with a workgroup per item), or 0 where the device reports none; the tests use small values to
 * walk many tiles, and the column boundary, in one workgroup. */
#define TVM_OPTION_LDE_PASS1_WORKGROUPS 10
/* TVM_OPTION_AIR_FORK_MAX_WORKGROUPS (default 256; 0 = never): tvm_all_quotients_combined / tvm_air_class_values on a quotient domain of at
 * most this many workgroups of 256 rows launch the parts of the AIR on four streams side by side (the context's and three of its
 * own, joined before the call returns to the context's stream), and on such a domain valid-trace mode evaluates row by row. */
#define TVM_OPTION_AIR_FORK_MAX_WORKGROUPS 5
/* TVM_OPTION_MERKLE_SUBTREES (default 1): the levels of a Merkle tree between 32768 and 64 parents are built up to seven to a launch
 * (a workgroup per subtree of 64 parents); 0: one launch per level (A/B). */
#define TVM_OPTION_MERKLE_SUBTREES 6
/* TVM_OPTION_AIR_REMAINDER_COSET (default 1): in valid-trace mode, tvm_all_quotients_combined evaluates each class of constraints on one
 * coset of the trace domain fewer than its quotient has blocks of trace-length coefficients, plus one block of rows of another coset
 * (the remainder set) that pays for the few coefficients beyond them; 0: the whole cosets (A/B).  The same words either way.
 * TVM_OPTION_AIR_REMAINDER_MIN_ROWS: the shortest trace domain this applies to (default 2^18; 0 restores it) -- the tests lower it. */
#define TVM_OPTION_AIR_REMAINDER_COSET 7
#define TVM_OPTION_AIR_REMAINDER_MIN_ROWS 8
/* TVM_OPTION_AIR_CHECK_CHUNK_ROWS: rows per chunk of tvm_check_constraints (a power of two in 16 .. 2^20; default 2^18, 0 restores it)
 * -- the tests lower it to reach the chunk boundaries with small traces.  The same report for every value. */
#define TVM_OPTION_AIR_CHECK_CHUNK_ROWS 9
/* TVM_OPTION_SEGMENTS_FROM_COEFFICIENTS (default 1): tvm_quotient_segments(_from_coefficients) hands the segment polynomials to the
 * table extension as coefficients -- one relayout pass, then the forward half of the extension -- where the LDT domain has 2 to 32
 * times n points and at least as many as a segment has coefficients; n is the largest power of two (at least 16) in a segment's
 * length max(n_coeffs / 4, n_rand), the coefficients beyond n are the randomizer part of the extension.  0: the segments' values on
 * the roots of unity first and the whole extension from there (A/B).  The same words either way. */
#define TVM_OPTION_SEGMENTS_FROM_COEFFICIENTS 11
/* TVM_OPTION_LDE_PASS2_SCALE_ABSORBED (default 1): the middle pass of tvm_lde_table on 256- to 1024-point axes (k_lde_pass2_fused) does
 * not multiply its coefficients by the coset's factors in every coset.  The part of the factor that is common to a lane's first
 * butterfly group moves into the next group's twiddle table, the rest is a power of two per coset -- the first group at shifted points,
 * the same instructions -- times a factor per class of cosets that the coefficients take once per class: 48 general multiplications
 * per lane and coset instead of 63.  Taken where the evaluation generator is the domains' own root of unity of order L (every
 * ArithmeticDomain's is; any offset); other generators run the table form whatever the value.  The same words either way. */
#define TVM_OPTION_LDE_PASS2_SCALE_ABSORBED 12
/* TVM_OPTION_COMBINATION_FROM_COEFFICIENTS (default 1): tvm_evaluate_extended takes its route (below); 0: it answers TVM_NOT_APPLICABLE
 * whatever the shape, so that a host that falls back to tvm_evaluate runs the general transform (A/B).  The same words either way. */
#define TVM_OPTION_COMBINATION_FROM_COEFFICIENTS 13
int32_t tvm_ctx_set_option(tvm_ctx* ctx, int32_t option, uint64_t value);
/* The value an option has now, for the options whose start value depends on the device or that select between two routes to the
 * same words (ids 10 to 13: a fresh context answers the device's compute-unit count, 1, 1, 1); TVM_ERR_INVALID_ARGUMENT for others. */
int32_t tvm_ctx_get_option(const tvm_ctx* ctx, int32_t option, uint64_t* value);
/* Cap on the bytes this context may hold through tvm_malloc / table handles (0 = no cap).  Requests beyond it fail
 * with TVM_ERR_OUT_OF_MEMORY exactly like a full device: the knob a host uses to share a GPU, and what the tests use to
 * walk the reference's out-of-memory fallback (master_table.rs:268-271 -> the coset-wise path). */
int32_t tvm_ctx_set_memory_limit(tvm_ctx* ctx, size_t bytes);
/* bytes currently held from the driver through this context (live blocks + cached blocks) */
int32_t tvm_ctx_memory_held(const tvm_ctx* ctx, size_t* bytes);
/* what this context could still obtain through tvm_malloc / table handles right now: the device's free memory plus the
 * context's own cached blocks (they are given back before a request fails), capped by the memory limit; and the device's
 * total.  Either pointer may be null.  The figure the host's memory policy plans with (master_table.rs:268-271: "does the
 * cached extension fit?") instead of running into the failure. */
int32_t tvm_ctx_memory_info(const tvm_ctx* ctx, size_t* available_bytes, size_t* device_total_bytes);
int32_t tvm_memcpy_h2d(tvm_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int32_t tvm_memcpy_d2h(tvm_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);
/* device to device, ordered on the context's stream, NOT synchronised (same device, or a peer-accessible one). */
int32_t tvm_memcpy_d2d(tvm_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);
/* the hipStream_t every call of this context is ordered on (so that a collective library -- RCCL -- can be enqueued
 * behind the kernels that produce its operands and ahead of those that consume its results; triton_vm_amd/host/rccl_comm.cpp) */
void* tvm_ctx_stream(const tvm_ctx* ctx);
/* The context's SIDE LANE: a second stream (created on first use) for exchanges that run UNDER the kernels of the context's stream --
 * the coefficient exchange of the column split (MasterTable::low_degree_extend_over, triton_vm_amd/host/triton_host.cpp) and its
 * communicators (rccl_comm.cpp enqueues ncclAllGather on it; the in-process communicator of sharded_host.cpp copies on it).  Ordering is
 * by events only, no host synchronisation:
 *   tvm_side_begin       the side lane waits for everything queued on the context's stream so far (the exchange's operands);
 *   tvm_side_memcpy_d2d  a device-to-device copy on the side lane;
 *   tvm_side_mark(slot)  records "everything queued on the side lane so far is done" in slot < TVM_SIDE_SLOTS;
 *   tvm_side_wait(slot)  the context's stream waits for that mark -- which also orders the pool's reuse of a freed block behind
 *                        the exchange that read or wrote it (a mark never recorded is no wait);
 *   tvm_side_sync        the HOST waits for the side lane (in-process communicators: a peer's copies out of this rank's buffer). */
#define TVM_SIDE_SLOTS 16
void* tvm_ctx_side_stream(tvm_ctx* ctx); /* NULL if it cannot be created */
int32_t tvm_side_begin(tvm_ctx* ctx);
int32_t tvm_side_memcpy_d2d(tvm_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);
int32_t tvm_side_mark(tvm_ctx* ctx, uint32_t slot);
int32_t tvm_side_wait(tvm_ctx* ctx, uint32_t slot);
int32_t tvm_side_sync(tvm_ctx* ctx);

/* HIP-event stopwatch on the context's stream (bench.py's live kernel timing) */
int32_t tvm_timer_start(tvm_ctx* ctx);
int32_t tvm_timer_stop(tvm_ctx* ctx, float* h_elapsed_ms); /* synchronises the stream */
/* Synthetic tables for benchmarks: n canonical Montgomery words < p from a counter-based generator */
int32_t tvm_synthetic_fill(tvm_ctx* ctx, uint64_t* d_data, uint64_t n_words, uint64_t seed);

/* Elementwise d_out[i] = d_a[i] op d_b[i] on Montgomery words through the device's field arithmetic
 * (op 0: +, 1: -, 2: *, 3: a^7, 4: a * 2^b for a plain integer b < 192): the known-answer hook for the hand-scheduled carry
 * chains in csrc/field.h (BFieldElement's Add/Sub/Mul, twenty-first; KAT triton-constraint-builder/src/codegen.rs:926-944)
 * and for the shift forms of csrc/ntt_shift.h.  op 32 + 4K + 2*dit + inverse (K = 1..4): the in-register transforms of
 * 2^K points with power-of-two twiddles on consecutive groups of 2^K words of d_a (d_b unused): dit = bit-reversed in /
 * natural out, else natural in / bit-reversed out; inverse = with the inverse root (no scaling by 2^-K).
 * The words that may leave the canonical range (csrc/ntt_shift.h: canon_plan): op 5 = bfe_add_folded (one operand canonical, the
 * other any 64-bit word; some 64-bit representative of the sum), op 6 = bfe_canon of d_a; ops 1 and 4 take any 64-bit word as the
 * minuend / the multiplicand.  op 64 + 2 (4K + 2*dit + inverse) + owed_all (K = 2..4): the lazy form of the transform above, its
 * outputs owed canonical all (1) or none (0) and the inputs the plan does not need canonical free to be any word;
 * op 112 + 2i + owed_all (i = 0..2): the same for the 16-point decimation-in-time transform at the points 2^(39 (i + 1)) w^j. */
int32_t tvm_field_op(tvm_ctx* ctx, int32_t op, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out, uint64_t n);
/* The 16-point transform with power-of-two twiddles (decimation in time: bit-reversed in, natural out, no scaling) on n_groups
 * consecutive groups of 16 words, in the two forms the device has: form bit 0 = with the inverse root, bit 1 = on the matrix cores
 * (csrc/ntt_mfma.h; clear: the shift form of csrc/ntt_shift.h, canonical inputs only), bit 2 (matrix cores only) = the output as
 * folded 64-bit representatives of the residues instead of canonical words.  The matrix-core form takes ANY 64-bit words as inputs.
 * The known-answer hook of csrc/ntt_mfma.h (tests/test_dft16_mfma.py). */
int32_t tvm_dft16_selfcheck(tvm_ctx* ctx, int32_t form, const uint64_t* d_in, uint64_t* d_out, uint64_t n_groups);

/* ---- L2 / L3: ArithmeticDomain::{evaluate, interpolate} (arithmetic_domain.rs:141-189) -------
 * d_coeffs: n_coeffs elements, d_values: domain.length elements, both arrays of field_kind-word
 * elements.  evaluate accepts n_coeffs > domain.length (chunk folding, :153-167). */
int32_t tvm_evaluate(tvm_ctx* ctx, int32_t field_kind, const uint64_t* d_coeffs, uint64_t n_coeffs,
                     tvm_domain domain, uint64_t* d_values);
/* The same values, word for word, for a polynomial a few times shorter than the domain -- the prover's combination of the trace
 * columns, trace length + randomizers coefficients on the short domain.  With n the largest power of two in n_coeffs the polynomial
 * is lo + X^n hi = (lo + hi) + (X^n - 1) hi, an n-coefficient interpolant plus zerofier times randomizer: one relayout pass over
 * the coefficients, the forward half of tvm_lde_table's extension into a scratch table, one pass that writes d_values in domain
 * order.  Taken where n >= 16, 2 <= domain.length / n <= 32 and domain.generator is the domains' own root of unity of its order
 * (ArithmeticDomain's; any offset), under TVM_OPTION_COMBINATION_FROM_COEFFICIENTS.  Elsewhere the status is TVM_NOT_APPLICABLE and
 * nothing is written: call tvm_evaluate. */
int32_t tvm_evaluate_extended(tvm_ctx* ctx, int32_t field_kind, const uint64_t* d_coeffs, uint64_t n_coeffs,
                              tvm_domain domain, uint64_t* d_values);
int32_t tvm_interpolate(tvm_ctx* ctx, int32_t field_kind, const uint64_t* d_values, tvm_domain domain,
                        uint64_t* d_coeffs);
/* twenty-first `ntt` / `intt` (used at stark.rs:872,877,997,1002,1176): in place, natural order,
 * with the root of unity given explicitly. */
int32_t tvm_ntt(tvm_ctx* ctx, int32_t field_kind, uint64_t* d_data, uint64_t length, uint64_t generator);
int32_t tvm_intt(tvm_ctx* ctx, int32_t field_kind, uint64_t* d_data, uint64_t length, uint64_t generator);

/* ---- L1 + L4: MasterTable::maybe_low_degree_extend_all_columns (master_table.rs:258-322) -----
 * d_trace: column-major [n_cols][n_rows] elements (Array2 `.f()` order, master_table.rs:888,1013);
 * d_randomizers: the h coefficients of trace_randomizer_for_column(c) (master_table.rs:423-434),
 * [n_cols][h] elements, generated by the host RNG.  The extended table stays on the device behind
 * the handle (row i = evaluation at eval.offset * eval.generator^i). */
int32_t tvm_lde_table(tvm_ctx* ctx, int32_t field_kind, const uint64_t* d_trace, uint64_t n_rows,
                      uint64_t n_cols, const uint64_t* d_randomizers, uint64_t num_trace_randomizers,
                      tvm_domain trace_domain, tvm_domain evaluation_domain, tvm_table** out);
/* The same extension split at the coefficients -- the COLUMN sharding of SURVEY 8(e): a rank interpolates a range of columns,
 * the coefficients are exchanged (an all-gather), every rank extends all columns onto its own part of the evaluation domain.
 * A "virtual column" is one base-field component of a column (n_cols * field_kind of them, in the order (column, component)).
 *   tvm_lde_column_coefficients   the inverse transforms of the virtual columns [first, first + n): n_rows words each into
 *                                 d_coeffs[(v - first) * n_rows ...], in the library's COEFFICIENT FORM -- the scaled
 *                                 coefficients in the order its extension kernels read them; opaque, position-independent
 *                                 (a block of it can be moved anywhere), consumed only by tvm_lde_table_add_columns of the
 *                                 same trace length.
 *   tvm_lde_table_begin           a table handle like tvm_lde_table's, its columns not yet written
 *   tvm_lde_table_add_columns     the virtual columns [first, first + n) of the table from their coefficient form, with the
 *                                 trace randomizers of master_table.rs:392-403 (d_randomizers as in tvm_lde_table: all columns)
 *   tvm_lde_table_end             once every column is written (the successor rows of the row-pair views)
 * begin + add_columns over all columns + end == tvm_lde_table, word for word. */
int32_t tvm_lde_column_coefficients(tvm_ctx* ctx, int32_t field_kind, const uint64_t* d_trace, uint64_t n_rows, uint64_t n_cols,
                                    tvm_domain trace, uint64_t first_virtual_column, uint64_t n_virtual_columns, uint64_t* d_coeffs);
int32_t tvm_lde_table_begin(tvm_ctx* ctx, int32_t field_kind, uint64_t n_rows, uint64_t n_cols, uint64_t num_trace_randomizers,
                            tvm_domain trace, tvm_domain eval, tvm_table** out);
int32_t tvm_lde_table_add_columns(tvm_ctx* ctx, tvm_table* table, const uint64_t* d_coeffs, uint64_t first_virtual_column,
                                  uint64_t n_virtual_columns, const uint64_t* d_randomizers, uint64_t num_trace_randomizers,
                                  tvm_domain trace, tvm_domain eval);
int32_t tvm_lde_table_end(tvm_ctx* ctx, tvm_table* table);
void tvm_table_free(tvm_ctx* ctx, tvm_table* table);
uint64_t tvm_table_num_rows(const tvm_table* table);
uint64_t tvm_table_num_columns(const tvm_table* table);
int32_t tvm_table_field_kind(const tvm_table* table);
/* the reference's row-major Array2 [rows][n_cols] (master_table.rs:304-305), into device memory */
int32_t tvm_table_export_row_major(tvm_ctx* ctx, const tvm_table* table, uint64_t* d_out);
/* MasterTable::reveal_rows, cached branch (master_table.rs:548-555): rows of the ldt-domain view
 * (stride rows/ldt_length) at the given indices, row-major into host memory */
int32_t tvm_table_reveal_rows(tvm_ctx* ctx, const tvm_table* table, uint64_t ldt_length,
                              const uint64_t* h_row_indices, uint64_t n_indices, uint64_t* h_out);

/* ---- H1 / H2: row hashing and Merkle trees (master_table.rs:443-468) ------------------------
 * Digest i = Tip5::hash_varlen(row i of the ldt-domain view, XFE rows flattened c0,c1,c2). */
int32_t tvm_hash_rows(tvm_ctx* ctx, const tvm_table* table, uint64_t ldt_length, uint64_t* d_digests);
/* MerkleTree::par_new: d_nodes holds 2*n_leaves digests in heap order (node 1 = root, node
 * n_leaves + i = leaf i, node 0 zeroed). */
int32_t tvm_merkle_tree(tvm_ctx* ctx, const uint64_t* d_leaf_digests, uint64_t n_leaves, uint64_t* d_nodes);
/* MasterTable::merkle_tree: both of the above, leaves hashed straight into the node array */
int32_t tvm_table_merkle_tree(tvm_ctx* ctx, const tvm_table* table, uint64_t ldt_length, uint64_t* d_nodes);
/* ProverRound::merkle_tree_from_codeword (fri.rs:343-347): leaf = Digest::from(xfe), no hashing */
int32_t tvm_codeword_merkle_tree(tvm_ctx* ctx, const uint64_t* d_xfe_codeword, uint64_t length, uint64_t* d_nodes);

/* ---- O1: MasterTable::out_of_domain_row (master_table.rs:348-390) ---------------------------
 * Every column of the trace-randomized table evaluated at n_points XFE indeterminates (the prover
 * uses alpha and omega*alpha, stark.rs:451-469).  h_rows_out: [n_points][n_cols] XFE on the host. */
int32_t tvm_out_of_domain_rows(tvm_ctx* ctx, int32_t field_kind, const uint64_t* d_trace, uint64_t n_rows,
                               uint64_t n_cols, const uint64_t* d_randomizers, uint64_t num_trace_randomizers,
                               tvm_domain trace_domain, const uint64_t* h_points, uint32_t n_points,
                               uint64_t* h_rows_out);

/* ---- C1: MasterTable::weighted_sum_of_columns (master_table.rs:512-542) -----------------------
 * d_poly receives the 2*n_rows XFE coefficients (zero padded above n_rows + h) of
 * sum_c w_c * (column_c interpolant + zerofier * randomizer_c).  h_weights: n_cols XFE. */
int32_t tvm_weighted_sum_of_columns(tvm_ctx* ctx, int32_t field_kind, const uint64_t* d_trace, uint64_t n_rows,
                                    uint64_t n_cols, const uint64_t* d_randomizers, uint64_t num_trace_randomizers,
                                    tvm_domain trace_domain, const uint64_t* h_weights, uint64_t* d_poly);
/* d_a[i] += d_b[i] for n XFE (main + aux combination polynomial, stark.rs:516) */
int32_t tvm_xfe_add_assign(tvm_ctx* ctx, uint64_t* d_a, const uint64_t* d_b, uint64_t n);
/* d_out[i] = sum_k h_weights[k] * d_vectors[k * stride + i], i < n: a weighted sum of XFE vectors (polynomials) that lie
 * `stride` elements apart -- the P and R combinations of the segment POLYNOMIALS (stark.rs:520-536), which the sharded
 * host evaluates on its own rows of the short domain when the quotient domain is shorter than the LDT domain. */
int32_t tvm_xfe_linear_combination(tvm_ctx* ctx, const uint64_t* d_vectors, uint32_t n_vectors, uint64_t stride, uint64_t n,
                                   const uint64_t* h_weights, uint64_t* d_out);
/* Polynomial::evaluate at XFE points (stark.rs:480,491,568,579,590,600): d_coeffs n XFE -> h_out n_points XFE */
int32_t tvm_evaluate_at_points(tvm_ctx* ctx, const uint64_t* d_coeffs, uint64_t n, const uint64_t* h_points,
                               uint32_t n_points, uint64_t* h_out);
/* The same for n_polys polynomials of n coefficients each, `stride` XFE apart in d_coeffs, at the same points, in ONE round trip:
 * h_out[(p * n_points + j) * 3 ..] = polynomial p at point j (the five quotient-segment polynomials at the two out-of-domain
 * points, stark.rs:474-495). */
int32_t tvm_evaluate_polys_at_points(tvm_ctx* ctx, const uint64_t* d_coeffs, uint64_t n, uint64_t stride, uint32_t n_polys,
                                     const uint64_t* h_points, uint32_t n_points, uint64_t* h_out);

/* ---- degree-lowering fill (second half) ---------------------------------------
 * The generated DegreeLoweringTable::fill_derived_main_columns / fill_derived_aux_columns
 * (triton-constraint-builder/src/substitutions.rs:128-205, row loops :236-400; called at the end of
 * MasterMainTable::pad, master_table.rs:980-982, and of MasterMainTable::extend, :1066-1072): 230 of the 379
 * main columns and 41 of the 90 non-randomizer aux columns are values of the substitution rules the degree
 * lowering introduced.  Tables are the column-major traces tvm_lde_table takes: main [379][n_rows] words, aux
 * [>= 90][n_rows][3] words, filled in place.  Single-row sections derive every row; the transition section
 * derives rows 0 .. n_rows-2 from a row and its successor and leaves 0 in the last row (the reference's table is
 * zero-initialised there).  main: columns 149..378 from columns 0..148; aux: columns 49..89 from the main
 * table (already filled), aux columns 0..48 and the 63 challenges (host, XFE). */
int32_t tvm_fill_derived_main_columns(tvm_ctx* ctx, uint64_t* d_main_trace, uint64_t n_rows);
int32_t tvm_fill_derived_aux_columns(tvm_ctx* ctx, const uint64_t* d_main_trace, uint64_t* d_aux_trace, uint64_t n_rows,
                                     const uint64_t* h_challenges);

/* ---- main-table fill from the AET (the `fill` half) ----------------------------------
 * MasterMainTable::new's table fills (master_table.rs:881-931; table/{op_stack,ram,jump_stack,processor,program,hash,
 * cascade,lookup,u32}.rs `fill`).  The AET is handed over as AlgebraicExecutionTrace holds it (aet.rs:41-96): trace arrays
 * row-major in Montgomery words, multiplicities as plain integers.  Every array may live in HOST memory (it is staged
 * through the context's pool: 327 MB of processor trace at 2^20 cycles, ~6 ms over PCIe) or in DEVICE memory of the
 * context's GPU (a host that keeps the trace resident next to the prover: the library reads it where it lies); the
 * library tells the two apart per pointer (hipPointerGetAttributes). */
typedef struct {
    const uint64_t* program_words;              /* Program::to_bwords(), program_len words */
    const uint32_t* instruction_multiplicities; /* [program_len] */
    uint64_t program_len;
    const uint64_t* processor_trace;            /* [processor_len][39] */
    uint64_t processor_len;
    const uint64_t* op_stack_trace;             /* op_stack_underflow_trace [op_stack_len][4] */
    uint64_t op_stack_len;
    const uint64_t* ram_trace;                  /* [ram_len][7] (RamTableCall::to_table_row: the last 3 columns are 0) */
    uint64_t ram_len;
    /* bezout_coefficient_polynomials_coefficients(unique RAM pointers in ascending order) (ram.rs:152-207), num_ram_pointers
     * words each, when the host has them (twenty-first polynomial arithmetic); both null and num_ram_pointers 0: they are
     * computed on the device from the sorted RAM table (tvm_bezout_coefficients' algorithm) */
    const uint64_t* bezout_coefficients_0;
    const uint64_t* bezout_coefficients_1;
    uint64_t num_ram_pointers;
    const uint64_t* program_hash_trace;         /* [program_hash_len][67] */
    uint64_t program_hash_len;
    const uint64_t* sponge_trace;               /* [sponge_len][67] */
    uint64_t sponge_len;
    const uint64_t* hash_trace;                 /* [hash_len][67] */
    uint64_t hash_len;
    const uint64_t* u32_entries;                /* u32_entries in IndexMap order: [u32_len][4] = opcode (plain integer),
                                                   left operand, right operand (Montgomery words), multiplicity (plain) */
    uint64_t u32_len;
    const uint64_t* cascade_entries;            /* cascade_table_lookup_multiplicities in IndexMap order: [cascade_len][2] =
                                                   16-bit limb, multiplicity (plain integers) */
    uint64_t cascade_len;
    const uint64_t* lookup_multiplicities;      /* [256] plain integers */
} tvm_aet;
/* d_main_trace: [379][n_rows] words; columns 0..148 are written (zeros below each table's length), n_rows = the padded
 * height.  h_table_lengths_out[9]: the tables' lengths in the order of tvm_pad_main_table, which is the next call. */
int32_t tvm_fill_main_table(tvm_ctx* ctx, const tvm_aet* aet, uint64_t* d_main_trace, uint64_t n_rows,
                            uint64_t* h_table_lengths_out);

/* ---- main-table pad (the `pad` half) ----------------------------------------------
 * MasterMainTable::pad (master_table.rs:932-983) without its degree-lowering tail (tvm_fill_derived_main_columns): the
 * nine table-specific padding rules (table/program.rs:77-127, processor.rs:70-96, op_stack.rs:205-219, ram.rs:86-101,
 * jump_stack.rs:144-199, hash.rs:280-309, cascade.rs:60-67, lookup.rs:114-118, u32.rs:127-152), in place.
 * d_main_trace: [379][n_rows] words whose columns 0..148 hold the filled tables in their first h_table_lengths[t]
 * rows (t = Program, Processor, OpStack, Ram, JumpStack, Hash, Cascade, Lookup, U32; all_table_lengths,
 * master_table.rs:985-1001) and zeros below; n_rows = the padded height (a power of two). */
int32_t tvm_pad_main_table(tvm_ctx* ctx, uint64_t* d_main_trace, uint64_t n_rows, const uint64_t* h_table_lengths);

/* ---- auxiliary-table extend (first half) ----------------------------------------
 * MasterMainTable::extend (master_table.rs:1006-1075) without its degree-lowering tail and without the batch-randomizer
 * column: the 49 cross-table-argument columns of the nine tables (table/{program,processor,op_stack,ram,jump_stack,
 * hash,cascade,lookup,u32}.rs `extend`: running products, running evaluations, logarithmic-derivative sums with
 * Challenges' initial values) from the padded main table.  d_main_trace: [379][n_rows] words (columns 0..148 are
 * read); d_aux_trace: [91][n_rows][3] words, columns 0..48 are written, the others left alone; h_challenges: the 63
 * challenges incl. the 4 derived ones (host, XFE).  Call tvm_fill_derived_aux_columns afterwards. */
int32_t tvm_extend_aux_table(tvm_ctx* ctx, const uint64_t* d_main_trace, uint64_t* d_aux_trace, uint64_t n_rows,
                             const uint64_t* h_challenges);

/* ---- A1-A3: all_quotients_combined (master_table.rs:1264-1363) ------------------------------
 * Evaluates the 81 + 97 + 403 + 23 = 604 AIR constraints of the (degree-lowered) Triton VM AIR on
 * every quotient-domain row of the two extended tables, including the zerofier inverses
 * (master_table.rs:1194-1250), and combines them with the quotient weights.  The quotient domain is
 * the stride-(rows/length) view of the tables.  h_challenges: 63 XFE (Challenges, challenges.rs:54);
 * h_weights: 604 XFE (stark.rs:396-401).  d_quotient_codeword: quotient_domain.length XFE. */
#define TVM_NUM_CHALLENGES 63
#define TVM_NUM_QUOTIENT_WEIGHTS 604
#define TVM_NUM_MAIN_COLUMNS 379
#define TVM_NUM_AUX_COLUMNS 91
int32_t tvm_all_quotients_combined(tvm_ctx* ctx, const tvm_table* main_table, const tvm_table* aux_table,
                                   tvm_domain trace_domain, tvm_domain quotient_domain,
                                   const uint64_t* h_challenges, const uint64_t* h_weights,
                                   uint64_t* d_quotient_codeword);

/* The same quotient as COEFFICIENTS, for the prover that only needs the segments (tvm_quotient_segments_from_coefficients): where
 * valid-trace mode evaluates the classes on cosets of the trace domain plus a remainder block (TVM_OPTION_AIR_VALID_TRACE and
 * TVM_OPTION_AIR_REMAINDER_COSET hold, the trace has at least TVM_OPTION_AIR_REMAINDER_MIN_ROWS rows, the tables were extended onto the
 * quotient domain, every class's quotient fits), the sum of the classes' quotients exists in coefficient form before any codeword does,
 * and the initial / terminal quotients of the degree-4 constraints are obtained the same way (four cosets and a block of a fifth).
 * d_coeffs: capacity XFE, at least 4 * trace_domain.length + n1 (n1 = the rows of one block of the tables; quotient_domain.length always
 * suffices); *n_coeffs: the number written -- every coefficient of the quotient beyond it is zero.  Evaluated on the quotient domain they
 * are the codeword of tvm_all_quotients_combined, word for word (valid trace).  TVM_NOT_APPLICABLE, *n_coeffs = 0 and nothing written
 * where those conditions do not hold: call tvm_all_quotients_combined.  (The conditions, as code: the remainder route of
 * csrc/quotient_plan.h, which decides the route of both entry points.) */
int32_t tvm_all_quotients_coefficients(tvm_ctx* ctx, const tvm_table* main_table, const tvm_table* aux_table,
                                       tvm_domain trace_domain, tvm_domain quotient_domain,
                                       const uint64_t* h_challenges, const uint64_t* h_weights,
                                       uint64_t* d_coeffs, uint64_t capacity, uint64_t* n_coeffs);

/* ---- the AIR on the trace itself: triton_constraints_evaluate_to_zero (stark.rs:2849-3016) on the device ----------------------
 * Initial constraints on row 0, consistency constraints on every row, transition constraints on the rows (r, r + 1), r < n_rows - 1,
 * terminal constraints on row n_rows - 1 -- the precondition of TVM_OPTION_AIR_VALID_TRACE.  d_main_trace [379][n_rows] words,
 * d_aux_trace [91][n_rows][3] words (the column-major traces tvm_lde_table takes), n_rows a power of two >= 2; h_challenges: 63 XFE;
 * seed: 32 bytes for the weights of the screen (NULL: a fixed seed).  The device screens every row with a random linear combination
 * of its applicable constraints (a row that fails passes the screen with probability 2^-192); the host evaluates the constraints of
 * the lowest failing rows (tvm_host_air_constraints) and reports which of them do not vanish.
 * *failing_rows: the number of rows with at least one applicable non-zero constraint.  h_failures [capacity][2]: (row, constraint
 * index 0..603, numbered as tvm_host_air_constraints numbers them) of the lowest failing rows, ascending by row, then by index (the
 * last row listed may be cut short by the capacity).  *n_failures: the number of entries written.  A row the screen flags on which
 * no applicable constraint fails on the host is an internal error (TVM_ERR_DEVICE).  Synchronises the context's stream. */
int32_t tvm_check_constraints(tvm_ctx* ctx, const uint64_t* d_main_trace, const uint64_t* d_aux_trace, uint64_t n_rows,
                              const uint64_t* h_challenges, const uint8_t seed[32], uint64_t capacity,
                              uint64_t* h_failures, uint64_t* n_failures, uint64_t* failing_rows);

/* ---- A3 in valid-trace mode, piecewise (for a host that distributes the evaluation over several GPUs).  The
 * constraints are generated in four classes by the length of their quotients: bit 0 = the initial / terminal quotients of degree-4
 * constraints (needed on every point of the quotient domain), bit 1 = "half" (fewer than 4N coefficients), bit 2 = "quarter"
 * (fewer than 2N), bit 3 = "three cosets" (fewer than 3N).  tvm_air_class_cosets: how many cosets of the trace domain determine
 * each class's quotient polynomial for these tables' interpolant lengths (out[class bit]; 0 = the degree bound -- csrc/quotient_plan.h: fits -- does not hold: use
 * tvm_all_quotients_combined on every point).  tvm_air_class_values: sum over the constraints of the classes in class_mask of
 * weight * constraint * zerofier inverse on coset `coset` of table_domain (the domain the tables were extended onto; X = its
 * length / N cosets, coset k = the points k + X j) -> trace_domain.length XFE in the coset's natural order.
 * tvm_coset_values_to_coefficients: the values of a polynomial of fewer than n_cosets * N coefficients on n_cosets <= 4 cosets
 * h_offsets[j] * <w_N> -> its coefficients, ADDED to d_coeffs (n_cosets * N XFE).  On a valid trace the sum over the classes,
 * evaluated on the quotient domain, plus the class-0 values is exactly the output of tvm_all_quotients_combined. */
#define TVM_AIR_CLASS_FULL 1
#define TVM_AIR_CLASS_HALF 2
#define TVM_AIR_CLASS_QUARTER 4
#define TVM_AIR_CLASS_THREE 8
int32_t tvm_air_class_cosets(const tvm_table* main_table, const tvm_table* aux_table, tvm_domain trace_domain, uint32_t out[4]);
int32_t tvm_air_class_values(tvm_ctx* ctx, const tvm_table* main_table, const tvm_table* aux_table, tvm_domain trace_domain,
                             tvm_domain table_domain, uint32_t coset, uint32_t class_mask, const uint64_t* h_challenges,
                             const uint64_t* h_weights, uint64_t* d_out);
int32_t tvm_coset_values_to_coefficients(tvm_ctx* ctx, tvm_domain trace_domain, uint32_t n_cosets, const uint64_t* h_offsets,
                                         const uint64_t* const* d_values, uint64_t* d_coeffs);

/* ---- Q3-Q5: interpolate_quotient_segments, ldt_domain_segment_polynomials and
 * randomize_quotient_segments (stark.rs:1224-1283, 1302-1356) in one call ---------------------
 * d_quotient_codeword: quotient_domain.length XFE (the output of all_quotients_combined).
 * h_randomizer: the n_rand XFE coefficients of the quotient-segment randomizer polynomial s_4
 * (host RNG, stark.rs:1316-1322).  zeta: Stark::ZETA as a Montgomery word (stark.rs:1801).
 * out_table: the [ldt.length][5] XFE table of randomized segment codewords (device handle, hashable
 * with tvm_table_merkle_tree); d_polys: [5][poly_len] XFE coefficients, poly_len >= max(quotient/4, n_rand). */
int32_t tvm_quotient_segments(tvm_ctx* ctx, const uint64_t* d_quotient_codeword, tvm_domain quotient_domain,
                              tvm_domain ldt_domain, const uint64_t* h_randomizer, uint64_t n_rand, uint64_t zeta,
                              tvm_table** out_table, uint64_t* d_polys, uint64_t poly_len);
/* The same from the quotient's coefficients (tvm_all_quotients_coefficients): d_coeffs n_coeffs XFE, the coefficients beyond them zero;
 * poly_len >= max(ceil(n_coeffs / 4), n_rand).  What tvm_quotient_segments does after interpolating its codeword. */
int32_t tvm_quotient_segments_from_coefficients(tvm_ctx* ctx, const uint64_t* d_coeffs, uint64_t n_coeffs, tvm_domain ldt_domain,
                                                const uint64_t* h_randomizer, uint64_t n_rand, uint64_t zeta,
                                                tvm_table** out_table, uint64_t* d_polys, uint64_t poly_len);
/* row-wise linear combination of a table's columns over its ldt-domain view: d_out[i] = sum_c w_c * cell(i, c)
 * (the P and R combinations of the randomized segments, stark.rs:520-540).  h_weights: n_cols XFE. */
int32_t tvm_table_linear_combination(tvm_ctx* ctx, const tvm_table* table, uint64_t ldt_length,
                                     const uint64_t* h_weights, uint64_t* d_out);

/* ---- D1 + D2: deep_codeword for up to 4 components and their weighted sum (stark.rs:566-625) --
 * d_out[i] = sum_k weight_k * (codeword_k[i] - value_k) / (domain.value(i) - point_k), all XFE. */
int32_t tvm_deep_codeword(tvm_ctx* ctx, uint32_t n_components, const uint64_t* const* d_codewords, tvm_domain domain,
                          const uint64_t* h_points, const uint64_t* h_values, const uint64_t* h_weights,
                          uint64_t* d_out);
/* The same with the three small arrays in device memory (n_components XFE each), where earlier kernels of the stream may have left
 * them: nothing is copied, nothing waits (csrc/proof_middle.hip: k_deep_dev, k_deep_short_dev). */
int32_t tvm_deep_codeword_device_args(tvm_ctx* ctx, uint32_t n_components, const uint64_t* const* d_codewords, tvm_domain domain,
                                      const uint64_t* d_points, const uint64_t* d_values, const uint64_t* d_weights,
                                      uint64_t* d_out);

/* ---- the PROOF MIDDLE: from the quotient's Merkle root to the DEEP codeword (Prover::prove steps 12-16, stark.rs:444-639) with the
 * transcript on the device, without the host in between (csrc/proof_middle.hip) ------------------------------
 * d_main_trace [n_main_cols][n_rows] words and d_aux_trace [n_aux_cols][n_rows][3] with their trace randomizers ([cols][h] elements),
 * column-major as tvm_out_of_domain_rows takes them, over trace_domain (offset 1, length n_rows); d_polys: the five segment
 * polynomials [5][poly_len] XFE and `segments` their table, as tvm_quotient_segments made them; d_quotient_nodes: the tree over that
 * table (tvm_table_merkle_tree), or null when h_sponge_state already holds the quotient root; short_domain: the shorter of the
 * quotient and the LDT domain, at most the table's rows; zeta: Stark::ZETA.  On the stream, in the order of Prover::prove:
 *     ProofItem::MerkleRoot(d_quotient_nodes[1]) absorbed (where given); sample_scalars(1) = alpha            stark.rs:444-452
 *     the points alpha, alpha * trace_domain.generator, alpha^4, (zeta alpha)^4                                stark.rs:454-476
 *     the out-of-domain rows of both tables at the first two (tvm_out_of_domain_rows), the five segment
 *     polynomials at the last two (tvm_evaluate_polys_at_points)                                               stark.rs:456-476
 *     the six out-of-domain items absorbed (main row, aux row, main next row, aux next row, segments 0..3 at
 *     alpha^4, segments 1..4 at (zeta alpha)^4); sample_scalars(3) = w0, w1, w2                                stark.rs:478-505
 *     the weighted sum of all columns with the powers of w0 (tvm_weighted_sum_of_columns of both tables, added),
 *     its codeword on short_domain and its values at alpha and alpha * generator; the segment combinations with
 *     (w1^0..w1^3, 0) and (0, w1^1..w1^4) on short_domain (tvm_table_linear_combination) and their values    stark.rs:507-543
 *     d_combination (short_domain.length XFE) = tvm_deep_codeword of those four with the weights w2^0..w2^3   stark.rs:545-625
 * h_block receives TVM_MIDDLE_BLOCK_WORDS(n_main_cols, n_aux_cols) words (block_capacity: at least that many), at the offsets
 * below.  The caller enqueues the root and the six items from it and replays both samplings on its own sponge, which must arrive at
 * the same alpha, w0..w2 and state.  ONE stream synchronisation, at the end.  On bad arguments nothing is queued. */
#define TVM_MIDDLE_ROOT 0u                                                  /* [5]; zeros without a tree */
#define TVM_MIDDLE_POINTS 5u                                                /* [4][3]: alpha, alpha * omega, alpha^4, (zeta alpha)^4 */
#define TVM_MIDDLE_MAIN_ROWS 17u                                            /* [2][n_main][3]: the row at alpha, the next row */
#define TVM_MIDDLE_AUX_ROWS(n_main) (17u + 6u * (n_main))                   /* [2][n_aux][3] */
#define TVM_MIDDLE_SEGMENTS(n_main, n_aux) (17u + 6u * ((n_main) + (n_aux))) /* [5][2][3]: polynomial k at alpha^4, (zeta alpha)^4 */
#define TVM_MIDDLE_VALUES(n_main, n_aux) (TVM_MIDDLE_SEGMENTS(n_main, n_aux) + 30u)   /* [4][3]: the DEEP values */
#define TVM_MIDDLE_WEIGHTS(n_main, n_aux) (TVM_MIDDLE_VALUES(n_main, n_aux) + 12u)    /* [3][3]: w0, w1, w2 */
#define TVM_MIDDLE_STATE(n_main, n_aux) (TVM_MIDDLE_WEIGHTS(n_main, n_aux) + 9u)      /* [16]: the sponge afterwards */
#define TVM_MIDDLE_BLOCK_WORDS(n_main, n_aux) (TVM_MIDDLE_STATE(n_main, n_aux) + 16u)
int32_t tvm_out_of_domain_to_deep(tvm_ctx* ctx, const uint64_t* d_main_trace, uint64_t n_main_cols, const uint64_t* d_main_randomizers,
                                  const uint64_t* d_aux_trace, uint64_t n_aux_cols, const uint64_t* d_aux_randomizers, uint64_t n_rows,
                                  uint64_t num_trace_randomizers, tvm_domain trace_domain, const uint64_t* d_polys, uint64_t poly_len,
                                  const tvm_table* segments, const uint64_t* d_quotient_nodes, tvm_domain short_domain, uint64_t zeta,
                                  const uint64_t* h_sponge_state, uint64_t* d_combination, uint64_t* h_block, uint64_t block_capacity);
uint64_t tvm_out_of_domain_to_deep_block_words(uint64_t n_main_cols, uint64_t n_aux_cols);   /* TVM_MIDDLE_BLOCK_WORDS */
/* The weight vectors of steps 14-15 alone, as tvm_out_of_domain_to_deep forms them on the device (k_weight_vectors), from host arrays
 * (an entry point of its own, as tvm_sponge_sample_indices is).  h_scalars [3][3]: w0, w1, w2; h_segments [5][2][3]: the segment
 * polynomials at the two points.  h_w_columns [n_columns][3] = w0^0 .. w0^(n_columns - 1); h_wp [5][3] = (w1^0 .. w1^3, 0);
 * h_wr [5][3] = (0, w1^1 .. w1^4); h_wd [4][3] = w2^0 .. w2^3; h_pr_values [2][3] = sum_{k<4} w1^k segments[k][0],
 * sum_{1<=k<5} w1^k segments[k][1].  One launch, one synchronisation. */
int32_t tvm_combination_weight_vectors(tvm_ctx* ctx, const uint64_t* h_scalars, const uint64_t* h_segments, uint32_t n_columns,
                                       uint64_t* h_w_columns, uint64_t* h_wp, uint64_t* h_wr, uint64_t* h_wd, uint64_t* h_pr_values);
/* tvm_out_of_domain_to_deep with the sponge state in device memory, where the proof's front left it (TVM_FRONT_STATE of its block):
 * d_sponge_state, 16 words, is read, and on return holds the state after the combination weights (what h_block carries at
 * TVM_MIDDLE_STATE).  Everything else, the block and the one synchronisation included, as tvm_out_of_domain_to_deep. */
int32_t tvm_out_of_domain_to_deep_device_state(tvm_ctx* ctx, const uint64_t* d_main_trace, uint64_t n_main_cols,
                                               const uint64_t* d_main_randomizers, const uint64_t* d_aux_trace, uint64_t n_aux_cols,
                                               const uint64_t* d_aux_randomizers, uint64_t n_rows, uint64_t num_trace_randomizers,
                                               tvm_domain trace_domain, const uint64_t* d_polys, uint64_t poly_len, const tvm_table* segments,
                                               const uint64_t* d_quotient_nodes, tvm_domain short_domain, uint64_t zeta,
                                               uint64_t* d_sponge_state, uint64_t* d_combination, uint64_t* h_block, uint64_t block_capacity);

/* ---- the PROOF FRONT: from the main table's Merkle root to the quotient weights (Prover::prove steps 5-10, stark.rs:369-401) with the
 * transcript on the device, without the host in between (csrc/proof_front.hip) -------------------------------
 * The front's state lives in a block of TVM_FRONT_BLOCK_WORDS words of device memory that the CALLER owns (tvm_malloc), because several
 * entry points queue work on it in turn; the kernels that take challenges and weights from device memory (the _device_args entry points
 * below) are pointed at its parts.  The long weight vector comes last: the first TVM_FRONT_HEAD_WORDS words are all a host replays. */
#define TVM_FRONT_MAIN_ROOT 0u        /* [5] */
#define TVM_FRONT_AUX_ROOT 5u         /* [5] */
#define TVM_FRONT_CHALLENGES 10u      /* [63][3]: the 59 sampled challenges, then the terminals of input, output, lookup table, digest */
#define TVM_FRONT_WEIGHT_SCALAR 199u  /* [3]: the scalar whose powers are the quotient weights */
#define TVM_FRONT_STATE 202u          /* [16]: the sponge, after the last front call queued */
#define TVM_FRONT_HEAD_WORDS 218u
#define TVM_FRONT_WEIGHTS 218u        /* [604][3]: the scalar's powers 0 .. 603 */
#define TVM_FRONT_BLOCK_WORDS 2030u
/* Steps 5-6: h_sponge_state (16 words), the claim's program digest (5 words), public input and public output (Montgomery words, any
 * length; null where the length is 0) are staged, then on the stream: ProofItem::MerkleRoot(d_main_nodes[1]) absorbed and handed out
 * (TVM_FRONT_MAIN_ROOT), sample_scalars(59), and the four derived challenges of Challenges::new (challenges.rs:85-121) --
 * EvalArg::compute_terminal of the input at challenge 1, the output at challenge 2, Tip5's lookup table at challenge 54 and the digest
 * at challenge 0.  d_main_nodes: the main table's tree [2 L][5].  Does NOT synchronise; on bad arguments nothing is queued. */
int32_t tvm_front_challenges(tvm_ctx* ctx, const uint64_t* d_main_nodes, const uint64_t* h_sponge_state, const uint64_t* h_program_digest,
                             const uint64_t* h_input, uint64_t n_input, const uint64_t* h_output, uint64_t n_output, uint64_t* d_front);
/* Steps 9-10: ProofItem::MerkleRoot(d_aux_nodes[1]) absorbed into the state in the block and handed out (TVM_FRONT_AUX_ROOT),
 * sample_scalars(1) (TVM_FRONT_WEIGHT_SCALAR), its powers 0 .. 603 (TVM_FRONT_WEIGHTS).  Does NOT synchronise. */
int32_t tvm_front_quotient_weights(tvm_ctx* ctx, const uint64_t* d_aux_nodes, uint64_t* d_front);
/* Queues the download of the block's first n_words words (1 .. TVM_FRONT_BLOCK_WORDS) into h_block.  wait != 0: synchronises the
 * stream.  wait == 0: h_block must stay alive, and its words are valid only after the context's next synchronisation (tvm_sync, or any
 * entry point that synchronises). */
int32_t tvm_front_block(tvm_ctx* ctx, const uint64_t* d_front, uint64_t* h_block, uint64_t n_words, uint32_t wait);
uint64_t tvm_front_block_words(void);   /* TVM_FRONT_BLOCK_WORDS */
/* The entry points that take challenges (63 XFE) and quotient weights (604 XFE) from HOST arrays, with those arrays in DEVICE memory
 * instead, where earlier work of the stream may have left them (TVM_FRONT_CHALLENGES, TVM_FRONT_WEIGHTS of a front block): the same
 * bodies without the staging copy -- nothing is copied, nothing waits.  The arrays are only read and must not be freed or overwritten
 * before the work queued here has run. */
int32_t tvm_extend_aux_table_device_args(tvm_ctx* ctx, const uint64_t* d_main_trace, uint64_t* d_aux_trace, uint64_t n_rows,
                                         const uint64_t* d_challenges);
int32_t tvm_fill_derived_aux_columns_device_args(tvm_ctx* ctx, const uint64_t* d_main_trace, uint64_t* d_aux_trace, uint64_t n_rows,
                                                 const uint64_t* d_challenges);
int32_t tvm_all_quotients_combined_device_args(tvm_ctx* ctx, const tvm_table* main_table, const tvm_table* aux_table,
                                               tvm_domain trace_domain, tvm_domain quotient_domain, const uint64_t* d_challenges,
                                               const uint64_t* d_weights, uint64_t* d_quotient_codeword);
int32_t tvm_all_quotients_coefficients_device_args(tvm_ctx* ctx, const tvm_table* main_table, const tvm_table* aux_table,
                                                   tvm_domain trace_domain, tvm_domain quotient_domain, const uint64_t* d_challenges,
                                                   const uint64_t* d_weights, uint64_t* d_coeffs, uint64_t capacity, uint64_t* n_coeffs);

/* ---- the PROOF TAIL: what follows the commit phase of Fri::prove (fri.rs:265-319) and the trace openings of Prover::prove
 * (stark.rs:665-716) with the transcript on the device (csrc/proof_tail.hip) ------------------------------------
 * Tip5::sample_indices [twenty-first] (proof_stream.rs:86-104) on the device, squeezing straight from the given sponge state (no
 * item is absorbed): the rate is read, an element whose canonical value is p - 1 is skipped, the others give value % upper_bound,
 * and the state is permuted whenever its ten rate words are used up.  upper_bound: a power of two, at most 2^32; n <= 2^16.
 * h_indices_out: n words; h_state_out: the 16 words of the sponge afterwards.  One launch, one synchronisation. */
int32_t tvm_sponge_sample_indices(tvm_ctx* ctx, const uint64_t* h_state, uint64_t upper_bound, uint64_t n,
                                  uint64_t* h_indices_out, uint64_t* h_state_out);
/* MerkleTree::authentication_structure [twenty-first] for n_trees trees at once, ONE launch (a workgroup per tree) and ONE
 * synchronisation.  Tree j has n_leaves[j] leaves (a power of two, 1 .. TVM_VERIFIER_MAX_LEAVES) and is opened at the n_indices[j]
 * leaf indices h_indices[j] (any order, duplicates allowed, at most TVM_TAIL_MAX_INDICES).  h_node_indices_out[j]: the heap indices
 * of the nodes a verifier cannot compute from the opened leaves, in descending heap order -- room for
 * min(n_indices[j], n_leaves[j]) * log2(n_leaves[j]) words; n_out[j]: their number.  d_nodes[j] (the array may be null, and so
 * may any entry): the tree's nodes [2 n_leaves][5] on the device, as tvm_merkle_tree writes them -- h_nodes_out[j] then receives
 * the n_out[j] digests at those heap indices; a null entry plans the index list alone, for a tree that is not in memory.
 * TVM_NOT_APPLICABLE and nothing written when a tree has more than TVM_TAIL_MAX_INDICES indices. */
#define TVM_TAIL_MAX_INDICES 1024u
int32_t tvm_authentication_structures(tvm_ctx* ctx, uint32_t n_trees, const uint64_t* n_leaves, const uint64_t* const* h_indices,
                                      const uint64_t* n_indices, const uint64_t* const* d_nodes, uint64_t* const* h_node_indices_out,
                                      uint64_t* const* h_nodes_out, uint64_t* n_out);
/* Everything of a FRI proof after the commit phase, and the trace openings, without the host in between.  d_codeword, domain,
 * n_rounds, d_codewords and d_nodes are the arguments of tvm_fri_commit_phase after it has returned; h_sponge_state is the sponge
 * after the commit phase's enqueues and samplings.  On the stream: the last codeword is interpolated (over the domain of its
 * length with offset 1); ProofItem::Polynomial(last polynomial, trailing zeros dropped) is absorbed (proof_stream.rs:54-59; the
 * last codeword is a proof item outside the Fiat-Shamir heuristic, proof_item.rs:96-150, and is only handed back);
 * n_checks indices are sampled below domain.length (the `a` indices);
 * the authentication structures of every answered round are computed; and the payloads of the items that follow are written in
 * proof-item order:
 *     round 0 at the a indices: leaves, authentication structure
 *     rounds 0 .. n_rounds - 1 at the b indices (a mod n + n/2) mod n, n the round's length: leaves, authentication structure
 *     main rows, main authentication structure, aux rows, aux ..., quotient-segment rows, quotient ...: the rows of tables[0..2] on
 *     the view of ldt_length rows (as tvm_table_reveal_rows) at the a indices; the three trees d_table_nodes[0..2] share the
 *     structure of round 0 at the a indices.  ldt_length must be domain.length.
 * That is TVM_TAIL_ITEMS(n_rounds) payloads.  h_directory [items][2]: (offset, words) of each payload in h_payload;
 * *payload_words: their sum -- they are copied when payload_capacity suffices, TVM_ERR_INVALID_ARGUMENT otherwise
 * (tvm_fri_query_and_open_payload_bound words always suffice). h_state_out: the sponge after the sampling (16 words); h_indices_out: n_checks
 * words; h_last_codeword, h_last_polynomial: 3 * (domain.length >> n_rounds) words each (the polynomial with its trailing zeros).
 * The caller replays the two enqueues and the sampling on its own sponge, which must arrive at h_state_out and h_indices_out.
 * Two stream synchronisations: the fixed-size part, then the payload.  TVM_NOT_APPLICABLE and nothing written when
 * n_checks > TVM_TAIL_MAX_INDICES. */
#define TVM_TAIL_ITEMS(n_rounds) (2u * ((n_rounds) ? (n_rounds) + 1u : 1u) + 6u)
int32_t tvm_fri_query_and_open(tvm_ctx* ctx, const uint64_t* h_sponge_state, const uint64_t* d_codeword, tvm_domain domain,
                               uint32_t n_rounds, const uint64_t* const* d_codewords, const uint64_t* const* d_nodes,
                               uint64_t n_checks, const tvm_table* const* tables, const uint64_t* const* d_table_nodes,
                               uint64_t ldt_length, uint64_t* h_state_out, uint64_t* h_indices_out, uint64_t* h_last_codeword,
                               uint64_t* h_last_polynomial, uint64_t* h_directory, uint64_t* h_payload, uint64_t payload_capacity,
                               uint64_t* payload_words);
/* an upper bound of *payload_words: every response and opening with an authentication structure of n_checks full paths */
uint64_t tvm_fri_query_and_open_payload_bound(tvm_domain domain, uint32_t n_rounds, uint64_t n_checks, const tvm_table* const* tables);

/* ---- the ROUNDS OF STIR: the whole of Stir::prove (stir.rs:885-993) with the transcript on the device, without the host in between
 * (csrc/stir_rounds.hip).  d_codeword: domain.length XFE, the codeword to be proven close to low degree;
 * round_queries [n_rounds][2] = (in-domain queries, out-of-domain queries) of the full rounds, final_queries those of the final
 * round, final_degree the instance's bound on the final polynomial (below domain.length / folding_factor^(n_rounds + 1), the
 * number of coefficients handed back); folding_factor: a power of two, 2 .. 16.  h_sponge_state: the sponge before Stir::prove.
 * On the stream, per full round r: sample_scalars(1) (the folding randomness); the folded polynomial, its codeword on the next
 * round's domain, the stacked Merkle tree of that (tree r + 1; tree 0 is over d_codeword), ProofItem::MerkleRoot absorbed;
 * sample_scalars(n_ood) (the out-of-domain points); the folded polynomial there, ProofItem::StirOutOfDomainValues absorbed (also
 * when it is empty); sample_indices(the round's domain length, n_in_domain); sample_scalars(1) (the degree-correction randomness);
 * the indices mod the folded domain's length without repeats, in order of first occurrence; the quotient set, the answer
 * polynomial and the next round's witness polynomial (as tvm_xfe_interpolate and tvm_stir_next_polynomial).  The final round:
 * sample_scalars(1), the fold, ProofItem::Polynomial absorbed, sample_indices(its domain's length, final_queries).  Then the
 * StirResponse payloads of trees 0 .. n_rounds in proof-item order -- per tree: the stacked leaves (folding_factor XFE per index, at
 * the indices without repeats), the authentication structure -- packed into h_payload.
 *   h_state_out         16 words: the sponge at the end
 *   h_roots             [n_rounds + 1][5]
 *   h_scalars           every sampled scalar in transcript order: per full round the folding randomness, the n_ood out-of-domain
 *                       points, the degree-correction randomness; then the final folding randomness: 3 (2 n_rounds + 1 + sum n_ood) words
 *   h_ood_values        [sum n_ood][3], round by round (may be null when there are none)
 *   h_indices           the sampled indices of rounds 0 .. n_rounds, one list behind the other (sum of the in-domain query counts words)
 *   h_unique            the same shape: each round's indices without repeats at the place of its sampled ones, h_unique_counts
 *                       [n_rounds + 1] of them valid
 *   h_final_polynomial  domain.length / folding_factor^(n_rounds + 1) XFE, with its trailing zeros
 *   h_directory         [2 (n_rounds + 1)][2]: (offset, words) of each payload in h_payload; *payload_words: their sum -- they are
 *                       copied when payload_capacity suffices, TVM_ERR_INVALID_ARGUMENT otherwise
 *                       (tvm_stir_prove_rounds_payload_bound words always suffice)
 * The caller replays every enqueue and every sampling on its own sponge, which must arrive at the same scalars, indices and state.
 * Two stream synchronisations: the fixed-size part, then the payload.  TVM_NOT_APPLICABLE, nothing written and nothing queued when a
 * round (the final one included) has more than TVM_TAIL_MAX_INDICES in-domain queries, or a full round more than 256 queries in all
 * (the limit of the one-workgroup interpolation; the final round has no quotient set).  TVM_ERR_INVALID_ARGUMENT afterwards if two points of a quotient set coincide. */
int32_t tvm_stir_prove_rounds(tvm_ctx* ctx, const uint64_t* h_sponge_state, const uint64_t* d_codeword, tvm_domain domain,
                              uint32_t folding_factor, uint32_t n_rounds, const uint64_t* round_queries, uint64_t final_queries,
                              uint64_t final_degree, uint64_t* h_state_out, uint64_t* h_roots, uint64_t* h_scalars,
                              uint64_t* h_ood_values, uint64_t* h_indices, uint64_t* h_unique, uint64_t* h_unique_counts,
                              uint64_t* h_final_polynomial, uint64_t* h_directory, uint64_t* h_payload, uint64_t payload_capacity,
                              uint64_t* payload_words);
/* an upper bound of *payload_words: every response with all its indices distinct and full authentication paths; 0 where
 * tvm_stir_prove_rounds does not apply */
uint64_t tvm_stir_prove_rounds_payload_bound(tvm_domain domain, uint32_t folding_factor, uint32_t n_rounds, const uint64_t* round_queries,
                                             uint64_t final_queries);

/* ---- F1: ProverRound::split_and_fold (fri.rs:349-366): domain.length XFE -> domain.length/2 XFE */
int32_t tvm_fri_split_and_fold(tvm_ctx* ctx, const uint64_t* d_codeword, tvm_domain domain,
                               const uint64_t* h_challenge, uint64_t* d_out);

/* ---- F1 + H2 + the transcript in between: the COMMIT PHASE of Fri::prove (fri.rs:212-263) without the host in the loop.
 * For r = 0 .. n_rounds: the Merkle tree of codeword r (d_nodes[r], 10 * (domain.length >> r) words, as
 * tvm_codeword_merkle_tree), its root absorbed into the Fiat-Shamir sponge as ProofItem::MerkleRoot (proof_item.rs:96,
 * proof_stream.rs:54-59: the encoding [0, root] padded with 1, 0, 0, 0 is exactly one absorbed block) and, for r < n_rounds,
 * one scalar sampled from the sponge (proof_stream.rs:81-84) and codeword r + 1 = split_and_fold(codeword r, that scalar)
 * written to d_codewords[r] (3 * (domain.length >> (r + 1)) words).  The sponge runs on the device: no stream
 * synchronisation until the roots and challenges are copied out at the end.
 * h_sponge_state: the 16 words of the Tip5 sponge before the first root is enqueued (not modified: the caller replays the
 * n_rounds + 1 enqueues and n_rounds samplings on its own sponge, which must reproduce h_challenges);
 * h_roots: (n_rounds + 1) * 5 words; h_challenges: n_rounds * 3 words. */
int32_t tvm_fri_commit_phase(tvm_ctx* ctx, const uint64_t* d_codeword, tvm_domain domain, uint32_t n_rounds,
                             const uint64_t* h_sponge_state, uint64_t* const* d_codewords, uint64_t* const* d_nodes,
                             uint64_t* h_roots, uint64_t* h_challenges);

/* ---- coset-wise ("just in time") evaluation: Prover::compute_quotient_segments_with_jit_lde and the JIT branch of
 * hash_all_ldt_domain_rows (stark.rs:805-1006, master_table.rs:470-503) -------------------------------------
 * When the extended tables do not fit, the reference evaluates them coset by coset.  Here a coset group is an
 * arithmetic domain of its own (offset * generator^r, generator^R, length / R), so tvm_lde_table,
 * tvm_hash_rows and tvm_all_quotients_combined are simply called on that domain (triton_vm_amd/jit.py);
 * the only extra primitive is putting a group's results back into row order:
 *   d_dst[(i * stride + offset) * elem_words + w] = d_src[i * elem_words + w],  i < n. */
int32_t tvm_scatter_strided(tvm_ctx* ctx, const uint64_t* d_src, uint32_t elem_words, uint64_t n, uint64_t stride,
                            uint64_t offset, uint64_t* d_dst);

/* ---- S1: the STIR prover (low_degree_test/stir.rs:885-993); the round loop, sampling and inclusion proofs stay on the
 * host (triton_vm_amd/low_degree_test.py is the mirror) ---------------------------------------------------------
 * StirMerkleTree::new (stir.rs:1380-1419): leaf i = hash_varlen(codeword[i], codeword[i + d], ...), d = length /
 * stack_height; d_nodes: [2 d][5] in heap order. */
int32_t tvm_stir_merkle_tree(tvm_ctx* ctx, const uint64_t* d_xfe_codeword, uint64_t length, uint32_t stack_height,
                             uint64_t* d_nodes);
/* Stir::fold_polynomial (stir.rs:1132-1147): d_out[i] = sum_j d_poly[ff*i + j] * r^j; ceil(n_coeffs / ff) XFE out */
int32_t tvm_fold_polynomial(tvm_ctx* ctx, const uint64_t* d_poly, uint64_t n_coeffs, uint32_t folding_factor,
                            const uint64_t* h_randomness, uint64_t* d_out);
/* The witness polynomial of the next round (stir.rs:945-966):
 *   ((folded - Ans) / prod_j (X - quotient_set[j])) * sum_{e <= k} (r X)^e
 * h_answer_poly: the k coefficients of Ans (Polynomial::interpolate over the quotient set, tvm_host_xfe_interpolate);
 * work_domain: any coset of at least n_coeffs points that avoids the quotient set (the caller's choice);
 * d_out_poly: work_domain.length XFE coefficients (zero above n_coeffs - 1). */
int32_t tvm_stir_next_polynomial(tvm_ctx* ctx, const uint64_t* d_folded_poly, uint64_t n_coeffs,
                                 const uint64_t* h_quotient_set, const uint64_t* h_answer_poly, uint32_t k,
                                 const uint64_t* h_degree_correction_randomness, tvm_domain work_domain,
                                 uint64_t* d_out_poly);
/* host: coefficients of the polynomial of degree < k through k XFE points (pairwise distinct) */
int32_t tvm_host_xfe_interpolate(const uint64_t* points, const uint64_t* values, uint32_t k, uint64_t* out_coeffs);
/* the same on the device (one workgroup; k <= 256, beyond that it calls the host function): the prover's round loop does not
 * leave the GPU idle for the 0.9 ms the host form takes at k = 204 */
int32_t tvm_xfe_interpolate(tvm_ctx* ctx, const uint64_t* h_points, const uint64_t* h_values, uint32_t k, uint64_t* h_out_coeffs);

/* ---- small transfers and host-side helpers ----------------------------------------------------
 * gather n elements of elem_words words each from a device array at the given element indices
 * (Merkle authentication-structure nodes, FRI leaves, single codeword entries) into host memory */
int32_t tvm_gather_elements(tvm_ctx* ctx, const uint64_t* d_src, uint32_t elem_words, const uint64_t* h_indices,
                            uint64_t n, uint64_t* h_out);
/* The same for n_jobs gathers at once -- all the FRI responses and authentication structures of a proof (fri.rs:295-319),
 * or the three trace openings (stark.rs:672-716) -- with ONE transfer of the indices, one of the results and two stream
 * synchronisations in all instead of two per gather.  Job j reads n[j] elements of elem_words[j] words from d_src[j] at
 * h_indices[j][0..n[j]) and writes them to h_out[j]. */
int32_t tvm_gather_elements_batch(tvm_ctx* ctx, uint32_t n_jobs, const uint64_t* const* d_src, const uint32_t* elem_words,
                                  const uint64_t* const* h_indices, const uint64_t* n, uint64_t* const* h_out);
/* Host-side (CPU) field helpers for callers that do not link twenty-first (the C++/Python test
 * drivers); a Rust host uses twenty-first instead.  No device work. */
void tvm_host_tip5_permutation(uint64_t state[16]);
/* overwrite-mode absorb of n words followed by the padding 1, 0, ... (variable-length domain) */
void tvm_host_sponge_pad_and_absorb(uint64_t state[16], const uint64_t* words, uint64_t n);
void tvm_host_xfe_mul(const uint64_t a[3], const uint64_t b[3], uint64_t out[3]);
void tvm_host_xfe_inv(const uint64_t a[3], uint64_t out[3]);
void tvm_host_xfe_powers(const uint64_t x[3], uint64_t first_exponent, uint64_t n, uint64_t* out /* n XFE */);
/* out[j] = sum_i coeffs[i] * points[j]^i, or with zerofier != 0: prod_i (points[j] - coeffs[i]); n, m XFE in, m XFE out */
void tvm_host_xfe_poly_eval(const uint64_t* coeffs, uint64_t n, const uint64_t* points, uint64_t m, int32_t zerofier,
                            uint64_t* out);
/* n draws of `rng.random::<BFieldElement>()` from `StdRng::from_seed(seed)` (the prover's trace, batch and quotient
 * randomizers: master_table.rs:423-434, 1006-1024, stark.rs:1315-1322; a Rust host uses rand itself), Montgomery words */
void tvm_host_stdrng_elements(const uint8_t seed[32], uint64_t n, uint64_t* out);
/* the same n elements into device memory, generated on the device (one ChaCha block per work-item); when a draw takes the
 * range sampler's rare short path the stream is regenerated sequentially on the host -- the result is always the host's */
int32_t tvm_stdrng_elements(tvm_ctx* ctx, const uint8_t seed[32], uint64_t n, uint64_t* d_out);
/* n_streams generators at once: stream s is `StdRng::from_seed(seed + s)` (the 256-bit little-endian sum: rng_from_offset_seed,
 * master_table.rs:630-662 -- a table's trace randomizers, one stream per column, master_table.rs:423-434), per_stream draws
 * each, d_out[s * per_stream + i].  One launch; the same rare-short-path rule as tvm_stdrng_elements (then every stream is drawn
 * on the host).  Replaces 1.3 ms of sequential ChaCha on the host per proof (470 streams at 198 randomizers). */
int32_t tvm_stdrng_streams(tvm_ctx* ctx, const uint8_t seed[32], uint64_t n_streams, uint64_t per_stream, uint64_t* d_out);

/* The RAM table's Bezout coefficient polynomials: bezout_coefficient_polynomials_coefficients (table/ram.rs:152-207) for n
 * pairwise distinct roots (the unique RAM pointers, device array): a and b with a * rp + b * rp' = 1, rp = prod (X - r_i),
 * n coefficients each (device arrays).  TVM_ERR_INVALID_ARGUMENT when two roots coincide. */
int32_t tvm_bezout_coefficients(tvm_ctx* ctx, const uint64_t* d_roots, uint64_t n, uint64_t* d_a, uint64_t* d_b);

/* ---- verifier batch work --------------------------------------------------------
 * Verifier::verify's work over the num_first_round_queries revealed rows (stark.rs:1388-1763), all host data in / out:
 * the leaf digests of revealed rows (Tip5::hash_varlen of each row, stark.rs:1598-1601, 1620-1660) ... */
int32_t tvm_verifier_row_digests(tvm_ctx* ctx, const uint64_t* h_rows, uint64_t n_rows, uint64_t row_words,
                                 uint64_t* h_digests);
/* ... and, per revealed row, linearly_sum_main_and_aux_row (stark.rs:1765-1787), the quotient-segment sums, the four
 * Stark::deep_update values (stark.rs:2096-2103) and their weighted sum (stark.rs:1678-1755), which must equal the
 * value the low-degree test revealed at that index (the comparison stays with the caller).  h_main_rows [n][379],
 * h_aux_rows [n][91][3], h_quot_rows [n][5][3], h_row_indices [n] (indices into ldt_domain), h_weights_main_aux
 * [470][3], h_weights_quot [5][3], h_weights_deep [4][3]; h_ood_points / h_ood_values [4][3] in the order current row,
 * next row, alpha^4, (zeta*alpha)^4 (stark.rs:1722-1745).  h_out: [n][3]. */
int32_t tvm_verifier_deep_values(tvm_ctx* ctx, const uint64_t* h_main_rows, const uint64_t* h_aux_rows,
                                 const uint64_t* h_quot_rows, const uint64_t* h_row_indices, uint64_t n_rows,
                                 tvm_domain ldt_domain, const uint64_t* h_weights_main_aux,
                                 const uint64_t* h_weights_quot, const uint64_t* h_weights_deep,
                                 const uint64_t* h_ood_points, const uint64_t* h_ood_values, uint64_t* h_out);

/* ---- verifier batch work outside the revealed rows (csrc/verify_ldt.hip) -------------------------------
 * Host data in, host data out; each call stages through the context's pool, is ONE launch on the context's stream and
 * synchronises it once.  A malformed input is a status or a per-job flag, never an abort.  Limits (TVM_ERR_UNSUPPORTED beyond): */
#define TVM_VERIFIER_MAX_TREES 4096u                 /* jobs per tvm_verifier_merkle_roots call */
#define TVM_VERIFIER_MAX_LEAVES (1ull << 40)         /* leaves of one tree (from 1) */
#define TVM_VERIFIER_MAX_QUERIES (1ull << 16)        /* leaf indices per tree, FRI checks, STIR queries per call */
#define TVM_VERIFIER_MAX_QUOTIENT_SET (1u << 20)     /* points of a STIR quotient set */
/* MerkleTreeInclusionProof::verify [twenty-first] up to the comparison, for all trees of a proof at once: the three row openings
 * (stark.rs:1592-1672), FRI's rounds (fri.rs:430-560), STIR's rounds (stir.rs:1157-1226).  Job j: a tree of n_leaves[j] leaves (a
 * power of two), n_indices[j] leaf indices h_indices[j] (duplicates allowed) with their digests h_leaf_digests[j] [n][5], and the
 * authentication structure h_auth[j] [n_auth[j]][5] in the order of MerkleTree::authentication_structure (descending heap index).
 * Out: the recomputed root h_roots[j][5] and h_flags[j]: non-zero (root all zero) when the job is malformed -- no index, an index
 * outside the tree, a repeated index with two digests, too few or too many authentication nodes.  The caller compares the roots.
 * At most 64 * TVM_VERIFIER_MAX_QUERIES authentication nodes per tree and 2^31 nodes per call. */
int32_t tvm_verifier_merkle_roots(tvm_ctx* ctx, uint32_t n_jobs, const uint64_t* n_leaves, const uint64_t* n_indices,
                                  const uint64_t* const* h_indices, const uint64_t* const* h_leaf_digests,
                                  const uint64_t* n_auth, const uint64_t* const* h_auth, uint64_t* h_roots, uint32_t* h_flags);
/* All collinearity checks of all rounds of Fri::verify (fri.rs:520-560, Polynomial::get_colinear_y): query j starts from its
 * revealed A-leaf h_a_leaves[j] at first-round index h_indices[j]; in round r it is folded with the revealed B-leaf
 * h_b_leaves[r][j] (index + half the round's domain) at h_challenges[r]; the round's domain is first_domain.pow(2^r).
 * h_out [n_checks][3]: the value after round n_rounds - 1, which the caller compares with the last codeword.
 * first_domain.length >= 2^n_rounds. */
int32_t tvm_verifier_fri_folds(tvm_ctx* ctx, tvm_domain first_domain, uint32_t n_rounds, const uint64_t* h_challenges,
                               const uint64_t* h_indices, uint64_t n_checks, const uint64_t* h_a_leaves,
                               const uint64_t* h_b_leaves, uint64_t* h_out);
/* The in-domain answers of one STIR round (stir.rs:1259-1340).  Query j: the folding_factor revealed values h_values[j][ff][3] on
 * the coset h_coset_roots[j] * kth_root^i, i < ff.  k == 0: initial_in_domain_answers -- the polynomial of degree < ff through
 * them at h_folding_randomness.  k > 0: subsequent_in_domain_answers -- the values first go through the previous round's quotient
 * (value - Ans(x)) / prod_i (x - h_quotient_set[i]) and degree correction sum_{e <= k} (rc x)^e (with its rc x = 1 branch);
 * h_answer_polynomial: the k coefficients of Ans (tvm_xfe_interpolate over the quotient set).  h_out [n_queries][3].
 * folding_factor <= 16; kth_root of order >= folding_factor. */
int32_t tvm_verifier_stir_answers(tvm_ctx* ctx, uint32_t folding_factor, uint64_t n_queries, const uint64_t* h_values,
                                  const uint64_t* h_coset_roots, uint64_t kth_root, const uint64_t* h_folding_randomness,
                                  uint32_t k, const uint64_t* h_quotient_set, const uint64_t* h_answer_polynomial,
                                  const uint64_t* h_degree_correction_randomness, uint64_t* h_out);

/* ---- verifier batch work for MANY proofs per call (csrc/verify_batch.hip) --------------------------------
 * The stages above that assume one domain, one set of challenges or one set of weights per launch, for n_groups "groups" at
 * once -- a group is a proof, or one STIR round of a proof.  Host data in, host data out; each call stages through the context's
 * pool, is ONE launch on the context's stream and synchronises it once, however many groups it is given.  Per-group arguments are
 * arrays indexed by group ([n_groups]; `const uint64_t* const*`: one host pointer per group; a flat array [n_groups][w]: w words
 * per group).  h_flags[g]: 0 = group g's results were written; 1 = the group is malformed (what its one-proof entry point answers
 * TVM_ERR_INVALID_ARGUMENT or TVM_ERR_UNSUPPORTED for) and TVM_NOT_APPLICABLE = the group is beyond the kernel's bound -- nothing
 * is written for either, and the other groups are not affected.  An error status is for null arguments and device failures.
 *
 * tvm_verifier_fri_folds as group g: first_domains[g], n_rounds[g], n_checks[g], h_challenges[g] [n_rounds][3], h_indices[g]
 * [n_checks], h_a_leaves[g] [n_checks][3], h_b_leaves[g] [n_rounds][n_checks][3] -> h_out[g] [n_checks][3]. */
int32_t tvm_verifier_fri_folds_batch(tvm_ctx* ctx, uint32_t n_groups, const tvm_domain* first_domains, const uint32_t* n_rounds,
                                     const uint64_t* n_checks, const uint64_t* const* h_challenges,
                                     const uint64_t* const* h_indices, const uint64_t* const* h_a_leaves,
                                     const uint64_t* const* h_b_leaves, uint64_t* const* h_out, uint32_t* h_flags);
/* The last round of Fri::verify (fri.rs:560-640) up to its comparisons.  Group g: the last codeword h_codewords[g]
 * [lengths[g]][3] (a power of two) and the point h_points[g][3].  h_roots[g][5]: the root of the codeword's Merkle tree, as
 * tvm_codeword_merkle_tree builds it; h_values[g][3]: the value at the point of the polynomial of degree < lengths[g] that
 * interpolates the codeword over ArithmeticDomain::of_length(lengths[g]) (offset one) -- what tvm_interpolate followed by
 * tvm_evaluate_at_points gives.  One workgroup per group, for codewords of at most TVM_VERIFIER_MAX_LAST_CODEWORD elements: every
 * last codeword of the parameters derived for security levels 32 to 160 and expansion factors 2 to 8 at 2^8 to 2^24 padded rows
 * (enumerated: 1024 at most; expansion factors 16 to 256 reach 16384).  A longer one is flagged TVM_NOT_APPLICABLE: take the three
 * calls named here for it. */
#define TVM_VERIFIER_MAX_LAST_CODEWORD 1024u
int32_t tvm_verifier_fri_last_rounds(tvm_ctx* ctx, uint32_t n_groups, const uint64_t* lengths, const uint64_t* const* h_codewords,
                                     const uint64_t* h_points, uint64_t* h_roots, uint64_t* h_values, uint32_t* h_flags);
/* tvm_xfe_interpolate as group g: k[g] points h_points[g] [k][3] with values h_values[g] [k][3] -> h_out_coeffs[g] [k][3].
 * k[g] == 0: nothing to do (flag 0).  k[g] > 256, the limit of the one-workgroup interpolation: TVM_NOT_APPLICABLE (call
 * tvm_host_xfe_interpolate for that group).  Two points of a group coincide: flag 1, for that group only. */
int32_t tvm_xfe_interpolate_batch(tvm_ctx* ctx, uint32_t n_groups, const uint32_t* k, const uint64_t* const* h_points,
                                  const uint64_t* const* h_values, uint64_t* const* h_out_coeffs, uint32_t* h_flags);
/* tvm_verifier_stir_answers as group g: folding_factors[g], kth_roots[g], h_folding_randomness [n_groups][3], k[g] (0: a first
 * round; such groups and k > 0 groups may share a call) with h_quotient_sets[g] and h_answer_polynomials[g] [k][3] and
 * h_degree_correction_randomness [n_groups][3] (read where k[g] > 0), then the n_queries[g] queries: h_values[g] [n][ff][3],
 * h_coset_roots[g] [n] -> h_out[g] [n][3].  One workgroup per query. */
int32_t tvm_verifier_stir_answers_batch(tvm_ctx* ctx, uint32_t n_groups, const uint32_t* folding_factors, const uint64_t* kth_roots,
                                        const uint64_t* h_folding_randomness, const uint32_t* k,
                                        const uint64_t* const* h_quotient_sets, const uint64_t* const* h_answer_polynomials,
                                        const uint64_t* h_degree_correction_randomness, const uint64_t* n_queries,
                                        const uint64_t* const* h_values, const uint64_t* const* h_coset_roots,
                                        uint64_t* const* h_out, uint32_t* h_flags);
/* tvm_verifier_deep_values as group g: ldt_domains[g], h_weights_main_aux[g] [470][3], h_weights_quot [n_groups][5][3],
 * h_weights_deep, h_ood_points and h_ood_values [n_groups][4][3], then the n_rows[g] rows: h_main_rows[g] [n][379], h_aux_rows[g]
 * [n][91][3], h_quot_rows[g] [n][5][3], h_row_indices[g] [n] -> h_out[g] [n][3].  One workgroup per row. */
int32_t tvm_verifier_deep_values_batch(tvm_ctx* ctx, uint32_t n_groups, const tvm_domain* ldt_domains,
                                       const uint64_t* const* h_weights_main_aux, const uint64_t* h_weights_quot,
                                       const uint64_t* h_weights_deep, const uint64_t* h_ood_points, const uint64_t* h_ood_values,
                                       const uint64_t* n_rows, const uint64_t* const* h_main_rows,
                                       const uint64_t* const* h_aux_rows, const uint64_t* const* h_quot_rows,
                                       const uint64_t* const* h_row_indices, uint64_t* const* h_out, uint32_t* h_flags);

/* host: the 604 AIR constraints on ONE row pair whose main rows are XFieldElements -- what Verifier::verify evaluates on the
 * out-of-domain rows (stark.rs:1466-1491; MasterAuxTable::evaluate_{initial,consistency,transition,terminal}_constraints in
 * this order).  h_main_* [379][3], h_aux_* [91][3], h_challenges [63][3]; h_out [604][3]: initial (81), consistency (97),
 * transition (403), terminal (23). */
int32_t tvm_host_air_constraints(const uint64_t* h_main_cur, const uint64_t* h_aux_cur, const uint64_t* h_main_next,
                                 const uint64_t* h_aux_next, const uint64_t* h_challenges, uint64_t* h_out);

#ifdef __cplusplus
}
#endif
#endif /* TRITON_HIP_H */
