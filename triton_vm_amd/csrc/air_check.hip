// air_check.hip -- the AIR on the trace itself: triton_constraints_evaluate_to_zero (/root/reference/triton-vm/src/stark.rs:2849-3016)
// for traces of any height, the precondition of valid-trace mode (TVM_OPTION_AIR_VALID_TRACE) checked instead of assumed.
//
// Screen on the device, pinpoint on the host.  The trace is taken in chunks of R rows (TVM_OPTION_AIR_CHECK_CHUNK_ROWS): a chunk and
// its successor row are copied into the row-block-major layout the generated parts read (k_check_relayout), and the ten parts run
// over it unchanged (air_on_rows) with 604 random weights and, in place of the zerofier inverses, the SELECTORS of the four sections
// -- [row == 0], 1, [row != n-1], [row == n-1] (k_check_selectors).  The value of row r is then  sum_k sel_k(r) * w_k * c_k(r): zero
// when every constraint that applies to the row vanishes, non-zero otherwise except with probability 2^-192.  The failing rows are
// counted and the lowest of them listed without atomics -- a count per workgroup, one prefix, a compaction (k_check_count,
// k_check_prefix, k_check_compact) -- so that the report is deterministic.  The host then evaluates all 604 constraints of each listed
// row pair (tvm_host_air_constraints) and reports those that apply and do not vanish.
#include "kernels.h"

namespace tvm {

#define CHECK_MAIN_W ((u64)TVM_NUM_MAIN_COLUMNS)
#define CHECK_AUX_W ((u64)3 * TVM_NUM_AUX_COLUMNS)
#define CHECK_GROUP 256   // rows per workgroup of the count and compaction kernels
#define CHECK_BATCH 1024  // listed rows per round trip of the host evaluation

// Rows first .. first + rows of the column-major traces (row n is row 0) -> rows 0 .. rows of the row-block-major tables the parts read.
// One thread per (row, column), rows fastest: blockIdx.y < 379 a main column (one word), above it an aux column (three words).  The
// reads of a wavefront are 64 consecutive words of a column (main) or 64 x 24 consecutive bytes (aux); the writes fill whole 128-byte
// lines of 16 rows.
__global__ void __launch_bounds__(256) k_check_relayout(const u64* __restrict__ main_trace, const u64* __restrict__ aux_trace, u64 n,
                                                        u64 first, u64 rows, u64* __restrict__ main_rows, u64* __restrict__ aux_rows) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > rows) return;
    u64 src = first + r;
    if (src == n) src = 0;
    const u64 col = blockIdx.y;
    if (col < CHECK_MAIN_W) {
        main_rows[tvm_tab_idx(r, col, CHECK_MAIN_W)] = main_trace[col * n + src];
    } else {
        const u64 a = col - CHECK_MAIN_W;
        const u64* s = aux_trace + 3 * (a * n + src);
        const u64 v0 = s[0], v1 = s[1], v2 = s[2];
        aux_rows[tvm_tab_idx(r, 3 * a, CHECK_AUX_W)] = v0;
        aux_rows[tvm_tab_idx(r, 3 * a + 1, CHECK_AUX_W)] = v1;
        aux_rows[tvm_tab_idx(r, 3 * a + 2, CHECK_AUX_W)] = v2;
    }
}

// the section selectors of the chunk's rows, [4][rows]: initial on row 0, consistency everywhere, transition but on row n-1, terminal
// on row n-1
__global__ void __launch_bounds__(256) k_check_selectors(u64* __restrict__ sel, u64 rows, u64 first, u64 n) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const u64 i = first + r;
    sel[r] = i == 0 ? TVM_ONE : 0;
    sel[rows + r] = TVM_ONE;
    sel[2 * rows + r] = i != n - 1 ? TVM_ONE : 0;
    sel[3 * rows + r] = i == n - 1 ? TVM_ONE : 0;
}

TVM_D u32 check_flag(const u64* vals, u64 rows, u64 r) { return r < rows && (vals[3 * r] | vals[3 * r + 1] | vals[3 * r + 2]) != 0; }

// the failing rows of each workgroup's CHECK_GROUP rows
__global__ void __launch_bounds__(CHECK_GROUP) k_check_count(const u64* __restrict__ vals, u64 rows, u32* __restrict__ counts) {
    __shared__ u32 s[CHECK_GROUP];
    const int tid = threadIdx.x;
    s[tid] = check_flag(vals, rows, (u64)blockIdx.x * CHECK_GROUP + tid);
    __syncthreads();
    for (int k = CHECK_GROUP / 2; k > 0; k >>= 1) {
        if (tid < k) s[tid] += s[tid + k];
        __syncthreads();
    }
    if (tid == 0) counts[blockIdx.x] = s[0];
}

// one workgroup: offsets[g] = failing rows before workgroup g, counted from the start of the trace (*total: those of the earlier
// chunks, advanced by this chunk's)
__global__ void __launch_bounds__(256) k_check_prefix(const u32* __restrict__ counts, u64 n_groups, u64* __restrict__ offsets, u64* total) {
    __shared__ u64 s[256];
    const int tid = threadIdx.x;
    const u64 per = (n_groups + 255) / 256, b = (u64)tid * per, e = b + per < n_groups ? b + per : n_groups;
    u64 sum = 0;
    for (u64 g = b; g < e; g++) sum += counts[g];
    s[tid] = sum;
    __syncthreads();
    for (int k = 1; k < 256; k <<= 1) {   // inclusive scan
        const u64 v = tid >= k ? s[tid - k] : 0;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
    u64 run = *total + s[tid] - sum;
    for (u64 g = b; g < e; g++) {
        offsets[g] = run;
        run += counts[g];
    }
    __syncthreads();   // every thread has read *total
    if (tid == 255) *total += s[255];
}

// the failing rows whose rank (from the start of the trace) is below capacity -> out[rank], ascending
__global__ void __launch_bounds__(CHECK_GROUP) k_check_compact(const u64* __restrict__ vals, u64 rows, u64 first, const u64* __restrict__ offsets,
                                                               u64 capacity, u64* __restrict__ out) {
    __shared__ u32 s[CHECK_GROUP];
    const u64 base = offsets[blockIdx.x];
    if (base >= capacity) return;   // (uniform over the workgroup)
    const int tid = threadIdx.x;
    const u64 r = (u64)blockIdx.x * CHECK_GROUP + tid;
    const u32 flag = check_flag(vals, rows, r);
    s[tid] = flag;
    __syncthreads();
    for (int k = 1; k < CHECK_GROUP; k <<= 1) {   // inclusive scan
        const u32 v = tid >= k ? s[tid - k] : 0;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
    const u64 rank = base + s[tid] - flag;
    if (flag && rank < capacity) out[rank] = first + r;
}

// rows idx[e] of the column-major traces -> out[e] = 379 main words, then 273 aux words
__global__ void __launch_bounds__(256) k_check_gather(const u64* __restrict__ main_trace, const u64* __restrict__ aux_trace, u64 n,
                                                      const u64* __restrict__ idx, u64 k, u64* __restrict__ out) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    constexpr u64 RW = CHECK_MAIN_W + CHECK_AUX_W;
    if (t >= k * RW) return;
    const u64 e = t / RW, v = t % RW, r = idx[e];
    out[t] = v < CHECK_MAIN_W ? main_trace[v * n + r] : aux_trace[((v - CHECK_MAIN_W) / 3 * n + r) * 3 + (v - CHECK_MAIN_W) % 3];
}

}  // namespace tvm

using namespace tvm;

extern "C" int32_t tvm_check_constraints(tvm_ctx* c, const uint64_t* d_main_trace, const uint64_t* d_aux_trace, uint64_t n,
                                         const uint64_t* h_challenges, const uint8_t seed[32], uint64_t capacity, uint64_t* h_failures,
                                         uint64_t* n_failures, uint64_t* failing_rows) {
    if (!c || !d_main_trace || !d_aux_trace || !h_challenges || !n_failures || !failing_rows || (capacity && !h_failures) || !is_pow2(n) || n < 2)
        return set_error(c, TVM_ERR_INVALID_ARGUMENT, "check_constraints arguments");
    *n_failures = 0;
    *failing_rows = 0;
    const u64 R = c->air_check_chunk_rows < n ? c->air_check_chunk_rows : n;
    const u64 groups = (R + CHECK_GROUP - 1) / CHECK_GROUP;
    const u64 listed_cap = capacity < n ? capacity : n;   // rows to list: each listed row is at least one entry
    // the screen's weights: 604 XFE from the caller's seed (never from a proof stream)
    static const uint8_t fixed_seed[32] = {0};
    std::vector<u64> weights(3 * TVM_NUM_QUOTIENT_WEIGHTS);
    tvm_host_stdrng_elements(seed ? seed : fixed_seed, weights.size(), weights.data());
    u64* staged = (u64*)scratch(c, Scratch::AirCheckInputs, (size_t)3 * (TVM_NUM_CHALLENGES + TVM_NUM_QUOTIENT_WEIGHTS) * sizeof(u64));
    u64* sel = (u64*)scratch(c, Scratch::AirCheckSelectors, (size_t)4 * R * sizeof(u64));
    u64* vals = (u64*)scratch(c, Scratch::AirCheckValues, (size_t)3 * R * sizeof(u64));
    u64* offsets = (u64*)scratch(c, Scratch::AirCheckOffsets, (size_t)(groups + 1) * sizeof(u64));   // [groups] offsets, then the running total
    u32* counts = (u32*)scratch(c, Scratch::AirCheckCounts, (size_t)groups * sizeof(u32));
    u64* listed = (u64*)scratch(c, Scratch::AirCheckListed, (size_t)(listed_cap ? listed_cap : 1) * sizeof(u64));
    if (!staged || !sel || !vals || !offsets || !counts || !listed) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "constraint check scratch");
    u64* total = offsets + groups;
    TVM_TRY(h2d_small(c, staged, h_challenges, 3 * TVM_NUM_CHALLENGES * sizeof(u64)));
    TVM_TRY(h2d_small(c, staged + 3 * TVM_NUM_CHALLENGES, weights.data(), weights.size() * sizeof(u64)));
    TVM_HIP_CHECK(c, hipMemsetAsync(total, 0, sizeof(u64), c->stream));
    {
        PoolBlock main_rows(c, (size_t)tvm_tab_words(R + 1, CHECK_MAIN_W) * sizeof(u64));
        PoolBlock aux_rows(c, (size_t)tvm_tab_words(R + 1, CHECK_AUX_W) * sizeof(u64));
        if (!main_rows.p || !aux_rows.p) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "constraint check rows");
        u64* const mr = (u64*)main_rows.p;
        u64* const ar = (u64*)aux_rows.p;
        for (u64 first = 0; first < n; first += R) {
            TVM_LAUNCH(k_check_relayout, dim3((unsigned)((R + 1 + 255) / 256), (unsigned)(TVM_NUM_MAIN_COLUMNS + TVM_NUM_AUX_COLUMNS)), dim3(256), 0,
                       c->stream, d_main_trace, d_aux_trace, n, first, R, mr, ar);
            TVM_LAUNCH(k_check_selectors, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, c->stream, sel, R, first, n);
            TVM_TRY(air_on_rows(c, mr, CHECK_MAIN_W, ar, CHECK_AUX_W, R, sel, staged,
                                staged + 3 * TVM_NUM_CHALLENGES, vals));
            TVM_LAUNCH(k_check_count, dim3((unsigned)groups), dim3(CHECK_GROUP), 0, c->stream, (const u64*)vals, R, counts);
            TVM_LAUNCH(k_check_prefix, dim3(1), dim3(256), 0, c->stream, (const u32*)counts, groups, offsets, total);
            if (listed_cap)
                TVM_LAUNCH(k_check_compact, dim3((unsigned)groups), dim3(CHECK_GROUP), 0, c->stream, (const u64*)vals, R, first,
                           (const u64*)offsets, listed_cap, listed);
            TVM_HIP_CHECK(c, hipGetLastError());
        }
        // (the row tables go back to the pool here, in stream order)
    }
    u64 n_failing = 0;
    TVM_HIP_CHECK(c, hipMemcpyAsync(&n_failing, total, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    TVM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    *failing_rows = n_failing;
    const u64 k = n_failing < listed_cap ? n_failing : listed_cap;
    if (!k) return TVM_OK;
    std::vector<u64> rows(k);
    TVM_HIP_CHECK(c, hipMemcpyAsync(rows.data(), listed, k * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    TVM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    // pinpoint: rows r and r + 1 of each listed row, all 604 constraints on the host, the applicable non-zero ones reported
    constexpr u64 RW = CHECK_MAIN_W + CHECK_AUX_W;
    const u64 batch = k < CHECK_BATCH ? k : CHECK_BATCH;
    u64* d_idx = (u64*)scratch(c, Scratch::AirCheckPairIndices, (size_t)2 * batch * sizeof(u64));
    u64* d_pairs = (u64*)scratch(c, Scratch::AirCheckPairs, (size_t)2 * batch * RW * sizeof(u64));
    if (!d_idx || !d_pairs) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "constraint check rows");
    std::vector<u64> idx(2 * batch), pairs(2 * batch * RW), main_cur(3 * TVM_NUM_MAIN_COLUMNS, 0), main_next(3 * TVM_NUM_MAIN_COLUMNS, 0),
        values(3 * TVM_NUM_QUOTIENT_WEIGHTS);
    u64 written = 0;
    for (u64 b = 0; b < k && written < capacity; b += batch) {
        const u64 m = k - b < batch ? k - b : batch;
        for (u64 e = 0; e < m; e++) idx[2 * e] = rows[b + e], idx[2 * e + 1] = (rows[b + e] + 1) & (n - 1);
        TVM_TRY(h2d_small(c, d_idx, idx.data(), 2 * m * sizeof(u64)));
        TVM_LAUNCH(k_check_gather, dim3((unsigned)((2 * m * RW + 255) / 256)), dim3(256), 0, c->stream, d_main_trace, d_aux_trace, n,
                   (const u64*)d_idx, 2 * m, d_pairs);
        TVM_HIP_CHECK(c, hipGetLastError());
        TVM_HIP_CHECK(c, hipMemcpyAsync(pairs.data(), d_pairs, 2 * m * RW * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        TVM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
        for (u64 e = 0; e < m && written < capacity; e++) {
            const u64 r = rows[b + e];
            const u64* cur = pairs.data() + 2 * e * RW;
            const u64* next = cur + RW;
            for (u64 v = 0; v < CHECK_MAIN_W; v++) main_cur[3 * v] = cur[v], main_next[3 * v] = next[v];   // (base field in XFE)
            TVM_TRY(tvm_host_air_constraints(main_cur.data(), cur + CHECK_MAIN_W, main_next.data(), next + CHECK_MAIN_W, h_challenges,
                                             values.data()));
            // sections by index: initial 0..80 on row 0, consistency 81..177 everywhere, transition 178..580 but on the last row,
            // terminal 581..603 on the last row
            const u64 bounds[4][2] = {{0, 81}, {81, 178}, {178, 581}, {581, 604}};
            const bool applies[4] = {r == 0, true, r != n - 1, r == n - 1};
            u64 found = 0;
            for (int s = 0; s < 4; s++) {
                if (!applies[s]) continue;
                for (u64 i = bounds[s][0]; i < bounds[s][1]; i++) {
                    if (!(values[3 * i] | values[3 * i + 1] | values[3 * i + 2])) continue;
                    found++;
                    if (written < capacity) h_failures[2 * written] = r, h_failures[2 * written + 1] = i, written++;
                }
            }
            if (!found) {
                *n_failures = written;
                return set_error(c, TVM_ERR_DEVICE, "check_constraints: the device screen flags a row on which no constraint fails on the host");
            }
        }
    }
    *n_failures = written;
    return TVM_OK;
}
