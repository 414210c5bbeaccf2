// tail_kernels.h -- what proof_tail.hip (the tail of a FRI proof) and stir_rounds.hip (the rounds of a STIR proof) share: the steps of
// the one-wavefront Fiat-Shamir sponge, the workgroup prefix sum, and the descriptors of the authentication-structure and gather
// kernels, which proof_tail.hip defines and launches for both (authentication_structures_launch, tail_gather_launch).
#pragma once
#include <algorithm>

#include "context.h"
#include "tip5.h"

namespace tvm {

// ---------------------------------------------------------------------------------------------- the sponge, one wavefront
// Lanes 0..15 hold the sponge state (x of lane `pos`), the other lanes follow along so that every lane joins the rotations of
// tip5_permute_lanes.  Every lane of the wavefront calls these with the same arguments.
//
// ProofStream::enqueue of an item in the Fiat-Shamir heuristic (proof_stream.rs:40-59): the item's encoding -- n_prefix <= 4 words
// p0.. (by selection, not from an indexed array: no scratch), then n_body words of a device array -- is padded with 1, 0, ... to
// whole blocks of the rate and absorbed in overwrite mode: total / 10 + 1 blocks, the last one holds the padding.
TVM_D u64 sponge_absorb_lanes(u64 x, int pos, int lane, const unsigned char* lut, u64 p0, u64 p1, u64 p2, u64 p3, u64 n_prefix, const u64* body,
                              u64 n_body) {
    const u64 total = n_prefix + n_body;
    for (u64 b = 0; b * TIP5_RATE <= total; b++) {
        if (pos < TIP5_RATE) {
            const u64 wi = b * TIP5_RATE + (u64)pos;
            if (wi < n_prefix) x = wi == 0 ? p0 : wi == 1 ? p1 : wi == 2 ? p2 : p3;
            else if (wi < total) x = body[wi - n_prefix];
            else x = wi == total ? TVM_ONE : 0;
        }
        x = tip5_permute_lanes(x, pos, lane, lut);
    }
    return x;
}
// ProofItem::Polynomial over n_coefficients XFE at w: a Polynomial drops its trailing zero coefficients (one past the highest
// non-zero one, over the wavefront), and its encoding (BFieldCodec: triton_host.cpp, encode_item) is
//     [discriminant, 2 + 3n, 1 + 3n, n, the 3n words]
TVM_D u64 sponge_absorb_polynomial_lanes(u64 x, int pos, int lane, const unsigned char* lut, u32 discriminant, const u64* w, u32 n_coefficients) {
    u32 n = 0;
    for (u32 e = (u32)lane; e < n_coefficients; e += 64)
        if (w[3 * (u64)e] | w[3 * (u64)e + 1] | w[3 * (u64)e + 2]) n = e + 1;
    for (int m = 32; m; m >>= 1) {
        const u32 other = (u32)__shfl_xor((u64)n, m, 64);
        n = other > n ? other : n;
    }
    const u64 total = 4 + 3 * (u64)n;
    return sponge_absorb_lanes(x, pos, lane, lut, bfe_from_u64(discriminant), bfe_from_u64(total - 2), bfe_from_u64(total - 3), bfe_from_u64(n), 4, w,
                               3 * (u64)n);
}
// Tip5::sample_indices: squeeze, skip p - 1, reduce below mask + 1 (a power of two); the squeezed elements left over when n is reached
// are dropped.  rate: TIP5_RATE words of LDS.
TVM_D u64 sponge_sample_indices_lanes(u64 x, int pos, int lane, const unsigned char* lut, u64* rate, u32 n, u64 mask, u64* indices) {
    u32 count = 0;
    while (count < n) {
        if (lane < TIP5_RATE) rate[lane] = x;
        __syncthreads();
        for (int k = 0; k < TIP5_RATE && count < n; k++) {
            const u64 v = bfe_mul(rate[k], 1);   // the canonical value of a Montgomery word
            if (v == TVM_P - 1) continue;
            if (lane == 0) indices[count] = v & mask;
            count++;
        }
        __syncthreads();   // (the rate words are read before the next squeeze overwrites them)
        x = tip5_permute_lanes(x, pos, lane, lut);
    }
    return x;
}
// ProofStream::sample_scalars(n) (proof_stream.rs:81-84): ceil(3 n / 10) squeezes, the first 3 n squeezed words are the scalars
TVM_D u64 sponge_sample_scalars_lanes(u64 x, int pos, int lane, const unsigned char* lut, u32 n, u64* scalars) {
    for (u32 s = 0; s < (3 * n + TIP5_RATE - 1) / TIP5_RATE; s++) {
        if (lane < TIP5_RATE && s * TIP5_RATE + (u32)lane < 3 * n) scalars[s * TIP5_RATE + (u32)lane] = x;
        x = tip5_permute_lanes(x, pos, lane, lut);
    }
    return x;
}

// ---------------------------------------------------------------------------------------------- a workgroup prefix sum
// inclusive prefix sum of v over the workgroup and the sum over all of it; the caller puts a barrier before the next call
TVM_D u32 as_block_scan(u32 v, u32* wave_sums, u32& total) {
    const int lane = (int)(threadIdx.x & 63);
    const u32 wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const u32 below = (u32)__shfl((u64)v, lane - d, 64);
        if (lane >= d) v += below;
    }
    if (lane == 63) wave_sums[wave] = v;
    __syncthreads();
    u32 before = 0;
    total = 0;
    for (u32 w = 0; w < n_waves; w++) {
        const u32 s = wave_sums[w];
        total += s;
        if (w < wave) before += s;
    }
    return v + before;
}

// ---------------------------------------------------------------------------------------------- k_authentication_structures
struct AuthJob {
    const u64* idx;     // [n_idx] on the device
    u64 n_leaves, add;  // leaf i of the job = (idx[i] + add) & (n_leaves - 1): the a indices of a round, or its b indices (add = n/2)
    u64* out_idx;       // heap indices out
    const u64* nodes;   // null, or the tree [2 n_leaves][5]: out_nodes receives the digests at out_idx
    u64* out_nodes;
    u64 n_idx;
    const u64* n_idx_device;   // not null: the number of indices is this word of device memory (at most n_idx: a list whose length
                               // only the device knows, STIR's indices without repeats)
};
// ---------------------------------------------------------------------------------------------- k_tail_gather
struct TailSegment {
    const u64* src;   // leaves: the round's codeword [n][3]; nodes: the tree [2 n][5]; rows: the table's storage
    u64 mask, add;    // leaves: element (a[i] + add) & mask
    u32 kind;         // 0: leaves at the a / b indices, 1: authentication nodes of list `which`, 2: rows of table `which` at the a indices
    u32 which;
    // leaves of a segment with an index list of its own (STIR's stacked leaves): `stack` elements per index, `stride` elements apart,
    // at the *count indices idx[]; all null / zero: one element at each of the n_checks indices a[]
    const u64 *idx, *count;
    u64 stride;
    u32 stack;
};
struct TailGatherArgs {
    const TailSegment* segments;
    const u64 *a, *auth_idx, *auth_counts;   // [n_checks]; [n_lists][auth_stride]; [n_lists]
    u64 n_checks, auth_stride;
    TabLayout layout[3];                     // the three tables
    u64 row_stride[3];                       // rows of a table per row of its LDT-domain view
    u32 W[3];
    u64 *out, *directory;                    // packed payloads; [segments][2] = (offset, words)
};
// words of an authentication structure's index list: no more than one sibling per level and path
inline u64 auth_capacity(u64 n_leaves, u64 n_idx) { return std::min(n_idx, n_leaves) * (u64)ilog2(n_leaves); }
// proof_tail.hip: one workgroup per job (most_indices: the largest n_idx of the jobs, at most TVM_TAIL_MAX_INDICES); d_counts [n_jobs]
int authentication_structures_launch(tvm_ctx* c, const AuthJob* d_jobs, u32 n_jobs, u64 most_indices, u64* d_counts);
int tail_gather_launch(tvm_ctx* c, const TailGatherArgs& g, u32 n_segments);

}  // namespace tvm
