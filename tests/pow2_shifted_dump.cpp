// pow2_shifted_dump.cpp -- host-only check of csrc/ntt_shift.h's transforms at shifted points (tests/test_pow2_shifted.py): for every
// shift exponent k_lde_pass2_fused instantiates, ntt_pow2_points_shifted<4, S> must equal the plain transform of the inputs multiplied
// by 2^(S a), a = brev4(e) the coefficient index at element e -- which is what the kernel's coset scale asks for (ntt.hip).
// Built by g++ with -DTVM_EMU (platform.h then needs no HIP headers); plain C++, so -fsanitize=undefined applies.
// Prints one line per shift, "shift S cases N mismatches M", and exits non-zero on a mismatch.
#include <cstdint>
#include <cstdio>

#include "ntt_shift.h"

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 next_word() {   // splitmix64, reduced below p
    u64 z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z >= TVM_P ? z - TVM_P : z;
}

template <int S>
static int check_case(const u64 (&in)[16]) {
    const u64 z = bfe_pow(bfe_from_u64(2), (u64)S);
    u64 shifted[16], plain[16];
    for (int e = 0; e < 16; e++) {
        shifted[e] = in[e];
        plain[e] = bfe_mul(in[e], bfe_pow(z, (u64)tvm::brev_k(e, 4)));
    }
    tvm::ntt_pow2_points_shifted<4, S>(shifted);
    tvm::ntt_pow2_points<4, true, false>(plain);
    int bad = 0;
    for (int e = 0; e < 16; e++) bad += shifted[e] != plain[e] || shifted[e] >= TVM_P;
    return bad;
}

template <int S>
static int check_shift() {
    // words (Montgomery representatives, any canonical word is one) at the edges of the carry chains
    const u64 edges[] = {0, 1, TVM_P - 1, 0xFFFFFFFFull, 0x100000000ull, TVM_P - 0x100000000ull};
    const int n_edges = (int)(sizeof(edges) / sizeof(edges[0]));
    int cases = 0, bad = 0;
    u64 in[16];
    for (int v = 0; v < n_edges; v++) {
        for (int e = 0; e < 16; e++) in[e] = edges[v];   // the edge word in every position at once
        bad += check_case<S>(in), cases++;
        for (int pos = 0; pos < 16; pos++) {   // ... in one position, zeros / random words elsewhere
            for (int e = 0; e < 16; e++) in[e] = 0;
            in[pos] = edges[v];
            bad += check_case<S>(in), cases++;
            for (int e = 0; e < 16; e++) in[e] = e == pos ? edges[v] : next_word();
            bad += check_case<S>(in), cases++;
        }
    }
    for (int r = 0; r < 2000; r++) {
        for (int e = 0; e < 16; e++) in[e] = next_word();
        bad += check_case<S>(in), cases++;
    }
    std::printf("shift %d cases %d mismatches %d\n", S, cases, bad);
    return bad;
}

int main() {
    // k_lde_pass2_fused: 2^(39 kappa), kappa < 4 (expansion >= 4) and 2^(78 kappa), kappa < 2 (expansion 2)
    int bad = check_shift<0>() + check_shift<39>() + check_shift<78>() + check_shift<117>();
    // (beyond what the kernel takes: the sign at 96 and the wrap at 192)
    bad += check_shift<96>() + check_shift<156>() + check_shift<191>() + check_shift<192 + 39>();
    return bad ? 1 : 0;
}
