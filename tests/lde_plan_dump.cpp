// lde_plan_dump -- prints the plan of csrc/lde_plan.h for every shape tests/test_lde_plan.py asks about, one line per shape:
//   log_n X h std_roots tiles_option mode | <pass 1> | <pass 2> | <pass 3>     with <pass> = kernel block lds_bytes rows tiles grid_y
// (h = -1 on input: n1, the most randomizers the fused kernel takes; -2: n1 + 1).  Includes nothing of the project but that header.
#include <cstdio>

#include "lde_plan.h"

using tvm::LdeKernel;

static const char* name(LdeKernel k) {
    switch (k) {
    case LdeKernel::none: return "-";
    case LdeKernel::ntt2_pass1: return "k_ntt2_pass1";
    case LdeKernel::ntt2_pass2: return "k_ntt2_pass2";
    case LdeKernel::lde_pass2: return "k_lde_pass2";
    case LdeKernel::lde_pass3: return "k_lde_pass3";
    case LdeKernel::pass1_rows_8_16: return "k_lde_pass1_rows<8,16>";
    case LdeKernel::pass1_rows_9_16: return "k_lde_pass1_rows<9,16>";
    case LdeKernel::pass1_rows_10_16: return "k_lde_pass1_rows<10,16>";
    case LdeKernel::pass1_rows_11_8: return "k_lde_pass1_rows<11,8>";
    case LdeKernel::pass2_fused_8: return "k_lde_pass2_fused<8>";
    case LdeKernel::pass2_fused_9: return "k_lde_pass2_fused<9>";
    case LdeKernel::pass2_fused_10: return "k_lde_pass2_fused<10>";
    case LdeKernel::pass2_fused_11: return "k_lde_pass2_fused<11>";
    case LdeKernel::pass2_v3_7_6: return "k_lde_pass2_v3<7,6>";
    case LdeKernel::pass2_v3_8_6: return "k_lde_pass2_v3<8,6>";
    case LdeKernel::pass2_v3_11_10: return "k_lde_pass2_v3<11,10>";
    case LdeKernel::pass2_v3_12_10: return "k_lde_pass2_v3<12,10>";
    case LdeKernel::pass3_rows_8_8: return "k_lde_pass3_rows<8,8>";
    case LdeKernel::pass3_rows_9_8: return "k_lde_pass3_rows<9,8>";
    case LdeKernel::pass3_rows_10_8: return "k_lde_pass3_rows<10,8>";
    case LdeKernel::pass3_rows_11_8: return "k_lde_pass3_rows<11,8>";
    case LdeKernel::pass3_halves_8: return "k_lde_pass3_halves<8>";
    case LdeKernel::pass3_v3_7_6: return "k_lde_pass3_v3<7,6>";
    case LdeKernel::pass3_v3_8_6: return "k_lde_pass3_v3<8,6>";
    case LdeKernel::pass3_v3_12_10: return "k_lde_pass3_v3<12,10>";
    case LdeKernel::count: break;
    }
    return "?";
}

static void print_pass(const tvm::LdePass& p) {
    std::printf(" | %s %d %zu %d %d %llu", name(p.kernel), p.block, p.lds_bytes, p.rows, p.tiles, (unsigned long long)p.grid_y);
}

int main() {
    long log_n, X, h, std_roots, tiles_option, mode;
    while (std::scanf("%ld %ld %ld %ld %ld %ld", &log_n, &X, &h, &std_roots, &tiles_option, &mode) == 6) {
        const long n1 = 1l << (log_n / 2);
        if (h < 0) h = h == -1 ? n1 : n1 + 1;
        const tvm::LdePlan plan = tvm::lde_plan({(int)log_n, (std::uint64_t)X, (std::uint64_t)h, std_roots != 0, (int)tiles_option, (int)mode});
        std::printf("%ld %ld %ld %ld %ld %ld", log_n, X, h, std_roots, tiles_option, mode);
        print_pass(plan.pass1);
        print_pass(plan.pass2);
        print_pass(plan.pass3);
        std::printf("\n");
    }
    return 0;
}
