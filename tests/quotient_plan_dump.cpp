// quotient_plan_dump -- prints the plan of csrc/quotient_plan.h for every shape tests/test_quotient_plan.py asks about.  In, one shape
// per line:   log_n h expansion remainder_option remainder_min_rows forked with_class_0
// (tables extended onto the quotient domain of expansion * N points: n1 = 2^(log_n / 2) rounded down, pitch = (n2 + 1) n1, X = expansion;
// valid-trace mode on).  Out, one line per shape:
//   <route> <n_coeffs> <class cosets: half quarter three> | <step> | <step> ...     with <step> = class_mask stride n_cosets cosets t_coset
// (cosets: comma-separated, "-" for a sub-domain step).  Includes nothing of the project but that header and the public one it names.
#include <cstdio>

#include "quotient_plan.h"

int main() {
    long log_n, h, expansion, option, min_rows, forked, with_class_0;
    while (std::scanf("%ld %ld %ld %ld %ld %ld %ld", &log_n, &h, &expansion, &option, &min_rows, &forked, &with_class_0) == 7) {
        const std::uint64_t N = 1ull << log_n, n1 = 1ull << (log_n / 2), n2 = N / n1, Q = N * (std::uint64_t)expansion;
        const tvm::QuotientShape shape = {N, Q, N + (std::uint64_t)h, n1, n2, (n2 + 1) * n1, (std::uint64_t)expansion, Q,
                                          true, forked != 0, option != 0, (std::uint64_t)min_rows};
        const tvm::QuotientPlan plan = tvm::quotient_plan(shape, with_class_0 != 0);
        std::uint32_t cosets[4];
        tvm::air_class_cosets(shape.m, N, cosets);
        const char* route = plan.route == tvm::QuotientRoute::row_by_row ? "row_by_row"
                            : plan.route == tvm::QuotientRoute::whole_cosets ? "whole_cosets" : "remainder_coset";
        std::printf("%s %llu %u %u %u", route, (unsigned long long)plan.n_coeffs, cosets[1], cosets[2], cosets[3]);
        for (int s = 0; s < plan.n_steps; s++) {
            const tvm::QuotientStep& step = plan.steps[s];
            std::printf(" | %u %u %u ", step.class_mask, step.stride, step.n_cosets);
            if (step.stride) std::printf("-");
            else for (std::uint32_t j = 0; j < step.n_cosets; j++) std::printf(j ? ",%u" : "%u", step.cosets[j]);
            std::printf(" %u", step.t_coset);
        }
        std::printf("\n");
    }
    return 0;
}
