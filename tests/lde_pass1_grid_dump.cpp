// lde_pass1_grid_dump -- walks the work items of pass 1's persistent row kernels the way the kernel does (csrc/lde_plan.h:
// lde_pass1_workgroups, lde_pass1_items, lde_pass1_item), for every launch tests/test_lde_pass1_plan.py asks about.  One line in:
//   log_n columns option
// one line out:  kernel G items | <workgroup 0's walk> | <workgroup 1's walk> ...   with a walk = column:tile column:tile ...
// Includes nothing of the project but that header.
#include <cstdio>

#include "lde_plan.h"

int main() {
    long log_n, columns, option;
    while (std::scanf("%ld %ld %ld", &log_n, &columns, &option) == 3) {
        const tvm::LdePlan plan = tvm::lde_plan({(int)log_n, 1, 1, true, 0, 0});
        const tvm::LdePass& p = plan.pass1;
        if (!tvm::is_pass1_persistent(p.kernel)) {
            std::printf("- 0 0\n");
            continue;
        }
        const int log_n2 = (int)log_n - (int)log_n / 2, log_tiles = log_n2 - 4;   // 16-row tiles of the n2 rows of pass 1
        const std::uint64_t items = tvm::lde_pass1_items((std::uint64_t)columns, log_tiles);
        const std::uint64_t G = tvm::lde_pass1_workgroups(items, (std::uint64_t)option);
        std::printf("%d %llu %llu", (int)p.kernel - (int)tvm::LdeKernel::pass1_rows_8_16 + 8, (unsigned long long)G, (unsigned long long)items);
        for (std::uint64_t g = 0; g < G; g++) {
            std::printf(" |");
            for (std::uint64_t index = g; index < items; index += G) {   // the kernel's loop
                const tvm::LdePass1Item item = tvm::lde_pass1_item(index, log_tiles);
                std::printf(" %llu:%llu", (unsigned long long)item.column, (unsigned long long)item.tile);
            }
        }
        std::printf("\n");
    }
    return 0;
}
