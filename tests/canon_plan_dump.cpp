// canon_plan_dump -- prints the canonicality plan of csrc/ntt_shift.h (canon_plan) for the forms tests/test_canonicality_plan.py asks
// about, one line per form read from standard input:
//   in:  K dit inverse shift in_canon owed          (masks in hexadecimal)
//   out: K dit inverse shift in_canon owed | fold[0] fold[1] fold[2] fold[3] | need_in out_canon folded ok
// Host only: built by g++ with -DTVM_EMU (platform.h then needs no HIP headers), ntt_shift.h and what it includes.
#include <cstdio>

#include "ntt_shift.h"

// (the plan is a constant expression: the forms the kernels instantiate are checked by the compiler as well)
static_assert(tvm::canon_plan(4, true, false, 0, 0xFFFFu, 0).ok && tvm::canon_plan(4, true, false, 0, 0xFFFEu, 0).ok, "pass 3, first and middle group");
static_assert(!tvm::canon_plan(4, true, false, 0, 0xFFFEu, 0xFFFFu).ok, "a last group cannot take a free x[0]");

int main() {
    int K, dit, inverse, shift;
    unsigned in_canon, owed;
    while (std::scanf("%d %d %d %d %x %x", &K, &dit, &inverse, &shift, &in_canon, &owed) == 6) {
        if (K < 1 || K > 4) return 2;
        const tvm::CanonPlan p = tvm::canon_plan(K, dit != 0, inverse != 0, shift, in_canon, owed);
        std::printf("%d %d %d %d %x %x | %x %x %x %x | %x %x %d %d\n", K, dit, inverse, shift, in_canon, owed, p.fold[0], p.fold[1], p.fold[2],
                    p.fold[3], p.need_in, p.out_canon, p.folded, p.ok ? 1 : 0);
    }
    return 0;
}
