"""Host-side scalar helpers over F_p (python ints).  Plumbing for building domains and arguments;
no table or codeword ever goes through here."""
P = 2**64 - 2**32 + 1
R = 2**64 % P
R_INV = pow(R, -1, P)
ONE = R  # Montgomery word of 1


def to_mont(v):
    return v % P * R % P


def from_mont(raw):
    return raw * R_INV % P


def mont_mul(a, b):
    return a * b % P * R_INV % P


def mont_pow(a, e):
    return to_mont(pow(from_mont(a), e, P))


def mont_inv(a):
    return to_mont(pow(from_mont(a), -1, P))


def generator():
    """[twenty-first, not in the reference tree] BFieldElement::generator() = 7."""
    return to_mont(7)


def primitive_root_of_unity(order):
    """[twenty-first, not in the reference tree] the 2^32-th root 7^((p-1)/2^32) squared down to `order`."""
    assert order and order & (order - 1) == 0 and order <= 2**32
    return to_mont(pow(7, (P - 1) // order, P))


# ---- tvm_field_op: the op codes of the device-arithmetic hook (csrc/capi.hip: k_field_op, k_pow2_points, k_pow2_points_lazy) ----
OP_ADD, OP_SUB, OP_MUL, OP_POW7, OP_MUL_POW2, OP_ADD_FOLDED, OP_CANON = range(7)
LAZY_SHIFTS = (39, 78, 117)   # the shifted 16-point forms k_lde_pass2_fused instantiates (csrc/ntt_shift.h)


def pow2_points_op(K, dit, inverse):
    """the 2^K-point transform with shift twiddles, every word canonical (K = 1 .. 4)"""
    assert 1 <= K <= 4
    return 32 + 4 * K + 2 * int(bool(dit)) + int(bool(inverse))


def lazy_pow2_points_op(K, dit, inverse, owed_all, shift=0):
    """the lazy form of the same transform (csrc/ntt_shift.h: canon_plan): outputs owed canonical all (`owed_all`) or none, the
    inputs the plan needs canonical declared so -- lazy_pow2_points_plan(...)['need_in'] -- and the others free.  `shift`: one of
    LAZY_SHIFTS, the 16-point decimation-in-time forward transform at the points 2^shift w^j."""
    if shift:
        assert (K, bool(dit), bool(inverse)) == (4, True, False) and shift in LAZY_SHIFTS
        return 112 + 2 * LAZY_SHIFTS.index(shift) + int(bool(owed_all))
    assert 2 <= K <= 4
    return 64 + 2 * (4 * K + 2 * int(bool(dit)) + int(bool(inverse))) + int(bool(owed_all))


def pow2_twiddle_log(K, inverse, T, M, shift=0):
    """log2 of the twiddle of the butterflies with index M in layer T (csrc/ntt_shift.h)"""
    root = ((36 if inverse else 156) << (4 - K)) % 192
    return ((root * M + shift % 192 + 192) * (((1 << K) // 2) >> T)) % 192


def lazy_pow2_points_plan(K, dit, inverse, shift, in_canon, owed):
    """csrc/ntt_shift.h: canon_plan, restated: which sums of the 2^K-point transform are folded when the outputs in the mask `owed`
    must be canonical, which inputs that needs canonical, and -- from the inputs `in_canon` -- which outputs come out canonical."""
    R = 1 << K
    layers = list(range(K)) if dit else list(range(K - 1, -1, -1))
    flies = [(T, q * 2 << T | M, 1 << T, pow2_twiddle_log(K, inverse, T, M, shift)) for T in layers for M in range(1 << T) for q in range(R >> (T + 1))]
    need, fold = owed & ((1 << R) - 1), [0] * 4
    for T, e, h, E in reversed(flies):
        tw, neg = E % 96 != 0, E >= 96
        n_lo, n_hi = need >> e & 1, need >> (e + h) & 1
        if dit:
            n_sum, n_diff = (n_hi, n_lo) if neg else (n_lo, n_hi)
            folded, need_u, need_v = not n_sum, n_sum or n_diff, not tw
        else:
            need_min = n_lo or (not tw and n_hi)
            folded, need_u, need_v = not n_lo, (True if neg else need_min), (need_min if neg else True)
        if folded:
            fold[T] |= 1 << e
        need = need & ~(1 << e | 1 << (e + h)) | int(bool(need_u)) << e | int(bool(need_v)) << (e + h)
    c, ok = in_canon & ((1 << R) - 1), True
    for T, e, h, E in flies:
        tw, neg, folded = E % 96 != 0, E >= 96, fold[T] >> e & 1
        cu, ch = c >> e & 1, c >> (e + h) & 1
        if dit:
            cv = tw or ch
            ok = ok and bool(cv) and bool((cu or cv) if folded else (cu and cv))
            c_sum, c_diff = not folded, cu
            c_lo, c_hi = (c_diff, c_sum) if neg else (c_sum, c_diff)
        else:
            ok = ok and bool(cu if neg else ch) and bool((cu or ch) if folded else (cu and ch))
            c_lo, c_hi = not folded, tw or (ch if neg else cu)
        c = c & ~(1 << e | 1 << (e + h)) | int(bool(c_lo)) << e | int(bool(c_hi)) << (e + h)
    ok = ok and not (owed & ((1 << R) - 1) & ~c)
    return dict(fold=fold, need_in=need, out_canon=c, folded=sum(bin(f).count("1") for f in fold), ok=ok)
