"""csrc/field.h, the arithmetic the lazy sums of the LDE butterflies stand on (csrc/ntt_shift.h: canon_plan), through tvm_field_op:
  * bfe_add_folded(a, b) with ONE canonical operand and any 64-bit word as the other: a representative of a + b;
  * bfe_sub(a, b) with a canonical subtrahend and any 64-bit minuend: a representative of a - b, THE canonical word when the
    minuend is canonical;
  * bfe_mul_pow2<S> of any 64-bit word: the canonical word of x 2^S, for every exponent the hook takes (0 .. 191);
  * bfe_canon: the canonical word of any representative.
Expected values are Python integers.  The canonical operand comes from the words around 0, EPS = 2^32 - 1, 2^32, 2^63 and p, the
free one from those and the words at and above p; every pair of the two sets, and random pairs."""
import numpy as np
import pytest

from triton_vm_amd import field

P, EPS = field.P, 0xFFFFFFFF
CANONICAL = [0, 1, EPS - 1, EPS, EPS + 1, 1 << 32, 1 << 63, P - EPS, P - 2, P - 1]
FREE = CANONICAL + [P, P + 1, (1 << 64) - EPS - 1, (1 << 64) - EPS, (1 << 64) - 2, (1 << 64) - 1]
ABOVE = sorted({f for f in FREE if f >= P})   # (2^64 - EPS - 1 is p - 1 and 2^64 - EPS is p: four words at and above p)
assert all(c < P for c in CANONICAL) and all(f < 1 << 64 for f in FREE) and ABOVE == [P, P + 1, (1 << 64) - 2, (1 << 64) - 1]
N_RANDOM = 4096


def pairs(seed):
    """(free operand, canonical operand): every pair of the edge sets, then random 64-bit words against random canonical ones"""
    rng = np.random.default_rng(seed)
    free = np.concatenate([np.repeat(np.array(FREE, np.uint64), len(CANONICAL)), rng.integers(0, 1 << 64, N_RANDOM, dtype=np.uint64)])
    canon = np.concatenate([np.tile(np.array(CANONICAL, np.uint64), len(FREE)), rng.integers(0, P, N_RANDOM, dtype=np.uint64)])
    return free, canon


def run(ctx, op, a, b):
    out, da, db = ctx.alloc(a.size), ctx.to_device(a), ctx.to_device(b)
    ctx._check(ctx.lib.tvm_field_op(ctx.handle, op, da.ptr, db.ptr, out.ptr, a.size), "field_op")
    return [int(v) for v in out.download()]


@pytest.mark.parametrize("canonical_first", [False, True])
def test_folded_add_is_residue_correct_with_one_canonical_operand(ctx, canonical_first):
    free, canon = pairs(5)
    a, b = (canon, free) if canonical_first else (free, canon)
    got = run(ctx, field.OP_ADD_FOLDED, a, b)
    for x, y, r in zip(a, b, got):
        assert 0 <= r < 1 << 64 and r % P == (int(x) + int(y)) % P, (hex(int(x)), hex(int(y)), hex(r))


def test_sub_takes_any_minuend_and_keeps_a_canonical_one_canonical(ctx):
    free, canon = pairs(1)
    got = run(ctx, field.OP_SUB, free, canon)
    for x, y, r in zip(free, canon, got):
        x, y = int(x), int(y)
        assert r % P == (x - y) % P, (hex(x), hex(y), hex(r))
        if x < P:
            assert r == (x - y) % P, (hex(x), hex(y), hex(r))
    assert sum(int(x) < P for x in free) >= len(CANONICAL) ** 2   # (every canonical pair was among them)


def test_mul_pow2_of_any_word_is_canonical(ctx):
    rng = np.random.default_rng(4)
    words = np.concatenate([np.array(ABOVE, np.uint64), rng.integers(P, 1 << 64, 12, dtype=np.uint64)])
    assert (words >= np.uint64(P)).all()
    a = np.tile(words, 192)
    s = np.repeat(np.arange(192, dtype=np.uint64), words.size)
    got = run(ctx, field.OP_MUL_POW2, a, s)
    for x, e, r in zip(a, s, got):
        assert r == int(x) * pow(2, int(e), P) % P, (hex(int(x)), int(e), hex(r))


def test_canon(ctx):
    rng = np.random.default_rng(6)
    a = np.concatenate([np.array(FREE, np.uint64), rng.integers(0, 1 << 64, 1024, dtype=np.uint64), rng.integers(P, 1 << 64, 1024, dtype=np.uint64)])
    got = run(ctx, field.OP_CANON, a, a)
    assert got == [int(x) % P for x in a]
