"""csrc/ntt_mfma.h: the 16-point transform with power-of-two twiddles on the matrix cores, through tvm_dft16_selfcheck -- word for word
against the shift form of csrc/ntt_shift.h (ntt_pow2_points<4, true, .>) and against the oracle's 16-point transform for the canonical
output, after reduction mod p for the folded output.  The inputs drive what the construction adds: the signed-byte offset and its
bias (the bytes 0x00, 0x7f, 0x80, 0xff in every byte position), the wrap signs of every column of the matrix (a single non-zero
point in each position), the extremes of the digit sums (all 0, all p - 1) and words that are no canonical representatives.
A host-only case rebuilds the 16 x 16 matrix from the generator's operands (tests/dft16_table_dump.cpp) and compares it with the
powers of the oracle's 16th root of unity.  Runs on the CPU fiber emulation of the same sources (-m "not gpu") and on the MI355X."""
import functools
import os
import subprocess

import numpy as np
import pytest

from triton_vm_amd import field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = field.P
MFMA, FOLDED = 2, 4   # include/triton_hip.h: the form bits of tvm_dft16_selfcheck (bit 0: inverse)
BREV = [int(format(i, "04b")[::-1], 2) for i in range(16)]
BYTES = (0x00, 0x7F, 0x80, 0xFF)


def special_groups():
    """64 groups of 16 words: the cases the module's docstring lists"""
    rng = np.random.default_rng(16)
    groups = [[0] * 16, [P - 1] * 16, [(1 << 64) - 1] * 16, [P + 1] * 16]
    for v in BYTES:                                          # one byte position at a time ...
        groups += [[v << (8 * b)] * 16 for b in range(8)]
    groups += [[int.from_bytes(bytes([v] * 8), "little")] * 16 for v in BYTES]   # ... and all together
    byte_words = [v << (8 * b) for v in BYTES for b in range(8)] + [int.from_bytes(bytes([v] * 8), "little") for v in BYTES]
    groups += [[byte_words[i] for i in rng.integers(0, len(byte_words), 16)] for _ in range(8)]
    for k in range(16):                                      # one column of the matrix each (every byte of the word non-zero)
        groups.append([0x0123456789ABCDEF if e == k else 0 for e in range(16)])
    assert len(groups) == 64
    return np.array(groups, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def inputs(n_groups):
    rng = np.random.default_rng(n_groups)
    a = rng.integers(0, P, size=(n_groups, 16), dtype=np.uint64)   # random canonical words
    a[:64] = special_groups()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def expected(n_groups, inverse):
    """the transform of every group in plain integer arithmetic (linear: Montgomery words stay Montgomery words), bit-reversed in,
    natural out, for any 64-bit input words"""
    w = pow(1753635133440165772, (1 << 32) >> 4, P)          # twenty-first: BFieldElement::primitive_root_of_unity(16)
    assert w == pow(2, 156, P)
    if inverse:
        w = pow(w, P - 2, P)
    m = [[pow(w, j * k, P) for k in range(16)] for j in range(16)]
    out = np.zeros((n_groups, 16), np.uint64)
    for g, x in enumerate(inputs(n_groups)):
        nat = [int(x[BREV[k]]) for k in range(16)]
        out[g] = [sum(mjk * xk for mjk, xk in zip(m[j], nat)) % P for j in range(16)]
    out.setflags(write=False)
    return out


def run(ctx, form, a):
    out, da = ctx.alloc(a.size), ctx.to_device(np.ascontiguousarray(a).reshape(-1))
    ctx._check(ctx.lib.tvm_dft16_selfcheck(ctx.handle, form, da.ptr, out.ptr, a.shape[0]), "dft16_selfcheck")
    return out.download().reshape(a.shape)


# 64: one wavefront's four sets; 576: several wavefronts and workgroups; 581: the same with a ragged tail
@pytest.mark.parametrize("n_groups", [64, 64 * 9, 64 * 9 + 5])
@pytest.mark.parametrize("inverse", [0, 1])
def test_matrix_core_form_against_shift_form_and_oracle(ctx, orc, n_groups, inverse):
    a = inputs(n_groups)
    want = expected(n_groups, inverse)
    canonical_in = (a < np.uint64(P)).all(axis=1)
    assert not canonical_in.all() and canonical_in.sum() >= n_groups - 16
    got = run(ctx, MFMA | inverse, a)
    assert (got < np.uint64(P)).all(), "a word of the canonical form is not canonical"
    assert (got == want).all()
    # the shift form takes canonical words only
    shift = run(ctx, inverse, a[canonical_in])
    assert (got[canonical_in] == shift).all()
    folded = run(ctx, MFMA | FOLDED | inverse, a)
    assert (folded % np.uint64(P) == want).all()
    # the oracle's own transform (natural order in and out; its inverse scales by 1/16) on the canonical groups
    for g in np.flatnonzero(canonical_in)[:: max(1, n_groups // 64)]:
        nat = a[g][BREV]
        if inverse:
            ref = orc.intt(np.array([int(v) * 16 % P for v in nat], np.uint64))
        else:
            ref = orc.ntt(nat)
        assert (got[g] == ref).all(), g


def test_entry_rejects_what_it_does_not_have(ctx):
    a = inputs(64)
    out, da = ctx.alloc(a.size), ctx.to_device(np.ascontiguousarray(a).reshape(-1))
    for form in (-1, 8, FOLDED, FOLDED | 1):   # folded words exist on the matrix cores only
        assert ctx.lib.tvm_dft16_selfcheck(ctx.handle, form, da.ptr, out.ptr, 64) != 0
    ctx._check(ctx.lib.tvm_dft16_selfcheck(ctx.handle, MFMA, da.ptr, out.ptr, 0), "no groups: nothing to do")


@pytest.fixture(scope="module")
def table_dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dft16") / "dft16_table_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "triton_vm_amd", "csrc"),
                           os.path.join(ROOT, "tests", "dft16_table_dump.cpp"), "-o", exe])
    return lambda root: [line.split() for line in subprocess.check_output([exe, str(root)], text=True).splitlines()]


@pytest.mark.parametrize("inverse", [0, 1])
def test_generated_operands_are_the_powers_of_the_root(table_dump, orc, inverse):
    """no GPU, no emulator: every non-zero byte of the 24 operands says `entry * 2^(8 digit)` for byte b of a point, which must be
    w^(jk) 2^(8b); the accumulator inputs undo the lowering of the bytes by 128 and carry biases that vanish mod p"""
    lines = table_dump(36 if inverse else 156)
    in_point = {int(e): int(i) for tag, e, i, _ in (l for l in lines if l[0] == "layout")}
    out_point = {int(e): int(o) for tag, e, _, o in (l for l in lines if l[0] == "layout")}
    assert in_point == {e: BREV[e] for e in range(16)} and out_point == {e: e for e in range(16)}
    powers = [int(v) for v in orc.from_mont(orc.domain_values(orc.domain_of_length(16)))]   # w^0 .. w^15
    assert powers[1] == pow(2, 156, P)
    if inverse:
        powers = [powers[0]] + powers[:0:-1]
    seen, row_sum = {}, {}
    for _, d, h, i, g, t, bb, entry in (l for l in lines if l[0] == "a"):
        d, h, i, g, t, bb, entry = int(d), int(h), int(i), int(g), int(t), int(bb), int(entry)
        j, k, b = out_point[i], in_point[4 * g + t], bb + 4 * h
        assert (j, k, b) not in seen, "a byte of a point meets one digit position per output"
        seen[j, k, b] = entry * pow(2, 8 * d, P) % P
        row_sum[d, i] = row_sum.get((d, i), 0) + entry
    assert len(seen) == 16 * 16 * 8
    for (j, k, b), got in seen.items():
        assert got == powers[j * k % 16] * pow(2, 8 * b, P) % P, (j, k, b)
    bias = {int(d): int(v) for _, d, v in (l for l in lines if l[0] == "bias")}
    assert len(bias) == 12 and all(1 << 16 <= v <= (1 << 16) + 256 for v in bias.values())
    assert sum(v << (8 * d) for d, v in bias.items()) % P == 0
    c = {(int(d), int(i)): int(v) for _, d, i, v in (l for l in lines if l[0] == "c")}
    assert len(c) == 12 * 16
    for (d, i), v in c.items():
        assert v == 128 * row_sum.get((d, i), 0) + bias[d]
        assert abs(row_sum.get((d, i), 0)) <= 16 * 16
