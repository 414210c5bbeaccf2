"""The combination codeword from its coefficients (csrc/capi.hip: tvm_evaluate_extended).  A polynomial of n_coeffs coefficients, n the
largest power of two in n_coeffs, is lo + X^n hi = (lo + hi) + (X^n - 1) hi: one relayout pass (lde_coefficient_form), the forward
half of the table extension into a scratch table of one column, one pass that writes the values in domain order (csrc/poly.hip:
table_rows).  The route must give tvm_evaluate's words, refuse outside its gate without writing, and leave a proof unchanged;
TVM_OPTION_COMBINATION_FROM_COEFFICIENTS = 0 makes it refuse everything."""
import os

import numpy as np
import pytest

from triton_vm_amd import ArithmeticDomain, field

NOT_APPLICABLE = 5   # TVM_NOT_APPLICABLE
PATTERN = np.uint64(0x5A5A_0123_4567_89AB)
# (log2 n, L / n) -> what runs the forward half (csrc/lde_plan.h)
SHAPES = {(10, 2): "generic", (10, 4): "generic", (10, 8): "generic", (13, 4): "v3<7,6>", (16, 4): "rows<8,.> / fused<8>"}


def n1_of(log_n):
    return 1 << (log_n // 2)   # csrc/ntt.hip: split_for


def extended(ctx, fk, coeffs, n_coeffs, dom):
    """-> (status, the output buffer's words on the host); the buffer starts filled with PATTERN"""
    out = ctx.to_device(np.full(dom.length * fk, PATTERN, np.uint64))
    d_coeffs = ctx.to_device(coeffs) if n_coeffs else None
    status = ctx.lib.tvm_evaluate_extended(ctx.handle, fk, d_coeffs.ptr if d_coeffs else None, n_coeffs, dom.c(), out.ptr)
    words = out.download((dom.length * fk,))
    out.free()
    if d_coeffs:
        d_coeffs.free()
    return status, words


def general(ctx, fk, coeffs, n_coeffs, dom):
    d_coeffs = ctx.to_device(coeffs)
    out = dom.evaluate(ctx, d_coeffs, n_coeffs, fk)
    words = out.download((dom.length * fk,))
    out.free()
    d_coeffs.free()
    return words


@pytest.fixture(scope="module")
def coefficients(orc):
    """2^17 + 3 random words, computed once: every case reads a prefix and nobody writes"""
    c = orc.random_elements(np.random.default_rng(4242), ((1 << 17) * 3,))
    c.setflags(write=False)
    return c


@pytest.mark.parametrize("fk", [3, 1])
@pytest.mark.parametrize("log_n,ratio", sorted(SHAPES))
def test_the_route_gives_tvm_evaluates_words(ctx, orc, coefficients, log_n, ratio, fk):
    """excess n_coeffs - n = 0, 1, n1, n1 + 1 and n on the domain of ratio * n points, offset = the field's generator.  An excess of n
    makes n_coeffs = 2 n a power of two itself: the split is made THERE (the largest power of two in n_coeffs), with no excess and
    half the ratio -- at ratio 2 that leaves one coset, and the entry point must refuse."""
    if log_n > 13 and ctx.kind == "emu":
        pytest.skip("CPU suite time: the 256-point axes run on the GPU")
    n, n1 = 1 << log_n, n1_of(log_n)
    dom = ArithmeticDomain.of_length(ratio * n).with_offset(field.generator())
    for excess in (0, 1, n1, n1 + 1, n):
        n_coeffs = n + excess
        co = np.ascontiguousarray(coefficients[:n_coeffs * fk])
        status, got = extended(ctx, fk, co, n_coeffs, dom)
        if excess == n and ratio == 2:
            assert status == NOT_APPLICABLE and (got == PATTERN).all()
            continue
        assert status == 0, (excess, status)
        want = general(ctx, fk, co, n_coeffs, dom)
        assert (got == want).all(), excess
        if excess == 0:
            assert (got == orc.coset_evaluate(co, orc.Domain(dom.offset, dom.generator, dom.length), fk)).all()


def test_other_offsets_and_the_option(ctx, coefficients):
    """offset 1 and a random offset at n = 2^10, ratio 4; with the option off the same call refuses and writes nothing, and the option
    comes back"""
    n_coeffs = 1024 + 33
    co = np.ascontiguousarray(coefficients[:3 * n_coeffs])
    for offset in (field.ONE, int(np.random.default_rng(7).integers(2, field.P, dtype=np.uint64))):
        dom = ArithmeticDomain.of_length(4096).with_offset(offset)
        status, got = extended(ctx, 3, co, n_coeffs, dom)
        assert status == 0 and (got == general(ctx, 3, co, n_coeffs, dom)).all()
    assert ctx.option(13) == 1
    ctx.combination_from_coefficients(False)
    try:
        status, got = extended(ctx, 3, co, n_coeffs, dom)
        assert ctx.option(13) == 0 and status == NOT_APPLICABLE and (got == PATTERN).all()
    finally:
        ctx.combination_from_coefficients(True)
    status, got = extended(ctx, 3, co, n_coeffs, dom)
    assert status == 0 and (got != PATTERN).any()


@pytest.mark.parametrize("what,n_coeffs,length,gen_power", [
    ("L / n = 1", 1024 + 5, 1024, 1),             # (more coefficients than points: tvm_evaluate folds them)
    ("L / n = 1, no excess", 1024, 1024, 1),
    ("L / n = 64", 1024 + 5, 65536, 1),
    ("excess > n", 1024 + 1025, 2048, 1),         # 2049 coefficients: the power of two in them is the domain's length
    ("non-standard generator", 1024 + 5, 4096, 3),
    ("n_coeffs = 0", 0, 4096, 1),
    ("fewer than 16 coefficients", 15, 64, 1),
])
def test_shapes_outside_the_gate_are_refused_and_nothing_is_written(ctx, coefficients, what, n_coeffs, length, gen_power):
    dom = ArithmeticDomain.of_length(length).with_offset(field.generator())
    dom.generator = field.mont_pow(dom.generator, gen_power)   # (an odd power: still a primitive root of that order)
    for fk in (3, 1):
        co = np.ascontiguousarray(coefficients[:max(n_coeffs, 1) * fk])
        status, got = extended(ctx, fk, co, n_coeffs, dom)
        assert status == NOT_APPLICABLE, what
        assert (got == PATTERN).all(), what
        if n_coeffs:   # ... and the general transform takes the same arguments
            assert general(ctx, fk, co, n_coeffs, dom).size == length * fk


def _host_library(ctx):
    from triton_vm_amd import native_host

    backend = ctx.lib._name
    if ctx.kind == "emu":
        return native_host.load_host_library(backend, os.path.join(os.path.dirname(backend), "libtriton_host_emu.so"))
    return native_host.load_host_library(backend)


def test_the_cpp_hosts_proof_is_the_same_with_either_route(ctx, orc):
    """A random trace of 2^4 rows with 5 randomizers (21 coefficients on a domain of 64 points: the shortest the route takes) through
    the C++ host (triton_host.cpp: WholeSteps::combination_codeword): the proof with the option on and with it off, word for word."""
    from triton_vm_amd import native_host
    from triton_vm_amd.prover import Claim, Prover, StarkParameters

    rng = np.random.default_rng(4)
    p = StarkParameters(4, num_trace_randomizers=5, num_collinearity_checks=4, log2_expansion=2)
    n = p.trace.length
    main_trace, aux_trace = orc.random_elements(rng, (379, n)), orc.random_elements(rng, (91, n, 3))
    claim = Claim(orc.random_elements(rng, 5), orc.random_elements(rng, 3), orc.random_elements(rng, 2))
    py = Prover(ctx, p, main_trace, aux_trace, seed=9, claim=claim)
    native = native_host.NativeProver(ctx, _host_library(ctx), p, py.main.d_trace, py.main.d_randomizers, py.aux.d_trace,
                                      py.aux.d_randomizers, py.quotient_randomizer, claim)
    try:
        on = native.prove()
        ctx.combination_from_coefficients(False)
        off = native.prove()
    finally:
        ctx.combination_from_coefficients(True)
    assert on.size == off.size and (on == off).all()


@pytest.mark.gpu
def test_prove_fib_at_2p10_rows_hashes_to_the_pinned_digest_with_either_route(orc):
    """prove_fib padded to 2^10 rows through the C++ host: the proof with the option on and with it off is the same word for word and
    hashes to the digest of the oracle prover's proof of the same program, input and prover seed -- the prover that reproduces the
    reference's proof digests.  tests/golden/oracle_proof_digests.json starts at 2^16 rows, so the record for this height, in the same
    format and from the same oracle/real_prover.py call as tests/golden/make_oracle_proof_digests.py makes (case fib:10:fri, 11 s of
    oracle prover), lies in a file of its own: tests/golden/combination_route_proof_digest.json."""
    import json

    from oracle.vm import workload
    from tests import test_proof_snapshot as snap
    from triton_vm_amd import Context, native_host
    from triton_vm_amd.proof_stream import Proof
    from triton_vm_amd.prover import Claim

    with open(os.path.join(os.path.dirname(__file__), "golden", "combination_route_proof_digest.json")) as f:
        want = json.load(f)["fib:10:fri"]
    e = workload.execution("fib", 10)
    assert [int(v) for v in orc.from_mont(e["public_input"])] == want["public_input"]
    claim = Claim(e["program_digest"], e["public_input"], e["public_output"])
    seed = snap.prover_seed(want["seed_u64"])
    ctx = Context(device=0)
    try:
        host = native_host.load_host_library()
        proofs = []
        for on in (True, False):
            ctx.combination_from_coefficients(on)
            proofs.append(native_host.prove_execution(ctx, host, e["aet"], e["padded_height"], claim, seed, ldt="fri"))
        assert proofs[0].size == want["proof_words"] == proofs[1].size and (proofs[0] == proofs[1]).all()
        assert [int(w) for w in Proof(proofs[0]).digest(ctx.lib)] == want["digest"]
    finally:
        ctx.close()
