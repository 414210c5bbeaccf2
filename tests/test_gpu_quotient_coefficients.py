"""tvm_all_quotients_coefficients and tvm_quotient_segments_from_coefficients at full size: the extended tables of prove_fib at
2^20 padded rows (BASELINE configs[1]; 1024-row blocks, 198 trace randomizers, the library's default gate), with the challenges and
quotient weights of the proof itself.  The emulation covers the same two equalities at 256 rows (tests/test_quotient_coefficients.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


class _Done(Exception):
    pass


def test_coefficient_form_equals_the_codeword_path_at_2p20_rows():
    from oracle.vm import workload
    from tests import test_proof_snapshot as snap
    from triton_vm_amd import Context, stark
    from triton_vm_amd.proof_stream import Claim
    from triton_vm_amd.prover import Prover

    ctx = Context(device=0)
    try:
        e = workload.execution("fib", 20)
        claim = Claim(e["program_digest"], e["public_input"], e["public_output"])
        prover = Prover.from_execution(ctx, e["aet"], e["padded_height"], claim, snap.prover_seed(7), ldt="fri", log2_expansion=2)
        p = prover.p
        n, q_len = p.trace.length, p.quotient.length
        assert n == 1 << 20 and q_len == 8 * n and p.ldt.length == q_len

        def at_the_quotient_step(challenges, weights):
            ctx.assume_valid_trace(True)
            try:
                d_codeword = stark.all_quotients_combined(ctx, prover.main, prover.aux, p.trace, p.quotient, challenges, weights)
                coefficients = stark.all_quotients_coefficients(ctx, prover.main, prover.aux, p.trace, p.quotient, challenges, weights)
            finally:
                ctx.assume_valid_trace(False)
            assert coefficients is not None, "the gate is open at 2^20 rows with the default parameters"
            d_coeffs, n_coeffs = coefficients
            assert n_coeffs == 4 * n + 1024
            # 1. evaluated on the quotient domain, the coefficients are the codeword
            codeword = d_codeword.download((q_len, 3))
            assert np.array_equal(p.quotient.evaluate(ctx, d_coeffs, n_coeffs, 3).download((q_len, 3)), codeword)
            assert codeword.any()
            del codeword
            # (4N + 4h - 3 coefficients at most: the rest of the remainder block is zero)
            tail = d_coeffs.download((q_len, 3))[4 * n:n_coeffs]
            assert tail[:4 * 198 - 3].any() and not tail[4 * 198 - 3:].any()
            # 2. the same segment polynomials and the same segment table
            want = stark.quotient_segments(ctx, d_codeword, p.quotient, p.ldt, prover.quotient_randomizer)
            got = stark.quotient_segments_from_coefficients(ctx, d_coeffs, n_coeffs, p.ldt, prover.quotient_randomizer, want.poly_len)
            assert np.array_equal(got.polys.download((5, want.poly_len, 3)), want.polys.download((5, want.poly_len, 3)))
            table = want.codewords()
            assert np.array_equal(got.codewords(), table)
            del table
            got.free()
            want.free()
            raise _Done

        prover._quotient_codeword = at_the_quotient_step
        with pytest.raises(_Done):
            prover.prove()
        prover.release()
    finally:
        ctx.close()
