"""triton_vm::Verifier (triton_vm_amd/host/verifier.cpp, tvmh_verify): Verifier::verify in the C++ host with the per-query work on
the device -- against the reference-pinned proofs and against both existing verifiers (triton_vm_amd.verifier.Verifier and
oracle.real_verifier): the same verdict on every input tried, and the same variant name as the Python product verifier."""
import os

import numpy as np
import pytest

from tests import test_proof_snapshot as snap
from tests import vm_fixture as vf
from tests.test_verify_proof import item_offsets, oracle_proof
from triton_vm_amd import field, native_host
from triton_vm_amd.proof_stream import Claim, ProofDecodingError
from triton_vm_amd.verifier import VerificationError, Verifier


@pytest.fixture(scope="module")
def host(ctx):
    backend = ctx.lib._name
    if ctx.kind == "emu":
        return native_host.load_host_library(backend, os.path.join(os.path.dirname(backend), "libtriton_host_emu.so"))
    return native_host.load_host_library(backend)


_STIR_PROOFS = {}


def oracle_stir_proof(which, seed_u64, security_level):
    """the oracle prover's STIR proof of a snapshot program: the proof tests/golden/stir_regression_digests.json pins"""
    key = (which, seed_u64, security_level)
    if key not in _STIR_PROOFS:
        from oracle import oracle as orc, real_prover
        from tests.test_wider_pins import stir_numbers

        program, aet, public_input, output = vf.run(which)
        proof = real_prover.prove(program, public_input, *vf.non_determinism(which), seed_u64=seed_u64, security_level=security_level,
                                  stir=stir_numbers(aet.padded_height(), security_level))
        _STIR_PROOFS[key] = (orc.to_mont(np.array(proof["proof"], dtype=object)), snap.claim_of(orc, program, public_input, output), proof["indices"])
    return _STIR_PROOFS[key]


def _name(error):
    """the variant name of a VerificationError: the text up to a colon ("ProofStreamError: ...")"""
    return str(error).split(":")[0]


def verdicts(ctx, host, words, claim, ldt, **kw):
    """(native, product, oracle) verdicts, and the variant names where native and the product raise a VerificationError"""
    from oracle import proof_decode, real_verifier

    rc, code, name, indices, _ = native_host.verify_verdict(ctx, host, claim, words, ldt=ldt, **kw)
    assert rc == 0, (rc, name)     # a rejection is a verdict, never an error status
    out, names = ["rejected" if code else "accepted"], [name if code else None]
    try:
        Verifier(ctx, ldt=ldt, **kw).verify(claim, words)
        out.append("accepted")
        names.append(None)
    except VerificationError as e:
        out.append("rejected")
        names.append(_name(e))
    except ProofDecodingError:
        out.append("rejected")
        names.append("ProofDecodingError")
    try:
        real_verifier.verify(proof_decode.VerifierView(words), claim, ldt_choice=ldt or "fri", **kw)
        out.append("accepted")
    except (real_verifier.VerificationError, proof_decode.DecodingError, ValueError):
        out.append("rejected")
    return out, names


@pytest.mark.parametrize("which,seed,security_level", [("tiny", snap.SEED_U64, 160), ("every", snap.SEED_U64_EVERY, 32)])
def test_native_verifier_accepts_the_reference_pinned_proofs_with_the_oracle_provers_indices(ctx, host, which, seed, security_level):
    words, claim, indices = oracle_proof(which, seed, security_level)
    assert native_host.verify(ctx, host, claim, words, security_level=security_level, ldt="fri") == indices
    assert native_host.verify(ctx, host, claim, words, security_level=security_level) == indices   # Stark::ldt's rule: FRI below 2^16 rows
    assert native_host.proof_padded_height(host, words) == vf.run(which)[1].padded_height()
    words, claim, indices = oracle_stir_proof(which, seed, security_level)
    assert native_host.verify(ctx, host, claim, words, security_level=security_level, ldt="stir") == indices
    with pytest.raises(VerificationError):
        native_host.verify(ctx, host, claim, words, security_level=security_level, ldt="fri")


@pytest.mark.parametrize("ldt", ["fri", "stir"])
def test_native_verifier_gives_the_verdict_of_both_existing_verifiers_on_the_corruption_walk(ctx, host, ldt):
    words, claim, indices = (oracle_proof if ldt == "fri" else oracle_stir_proof)("tiny", snap.SEED_U64, 160)
    out, _ = verdicts(ctx, host, words, claim, ldt)
    assert out == ["accepted"] * 3

    def check(bad_words, bad_claim, what, **kw):
        out, names = verdicts(ctx, host, bad_words, bad_claim, ldt, **kw)
        assert out == ["rejected"] * 3, (what, out, names)
        assert names[0] == names[1], (what, names)

    rng = np.random.default_rng(6)
    offsets = item_offsets(ctx.lib, words)
    assert ("StirResponse" if ldt == "stir" else "FriResponse") in offsets
    for name, places in offsets.items():
        if name == "Log2PaddedHeight":
            continue
        start, size = places[int(rng.integers(len(places)))]
        bad = words.copy()
        bad[start + (size // 2 if size > 8 else size - 1)] ^= np.uint64(1)
        check(bad, claim, name)
    check(words, Claim(claim.program_digest, claim.input, claim.output, version=5), "version")
    check(words, Claim(claim.program_digest, claim.input[::-1].copy(), claim.output), "reversed input")
    check(words, Claim(claim.program_digest[::-1].copy(), claim.input, claim.output), "reversed digest")
    check(words[:-7], claim, "seven words cut off")
    check(np.concatenate([words, words[-3:]]), claim, "three words appended")
    check(words, claim, "security level 128", security_level=128)


def test_native_decoder_rejects_statically_sized_items_of_the_wrong_length(ctx, host):
    """the construction of tests/test_product_verifier.py: test_statically_sized_items_of_the_wrong_length_do_not_decode"""
    from triton_vm_amd.proof_stream import PROOF_ITEMS, STATIC_WORDS, ProofStream

    words, claim, indices = oracle_proof("tiny", snap.SEED_U64, 160)
    w = [field.from_mont(int(x)) for x in words]
    items, pos = [], 2
    for _ in range(w[1]):
        size = w[pos]
        items.append(np.array(words[pos + 1:pos + 1 + size]))
        pos += 1 + size

    def proof_of(item_list):
        parts = [np.array([field.to_mont(len(item_list))], np.uint64)]
        for it in item_list:
            parts += [np.array([field.to_mont(it.size)], np.uint64), it]
        body = np.concatenate(parts)
        return np.concatenate([[np.uint64(field.to_mont(body.size))], body])

    def decoding_failure(bad):
        with pytest.raises(ProofDecodingError):
            ProofStream.from_proof(ctx.lib, bad)
        rc, code, name, _, _ = native_host.verify_verdict(ctx, host, claim, bad)
        assert (rc, code, name) == (0, 1, "ProofDecodingError")
        with pytest.raises(ProofDecodingError):
            native_host.proof_padded_height(host, bad)

    assert native_host.verify(ctx, host, claim, proof_of(items)) == indices
    seen = set()
    for k, it in enumerate(items):
        name, kind, _ = PROOF_ITEMS[field.from_mont(int(it[0]))]
        if kind != "static" or name in seen:
            continue
        seen.add(name)
        for mutated in (np.concatenate([it, it[-1:]]), it[:-1]):
            decoding_failure(proof_of(items[:k] + [mutated] + items[k + 1:]))
    assert seen == set(STATIC_WORDS)
    k = next(i for i, it in enumerate(items) if PROOF_ITEMS[field.from_mont(int(it[0]))][0] == "Log2PaddedHeight")
    big = items[k].copy()
    big[1] = np.uint64(field.to_mont(1 << 32))       # a u32 that is not one
    decoding_failure(proof_of(items[:k] + [big] + items[k + 1:]))
    # Proof::padded_height wants exactly one Log2PaddedHeight
    for item_list in (items[:k] + items[k + 1:], items + [items[k]]):
        with pytest.raises(ProofDecodingError):
            native_host.proof_padded_height(host, proof_of(item_list))


@pytest.mark.parametrize("ldt", ["fri", "stir"])
def test_random_corruptions_end_in_a_rejecting_verdict_and_nothing_else(ctx, host, ldt):
    """tests/test_verify_proof.py: test_arbitrary_corruptions_never_escape_as_other_errors, for tvmh_verify: TVM_OK and a rejecting
    verdict, no other status"""
    words, claim, _ = (oracle_proof if ldt == "fri" else oracle_stir_proof)("tiny", snap.SEED_U64, 160)
    rng = np.random.default_rng(99)
    seen = set()
    for trial in range(160):
        bad = words.copy()
        kind = trial % 4
        if kind == 0:      # a few random words anywhere (length prefixes included)
            for k in rng.integers(0, bad.size, int(rng.integers(1, 4))):
                bad[k] = np.uint64(rng.integers(0, 2**63))
        elif kind == 1:    # truncation
            bad = bad[:int(rng.integers(0, bad.size))]
        elif kind == 2:    # small canonical values where length prefixes tend to live: the head of the proof
            bad[int(rng.integers(0, 64))] = np.uint64(field.to_mont(int(rng.integers(0, 40))))
        else:              # a block moved elsewhere
            a, b = sorted(int(v) for v in rng.integers(0, bad.size, 2))
            bad = np.concatenate([bad[:a], bad[b:], bad[a:b]])
        rc, code, name, indices, _ = native_host.verify_verdict(ctx, host, claim, bad, ldt=ldt)
        if np.array_equal(bad, words):
            continue
        assert rc == 0 and code != 0 and not indices, (trial, rc, code, name)
        seen.add(name)
    assert len(seen) >= 3, seen
    assert native_host.verify_verdict(ctx, host, claim, words, ldt=ldt)[1] == 0   # the context is as usable as before


def test_words_that_are_no_field_elements_do_not_decode_and_no_verifier_accepts_them(ctx, host):
    """a word in [p, 2^64) is not the raw word of a BFieldElement: the native decoder refuses it wherever it stands (length prefix,
    discriminant or payload); the two existing verifiers, which read such a word's residue, reject these proofs too"""
    words, claim, _ = oracle_proof("tiny", snap.SEED_U64, 160)
    rng = np.random.default_rng(7)
    places = [0, 1, 2, 3] + [int(k) for k in rng.integers(0, words.size, 36)]
    for k in places:
        bad = words.copy()
        bad[k] = np.uint64(field.P + int(rng.integers(0, 2**32 - 1)))
        rc, code, name, indices, _ = native_host.verify_verdict(ctx, host, claim, bad, ldt="fri")
        assert (rc, code, name, indices) == (0, 1, "ProofDecodingError", []), (k, rc, code, name)
        out, _ = verdicts(ctx, host, bad, claim, "fri")
        assert out == ["rejected"] * 3, (k, out)


@pytest.mark.gpu
@pytest.mark.parametrize("index,log2_padded_height,ldt", [(100, 10, "fri"), (100, 10, "stir"), (6000, 16, None)])
def test_device_proofs_of_prove_fib_are_accepted_natively(orc, index, log2_padded_height, ldt):
    """prove_fib on the device, verified by the C++ host: the Python product verifier's indices; a wrong public input is rejected.
    At 2^16 rows Stark::ldt's rule picks STIR (four full rounds)."""
    import time

    from oracle.vm import workload
    from triton_vm_amd import Context

    if log2_padded_height == 10:
        program, aet, public_input, output = vf.run(("fib", index))
        e = None
        assert aet.padded_height() == 1 << log2_padded_height
    else:
        e = workload.execution("fib", log2_padded_height)
    ctx = Context(device=0)
    try:
        host_lib = native_host.load_host_library(ctx.lib._name)
        if e is None:
            words = snap.device_proof(ctx, orc, ("fib", index), 7, 160, ldt=ldt).words
            claim = snap.claim_of(orc, program, public_input, output)
            wrong = snap.claim_of(orc, program, [index + 1], output)
        else:
            claim = Claim(e["program_digest"], e["public_input"], e["public_output"])
            wrong = Claim(e["program_digest"], [field.to_mont(field.from_mont(int(e["public_input"][0])) + 1)], e["public_output"])
            words = native_host.prove_execution(ctx, host_lib, e["aet"], e["padded_height"], claim, snap.prover_seed(7))
        t0 = time.perf_counter()
        indices = native_host.verify(ctx, host_lib, claim, words, ldt=ldt)
        print(f"native verification at 2^{log2_padded_height} rows ({ldt or 'stir by rule'}): {1e3 * (time.perf_counter() - t0):.1f} ms")
        assert indices == Verifier(ctx, ldt=ldt).verify(claim, words)
        with pytest.raises(VerificationError):
            native_host.verify(ctx, host_lib, wrong, words, ldt=ldt)
    finally:
        ctx.close()
