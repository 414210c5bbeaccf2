"""tvmh_verify_batch (triton_vm_amd/host/verify_batch.cpp): many proofs per call with the device work shared.  The contract: the verdict,
the revealed indices and their number of every job are exactly what tvmh_verify answers for that job alone, whatever else is in the batch
and in whatever order.  Every comparison is against tvmh_verify (native_host.verify_verdict) on the same words, code for code."""
import numpy as np
import pytest

from tests import test_proof_snapshot as snap
from tests import vm_fixture as vf
from tests.test_native_verifier import host, item_offsets, oracle_proof, oracle_stir_proof  # noqa: F401  (host: the fixture)
from triton_vm_amd import native_host
from triton_vm_amd.native_host import verify_batch_verdicts, verify_job, verify_verdict
from triton_vm_amd.proof_stream import Claim

ACCEPTED = 0


def single(ctx, host, job):
    """tvmh_verify for one job of a batch -> (verdict code, indices)"""
    claim, words, security_level, log2_expansion, ldt = job
    rc, code, name, indices, _ = verify_verdict(ctx, host, claim, words, security_level=security_level, log2_expansion=log2_expansion, ldt=ldt)
    assert rc == 0, (rc, name)
    return code, indices


def batch(ctx, host, jobs, **kw):
    rc, error, verdicts, indices, counts, stages = verify_batch_verdicts(ctx, host, jobs, **kw)
    assert rc == 0, (rc, error)     # a rejection is a verdict, never an error status
    return verdicts, indices, counts


_SINGLE = {}


def singles(ctx, host, jobs):
    """tvmh_verify's answers for the jobs; a job is verified once per backend however many tests and batches hold it (an emulated
    verification takes seconds)"""
    out = []
    for job in jobs:
        claim, words, security_level, log2_expansion, ldt = job
        key = (ctx.kind, np.asarray(words).tobytes(), claim.program_digest.tobytes(), claim.input.tobytes(), claim.output.tobytes(), claim.version,
               security_level, log2_expansion, ldt)
        if key not in _SINGLE:
            _SINGLE[key] = single(ctx, host, job)
        out.append(_SINGLE[key])
    return out


@pytest.fixture(scope="module")
def gpu_ctx():
    from triton_vm_amd import Context

    c = Context(device=0)
    c.kind = "gpu"
    yield c
    c.close()


@pytest.fixture(scope="module")
def gpu_host(gpu_ctx):
    return native_host.load_host_library(gpu_ctx.lib._name)


def proofs():
    """(words, claim, indices, security level, ldt) of the four oracle-prover proofs"""
    out = []
    for which, seed, level in (("tiny", snap.SEED_U64, 160), ("every", snap.SEED_U64_EVERY, 32)):
        out.append(oracle_proof(which, seed, level) + (level, "fri"))
        out.append(oracle_stir_proof(which, seed, level) + (level, "stir"))
    return out


def mixed_jobs():
    """eight accepting jobs: the FRI proofs with the choice explicit and by Stark::ldt's rule (FRI below 2^16 rows), the STIR proofs with the
    choice explicit, twice (the rule never picks STIR at these heights); two heights, two security levels -> (jobs, expected indices)"""
    jobs, want = [], []
    for words, claim, indices, level, ldt in proofs():
        for choice in (("fri", None) if ldt == "fri" else ("stir", "stir")):
            jobs.append(verify_job(claim, words, security_level=level, ldt=choice))
            want.append(indices)
    return jobs, want


def test_a_mixed_batch_is_accepted_with_the_oracle_provers_indices_in_either_order(ctx, host):
    jobs, want = mixed_jobs()
    assert len(jobs) == 8
    verdicts, indices, counts = batch(ctx, host, jobs)
    assert verdicts == [ACCEPTED] * 8
    assert indices == want and counts == [len(w) for w in want]
    verdicts, indices, counts = batch(ctx, host, jobs[::-1])
    assert verdicts == [ACCEPTED] * 8 and indices == want[::-1]


def corruption_walk(ctx, ldt):
    """the inputs of test_native_verifier's corruption walk, as jobs: the clean proof at both ends"""
    words, claim, _ = (oracle_proof if ldt == "fri" else oracle_stir_proof)("tiny", snap.SEED_U64, 160)
    jobs = [verify_job(claim, words, ldt=ldt)]
    rng = np.random.default_rng(6)
    offsets = item_offsets(ctx.lib, words)
    assert ("StirResponse" if ldt == "stir" else "FriResponse") in offsets
    for name, places in offsets.items():
        if name == "Log2PaddedHeight":
            continue
        start, size = places[int(rng.integers(len(places)))]
        bad = words.copy()
        bad[start + (size // 2 if size > 8 else size - 1)] ^= np.uint64(1)
        jobs.append(verify_job(claim, bad, ldt=ldt))
    jobs.append(verify_job(Claim(claim.program_digest, claim.input, claim.output, version=5), words, ldt=ldt))
    jobs.append(verify_job(Claim(claim.program_digest, claim.input[::-1].copy(), claim.output), words, ldt=ldt))
    jobs.append(verify_job(Claim(claim.program_digest[::-1].copy(), claim.input, claim.output), words, ldt=ldt))
    jobs.append(verify_job(claim, words[:-7], ldt=ldt))
    jobs.append(verify_job(claim, np.concatenate([words, words[-3:]]), ldt=ldt))
    jobs.append(verify_job(claim, words, security_level=128, ldt=ldt))
    jobs.append(verify_job(claim, words, ldt=ldt))
    return jobs


@pytest.mark.parametrize("ldt", ["fri", "stir"])
def test_the_corruption_walk_as_one_batch_gives_every_jobs_own_verdict(ctx, host, ldt):
    jobs = corruption_walk(ctx, ldt)
    want = singles(ctx, host, jobs)
    verdicts, indices, counts = batch(ctx, host, jobs)
    assert verdicts == [code for code, _ in want]
    assert indices == [idx for _, idx in want]
    assert verdicts[0] == verdicts[-1] == ACCEPTED and all(verdicts[1:-1])
    assert len(set(verdicts)) >= 6, verdicts   # the walk reaches many kinds of check


def test_of_two_faults_the_one_the_reference_meets_first_is_the_verdict(ctx, host):
    words, claim, _ = oracle_proof("tiny", snap.SEED_U64, 160)
    offsets = item_offsets(ctx.lib, words)

    def flipped(*places):
        bad = words.copy()
        for name, which in places:
            start, size = offsets[name][which]
            bad[start + size // 2] ^= np.uint64(1)
        return verify_job(claim, bad, ldt="fri")

    jobs = [flipped(("FriResponse", 0), ("OutOfDomainQuotientSegments", 0)),   # a deferred inclusion, and an earlier host-decidable failure
            flipped(("MasterMainTableRows", 0), ("FriCodeword", 0)),           # a later deferred inclusion, and an earlier device check
            flipped(("FriResponse", 0)), flipped(("OutOfDomainQuotientSegments", 0)), flipped(("MasterMainTableRows", 0)),
            flipped(("FriCodeword", 0))]
    want = [code for code, _ in singles(ctx, host, jobs)]
    assert len(set(want[2:])) == 4, want    # four different single faults ...
    assert want[0] == want[3] and want[1] == want[5], want   # ... of which the earlier one decides a pair
    verdicts, _, _ = batch(ctx, host, jobs)
    assert verdicts == want


def isolation_jobs():
    jobs, corrupted = [], []
    rng = np.random.default_rng(40)
    sources = proofs()[:2]   # the FRI and the STIR proof of "tiny"
    for trial in range(40):
        words, claim, _, level, ldt = sources[trial % 2]
        bad = words.copy()
        k = int(rng.integers(0, bad.size))
        bad[k] = np.uint64(rng.integers(0, 2**63))
        corrupted.append(not np.array_equal(bad, words))
        jobs.append(verify_job(claim, bad, security_level=level, ldt=ldt))
        jobs.append(verify_job(claim, words, security_level=level, ldt=ldt))
    return jobs, corrupted


@pytest.mark.gpu
def test_a_corrupted_job_changes_no_other_jobs_verdict(gpu_ctx, gpu_host):
    """120 verifications, most of them whole: eight minutes on the emulation (seconds per emulated verification, whatever the proof), so on
    the GPU only, like the device proofs below.  On the emulation the corruption walks above hold clean jobs among corrupted ones."""
    ctx, host = gpu_ctx, gpu_host
    jobs, corrupted = isolation_jobs()
    assert len(jobs) == 80
    want = singles(ctx, host, jobs[0::2])
    verdicts, indices, _ = batch(ctx, host, jobs)
    assert verdicts[1::2] == [ACCEPTED] * 40 and all(indices[1::2])
    assert verdicts[0::2] == [code for code, _ in want]
    assert all(code != ACCEPTED for code, changed in zip(verdicts[0::2], corrupted) if changed)


_WHOLE = {}


@pytest.mark.parametrize("chunk", [1, 3])
def test_chunks_give_the_verdicts_and_indices_of_the_unchunked_call(ctx, host, chunk):
    jobs, want = mixed_jobs()
    words, claim, _, level, ldt = proofs()[0]
    bad = words.copy()
    bad[bad.size // 2] ^= np.uint64(1)
    jobs = jobs[:3] + [verify_job(claim, bad, security_level=level, ldt=ldt)] + jobs[5:]
    assert len(jobs) == 7
    if ctx.kind not in _WHOLE:
        _WHOLE[ctx.kind] = batch(ctx, host, jobs)   # the unchunked call, once per backend
    whole = _WHOLE[ctx.kind]
    assert whole[0][3] != ACCEPTED and whole[0].count(ACCEPTED) == 6
    assert host.tvmh_get_option(native_host.OPTION_VERIFY_BATCH_CHUNK) == 0
    with native_host.host_option(host, native_host.OPTION_VERIFY_BATCH_CHUNK, chunk):
        assert batch(ctx, host, jobs) == whole
    assert host.tvmh_get_option(native_host.OPTION_VERIFY_BATCH_CHUNK) == 0


def test_arguments(ctx, host):
    words, claim, want = oracle_proof("tiny", snap.SEED_U64, 160)
    good = verify_job(claim, words, ldt="fri")
    rc, error, verdicts, _, _, _ = verify_batch_verdicts(ctx, host, [])
    assert rc == 0                                                     # no job: nothing to do
    rc, error, verdicts, _, counts, _ = verify_batch_verdicts(ctx, host, [good, good, verify_job(claim, None)])
    assert rc == 1 and "job 2" in error, (rc, error)                   # a null proof with a non-zero length names its job ...
    assert verdicts == [0xFFFFFFFF] * 3 and counts == [0xFFFFFFFFFFFFFFFF] * 3   # ... and no verdict is written
    rc, error, verdicts, _, _, _ = verify_batch_verdicts(ctx, host, [good, verify_job(claim, words, ldt=3)])
    assert rc == 1 and "job 1" in error and verdicts == [0xFFFFFFFF] * 2, (rc, error)
    for kw in (dict(security_level=0), dict(security_level=513), dict(log2_expansion=0), dict(log2_expansion=9)):
        rc, error, verdicts, _, _, _ = verify_batch_verdicts(ctx, host, [verify_job(claim, words, **kw), good])
        assert rc == 1 and "job 0" in error and verdicts == [0xFFFFFFFF] * 2, (kw, rc, error)
    # (a stride too small for the indices: test_the_stride_is_never_written_past)
    # an empty proof is a decoding verdict, not an error
    empty = verify_job(claim, np.zeros(0, np.uint64))
    rc, error, verdicts, indices, counts, _ = verify_batch_verdicts(ctx, host, [good, empty, good], indices_stride=len(want))   # the exact stride
    assert (rc, verdicts, counts) == (0, [ACCEPTED, single(ctx, host, empty)[0], ACCEPTED], [len(want), 0, len(want)])
    assert indices == [want, [], want]
    assert verdicts[1] == 1    # VERDICT_PROOF_DECODING_ERROR
    # the wrapper that raises nothing for a rejection but returns it in the job's place
    from triton_vm_amd.verifier import VerificationError

    answers = native_host.verify_batch(ctx, host, [empty, good])
    assert answers[1] == want and isinstance(answers[0], VerificationError) and str(answers[0]) == "ProofDecodingError"
    with pytest.raises(native_host.NativeHostError):
        native_host.verify_batch(ctx, host, [verify_job(claim, None)])


def test_the_stride_is_never_written_past(ctx, host):
    words, claim, want = oracle_proof("tiny", snap.SEED_U64, 160)
    import ctypes as C

    job = native_host.VerifyJob(words.ctypes.data, words.size, claim.program_digest.ctypes.data, claim.version, claim.input.ctypes.data,
                                claim.input.size, claim.output.ctypes.data, claim.output.size, 160, 2, 0)
    jobs = (native_host.VerifyJob * 2)(job, job)
    stride = len(want) - 1
    verdicts, counts, indices = np.zeros(2, np.uint32), np.zeros(2, np.uint64), np.full(2 * stride + 8, 0xABAB, np.uint64)
    rc = host.tvmh_verify_batch(ctx.handle, C.addressof(jobs), 2, verdicts.ctypes.data, indices.ctypes.data, stride, counts.ctypes.data, None, None, 0)
    assert rc == 0 and list(counts) == [len(want)] * 2 and (indices == 0xABAB).all()


@pytest.mark.gpu
def test_device_proofs_of_prove_fib_in_one_batch(orc):
    """prove_fib on the device at 2^9 (the smallest trace prove_fib has), 2^10 and 2^12 rows, FRI and STIR, each twice: twelve jobs, one
    of them with a word flipped.  Slow on the emulation, so on the GPU only, as test_native_verifier has it."""
    from triton_vm_amd import Context

    ctx = Context(device=0)
    try:
        host_lib = native_host.load_host_library(ctx.lib._name)
        jobs = []
        for index, log2_padded_height in ((5, 9), (100, 10), (300, 12)):
            program, aet, public_input, output = vf.run(("fib", index))
            assert aet.padded_height() == 1 << log2_padded_height
            claim = snap.claim_of(orc, program, public_input, output)
            for ldt in ("fri", "stir"):
                words = snap.device_proof(ctx, orc, ("fib", index), 7, 160, ldt=ldt).words
                jobs += [verify_job(claim, words, ldt=ldt)] * 2
        assert len(jobs) == 12
        bad = jobs[7][1].copy()
        bad[bad.size // 3] ^= np.uint64(1)
        jobs[7] = verify_job(jobs[7][0], bad, ldt=jobs[7][4])
        want = [single(ctx, host_lib, job) for job in jobs]
        assert [code for code, _ in want].count(ACCEPTED) == 11 and want[7][0] != ACCEPTED
        verdicts, indices, _ = batch(ctx, host_lib, jobs)
        assert verdicts == [code for code, _ in want]
        assert indices == [idx for _, idx in want]
    finally:
        ctx.close()
