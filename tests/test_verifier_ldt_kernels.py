"""The verifier's batch work outside the revealed rows (csrc/verify_ldt.hip: tvm_verifier_merkle_roots, tvm_verifier_fri_folds,
tvm_verifier_stir_answers) against the Python verifier's own loops (triton_vm_amd/verifier.py: verify_inclusion, the collinearity
loop of _fri_verify, in_domain_answers of _stir_verify): the same values and the same verdicts on every input tried."""
import ctypes

import numpy as np
import pytest

from triton_vm_amd import field, stark, verifier_ldt
from triton_vm_amd.verifier import VerificationError, Verifier, _xfe, verify_inclusion


def _tree(ctx, orc, rng, n):
    leaves = orc.random_elements(rng, (n, 5))
    d_nodes, d_leaves = ctx.alloc(10 * n), ctx.to_device(leaves)
    ctx._check(ctx.lib.tvm_merkle_tree(ctx.handle, d_leaves.ptr, n, d_nodes.ptr), "merkle")
    return d_nodes.download((2 * n, 5))


def _python_verdict(ctx, root, n, idx, leaves, auth):
    try:
        verify_inclusion(ctx.lib, root, n, idx, leaves, auth, "BadMerkleAuthenticationPath")
        return "accepted"
    except VerificationError:
        return "rejected"


def _query_sets(rng, n):
    sets = [[int(rng.integers(n))], list(range(n)), [0, n - 1], [0], [n - 1], [2 * int(rng.integers(n // 2)), 0]]
    sets[-1][1] = sets[-1][0] + 1                                     # both children of one parent
    sets += [[int(i) for i in rng.integers(n, size=q)] for q in (80, 300)]   # with duplicates
    return sets


def test_partial_tree_roots_equal_the_tree_and_verdicts_equal_verify_inclusion(ctx, orc):
    rng = np.random.default_rng(21)
    jobs, want_roots, want_verdicts = [], [], []
    for log_n in range(1, 13):
        n = 1 << log_n
        nodes = _tree(ctx, orc, rng, n)
        for k, idx in enumerate(_query_sets(rng, n)):
            leaves = nodes[n + np.array(idx)]
            auth = nodes[stark.auth_node_indices(n, idx).astype(np.int64)].reshape(-1, 5)
            variants = [(leaves, auth)]
            if (log_n + k) % 3 == 0:   # tampering: a leaf word, an authentication node word, one node dropped, one appended
                bad_leaf = leaves.copy()
                bad_leaf[int(rng.integers(len(idx))), int(rng.integers(5))] ^= np.uint64(1)
                variants.append((bad_leaf, auth))
                if len(auth):
                    bad_auth = auth.copy()
                    bad_auth[int(rng.integers(len(auth))), int(rng.integers(5))] ^= np.uint64(1)
                    variants += [(leaves, bad_auth), (leaves, auth[:-1])]
                variants.append((leaves, np.concatenate([auth, nodes[1:2]])))
            for lv, au in variants:
                jobs.append((n, idx, lv, au))
                want_roots.append(nodes[1])
                want_verdicts.append(_python_verdict(ctx, nodes[1], n, idx, lv, au))
    assert want_verdicts.count("rejected") > 20 and want_verdicts.count("accepted") > 60
    roots, flags = verifier_ldt.merkle_roots(ctx, jobs)     # trees of every height in ONE call
    for j, (job, root, verdict) in enumerate(zip(jobs, want_roots, want_verdicts)):
        got = "accepted" if not flags[j] and (roots[j] == root).all() else "rejected"
        assert got == verdict, (j, job[0], len(job[1]), len(job[3]))
        if flags[j]:
            assert not roots[j].any()
    # and the same jobs one per call
    for j in rng.integers(len(jobs), size=12):
        r1, f1 = verifier_ldt.merkle_roots(ctx, [jobs[j]])
        assert f1[0] == flags[j] and (r1[0] == roots[j]).all()


def test_partial_tree_malformed_jobs_are_flags_and_bad_arguments_are_statuses(ctx, orc):
    from triton_vm_amd.capi import TritonHipError

    rng = np.random.default_rng(22)
    n = 16
    nodes = _tree(ctx, orc, rng, n)
    idx = [3, 3, 9]
    leaves, auth = nodes[n + np.array(idx)], nodes[stark.auth_node_indices(n, idx).astype(np.int64)]
    conflicting = leaves.copy()
    conflicting[1, 0] ^= np.uint64(1)                      # the same index twice, with two digests
    jobs = [(n, idx, leaves, auth), (n, idx, conflicting, auth), (n, [3, 16], leaves[:2], auth), (n, [], np.zeros((0, 5)), np.zeros((0, 5))),
            (1, [0], nodes[n:n + 1], np.zeros((0, 5)))]
    roots, flags = verifier_ldt.merkle_roots(ctx, jobs)
    assert list(flags) == [0, 1, 1, 1, 0]
    assert (roots[0] == nodes[1]).all() and (roots[4] == nodes[n]).all()   # a tree of one leaf is its leaf
    assert _python_verdict(ctx, nodes[1], n, idx, conflicting, auth) == "rejected"
    with pytest.raises(TritonHipError):
        verifier_ldt.merkle_roots(ctx, [(12, [1], leaves[:1], auth)])      # not a power of two
    with pytest.raises(TritonHipError) as e:
        verifier_ldt.merkle_roots(ctx, [(1 << 41, [1], leaves[:1], auth)])
    assert e.value.status == 4                                               # TVM_ERR_UNSUPPORTED
    assert (verifier_ldt.merkle_roots(ctx, jobs[:1])[0][0] == nodes[1]).all()   # the context is usable afterwards


def _python_folds(ctx, dom, challenges, a0, a_leaves, b_leaves):
    """the loop of verifier.py: Verifier._fri_verify, lines 289-300"""
    X = _xfe(ctx.lib)
    partial_a, d = a_leaves, dom
    for r, challenge in enumerate(challenges):
        ia = [i % d.length for i in a0]
        ib = [(i + d.length // 2) % d.length for i in a0]
        folded = []
        for j in range(len(a0)):
            xa, xb = X.lift(d.value(ia[j])), X.lift(d.value(ib[j]))
            slope = X.mul(X.sub(b_leaves[r][j], partial_a[j]), X.inv(X.sub(xb, xa)))
            folded.append(X.add(partial_a[j], X.mul(slope, X.sub(challenge, xa))))
        partial_a = np.array(folded, np.uint64)
        d = d.pow(2)
    return partial_a


@pytest.mark.parametrize("log_n,n_rounds", [(7, 3), (8, 4), (9, 5), (10, 6)])
def test_fri_folds_equal_the_folded_codeword_and_the_python_loop(ctx, orc, log_n, n_rounds):
    from triton_vm_amd.arithmetic_domain import ArithmeticDomain

    rng = np.random.default_rng(log_n)
    n = 1 << log_n
    dom = ArithmeticDomain.of_length(n).with_offset(field.to_mont(7))
    poly = orc.random_elements(rng, (n // 4, 3))
    codewords = [orc.coset_evaluate(poly, orc.Domain(dom.offset, dom.generator, dom.length), 3).reshape(-1, 3)]
    challenges = orc.random_elements(rng, (n_rounds, 3))
    d, d_cw = dom, ctx.to_device(codewords[0])
    for r in range(n_rounds):
        d_cw = stark.split_and_fold(ctx, d_cw, d, challenges[r])
        d = d.pow(2)
        codewords.append(d_cw.download((d.length, 3)))
    a0 = [int(i) for i in rng.integers(n, size=45)] + [0, n - 1, n // 2]
    b = np.array([codewords[r][[(i + (n >> r) // 2) % (n >> r) for i in a0]] for r in range(n_rounds)], np.uint64)
    got = verifier_ldt.fri_folds(ctx, dom, challenges, a0, codewords[0][a0], b)
    assert (got == codewords[-1][[i % (n >> n_rounds) for i in a0]]).all()
    assert (got == _python_folds(ctx, dom, challenges, a0, codewords[0][a0], b)).all()
    # leaves that come from no low-degree codeword: still the Python loop, word for word
    a_rand, b_rand = orc.random_elements(rng, (len(a0), 3)), orc.random_elements(rng, (n_rounds, len(a0), 3))
    assert (verifier_ldt.fri_folds(ctx, dom, challenges, a0, a_rand, b_rand) == _python_folds(ctx, dom, challenges, a0, a_rand, b_rand)).all()


class _Spy:
    """an object that stands in for `target` and lets `hooks` replace some of its attributes"""

    def __init__(self, target, **hooks):
        self.__dict__.update(_target=target, _hooks=hooks)

    def __getattr__(self, name):
        hooks = self.__dict__["_hooks"]
        return hooks[name] if name in hooks else getattr(self.__dict__["_target"], name)


def _python_in_domain_answers(ctx, stream, stir, force=None):
    """Verifier._stir_verify on `stream`, with every fold_at result recorded: the in-domain answers, query by query, in the order
    the rounds ask for them.  force = (k, value): the k-th sample_scalars(1) call returns `value` instead of what the sponge
    gives (the sponge still advances: the indices of later rounds do not change)."""
    recorded = []

    def poly_eval(coeffs, n, points, m, zerofier, out):
        ctx.lib.tvm_host_xfe_poly_eval(coeffs, n, points, m, zerofier, out)
        if m == 1 and not zerofier:
            recorded.append(np.array((ctypes.c_uint64 * 3).from_address(out), np.uint64))

    spy_ctx = _Spy(ctx, lib=_Spy(ctx.lib, tvm_host_xfe_poly_eval=poly_eval))
    view = stream.verifier_view()
    calls = [0]

    def sample_scalars(n):
        out = view.sample_scalars(n)
        if n == 1:
            calls[0] += 1
            if force is not None and calls[0] == force[0]:
                return np.array([force[1]], np.uint64)
        return out

    try:
        Verifier(spy_ctx, ldt="stir")._stir_verify(_Spy(view, sample_scalars=sample_scalars), view.dequeue, stir, _xfe(ctx.lib))
        verdict = "accepted"
    except VerificationError:
        verdict = "rejected"
    return recorded, verdict


def _kernel_in_domain_answers(ctx, stream, stir, force=None):
    """the same walk over the transcript with tvm_verifier_stir_answers (and tvm_xfe_interpolate for the answer polynomial)"""
    from triton_vm_amd.low_degree_test import Stir

    X, ff = _xfe(ctx.lib), stir.folding_factor
    view = stream.verifier_view()
    calls = [0]

    def sample(n):   # counts the sample_scalars(1) calls exactly as the spy of _python_in_domain_answers does
        out = view.sample_scalars(n)
        if n == 1:
            calls[0] += 1
            if force is not None and calls[0] == force[0]:
                return np.array([force[1]], np.uint64)
        return out

    sample_one = lambda: sample(1)[0]

    def round_answers(domain, num_queries, randomness, previous):
        indices = view.sample_indices(domain.length, num_queries)
        leafs, _ = view.dequeue("stir response leafs"), view.dequeue("stir response auth")
        folded_len = domain.length // ff
        by_index = dict(zip(dict.fromkeys(i % folded_len for i in indices), leafs))
        values = np.array([by_index[i % folded_len] for i in indices], np.uint64)
        roots = [domain.value(i % folded_len) for i in indices]
        if previous is not None:
            quotient_set, quotient_answers, rc = previous
            poly = np.zeros_like(quotient_set)
            ctx._check(ctx.lib.tvm_xfe_interpolate(ctx.handle, quotient_set.ctypes.data, quotient_answers.ctypes.data, len(quotient_set),
                                                   poly.ctypes.data), "tvm_xfe_interpolate")
            previous = (quotient_set, poly, rc)
        answers = verifier_ldt.stir_answers(ctx, values, roots, field.mont_pow(domain.generator, folded_len), randomness, previous)
        return answers, [domain.pow(ff).value(i % folded_len) for i in indices], roots

    out, coset_roots, last_rc_call = [], [], 0
    domain, previous = stir.initial_domain, None
    view.dequeue("MerkleRoot")
    for in_domain, out_of_domain in stir.round_queries:
        randomness = sample_one()
        view.dequeue("MerkleRoot")
        ood_queries = sample(out_of_domain)
        ood_answers = np.ascontiguousarray(view.dequeue("StirOutOfDomainValues"), dtype=np.uint64).reshape(-1, 3)
        answers, points, roots = round_answers(domain, in_domain, randomness, previous)
        out.append(answers)
        coset_roots.append(roots)
        quotient_set, quotient_answers, seen = [], [], set()
        for point, answer in list(zip([X.lift(p) for p in points], answers)) + list(zip(ood_queries, ood_answers)):
            key = tuple(int(c) for c in point)
            if key not in seen:
                seen.add(key)
                quotient_set.append(point)
                quotient_answers.append(answer)
        previous = (np.array(quotient_set, np.uint64), np.array(quotient_answers, np.uint64), sample_one())
        last_rc_call = calls[0]
        domain = Stir.next_round_domain(domain)
    randomness = sample_one()
    view.dequeue("Polynomial")
    answers, _, roots = round_answers(domain, stir.final_num_in_domain_queries, randomness, previous)
    return out + [answers], coset_roots + [roots], field.mont_pow(domain.generator, domain.length // ff), last_rc_call


@pytest.mark.parametrize("log2_bound,queries", [(6, [(3, 1), (2, 0)]), (8, [(5, 2), (3, 1), (4, 0)]), (4, [(3, 0)])])
def test_stir_answers_equal_the_python_verifiers_in_domain_answers(ctx, orc, log2_bound, queries):
    from tests.test_stir import odom, small_stir
    from triton_vm_amd.prover import ProofStream

    rng = np.random.default_rng(log2_bound)
    stir = small_stir(log2_bound, queries)
    poly = orc.random_elements(rng, (1 << log2_bound, 3))
    codeword = orc.coset_evaluate(poly, odom(orc, stir.initial_domain), 3).reshape(-1, 3)
    ps = ProofStream(ctx.lib)
    stir.prove(ctx, ctx.to_device(codeword), ps)
    want, verdict = _python_in_domain_answers(ctx, ps, stir)
    assert verdict == "accepted" and len(want) == sum(q[0] for q in queries)
    got, coset_roots, last_kth_root, last_rc_call = _kernel_in_domain_answers(ctx, ps, stir)
    assert len(got) == len(queries) and (np.concatenate(got) == np.array(want, np.uint64)).all()   # first and subsequent rounds
    if len(queries) < 2:
        return
    # r x = 1 forced: the last degree-correction randomness is the inverse of a point of the last round's first coset
    X = _xfe(ctx.lib)
    x = field.mont_mul(coset_roots[-1][0], last_kth_root)
    force = (last_rc_call, X.inv(X.lift(x)))
    want, _ = _python_in_domain_answers(ctx, ps, stir, force)
    got = _kernel_in_domain_answers(ctx, ps, stir, force)[0]
    assert len(want) == sum(q[0] for q in queries) and (np.concatenate(got) == np.array(want, np.uint64)).all()
    unforced = _kernel_in_domain_answers(ctx, ps, stir)[0]
    assert not (got[-1][0] == unforced[-1][0]).all()            # (the forced randomness did reach the last round)
