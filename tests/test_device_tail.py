"""The tail of a FRI proof in one device round trip (csrc/proof_tail.hip: tvm_fri_query_and_open; the C++ host under
TVMH_OPTION_DEVICE_TAIL).  Kernel level: every payload equals what the existing calls give -- the host's sample_indices,
tvm_gather_elements_batch at stark.auth_node_indices, tvm_table_reveal_rows -- and the host's sponge, replayed, agrees.  Host level:
the same proof word for word with the option on and off, the reference-pinned digest, the native verifier's acceptance."""
import ctypes as C

import numpy as np
import pytest

from triton_vm_amd import field, native_host, proof_tail, stark
from triton_vm_amd.arithmetic_domain import ArithmeticDomain
from triton_vm_amd.prover import Claim, ProofStream, Prover, StarkParameters


def _h(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _pointers(buffers):
    return (C.c_void_p * max(len(buffers), 1))(*[b.ptr for b in buffers])


def _default_rounds(log_n, checks):
    """Fri::num_rounds at expansion factor 4 (fri.rs:907-920; StarkParameters in the C++ host)"""
    return max(0, (log_n - 2) - (checks.bit_length() - 1) - 1)


def _gather_batch(ctx, jobs):
    """tvm_gather_elements_batch: jobs [(device pointer, words per element, element indices)] -> [array [n][words]]"""
    n = len(jobs)
    idx = [_h(j[2]).reshape(-1) for j in jobs]
    out = [np.zeros((len(i), j[1]), np.uint64) for i, j in zip(idx, jobs)]
    src, words, counts = (C.c_void_p * n)(*[j[0] for j in jobs]), np.array([j[1] for j in jobs], np.uint32), _h([len(i) for i in idx])
    p_idx, p_out = (C.c_void_p * n)(*[i.ctypes.data for i in idx]), (C.c_void_p * n)(*[o.ctypes.data for o in out])
    ctx._check(ctx.lib.tvm_gather_elements_batch(ctx.handle, n, src, words.ctypes.data, p_idx, counts.ctypes.data, p_out), "tvm_gather_elements_batch")
    return out


class _Tables:
    """three small random tables over `dom` with their trees: two through tvm_lde_table (a base-field and an extension-field one, in
    the coset-major storage order of the last LDE pass), one through tvm_quotient_segments (natural row order)"""

    def __init__(self, ctx, orc, rng, dom):
        L, n, h = dom.length, dom.length // 4, 3
        trace_dom = ArithmeticDomain.of_length(n)
        self.ctx, self.L, self.handles, self.keep = ctx, L, [], []
        for fk, n_cols in ((1, 7), (3, 5)):
            d_trace, d_rnd = ctx.to_device(orc.random_elements(rng, n_cols * n * fk)), ctx.to_device(orc.random_elements(rng, n_cols * h * fk))
            t = C.c_void_p()
            ctx._check(ctx.lib.tvm_lde_table(ctx.handle, fk, d_trace.ptr, n, n_cols, d_rnd.ptr, h, trace_dom.c(), dom.c(), C.byref(t)), "tvm_lde_table")
            self.handles.append(t.value)
        self.segments = stark.quotient_segments(ctx, ctx.to_device(orc.random_elements(rng, (L, 3))), dom, dom, orc.random_elements(rng, (4, 3)))
        self.handles.append(self.segments.table)
        self.widths = [7, 15, 15]
        self.trees = []
        for t in self.handles:
            d_nodes = ctx.alloc(10 * L)
            ctx._check(ctx.lib.tvm_table_merkle_tree(ctx.handle, t, L, d_nodes.ptr), "tvm_table_merkle_tree")
            self.trees.append(d_nodes)

    def reveal(self, which, indices):
        idx = _h(indices)
        out = np.zeros((len(idx), self.widths[which]), np.uint64)
        self.ctx._check(self.ctx.lib.tvm_table_reveal_rows(self.ctx.handle, self.handles[which], self.L, idx.ctypes.data, len(idx), out.ctypes.data),
                        "tvm_table_reveal_rows")
        return out

    def free(self):
        for t in self.handles[:2]:
            self.ctx.lib.tvm_table_free(self.ctx.handle, t)
        self.segments.free()
        for d_nodes in self.trees:
            d_nodes.free()


@pytest.fixture(scope="module")
def tables_of(ctx, orc):
    """one set of tables per domain, shared by the cases (they are only read) and freed before the context closes"""
    cache = {}

    def get(log_n, dom):
        if log_n not in cache:
            cache[log_n] = _Tables(ctx, orc, np.random.default_rng(log_n), dom)
        return cache[log_n]

    yield get
    for tables in cache.values():
        tables.free()


@pytest.mark.parametrize("log_n,n_rounds,checks", [(6, 0, 16), (6, 3, 16), (9, 0, 173), (9, 3, 16), (9, None, 16), (12, 0, 16), (12, 3, 173),
                                                   (12, None, 173), (12, None, 16)])
def test_every_item_equals_what_the_existing_calls_give(ctx, orc, tables_of, log_n, n_rounds, checks):
    lib, L = ctx.lib, 1 << log_n
    if n_rounds is None:
        n_rounds = _default_rounds(log_n, checks)
        assert n_rounds not in (0, 3)
    rng = np.random.default_rng(1000 * log_n + 10 * n_rounds + checks)
    dom = ArithmeticDomain.of_length(L).with_offset(field.to_mont(7))
    d_cw = ctx.to_device(orc.random_elements(rng, (L, 3)))
    d_cws = [ctx.alloc(3 * (L >> (r + 1))) for r in range(n_rounds)]
    d_nodes = [ctx.alloc(10 * (L >> r)) for r in range(n_rounds + 1)]
    state = orc.random_elements(rng, 16)
    roots, challenges = np.zeros((n_rounds + 1, 5), np.uint64), np.zeros((max(n_rounds, 1), 3), np.uint64)
    ctx._check(lib.tvm_fri_commit_phase(ctx.handle, d_cw.ptr, dom.c(), n_rounds, state.ctypes.data, _pointers(d_cws), _pointers(d_nodes),
                                        roots.ctypes.data, challenges.ctypes.data), "tvm_fri_commit_phase")
    ps = ProofStream(lib)   # the host's sponge, replayed
    ps.state[:] = state
    for r in range(n_rounds + 1):
        ps.enqueue(f"fri root {r}", roots[r])
        if r < n_rounds:
            assert (ps.sample_scalars(1)[0] == challenges[r]).all()
    tables = tables_of(log_n, dom)

    got = proof_tail.fri_query_and_open(ctx, ps.state, d_cw, dom, d_cws, d_nodes, checks, tables.handles, tables.trees)

    codewords, n_last = [d_cw] + d_cws, L >> n_rounds
    last = codewords[-1].download()[:3 * n_last].reshape(n_last, 3)
    last_poly = ArithmeticDomain.of_length(n_last).interpolate(ctx, codewords[-1], 3).download()[:3 * n_last].reshape(n_last, 3)
    ps.enqueue("fri last codeword", last, fiat_shamir=False)
    ps.enqueue("fri last polynomial", last_poly)
    a = ps.sample_indices(L, checks)
    assert got["indices"].tolist() == a and (got["state"] == ps.state).all()
    assert (got["last_codeword"] == last).all() and (got["last_polynomial"] == last_poly).all()
    jobs = []
    for r in range(n_rounds + 1):
        n = L >> r
        b = [(i % n + n // 2) % n for i in a]
        for which in ((a, b) if r == 0 else (b,)):
            if r == n_rounds and which is b:
                continue   # the last round answers nothing; when it is round 0, only `a`
            jobs += [(codewords[r].ptr, 3, which), (d_nodes[r].ptr, 5, stark.auth_node_indices(n, which))]
    trace_auth = stark.auth_node_indices(L, a)
    jobs += [(t.ptr, 5, trace_auth) for t in tables.trees]
    gathered = _gather_batch(ctx, jobs)
    want = gathered[:-3]
    for w in range(3):
        want += [tables.reveal(w, a), gathered[len(gathered) - 3 + w]]
    assert len(want) == proof_tail.tail_items(n_rounds) == len(got["payloads"]) == (8 if n_rounds == 0 else 2 * n_rounds + 8)
    offset = 0
    for k, (w, g) in enumerate(zip(want, got["payloads"])):
        assert got["directory"][k].tolist() == [offset, w.size], k
        assert (g == w.reshape(-1)).all(), k
        offset += w.size
    assert got["words"] == offset


def test_more_checks_than_the_limit_is_not_applicable(ctx, orc, tables_of):
    rng = np.random.default_rng(5)
    L = 64
    dom = ArithmeticDomain.of_length(L).with_offset(field.to_mont(7))
    d_cw, d_nodes = ctx.to_device(orc.random_elements(rng, (L, 3))), ctx.alloc(10 * L)
    ctx._check(ctx.lib.tvm_codeword_merkle_tree(ctx.handle, d_cw.ptr, L, d_nodes.ptr), "tvm_codeword_merkle_tree")
    tables = tables_of(6, dom)
    state = orc.random_elements(rng, 16)
    assert proof_tail.fri_query_and_open(ctx, state, d_cw, dom, [], [d_nodes], proof_tail.MAX_INDICES + 1, tables.handles, tables.trees) is None
    assert len(proof_tail.fri_query_and_open(ctx, state, d_cw, dom, [], [d_nodes], proof_tail.MAX_INDICES, tables.handles, tables.trees)["indices"]) == 1024


# ---------------------------------------------------------------------------------------------------- the C++ host
@pytest.fixture()
def host(ctx):
    from tests.test_native_host import _host_library

    lib = _host_library(ctx)
    assert lib.tvmh_get_option(native_host.OPTION_DEVICE_TAIL) == 0
    yield lib
    assert lib.tvmh_get_option(native_host.OPTION_DEVICE_TAIL) == 0   # whatever a test did, the option is off again


def _off_and_on(host, prove):
    """prove() with the option off and on -> (proof off, proof on, how many proofs took the device tail with it off / on)"""
    before = host.tvmh_device_tail_proofs()
    off = prove()
    between = host.tvmh_device_tail_proofs()
    with native_host.host_option(host, native_host.OPTION_DEVICE_TAIL, 1):
        on = prove()
    return off, on, between - before, host.tvmh_device_tail_proofs() - between


@pytest.mark.parametrize("log2_rows,h,checks", [(3, 3, 2), (4, 5, 4)])
def test_hot_path_proof_is_the_same_word_for_word(ctx, orc, host, log2_rows, h, checks):
    rng = np.random.default_rng(log2_rows)
    p = StarkParameters(log2_rows, num_trace_randomizers=h, num_collinearity_checks=checks)
    n = p.trace.length
    claim = Claim(orc.random_elements(rng, 5), orc.random_elements(rng, 3), orc.random_elements(rng, 2))
    py = Prover(ctx, p, orc.random_elements(rng, (379, n)), orc.random_elements(rng, (91, n, 3)), seed=9, claim=claim)
    native = native_host.NativeProver(ctx, host, p, py.main.d_trace, py.main.d_randomizers, py.aux.d_trace, py.aux.d_randomizers,
                                      py.quotient_randomizer, claim)
    off, on, taken_off, taken_on = _off_and_on(host, native.prove)
    assert (taken_off, taken_on) == (0, 1)
    assert off.size == on.size and (off == on).all()


def test_stir_proofs_keep_the_hosts_path(ctx, orc, host):
    if ctx.kind == "emu":
        pytest.skip("two STIR proofs at security level 160 take minutes on the emulation (CPU suite time); on the GPU")
    p = StarkParameters(3, ldt="stir")
    py = Prover(ctx, p, seed=12)
    native = native_host.NativeProver(ctx, host, p, py.main.d_trace, py.main.d_randomizers, py.aux.d_trace, py.aux.d_randomizers,
                                      py.quotient_randomizer)
    off, on, taken_off, taken_on = _off_and_on(host, native.prove)
    assert (taken_off, taken_on) == (0, 0)
    assert off.size == on.size and (off == on).all()


def test_proof_from_an_execution_trace_is_the_reference_pinned_one_and_verifies(ctx, orc, host):
    """the program, claim and seed of the reference's proof-digest snapshot (tests/test_proof_snapshot.py), FRI"""
    from tests import test_proof_snapshot as snap
    from tests import vm_fixture as vf
    from tests.test_fill import aet_arrays
    from triton_vm_amd.proof_stream import Proof

    program, aet, public_input, output = vf.run("tiny")
    claim, arrays = snap.claim_of(orc, program, public_input, output), aet_arrays(orc, aet)
    prove = lambda: native_host.prove_execution(ctx, host, arrays, aet.padded_height(), claim, snap.prover_seed(snap.SEED_U64), ldt="fri")
    if ctx.kind == "emu":   # (CPU suite time: the option-off proof of this trace is tests/test_native_host.py's, pinned by the same digest)
        with native_host.host_option(host, native_host.OPTION_DEVICE_TAIL, 1):
            taken, on = host.tvmh_device_tail_proofs(), prove()
        assert host.tvmh_device_tail_proofs() - taken == 1
    else:
        off, on, taken_off, taken_on = _off_and_on(host, prove)
        assert (taken_off, taken_on) == (0, 1)
        assert off.size == on.size and (off == on).all()
    assert Proof(on).digest(ctx.lib) == snap.SNAPSHOT
    assert len(native_host.verify(ctx, host, claim, on, ldt="fri")) == 173
