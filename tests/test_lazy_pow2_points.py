"""csrc/ntt_shift.h: the lazy forms of the 2^K-point transforms with shift twiddles -- sums folded wherever canon_plan allows it --
through tvm_field_op (k_pow2_points_lazy), against the canonical transform of the same hook (k_pow2_points), word for word after
reducing the lazy form's outputs mod p on the host:
  (a) on groups of canonical words from the edges of the carry chains: every all-equal group and 2^14 random draws of the set;
  (b) on the same groups with words >= p at exactly the input positions the plan declares free (the canonical transform is given
      those words reduced).
Outputs the form owes canonical are below p.  Every form the hook has: K = 2, 3, 4, decimation in time and in frequency, forward
and inverse roots, the 16-point transform at the shifted points 2^39, 2^78, 2^117, outputs owed canonical none / all."""
import numpy as np
import pytest

from triton_vm_amd import field

P, EPS = field.P, 0xFFFFFFFF
CANONICAL = np.array([0, 1, EPS - 1, EPS, EPS + 1, 1 << 32, 1 << 63, P - EPS, P - 2, P - 1], np.uint64)
ABOVE = np.array([P, P + 1, P + EPS - 2, (1 << 64) - 2, (1 << 64) - 1], np.uint64)   # p .. 2^64 - 1 holds 2^32 - 1 words: its edges
DRAWS = 1 << 14
FORMS = [(K, dit, inverse, 0) for K in (2, 3, 4) for dit in (1, 0) for inverse in (0, 1)] + [(4, 1, 0, s) for s in field.LAZY_SHIFTS]


def plan_of(K, dit, inverse, shift, owed_all):
    R = 1 << K
    return field.lazy_pow2_points_plan(K, dit, inverse, shift, (1 << R) - 1, ((1 << R) - 1) if owed_all else 0)


def free_inputs(K, dit, inverse, shift, owed_all):
    return [e for e in range(1 << K) if not plan_of(K, dit, inverse, shift, owed_all)["need_in"] >> e & 1]


# case (b) exists for the forms that declare an input free (a decimation-in-frequency butterfly subtracts one input from the other
# and, where the sum is owed canonical, adds them with bfe_add: those forms need every input canonical)
FORMS_WITH_FREE_INPUTS = [(*f, owed_all) for f in FORMS for owed_all in (0, 1) if free_inputs(*f, owed_all)]


def reduce(words):
    return np.where(words >= np.uint64(P), words - np.uint64(P), words)


def run(ctx, op, a):
    out, da = ctx.alloc(a.size), ctx.to_device(a)
    ctx._check(ctx.lib.tvm_field_op(ctx.handle, op, da.ptr, da.ptr, out.ptr, a.size), "field_op")
    return out.download()


def canonical_transform(ctx, K, dit, inverse, shift, groups):
    """the existing transform on canonical inputs; at shifted points it is the plain transform of x[e] 2^(shift brev(e))"""
    if shift:
        brev = lambda e: int(format(e, f"0{K}b")[::-1], 2)
        scale = [pow(2, shift * brev(e), P) for e in range(1 << K)]
        groups = np.array([[int(v) * scale[e] % P for e, v in enumerate(g)] for g in groups.tolist()], np.uint64)
    return run(ctx, field.pow2_points_op(K, dit, inverse), np.ascontiguousarray(groups).reshape(-1)).reshape(groups.shape)


@pytest.fixture(scope="module")
def cases(ctx):
    """per form: the canonical groups and the canonical transform's outputs on them, computed once"""
    made = {}

    def get(K, dit, inverse, shift):
        key = (K, dit, inverse, shift)
        if key not in made:
            R = 1 << K
            rng = np.random.default_rng(1000 * K + 100 * dit + 10 * inverse + shift)
            groups = np.concatenate([np.repeat(CANONICAL[:, None], R, axis=1), CANONICAL[rng.integers(0, CANONICAL.size, (DRAWS, R))]])
            made[key] = (groups, canonical_transform(ctx, K, dit, inverse, shift, groups))
        return made[key]

    return get


@pytest.mark.parametrize("owed_all", [0, 1])
@pytest.mark.parametrize("K,dit,inverse,shift", FORMS)
def test_lazy_form_on_canonical_groups(ctx, cases, K, dit, inverse, shift, owed_all):
    groups, want = cases(K, dit, inverse, shift)
    got = run(ctx, field.lazy_pow2_points_op(K, dit, inverse, owed_all, shift), groups.reshape(-1)).reshape(groups.shape)
    assert (reduce(got) == want).all()
    if owed_all:
        assert (got < np.uint64(P)).all()


@pytest.mark.parametrize("K,dit,inverse,shift,owed_all", FORMS_WITH_FREE_INPUTS)
def test_lazy_form_with_words_above_p_at_the_free_inputs(ctx, cases, K, dit, inverse, shift, owed_all):
    assert plan_of(K, dit, inverse, shift, owed_all)["ok"]
    free = free_inputs(K, dit, inverse, shift, owed_all)
    groups = cases(K, dit, inverse, shift)[0].copy()
    rng = np.random.default_rng(7 + K)
    head = len(CANONICAL)
    # the all-equal groups: each word above p at every free position in turn; the random draws: a random one at every free position
    groups[:head, free] = ABOVE[np.arange(head) % ABOVE.size][:, None]
    groups[head:, free] = ABOVE[rng.integers(0, ABOVE.size, (groups.shape[0] - head, len(free)))]
    assert (groups[:, free] >= np.uint64(P)).all()
    want = canonical_transform(ctx, K, dit, inverse, shift, reduce(groups))
    got = run(ctx, field.lazy_pow2_points_op(K, dit, inverse, owed_all, shift), groups.reshape(-1)).reshape(groups.shape)
    assert (reduce(got) == want).all()
    if owed_all:
        assert (got < np.uint64(P)).all()


def test_which_forms_declare_free_inputs():
    """every decimation-in-time form frees at least the inputs its first layer multiplies by a power of two other than 1 -- at the
    shifted points all eight of them -- whoever is owed the outputs"""
    for K, dit, inverse, shift in FORMS:
        for owed_all in (0, 1):
            free = free_inputs(K, dit, inverse, shift, owed_all)
            assert ((K, dit, inverse, shift, owed_all) in FORMS_WITH_FREE_INPUTS) == bool(free)
            if shift:
                assert set(range(1, 16, 2)) <= set(free)
