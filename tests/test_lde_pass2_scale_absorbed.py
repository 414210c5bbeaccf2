"""TVM_OPTION_LDE_PASS2_SCALE_ABSORBED (csrc/ntt.hip: k_lde_pass2_fused): the middle pass of the table extension without the
multiplication by the coset's factors in the coset loop -- classes of cosets whose factors differ by powers of two, the first
butterfly group at shifted points, the rest of the scale in the middle group's factor table.  The option must never change a word:
option 0 against option 1 through tvm_lde_table on the smallest height of every instantiation of the kernel, both against the oracle,
the generators the gate meets, and the forward-only route of the quotient segments."""
import numpy as np
import pytest

from triton_vm_amd import ArithmeticDomain, MasterTable, field, stark

N_COLS = 3
# the smallest height of every instantiation that contains the absorbed form (csrc/lde_plan.h): log2 rows -> LOGN of the kernel
HEIGHTS = {15: 8, 17: 9, 19: 10}   # (2^21 rows, 2048-point axes: that instantiation keeps the table form alone)
EXPANSIONS = (1, 2, 4, 8, 16, 32)   # one, two, four and eight classes of cosets; one, two and four cosets per class


def odom(orc, d):
    return orc.Domain(d.offset, d.generator, d.length)


def n1_of(log_n):
    return 1 << (log_n // 2)   # csrc/ntt.hip: split_for


def offsets():
    g = field.generator()
    return {"generator": g, "generator^5": field.mont_pow(g, 5), "random": int(np.random.default_rng(5).integers(2, field.P, dtype=np.uint64))}


@pytest.fixture
def absorbed(ctx, request):
    """switches the option on the module's context; the default comes back after the test"""
    request.addfinalizer(lambda: ctx.lde_pass2_scale_absorbed(False))
    return ctx.lde_pass2_scale_absorbed


@pytest.fixture(scope="module")
def inputs(ctx, orc):
    """inputs(log_n, fk) -> one random trace of three columns and n1 randomizer rows per height and field, on the host and in device
    memory: computed once, shared by the cases of a height, written by nobody"""
    made = {}

    def get(log_n, fk):
        if (log_n, fk) not in made:
            for key in [key for key in made if key[0] != log_n]:   # (the previous height's trace goes back to the pool)
                made.pop(key)[2].free()
            rng = np.random.default_rng(100 * log_n + fk)
            shape = lambda rows: (N_COLS, rows) + ((3,) if fk == 3 else ())
            trace, rnd = orc.random_elements(rng, shape(1 << log_n)), orc.random_elements(rng, shape(n1_of(log_n)))
            made[(log_n, fk)] = (trace, rnd, ctx.to_device(trace))
        return made[(log_n, fk)]

    yield get
    for _, _, d_trace in made.values():
        d_trace.free()


def sample_rows(rng, expansion, n):
    """every row up to 2^15 rows of trace, else the edges of the first block of cosets, the last row and 500 random ones"""
    L = expansion * n
    if n <= 1 << 15:
        return None
    edges = [0, 1, expansion - 1, expansion, L - 1]
    return np.unique(np.concatenate([[r for r in edges if 0 <= r < L], rng.integers(0, L, 500)])).astype(np.uint64)


def extension(ctx, d_trace, rnd, h, log_n, fk, ev, rows, trace_dom=None):
    n = 1 << log_n
    d_rnd = ctx.to_device(np.ascontiguousarray(rnd[:, :h])) if h else ctx.alloc(1)
    mt = MasterTable.from_device(ctx, d_trace, d_rnd, N_COLS, n, h, trace_dom or ArithmeticDomain.of_length(n), ev, ev, fk)
    mt.maybe_low_degree_extend_all_columns()
    got = mt.low_degree_extended_table() if rows is None else mt.reveal_rows(rows)
    mt.clear_cache()
    d_rnd.free()
    return got


def device_only(ctx, log_n, expansion=1):
    """the CPU emulation runs 2^15 rows in full and 2^17 rows up to eight cosets (two classes, four cosets per class); the device all"""
    if ctx.kind == "emu" and (log_n > 17 or (log_n == 17 and expansion > 8)):
        pytest.skip("CPU suite time: the 1024- and 2048-point axes, and 512-point axes with 16 and 32 cosets, run on the GPU")


@pytest.mark.parametrize("fk", [1, 3])
@pytest.mark.parametrize("expansion", EXPANSIONS)
@pytest.mark.parametrize("log_n", sorted(HEIGHTS))
def test_the_option_never_changes_the_table(ctx, orc, absorbed, inputs, log_n, expansion, fk):
    """option 0 against option 1, word for word: h = 0, 1, min(198, n1) and n1 randomizer rows (n1: the most the kernel takes), the
    field generator, its fifth power and a random element as the offset"""
    device_only(ctx, log_n, expansion)
    n, n1 = 1 << log_n, n1_of(log_n)
    trace, rnd, d_trace = inputs(log_n, fk)
    rows = sample_rows(np.random.default_rng(log_n + expansion), expansion, n)
    for name, offset in offsets().items():
        ev = ArithmeticDomain.of_length(expansion * n).with_offset(offset)
        for h in (0, 1, min(198, n1), n1):
            absorbed(False)
            want = extension(ctx, d_trace, rnd, h, log_n, fk, ev, rows)
            absorbed(True)
            got = extension(ctx, d_trace, rnd, h, log_n, fk, ev, rows)
            assert (got == want).all(), (name, h)


@pytest.mark.parametrize("log_n,expansion,fk,h", [(15, 2, 3, 1), (15, 8, 1, 128), (15, 32, 1, 0), (19, 8, 1, 198), (19, 4, 3, 512)])
def test_the_absorbed_form_against_the_oracle(ctx, orc, absorbed, inputs, log_n, expansion, fk, h):
    """the whole table at 2^15 rows, sampled rows at 2^19, with the option on"""
    device_only(ctx, log_n)
    n = 1 << log_n
    trace, rnd, d_trace = inputs(log_n, fk)
    ev = ArithmeticDomain.of_length(expansion * n).with_offset(field.generator())
    rows = sample_rows(np.random.default_rng(h), expansion, n)
    absorbed(True)
    got = extension(ctx, d_trace, rnd, h, log_n, fk, ev, rows)
    want = orc.lde_table(trace, np.ascontiguousarray(rnd[:, :h]), odom(orc, ev), fk)
    assert (got == (want if rows is None else want[rows.astype(np.int64)])).all()


@pytest.mark.parametrize("expansion", [2, 8])
def test_generators_that_are_not_the_domains_own(ctx, orc, absorbed, inputs, expansion):
    """The gate (csrc/ntt.hip: lde_table).  An evaluation generator w^(1 + n), w the domains' own root of order X n: the same trace
    domain, another order of the cosets -- the entry point accepts it, the table must be the oracle's and the option must not matter.
    The cube of the domains' generators (trace domain and evaluation domain alike, or the entry point refuses it) takes the generic
    kernels: the option must not matter either."""
    log_n, fk, h = 15, 1, 70
    n = 1 << log_n
    trace, rnd, d_trace = inputs(log_n, fk)
    own = ArithmeticDomain.of_length(expansion * n)
    ev = ArithmeticDomain(field.generator(), field.mont_pow(own.generator, 1 + n), own.length)
    assert field.mont_pow(ev.generator, expansion) == ArithmeticDomain.of_length(n).generator and ev.generator != own.generator
    want = orc.lde_table(trace, np.ascontiguousarray(rnd[:, :h]), odom(orc, ev), fk)
    for on in (False, True):
        absorbed(on)
        assert (extension(ctx, d_trace, rnd, h, log_n, fk, ev, None) == want).all(), on
    cubed = ArithmeticDomain(field.generator(), field.mont_pow(own.generator, 3), own.length)
    trace_cubed = ArithmeticDomain(field.ONE, field.mont_pow(ArithmeticDomain.of_length(n).generator, 3), n)
    tables = []
    for on in (False, True):
        absorbed(on)
        tables.append(extension(ctx, d_trace, rnd, h, log_n, fk, cubed, None, trace_dom=trace_cubed))
    assert (tables[0] == tables[1]).all()


@pytest.mark.parametrize("log_n,log_ldt,h", [(16, 18, 256), (18, 19, 1), (19, 22, 512)])
def test_the_forward_only_route_of_the_segments(ctx, orc, absorbed, log_n, log_ldt, h):
    """tvm_quotient_segments_from_coefficients hands the segments' coefficients to the forward half of the extension
    (TVM_LDE_FORWARD_ONLY) -- the same kernel: codewords and tree root with the option off and on, at the heights
    tests/test_segments_coefficient_route.py runs on the fused kernels"""
    if ctx.kind == "emu":
        pytest.skip("CPU suite time: the 256-, 512- and 1024-point axes of this route run on the GPU")
    n = 1 << log_n
    ldt = ArithmeticDomain.of_length(1 << log_ldt).with_offset(field.generator())
    q = orc.random_elements(np.random.default_rng(log_n), (4 * (n + h), 3))
    rnd = orc.random_elements(np.random.default_rng(h), (h, 3))
    d_q = ctx.to_device(q)
    results = []
    for on in (False, True):
        absorbed(on)
        qs = stark.quotient_segments_from_coefficients(ctx, d_q, len(q), ldt, rnd, n + h)
        results.append((qs.codewords(), qs.merkle_tree()[1].copy()))
        qs.free()
    d_q.free()
    assert (results[0][1] == results[1][1]).all()
    assert (results[0][0] == results[1][0]).all()
