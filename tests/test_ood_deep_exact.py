"""Out-of-domain rows and DEEP word for word against the oracle at the shapes where their indexing can go wrong (csrc/poly.hip:
k_ood_weights -- a run of rows per work-item, one base-field inversion per run and point --, k_column_dot -- a base-field row's
operands loaded a row ahead --, k_deep -- one base-field inversion for the norms of sixteen denominators -- and csrc/proof_middle.hip:
k_deep_dev, the same body with its operands in device memory).  Everything is exact field arithmetic: canonical words, equality.
Once on the CPU emulation of the kernel sources and once on the real device (-m gpu), as tests/test_kernels_poly.py."""
import numpy as np
import pytest

from triton_vm_amd import ArithmeticDomain, MasterTable, field, proof_middle, stark


def _odom(orc, d):
    return orc.Domain(d.offset, d.generator, d.length)


# rows: fewer than a wavefront, one wavefront, several workgroups of weights, and 2^14 -- two row chunks at the small chunk length
# (2^13, what a table of fewer than 64 column groups gets); the entry point takes powers of two only.
# columns: fewer than, equal to and not a multiple of the columns a workgroup owns (2 base-field, 1 extension-field), and many groups.
@pytest.mark.parametrize("h", [0, 5])
@pytest.mark.parametrize("fk", [1, 3])
@pytest.mark.parametrize("n_cols", [1, 2, 3, 7, 130])
@pytest.mark.parametrize("log_n", [4, 6, 10, 14])
def test_out_of_domain_rows_exact(ctx, orc, log_n, n_cols, fk, h):
    """1, 2 and 3 points (the kernel takes two per pass: a full pass, a pass with one, and both) against the oracle's row per point"""
    rng = np.random.default_rng(1000 * log_n + 10 * n_cols + fk + 7 * h)
    n = 1 << log_n
    shape = lambda k: (n_cols, k) + ((3,) if fk == 3 else ())
    trace, rnd = orc.random_elements(rng, shape(n)), orc.random_elements(rng, shape(h))
    ev = ArithmeticDomain.of_length(4 * n).with_offset(field.generator())
    mt = MasterTable(ctx, trace, rnd, ArithmeticDomain.of_length(n), ev, ev, fk)
    pts = orc.random_elements(rng, (3, 3))
    want = np.stack([orc.out_of_domain_row(trace, rnd, pts[p], fk) for p in range(3)])
    for n_points in (1, 2, 3):
        got = mt.out_of_domain_rows(pts[:n_points])
        assert got.shape == (n_points, n_cols, 3)
        assert (got == want[:n_points]).all(), (n_points, np.argwhere(got != want[:n_points])[:4])


_DEEP_REFERENCE = {}


def _deep_reference(orc, log_n):
    """four random codewords on a domain of 2^log_n points with their (point, value, weight) triples, and the weighted DEEP
    component of each from the oracle -- computed once per length and shared by the cases"""
    if log_n not in _DEEP_REFERENCE:
        rng = np.random.default_rng(50 + log_n)
        dom = ArithmeticDomain.of_length(1 << log_n).with_offset(field.generator())
        cws = [orc.random_elements(rng, (len(dom), 3)) for _ in range(4)]
        pts, vals, ws = (orc.random_elements(rng, (4, 3)) for _ in range(3))
        terms = []
        for k in range(4):
            comp = orc.deep_codeword(cws[k], _odom(orc, dom), pts[k], vals[k])
            terms.append(np.stack([orc.xfe_mul(comp[i], ws[k]) for i in range(len(dom))]))
        _DEEP_REFERENCE[log_n] = (dom, cws, pts, vals, ws, terms)
    return _DEEP_REFERENCE[log_n]


# lengths: 2 (one point per work-item), 4 and 8 (one and two work-items of four points), 64, 512 and 1024 (part of and exactly one
# workgroup of 256 work-items x 4 points), 4096 (several workgroups); a domain's length is a power of two, so the length that is
# no multiple of batch x workgroup is the one below it.
@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("log_n", [1, 2, 3, 6, 9, 10, 12])
def test_deep_codeword_exact(ctx, orc, log_n, k):
    """tvm_deep_codeword and tvm_deep_codeword_device_args against each other and against the oracle"""
    dom, cws, pts, vals, ws, terms = _deep_reference(orc, log_n)
    want = terms[0].copy()
    for j in range(1, k):
        want = np.stack([orc.xfe_add(want[i], terms[j][i]) for i in range(len(dom))])
    bufs = [ctx.to_device(c) for c in cws[:k]]
    host_args = stark.deep_codeword(ctx, bufs, dom, pts[:k], vals[:k], ws[:k]).download((len(dom), 3))
    device_args = proof_middle.deep_codeword_device_args(ctx, bufs, dom, ctx.to_device(pts[:k]), ctx.to_device(vals[:k]),
                                                         ctx.to_device(ws[:k])).download((len(dom), 3))
    assert (host_args == want).all(), np.argwhere(host_args != want)[:4]
    assert (device_args == host_args).all(), np.argwhere(device_args != host_args)[:4]
