"""The middle of a proof with the transcript on the device, over the C ABI (csrc/proof_middle.hip): from the quotient's Merkle root to
the DEEP codeword in one call, and tvm_deep_codeword with its small operands in device memory.  Thin wrappers: device buffers and host
arrays in, host arrays out (the C++ host's ProofSteps::prove is the product caller under TVMH_OPTION_DEVICE_MIDDLE, the tests are the
other; the Python Prover keeps the host's path)."""
import ctypes as C

import numpy as np

from .stark import ZETA


def _h(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _ptr(b):
    return getattr(b, "ptr", b)


def block_words(n_main, n_aux):
    """TVM_MIDDLE_BLOCK_WORDS"""
    return 84 + 6 * (n_main + n_aux)


def split_block(block, n_main, n_aux):
    """the block tvm_out_of_domain_to_deep hands back, by the offsets of include/triton_hip.h (TVM_MIDDLE_*)"""
    at, out = 0, {}
    for name, shape in (("root", (5,)), ("points", (4, 3)), ("main_rows", (2, n_main, 3)), ("aux_rows", (2, n_aux, 3)),
                        ("segments", (5, 2, 3)), ("values", (4, 3)), ("weights", (3, 3)), ("state", (16,))):
        n = int(np.prod(shape))
        out[name] = block[at:at + n].reshape(shape)
        at += n
    assert at == block.size == block_words(n_main, n_aux)
    return out


def out_of_domain_to_deep(ctx, d_main_trace, n_main, d_main_randomizers, d_aux_trace, n_aux, d_aux_randomizers, n_rows, h, trace_domain,
                          d_polys, poly_len, segments, d_quotient_nodes, short_domain, sponge_state, zeta=ZETA):
    """tvm_out_of_domain_to_deep.  The traces and their randomizers: column-major device arrays (DeviceBuffers or pointers);
    d_polys / segments: the five segment polynomials and their table handle; d_quotient_nodes: the tree over that table, or None
    when sponge_state already holds its root.  -> (the DEEP codeword on short_domain, a DeviceBuffer; the block as a dict: root,
    points [4][3], main_rows / aux_rows [2][n][3], segments [5][2][3], values [4][3], weights [3][3], state [16])"""
    state = _h(sponge_state).reshape(16)
    block = np.zeros(block_words(n_main, n_aux), np.uint64)
    assert block.size == ctx.lib.tvm_out_of_domain_to_deep_block_words(n_main, n_aux)
    d_out = ctx.alloc(3 * short_domain.length)
    ctx._check(ctx.lib.tvm_out_of_domain_to_deep(ctx.handle, _ptr(d_main_trace), n_main, _ptr(d_main_randomizers), _ptr(d_aux_trace), n_aux,
                                                 _ptr(d_aux_randomizers), n_rows, h, trace_domain.c(), _ptr(d_polys), poly_len, segments,
                                                 _ptr(d_quotient_nodes), short_domain.c(), zeta, state.ctypes.data, d_out.ptr,
                                                 block.ctypes.data, block.size), "tvm_out_of_domain_to_deep")
    return d_out, split_block(block, n_main, n_aux)


def deep_codeword_device_args(ctx, d_codewords, domain, d_points, d_values, d_weights):
    """tvm_deep_codeword_device_args: stark.deep_codeword with the points, values and weights (len(d_codewords) XFE each) in device
    memory -> the codeword, a DeviceBuffer"""
    k = len(d_codewords)
    ptrs = (C.c_void_p * max(k, 1))(*[_ptr(b) for b in d_codewords])
    out = ctx.alloc(domain.length * 3)
    ctx._check(ctx.lib.tvm_deep_codeword_device_args(ctx.handle, k, ptrs, domain.c(), _ptr(d_points), _ptr(d_values), _ptr(d_weights),
                                                     out.ptr), "tvm_deep_codeword_device_args")
    return out


def combination_weight_vectors(ctx, scalars, segments, n_columns):
    """tvm_combination_weight_vectors: the weight vectors of the linear combinations from w0, w1, w2 [3][3] and the segment values
    [5][2][3] -> dict(w_columns [n_columns][3], wp [5][3], wr [5][3], wd [4][3], pr_values [2][3])"""
    sc, seg = _h(scalars).reshape(3, 3), _h(segments).reshape(5, 2, 3)
    out = dict(w_columns=np.zeros((n_columns, 3), np.uint64), wp=np.zeros((5, 3), np.uint64), wr=np.zeros((5, 3), np.uint64),
               wd=np.zeros((4, 3), np.uint64), pr_values=np.zeros((2, 3), np.uint64))
    ctx._check(ctx.lib.tvm_combination_weight_vectors(ctx.handle, sc.ctypes.data, seg.ctypes.data, n_columns, *[a.ctypes.data for a in out.values()]),
               "tvm_combination_weight_vectors")
    return out
