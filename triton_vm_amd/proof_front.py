"""The front of a proof with the transcript on the device, over the C ABI (csrc/proof_front.hip): the main root into the sponge and the
63 challenges, the aux root into the sponge and the 604 quotient weights, in a block of device memory the caller owns -- and the entry
points that take challenges and weights from device memory (the _device_args twins), which is where that block leaves them.  Thin
wrappers: device buffers and host arrays in, host arrays out (the C++ host's ProofSteps::prove is the product caller under
TVMH_OPTION_DEVICE_FRONT, the tests are the other; the Python Prover keeps the host's path)."""
import ctypes as C

import numpy as np

from .stark import NOT_APPLICABLE, ZETA

MAIN_ROOT, AUX_ROOT, CHALLENGES, WEIGHT_SCALAR, STATE, HEAD_WORDS, WEIGHTS, BLOCK_WORDS = 0, 5, 10, 199, 202, 218, 218, 2030   # TVM_FRONT_*
NUM_CHALLENGES, NUM_QUOTIENT_WEIGHTS = 63, 604


def _h(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _ptr(b):
    return getattr(b, "ptr", b)


def split_block(block):
    """the front's block (or its head alone), by the offsets of include/triton_hip.h (TVM_FRONT_*)"""
    at, out = 0, {}
    for name, shape in (("main_root", (5,)), ("aux_root", (5,)), ("challenges", (NUM_CHALLENGES, 3)), ("weight_scalar", (3,)),
                        ("state", (16,)), ("weights", (NUM_QUOTIENT_WEIGHTS, 3))):
        n = int(np.prod(shape))
        if at + n > block.size:
            break
        out[name] = block[at:at + n].reshape(shape)
        at += n
    assert at == block.size and at in (HEAD_WORDS, BLOCK_WORDS)
    return out


def alloc_block(ctx):
    """a front block: TVM_FRONT_BLOCK_WORDS words of device memory"""
    assert ctx.lib.tvm_front_block_words() == BLOCK_WORDS
    return ctx.alloc(BLOCK_WORDS)


def front_challenges(ctx, d_main_nodes, sponge_state, program_digest, public_input, public_output, d_front):
    """tvm_front_challenges: queued, not waited for.  The claim's words: Montgomery words, as Claim holds them."""
    state, digest, inp, out = _h(sponge_state).reshape(16), _h(program_digest).reshape(5), _h(public_input).ravel(), _h(public_output).ravel()
    ctx._check(ctx.lib.tvm_front_challenges(ctx.handle, _ptr(d_main_nodes), state.ctypes.data, digest.ctypes.data,
                                            inp.ctypes.data if inp.size else None, inp.size, out.ctypes.data if out.size else None, out.size,
                                            _ptr(d_front)), "tvm_front_challenges")


def front_quotient_weights(ctx, d_aux_nodes, d_front):
    """tvm_front_quotient_weights: queued, not waited for"""
    ctx._check(ctx.lib.tvm_front_quotient_weights(ctx.handle, _ptr(d_aux_nodes), _ptr(d_front)), "tvm_front_quotient_weights")


def front_block(ctx, d_front, n_words=BLOCK_WORDS, wait=True, out=None):
    """tvm_front_block -> the block's first n_words words; wait=False: the array is valid after the context's next synchronisation"""
    block = np.zeros(n_words, np.uint64) if out is None else out
    ctx._check(ctx.lib.tvm_front_block(ctx.handle, _ptr(d_front), block.ctypes.data, n_words, 1 if wait else 0), "tvm_front_block")
    return block


def extend_aux_table_device_args(ctx, d_main_trace, d_aux_trace, n_rows, d_challenges):
    ctx._check(ctx.lib.tvm_extend_aux_table_device_args(ctx.handle, _ptr(d_main_trace), _ptr(d_aux_trace), n_rows, _ptr(d_challenges)),
               "tvm_extend_aux_table_device_args")


def fill_derived_aux_columns_device_args(ctx, d_main_trace, d_aux_trace, n_rows, d_challenges):
    ctx._check(ctx.lib.tvm_fill_derived_aux_columns_device_args(ctx.handle, _ptr(d_main_trace), _ptr(d_aux_trace), n_rows, _ptr(d_challenges)),
               "tvm_fill_derived_aux_columns_device_args")


def all_quotients_combined_device_args(ctx, main_table, aux_table, trace_domain, quotient_domain, d_challenges, d_weights):
    """tvm_all_quotients_combined_device_args -> the quotient codeword, a DeviceBuffer"""
    out = ctx.alloc(quotient_domain.length * 3)
    ctx._check(ctx.lib.tvm_all_quotients_combined_device_args(ctx.handle, main_table._need_table(), aux_table._need_table(), trace_domain.c(),
                                                              quotient_domain.c(), _ptr(d_challenges), _ptr(d_weights), out.ptr),
               "tvm_all_quotients_combined_device_args")
    return out


def all_quotients_coefficients_device_args(ctx, main_table, aux_table, trace_domain, quotient_domain, d_challenges, d_weights, capacity=None):
    """tvm_all_quotients_coefficients_device_args -> (DeviceBuffer of `capacity` XFE, the number of coefficients written), or None
    where the remainder route does not apply (TVM_NOT_APPLICABLE)"""
    capacity = quotient_domain.length if capacity is None else capacity
    out, n = ctx.alloc(capacity * 3), C.c_uint64(0)
    status = ctx.lib.tvm_all_quotients_coefficients_device_args(ctx.handle, main_table._need_table(), aux_table._need_table(), trace_domain.c(),
                                                                quotient_domain.c(), _ptr(d_challenges), _ptr(d_weights), out.ptr, capacity,
                                                                C.byref(n))
    if status == NOT_APPLICABLE:
        out.free()
        return None
    try:
        ctx._check(status, "tvm_all_quotients_coefficients_device_args")
    except Exception:
        out.free()
        raise
    return out, n.value


def out_of_domain_to_deep_device_state(ctx, d_main_trace, n_main, d_main_randomizers, d_aux_trace, n_aux, d_aux_randomizers, n_rows, h,
                                       trace_domain, d_polys, poly_len, segments, d_quotient_nodes, short_domain, d_sponge_state, zeta=ZETA):
    """tvm_out_of_domain_to_deep_device_state: proof_middle.out_of_domain_to_deep with the sponge state in device memory (16 words, read,
    and left holding the state after the combination weights) -> (the DEEP codeword, the block as proof_middle.split_block's dict)"""
    from . import proof_middle

    block = np.zeros(proof_middle.block_words(n_main, n_aux), np.uint64)
    d_out = ctx.alloc(3 * short_domain.length)
    ctx._check(ctx.lib.tvm_out_of_domain_to_deep_device_state(ctx.handle, _ptr(d_main_trace), n_main, _ptr(d_main_randomizers), _ptr(d_aux_trace),
                                                              n_aux, _ptr(d_aux_randomizers), n_rows, h, trace_domain.c(), _ptr(d_polys), poly_len,
                                                              segments, _ptr(d_quotient_nodes), short_domain.c(), zeta, _ptr(d_sponge_state),
                                                              d_out.ptr, block.ctypes.data, block.size), "tvm_out_of_domain_to_deep_device_state")
    return d_out, proof_middle.split_block(block, n_main, n_aux)
