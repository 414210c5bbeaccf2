"""Python binding of the C++ host side (triton_vm_amd/host/triton_host.cpp): `NativeProver.prove` runs the C++
`Prover::prove` mirror on device-resident traces and returns its transcript.  Used by the tests (the C++ and the
Python mirrors must produce the same transcript) and by bench.py, whose timed step is the C++ host by default."""
import ctypes as C

import numpy as np

from .build import build_host


def load_host_library(backend_path=None, out=None):
    lib = C.CDLL(build_host(backend_path, out))
    lib.tvmh_prove.restype = C.c_int32
    lib.tvmh_prove.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64,
                               C.POINTER(C.c_uint64), C.c_char_p, C.c_uint64]
    lib.tvmh_prove_execution.restype = C.c_int32
    lib.tvmh_prove_execution.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_void_p, C.c_void_p,
                                         C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_char_p,
                                         C.c_uint64]
    lib.tvmh_stir_prove.restype = C.c_int32
    from .capi import Domain

    lib.tvmh_stir_prove.argtypes = [C.c_void_p, Domain, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_char_p, C.c_uint64]
    lib.tvmh_stir_parameters.restype = C.c_uint64
    lib.tvmh_stir_parameters.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64]
    lib.tvmh_prove_execution_sharded.restype = C.c_int32
    lib.tvmh_prove_execution_sharded.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                 C.c_uint32, C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                                 C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]
    lib.tvmh_prove_sharded.restype = C.c_int32
    lib.tvmh_prove_sharded.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                       C.POINTER(C.c_uint64), C.c_char_p, C.c_uint64]
    lib.tvmh_check_execution.restype = C.c_int32
    lib.tvmh_check_execution.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                         C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_char_p,
                                         C.c_uint64]
    lib.tvmh_verify.restype = C.c_int32
    lib.tvmh_verify.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                C.c_void_p, C.c_char_p, C.c_uint64]
    lib.tvmh_verify_batch.restype = C.c_int32
    lib.tvmh_verify_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_char_p,
                                      C.c_uint64]
    lib.tvmh_proof_padded_height.restype = C.c_int32
    lib.tvmh_proof_padded_height.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    lib.tvmh_verdict_name.restype = C.c_char_p
    lib.tvmh_verdict_name.argtypes = [C.c_uint32]
    lib.tvmh_set_option.restype = None
    lib.tvmh_set_option.argtypes = [C.c_uint32, C.c_uint64]
    lib.tvmh_get_option.restype = C.c_uint64
    lib.tvmh_get_option.argtypes = [C.c_uint32]
    lib.tvmh_device_tail_proofs.restype = C.c_uint64
    lib.tvmh_device_tail_proofs.argtypes = []
    lib.tvmh_device_stir_proofs.restype = C.c_uint64
    lib.tvmh_device_stir_proofs.argtypes = []
    lib.tvmh_device_middle_proofs.restype = C.c_uint64
    lib.tvmh_device_middle_proofs.argtypes = []
    lib.tvmh_device_front_proofs.restype = C.c_uint64
    lib.tvmh_device_front_proofs.argtypes = []
    lib.tvmh_local_comms_create.restype = C.c_int32
    lib.tvmh_local_comms_create.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    lib.tvmh_local_comms_destroy.restype = None
    lib.tvmh_local_comms_destroy.argtypes = [C.c_void_p]
    lib.tvmh_local_comms_abort.restype = None
    lib.tvmh_local_comms_abort.argtypes = [C.c_void_p]
    lib.tvmh_local_comms_report.restype = C.c_uint64
    lib.tvmh_local_comms_report.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
    return lib


OPTION_EXACT_AIR = 1   # tvmh_set_option: prove_execution evaluates the AIR row by row instead of in valid-trace mode
OPTION_SHARE_REPLICATED_TABLES = 2   # in-process ranks use ONE copy of the replicated trace-side tables (triton_host.hpp)
OPTION_TRACE = 3   # host wall time of the steps of prove_execution on stderr
OPTION_COLUMN_SPLIT = 4   # k > 0: the sharded prover splits the inverse transforms by columns, coefficients exchanged in k chunks
OPTION_CHECK_TRACE = 5   # prove_execution checks the AIR on the trace first and proves a trace that fails in exact mode
OPTION_DEVICE_TAIL = 6   # single-GPU FRI proofs: the query phase and the trace openings in one device round trip (proof_tail.py)
OPTION_DEVICE_STIR = 7   # Stir::prove: all rounds in one call with the sponge on the device (stir_rounds.py)
OPTION_DEVICE_MIDDLE = 8   # single-GPU proofs: the quotient root, the out-of-domain rows, the combinations and DEEP in one device round trip (proof_middle.py)
OPTION_DEVICE_FRONT = 9    # single-GPU proofs: main root to the segment table queued without a wait, challenges and quotient weights made on the device (proof_front.py)
OPTION_VERIFY_BATCH_CHUNK = 10   # tvmh_verify_batch: jobs per chunk (0: the default, 16)


class host_option:
    """`with host_option(lib, OPTION_CHECK_TRACE, 1): ...` -- a process-wide switch of the C++ host (tvmh_set_option) for the calls
    inside the block; the previous value is restored on the way out, exception or not"""

    def __init__(self, host_lib, option, value):
        self.lib, self.option, self.value = host_lib, option, value

    def __enter__(self):
        self.previous = self.lib.tvmh_get_option(self.option)
        self.lib.tvmh_set_option(self.option, self.value)
        return self

    def __exit__(self, *exc):
        self.lib.tvmh_set_option(self.option, self.previous)
        return False


# ---- communicators for the sharded C++ host (triton_host.hpp: tvmh_comm) -----------------------------------------------
_COLLECTIVE = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
_HOOK = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)
_MARK = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_char_p)
_ABORT = C.CFUNCTYPE(None, C.c_void_p)
_SHARE = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_ASYNC = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32)
_WAIT = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_uint32)


class CommStruct(C.Structure):
    """struct tvmh_comm"""
    _fields_ = [("self", C.c_void_p), ("rank", C.c_uint32), ("world", C.c_uint32), ("all_gather", _COLLECTIVE), ("all_to_all", _COLLECTIVE),
                ("begin", _HOOK), ("mark", _MARK), ("end", _HOOK), ("abort", _ABORT), ("share", _SHARE),
                ("all_gather_async", _ASYNC), ("wait", _WAIT)]


class LocalComms:
    """`world` communicators between the contexts of THIS process, one proving thread per rank (tvmh_local_comms_create):
    collectives are a rendezvous plus device-to-device copies.  lockstep: one rank computes at a time and the per-rank,
    per-stage compute time is recorded (`report()`), which on one GPU measures what the ranks of a real run do concurrently."""

    def __init__(self, host_lib, world, lockstep=False):
        self.lib, self.world = host_lib, world
        arr = (C.c_void_p * world)()
        if host_lib.tvmh_local_comms_create(world, 1 if lockstep else 0, arr) != 0:
            raise RuntimeError("tvmh_local_comms_create failed")
        self.ptrs = [arr[r] for r in range(world)]

    def report(self):
        import json

        buf = C.create_string_buffer(1 << 16)
        self.lib.tvmh_local_comms_report(self.ptrs[0], buf, len(buf))
        return json.loads(buf.value.decode() or "{}")

    def abort(self):
        """a rank failed: release the ranks that wait for it in a collective (they report a device error)"""
        if self.ptrs:
            self.lib.tvmh_local_comms_abort(self.ptrs[0])

    def close(self):
        if self.ptrs:
            self.lib.tvmh_local_comms_destroy(self.ptrs[0])
            self.ptrs = []


class RcclComm:
    """The production communicator: RCCL collectives on the context's stream (triton_vm_amd/host/rccl_comm.cpp).  One per
    rank; `unique_id` is drawn on rank 0 (RcclComm.unique_id) and handed to the other ranks by the launcher's channel."""

    _lib = None

    @classmethod
    def library(cls):
        if cls._lib is None:
            from .build import build_rccl

            lib = C.CDLL(build_rccl())
            lib.tvmh_rccl_unique_id.restype = C.c_int32
            lib.tvmh_rccl_unique_id.argtypes = [C.c_void_p]
            lib.tvmh_rccl_comm_create.restype = C.c_int32
            lib.tvmh_rccl_comm_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(C.c_void_p)]
            lib.tvmh_rccl_comm_destroy.restype = None
            lib.tvmh_rccl_comm_destroy.argtypes = [C.c_void_p]
            lib.tvmh_rccl_last_error.restype = C.c_char_p
            cls._lib = lib
        return cls._lib

    @classmethod
    def unique_id(cls):
        out = np.zeros(128, np.uint8)
        if cls.library().tvmh_rccl_unique_id(out.ctypes.data) != 0:
            raise RuntimeError("ncclGetUniqueId: " + cls.library().tvmh_rccl_last_error().decode())
        return out

    def __init__(self, unique_id, rank, world, device):
        lib = self.library()
        uid = np.ascontiguousarray(unique_id, dtype=np.uint8)
        assert uid.size == 128
        ptr = C.c_void_p()
        if lib.tvmh_rccl_comm_create(uid.ctypes.data, rank, world, device, C.byref(ptr)) != 0:
            raise RuntimeError("tvmh_rccl_comm_create: " + lib.tvmh_rccl_last_error().decode())
        self.ptr, self.rank, self.world = ptr.value, rank, world

    def close(self):
        if self.ptr:
            self.library().tvmh_rccl_comm_destroy(self.ptr)
            self.ptr = None


class CallbackComm:
    """A tvmh_comm whose collectives are Python callables over (send pointer, receive pointer, words) -- the CPU tests put
    torch.distributed's gloo backend behind it (the "device" buffers of the emulation are host memory)."""

    def __init__(self, rank, world, all_gather, all_to_all):
        def wrap(fn):
            def call(_self, _ctx, send, recv, words):
                try:
                    fn(send, recv, int(words))
                    return 0
                except Exception:   # noqa: BLE001 -- reported to the C++ host as a device error, with the traceback on stderr
                    import traceback

                    traceback.print_exc()
                    return 3
            return _COLLECTIVE(call)

        self._keep = (wrap(all_gather), wrap(all_to_all))
        self.struct = CommStruct(None, rank, world, self._keep[0], self._keep[1], _HOOK(), _MARK(), _HOOK(), _ABORT(), _SHARE(), _ASYNC(), _WAIT())
        self.ptr = C.addressof(self.struct)


def gloo_comm(dist):
    """CallbackComm over an initialised torch.distributed gloo group, for buffers in host memory (the CPU emulation)"""
    import torch

    rank, world = dist.get_rank(), dist.get_world_size()

    def view(ptr, words):
        return torch.from_numpy(np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int64)), shape=(words,)))

    def all_gather(send, recv, words):
        dist.all_gather_into_tensor(view(recv, words * world), view(send, words).clone())

    def all_to_all(send, recv, words):   # gloo has no all-to-all on CPU tensors: one all-gather of everything, then this rank's blocks
        everything = torch.empty(world * world * words, dtype=torch.int64)
        dist.all_gather_into_tensor(everything, view(send, words * world).clone())
        out = view(recv, words * world)
        for r in range(world):
            out[r * words:(r + 1) * words] = everything[(r * world + rank) * words:(r * world + rank + 1) * words]

    return CallbackComm(rank, world, all_gather, all_to_all)


def prove_execution_sharded(ctx, host_lib, comm_ptr, aet, padded_height, claim, randomness_seed, security_level=160, log2_expansion=2,
                            ldt=None, jit_passes=0, split_tree_min_leaves=1 << 21, profile=False):
    """The C++ host's Prover::prove(claim, aet) over the ranks of a communicator (comm_ptr: a tvmh_comm*, or None for this
    process alone) and / or coset by coset (jit_passes; 0 = the reference's memory policy: cached, else as few passes as fit).
    -> (proof words, stats dict)"""
    import json

    from .master_table import aet_struct

    s, keep = aet_struct(aet)
    log2 = padded_height.bit_length() - 1
    err, stats, n = C.create_string_buffer(512), C.create_string_buffer(1 << 14), C.c_uint64(0)
    out = getattr(_PROOF_BUFFERS, "buffer", None)   # one buffer per proving thread, kept between calls (its pages are mapped)
    if out is None:
        out = np.empty(1 << 20, np.uint64)
    while True:
        rc = host_lib.tvmh_prove_execution_sharded(ctx.handle, comm_ptr, jit_passes, split_tree_min_leaves, C.addressof(s), log2, security_level,
                                                   log2_expansion, {"fri": 0, "stir": 1, None: 2}[ldt], bytes(randomness_seed),
                                                   claim.program_digest.ctypes.data, claim.input.ctypes.data, claim.input.size,
                                                   claim.output.ctypes.data, claim.output.size, out.ctypes.data, out.size, C.byref(n),
                                                   1 if profile else 0, stats, len(stats), err, len(err))
        if rc != 0:
            raise NativeHostError(rc, f"tvmh_prove_execution_sharded failed ({rc}): {err.value.decode()}")
        if n.value <= out.size:
            _PROOF_BUFFERS.buffer = out
            return out[:n.value].copy(), json.loads(stats.value.decode() or "{}")
        out = np.empty(int(n.value), np.uint64)


def prove_sharded(ctx, host_lib, comm_ptr, params, d_main_trace, d_main_randomizers, d_aux_trace, d_aux_randomizers, quotient_randomizer,
                  jit_passes=1, split_tree_min_leaves=1 << 21, stir_security_level=160):
    """The hot path alone (as NativeProver.prove) through the sharded / coset-wise C++ prover -> proof words"""
    qr = np.ascontiguousarray(quotient_randomizer, dtype=np.uint64).reshape(-1, 3)
    err, n = C.create_string_buffer(512), C.c_uint64(0)
    out = np.empty(1 << 20, np.uint64)
    log2 = params.padded_height.bit_length() - 1
    while True:
        rc = host_lib.tvmh_prove_sharded(ctx.handle, comm_ptr, jit_passes, split_tree_min_leaves, log2, params.h, params.num_collinearity_checks,
                                         params.log2_expansion, d_main_trace.ptr, d_main_randomizers.ptr, d_aux_trace.ptr, d_aux_randomizers.ptr,
                                         qr.ctypes.data, 1 if params.stir is not None else 0, stir_security_level, out.ctypes.data, out.size,
                                         C.byref(n), err, len(err))
        if rc != 0:
            raise NativeHostError(rc, f"tvmh_prove_sharded failed ({rc}): {err.value.decode()}")
        if n.value <= out.size:
            return out[:n.value].copy()
        out = np.empty(int(n.value), np.uint64)


class NativeHostError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


def stir_parameters(host_lib, padded_height, security_level=160, log2_expansion=2):
    """Stark::stir's instance as the C++ host derives it -> dict"""
    out = np.zeros(128, np.uint64)
    n = host_lib.tvmh_stir_parameters(padded_height, security_level, log2_expansion, out.ctypes.data, out.size)
    if not n:
        raise RuntimeError("tvmh_stir_parameters failed")
    rounds = int(out[4])
    return dict(domain_length=int(out[0]), folding_factor=int(out[1]), final_num_in_domain_queries=int(out[2]), final_degree=int(out[3]),
                round_queries=[(int(out[5 + 2 * r]), int(out[6 + 2 * r])) for r in range(rounds)])


def stir_prove(ctx, host_lib, stir, d_codeword):
    """the C++ host's Stir::prove for the instance `stir` (low_degree_test.Stir) -> (first-round indices, proof words of a
    stream that holds only the STIR items)"""
    rounds = np.array(stir.round_queries, np.uint64).reshape(-1, 2)
    n_first = stir.num_first_round_queries()
    first, out = np.zeros(n_first, np.uint64), np.empty(1 << 20, np.uint64)
    err, n = C.create_string_buffer(512), C.c_uint64(0)
    rc = host_lib.tvmh_stir_prove(ctx.handle, stir.initial_domain.c(), stir.folding_factor, rounds.ctypes.data, len(rounds),
                                  stir.final_num_in_domain_queries, stir.final_degree, d_codeword.ptr, first.ctypes.data, out.ctypes.data,
                                  out.size, C.byref(n), err, len(err))
    if rc != 0 or n.value > out.size:
        raise RuntimeError(f"tvmh_stir_prove failed ({rc}): {err.value.decode()}")
    return [int(i) for i in first], out[:n.value].copy()


_PROOF_BUFFERS = __import__("threading").local()   # one buffer per proving thread: ctypes releases the GIL inside the C++ host,
#                                                     and the backend's contract is one context per proving thread


def prove_execution(ctx, host_lib, aet, padded_height, claim, randomness_seed, security_level=160, log2_expansion=2, ldt=None):
    """The C++ host's Prover::prove(claim, aet) (triton_vm::prove_execution): fill, pad, extend and the hot path on the
    device, the seeded randomness and the transcript in C++.  aet: the arrays master_table.fill takes (host arrays, or
    master_table.aet_to_device's device-resident copy).  ldt: "fri", "stir" or None = Stark::ldt's rule (STIR from 2^16 padded
    rows on, stark.rs:1944-1951).  -> the proof words"""
    from .master_table import aet_struct

    s, keep = aet_struct(aet)
    log2 = padded_height.bit_length() - 1
    err, n = C.create_string_buffer(512), C.c_uint64(0)
    out = getattr(_PROOF_BUFFERS, "buffer", None)
    if out is None:
        out = np.empty(1 << 20, np.uint64)   # a 2^20-row proof is ~0.3 M words
    while True:
        rc = host_lib.tvmh_prove_execution(ctx.handle, C.addressof(s), log2, security_level, log2_expansion, {"fri": 0, "stir": 1, None: 2}[ldt],
                                           bytes(randomness_seed),
                                           claim.program_digest.ctypes.data, claim.input.ctypes.data, claim.input.size,
                                           claim.output.ctypes.data, claim.output.size, out.ctypes.data, out.size, C.byref(n), err, len(err))
        if rc != 0:
            raise RuntimeError(f"tvmh_prove_execution failed ({rc}): {err.value.decode()}")
        if n.value <= out.size:
            _PROOF_BUFFERS.buffer = out               # (kept: its pages are mapped by now)
            return out[:n.value].copy()
        out = np.empty(int(n.value), np.uint64)   # the proof did not fit: grow and run again


def check_execution(ctx, host_lib, aet, padded_height, claim, seed, capacity=1024):
    """tvmh_check_execution: the device's fill, pad and extend of `aet` (as prove_execution builds the trace; challenges drawn from
    `seed`, 32 bytes, and derived from `claim`), then the AIR on that trace (tvm_check_constraints).  No proof.
    -> (the number of failing rows, [(row, section, constraint index)] of the lowest failing rows, at most `capacity` entries)"""
    from .capi import constraint_section
    from .master_table import aet_struct

    s, keep = aet_struct(aet)
    log2 = padded_height.bit_length() - 1
    out = np.zeros((max(capacity, 1), 2), np.uint64)
    err, n_fail, failing = C.create_string_buffer(512), C.c_uint64(0), C.c_uint64(0)
    rc = host_lib.tvmh_check_execution(ctx.handle, C.addressof(s), log2, bytes(seed), claim.program_digest.ctypes.data, claim.input.ctypes.data,
                                       claim.input.size, claim.output.ctypes.data, claim.output.size, capacity, out.ctypes.data,
                                       C.byref(n_fail), C.byref(failing), err, len(err))
    if rc != 0:
        raise NativeHostError(rc, f"tvmh_check_execution failed ({rc}): {err.value.decode()}")
    return failing.value, [(int(r), constraint_section(int(i)), int(i)) for r, i in out[:n_fail.value]]


VERIFY_STAGES = ("decode", "transcript and out-of-domain AIR", "low-degree test", "Merkle inclusion", "row digests", "DEEP values")


def verify_verdict(ctx, host_lib, claim, proof_words, security_level=160, log2_expansion=2, ldt=None):
    """tvmh_verify as it is: -> (status, verdict code, variant name, indices, {stage: ms}); no exception for a rejection"""
    words = np.ascontiguousarray(proof_words, dtype=np.uint64).reshape(-1)
    digest = np.ascontiguousarray(claim.program_digest, dtype=np.uint64)
    public_input, output = np.ascontiguousarray(claim.input, dtype=np.uint64), np.ascontiguousarray(claim.output, dtype=np.uint64)
    verdict, n, err = C.c_uint32(0xFFFFFFFF), C.c_uint64(0), C.create_string_buffer(256)
    indices, stages = np.zeros(1 << 12, np.uint64), np.zeros(len(VERIFY_STAGES), np.float64)
    rc = host_lib.tvmh_verify(ctx.handle, words.ctypes.data, words.size, digest.ctypes.data, claim.version, public_input.ctypes.data,
                              public_input.size, output.ctypes.data, output.size, security_level, log2_expansion,
                              {"fri": 0, "stir": 1, None: 2}[ldt], C.byref(verdict), indices.ctypes.data, indices.size, C.byref(n),
                              stages.ctypes.data, err, len(err))
    return rc, verdict.value, err.value.decode(), [int(i) for i in indices[:min(n.value, indices.size)]], dict(zip(VERIFY_STAGES, stages.tolist()))


def verify(ctx, host_lib, claim, proof_words, security_level=160, log2_expansion=2, ldt=None):
    """The C++ host's Verifier::verify (triton_vm::Verifier, host/verifier.cpp) with the per-query work on the device.  claim: a
    proof_stream.Claim; ldt: "fri", "stir" or None = Stark::ldt's rule.  -> the revealed first-round indices; raises
    verifier.VerificationError carrying the variant's name on a rejection, NativeHostError on a bad argument or a device failure."""
    from .verifier import VerificationError

    rc, verdict, name, indices, _ = verify_verdict(ctx, host_lib, claim, proof_words, security_level, log2_expansion, ldt)
    if rc != 0:
        raise NativeHostError(rc, f"tvmh_verify failed ({rc}): {name}")
    if verdict != 0:
        raise VerificationError(name)
    return indices


class VerifyJob(C.Structure):
    """struct tvmh_verify_job"""
    _fields_ = [("h_proof", C.c_void_p), ("proof_words", C.c_uint64), ("h_program_digest", C.c_void_p), ("version", C.c_uint32),
                ("h_public_input", C.c_void_p), ("n_public_input", C.c_uint64), ("h_public_output", C.c_void_p), ("n_public_output", C.c_uint64),
                ("security_level", C.c_uint32), ("log2_expansion", C.c_uint32), ("ldt_choice", C.c_uint32)]


def verify_job(claim, proof_words, security_level=160, log2_expansion=2, ldt=None):
    """one job of verify_batch: (claim, proof words, parameters as verify takes them); ldt may also be the number tvmh_verify takes"""
    return (claim, proof_words, security_level, log2_expansion, ldt)


def verify_batch_verdicts(ctx, host_lib, jobs, indices_stride=1 << 12):
    """tvmh_verify_batch as it is.  jobs: [verify_job(...)] -> (status, error text, [verdict code], [indices of job i, [] unless accepted
    and within the stride], [number of indices], {stage: ms summed over the batch}); no exception for a rejection.  A proof given as None
    is passed as a null pointer with the length 1 (an argument error)."""
    n = len(jobs)
    array, keep = (VerifyJob * max(n, 1))(), []
    for i, (claim, proof_words, security_level, log2_expansion, ldt) in enumerate(jobs):
        words = None if proof_words is None else np.ascontiguousarray(proof_words, dtype=np.uint64).reshape(-1)
        digest = np.ascontiguousarray(claim.program_digest, dtype=np.uint64)
        public_input, output = np.ascontiguousarray(claim.input, dtype=np.uint64), np.ascontiguousarray(claim.output, dtype=np.uint64)
        keep.append((words, digest, public_input, output))
        array[i] = VerifyJob(None if words is None else words.ctypes.data, 1 if words is None else words.size, digest.ctypes.data, claim.version,
                             public_input.ctypes.data, public_input.size, output.ctypes.data, output.size, security_level, log2_expansion,
                             ldt if isinstance(ldt, int) else {"fri": 0, "stir": 1, None: 2}[ldt])
    verdicts, counts = np.full(max(n, 1), 0xFFFFFFFF, np.uint32), np.full(max(n, 1), 0xFFFFFFFFFFFFFFFF, np.uint64)
    indices = np.full((max(n, 1), max(indices_stride, 1)), 0xFFFFFFFFFFFFFFFF, np.uint64)
    stages, err = np.zeros(len(VERIFY_STAGES), np.float64), C.create_string_buffer(256)
    rc = host_lib.tvmh_verify_batch(ctx.handle, C.addressof(array), n, verdicts.ctypes.data, indices.ctypes.data if indices_stride else None,
                                    indices_stride, counts.ctypes.data, stages.ctypes.data, err, len(err))
    revealed = [[int(v) for v in indices[i, :counts[i]]] if rc == 0 and verdicts[i] == 0 and counts[i] <= indices_stride else [] for i in range(n)]
    return rc, err.value.decode(), [int(v) for v in verdicts[:n]], revealed, [int(v) for v in counts[:n]], dict(zip(VERIFY_STAGES, stages.tolist()))


def verify_batch(ctx, host_lib, jobs):
    """The C++ host's Verifier::verify for many proofs in one call, the device work shared between them (tvmh_verify_batch,
    host/verify_batch.cpp).  jobs: [verify_job(claim, proof_words, ...)] -> per job the revealed first-round indices, or the
    verifier.VerificationError that verify() would raise for it (returned, not raised: a rejected job does not hide the others);
    raises NativeHostError on a bad argument or a device failure."""
    from .verifier import VerificationError

    rc, error, verdicts, revealed, _, _ = verify_batch_verdicts(ctx, host_lib, jobs)
    if rc != 0:
        raise NativeHostError(rc, f"tvmh_verify_batch failed ({rc}): {error}")
    return [indices if verdict == 0 else VerificationError(host_lib.tvmh_verdict_name(verdict).decode()) for verdict, indices in zip(verdicts, revealed)]


def proof_padded_height(host_lib, proof_words):
    """Proof::padded_height through the C++ decoder (proof.rs:45-59); raises proof_stream.ProofDecodingError"""
    from .proof_stream import ProofDecodingError

    words = np.ascontiguousarray(proof_words, dtype=np.uint64).reshape(-1)
    verdict, height = C.c_uint32(0), C.c_uint64(0)
    if host_lib.tvmh_proof_padded_height(words.ctypes.data, words.size, C.byref(verdict), C.byref(height)) != 0:
        raise RuntimeError("tvmh_proof_padded_height failed")
    if verdict.value:
        raise ProofDecodingError(host_lib.tvmh_verdict_name(verdict.value).decode())
    return int(height.value)


class NativeProver:
    """Same constructor data as triton_vm_amd.prover.Prover (device traces, device randomizers, the quotient randomizer,
    the claim); `prove()` returns the proof: the words of the reference's `Proof`."""

    def __init__(self, ctx, host_lib, params, d_main_trace, d_main_randomizers, d_aux_trace, d_aux_randomizers,
                 quotient_randomizer, claim=None):
        from .proof_stream import Claim

        self.ctx, self.lib, self.p = ctx, host_lib, params
        self.bufs = (d_main_trace, d_main_randomizers, d_aux_trace, d_aux_randomizers)  # keep them alive
        self.qr = np.ascontiguousarray(quotient_randomizer, dtype=np.uint64).reshape(-1, 3)
        assert self.qr.shape[0] == params.num_quotient_randomizers
        self.claim = claim or Claim()
        self.capacity = 1 << 21   # words; a 2^20-row proof (173 opened rows of 3 tables + authentication nodes) is ~0.4 M words
        self.out = np.empty(self.capacity, np.uint64)

    def prove(self, parse=True):
        p, claim = self.p, self.claim
        log2 = p.padded_height.bit_length() - 1
        err = C.create_string_buffer(512)
        n = C.c_uint64(0)
        while True:
            rc = self.lib.tvmh_prove(self.ctx.handle, log2, p.h, p.num_collinearity_checks, p.log2_expansion, self.bufs[0].ptr, self.bufs[1].ptr,
                                     self.bufs[2].ptr, self.bufs[3].ptr, self.qr.ctypes.data, claim.program_digest.ctypes.data,
                                     claim.input.ctypes.data, claim.input.size, claim.output.ctypes.data, claim.output.size,
                                     1 if p.stir is not None else 0, self.out.ctypes.data, self.capacity, C.byref(n), err, len(err))
            if rc != 0:
                raise RuntimeError(f"tvmh_prove failed ({rc}): {err.value.decode()}")
            if n.value <= self.capacity:
                break
            self.capacity = int(n.value)      # the proof did not fit: grow and run again
            self.out = np.empty(self.capacity, np.uint64)
        return self.out[:n.value].copy() if parse else None
