"""Python mirror of the reed-solomon-novelpoly crate surface over the C ABI.

This is plumbing for tests and the bench: every call goes through
``libnovelpoly_hip.so`` (include/novelpoly.h), whose work runs in HIP kernels
on a gfx950 GPU.  There is no CPU fallback: if the library is missing or no
MI355X is visible, calls raise.

Names follow the crate (paths relative to /root/reference/reed-solomon-novelpoly):

* :func:`encode` / :func:`reconstruct`        -- src/novel_poly_basis/{encode,reconstruct}.rs
* :class:`CodeParams`, :class:`ReedSolomon`    -- src/novel_poly_basis/mod.rs:24-285
* :class:`WrappedShard`                        -- src/wrapped_shard.rs
* :class:`Error` and its variants              -- src/errors.rs:4-28
* :func:`recoverablity_subset_size` etc.       -- src/util.rs
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import List, Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.abspath(os.path.join(_HERE, "..", ".."))
# NP_LIB_PATH: an experiment build of the same library (tools/exp_variants.sh)
LIB_PATH = os.environ.get("NP_LIB_PATH") or os.path.join(PKG_ROOT, "lib", "libnovelpoly_hip.so")
FIELD_SIZE = 65536

_sz = C.c_size_t
_lib = None
_lib_lock = threading.Lock()


class _Params(C.Structure):
    _fields_ = [("n", _sz), ("k", _sz), ("wanted_n", _sz)]


class RaggedItem(C.Structure):
    """np_ragged_item: one payload of a ragged device batch (offsets into the
    caller's buffers, lengths in bytes)."""

    _fields_ = [("payload_off", C.c_uint64), ("payload_len", C.c_uint64), ("shards_off", C.c_uint64),
                ("shard_len", C.c_uint64)]


def lib() -> C.CDLL:
    """Load libnovelpoly_hip.so (fails loudly if it was not built)."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not built; run `make -C {PKG_ROOT}` (hipcc, gfx950)")
        L = C.CDLL(LIB_PATH)
        P = C.POINTER(_Params)
        vp = C.c_void_p
        sig = {
            "np_last_error_detail": (None, [C.POINTER(_sz)]),
            "np_last_error_site": (C.c_char_p, []),
            "np_status_message": (C.c_char_p, [C.c_int]),
            "np_version": (C.c_char_p, []),
            "np_recoverability_subset_size": (_sz, [_sz]),
            "np_derive_parameters": (C.c_int, [_sz, _sz, P]),
            "np_params_new": (C.c_int, [_sz, _sz, _sz, P]),
            "np_shard_len": (_sz, [P, _sz]),
            "np_is_fast_path": (C.c_int, [P]),
            "np_kernel_family": (C.c_int, [P, _sz, C.c_int]),
            "np_ctx_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
            "np_ctx_destroy": (None, [vp]),
            "np_ctx_stream": (vp, [vp]),
            "np_ctx_device": (C.c_int, [vp]),
            "np_ctx_synchronize": (C.c_int, [vp]),
            "np_encode": (C.c_int, [vp, C.c_char_p, _sz, _sz, vp, _sz]),
            "np_rs_encode": (C.c_int, [vp, P, C.c_char_p, _sz, vp, _sz]),
            "np_reconstruct": (C.c_int, [vp, C.POINTER(vp), C.POINTER(_sz), _sz, _sz, vp, _sz, C.POINTER(_sz)]),
            "np_rs_reconstruct": (C.c_int, [vp, P, C.POINTER(vp), C.POINTER(_sz), _sz, vp, _sz, C.POINTER(_sz)]),
            "np_rs_reconstruct_from_systematic": (
                C.c_int, [vp, P, C.POINTER(vp), C.POINTER(_sz), _sz, vp, _sz, C.POINTER(_sz)]),
            "np_encode_batch_dev": (C.c_int, [vp, P, vp, _sz, _sz, _sz, vp, _sz, vp]),
            "np_reconstruct_batch_dev": (C.c_int, [vp, P, vp, _sz, _sz, vp, _sz, vp, _sz, vp]),
            "np_reconstruct_batch_dev3": (C.c_int, [vp, P, vp, _sz, _sz, vp, vp, _sz, vp, _sz, vp, vp]),
            "np_reconstruct_batch_dev2": (C.c_int, [vp, P, vp, _sz, _sz, vp, vp, _sz, vp, _sz, vp]),
            "np_reconstruct_codewords_batch_dev": (C.c_int, [vp, P, vp, _sz, _sz, vp, _sz, vp, _sz, vp, vp]),
            "np_restore_shards_batch_dev": (C.c_int, [vp, P, vp, _sz, _sz, vp, _sz, vp, vp]),
            "np_rs_restore_shards": (C.c_int, [vp, P, C.POINTER(vp), C.POINTER(_sz), _sz, C.POINTER(vp), _sz]),
            "np_verify_shards_batch_dev": (C.c_int, [vp, P, vp, _sz, _sz, vp, _sz, vp, vp, vp, vp]),
            "np_rs_verify_shards": (C.c_int, [vp, P, C.POINTER(vp), C.POINTER(_sz), _sz, C.POINTER(_sz), vp]),
            "np_recover_batch_dev": (C.c_int, [vp, P, vp, _sz, _sz, vp, _sz, vp, _sz, C.c_int, vp, vp, vp, vp]),
            "np_rs_recover": (C.c_int, [vp, P, C.POINTER(vp), C.POINTER(_sz), _sz, vp, _sz, C.POINTER(_sz),
                                        C.POINTER(vp), _sz, C.POINTER(_sz), vp]),
            "np_encode_ragged_dev": (C.c_int, [vp, P, vp, _sz, vp, _sz, C.POINTER(RaggedItem), _sz, vp]),
            "np_reconstruct_ragged_dev": (C.c_int, [vp, P, vp, _sz, vp, vp, _sz, C.POINTER(RaggedItem), _sz, vp, vp]),
            "np_restore_shards_ragged_dev": (C.c_int, [vp, P, vp, _sz, vp, C.POINTER(RaggedItem), _sz, vp, vp]),
            "np_verify_shards_ragged_dev": (C.c_int, [vp, P, vp, _sz, vp, C.POINTER(RaggedItem), _sz, vp, vp, vp, vp]),
            "np_recover_ragged_dev": (C.c_int, [vp, P, vp, _sz, vp, vp, _sz, C.POINTER(RaggedItem), _sz, C.c_int, vp,
                                                vp, vp, vp]),
            "np_ragged_plan": (C.c_int, [P, C.POINTER(RaggedItem), _sz, C.c_int, _sz, _sz, C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint32), _sz, C.POINTER(_sz)]),
            "np_error_locator_dev": (C.c_int, [vp, _sz, vp, _sz, vp, vp]),
            "np_reconstruct_from_systematic_batch_dev": (C.c_int, [vp, P, vp, _sz, _sz, _sz, vp, _sz, vp]),
            "np_encode_batch_host": (C.c_int, [vp, P, vp, _sz, _sz, _sz, vp, _sz]),
            "np_reconstruct_batch_host": (C.c_int, [vp, P, vp, _sz, _sz, vp, _sz, vp, _sz]),
            "np_recover_batch_host": (C.c_int, [vp, P, vp, _sz, _sz, vp, _sz, vp, _sz, C.c_int, vp, vp, vp]),
            "np_batch_split": (None, [_sz, _sz, _sz, C.POINTER(_sz), C.POINTER(_sz)]),
            "np_encode_batch_multi": (C.c_int, [C.POINTER(vp), _sz, P, C.POINTER(vp), _sz, _sz, _sz, C.POINTER(vp), _sz]),
            "np_reconstruct_batch_multi": (C.c_int, [C.POINTER(vp), _sz, P, C.POINTER(vp), _sz, _sz, C.POINTER(vp), _sz,
                                                     C.POINTER(vp), _sz, C.POINTER(vp)]),
            "np_encode_batch_host_multi": (C.c_int, [C.POINTER(vp), _sz, P, vp, _sz, _sz, _sz, vp, _sz]),
            "np_reconstruct_batch_host_multi": (C.c_int, [C.POINTER(vp), _sz, P, vp, _sz, _sz, vp, _sz, vp, _sz]),
            "np_recover_batch_multi": (C.c_int, [C.POINTER(vp), _sz, P, C.POINTER(vp), _sz, _sz, C.POINTER(vp), _sz,
                                                 C.POINTER(vp), _sz, C.c_int, C.POINTER(vp), C.POINTER(vp),
                                                 C.POINTER(vp)]),
            "np_recover_batch_host_multi": (C.c_int, [C.POINTER(vp), _sz, P, vp, _sz, _sz, vp, _sz, vp, _sz, C.c_int, vp,
                                                      vp, vp]),
            "np_afft_dev": (C.c_int, [vp, vp, _sz, _sz, _sz, vp]),
            "np_inverse_afft_dev": (C.c_int, [vp, vp, _sz, _sz, _sz, vp]),
            "np_walsh_dev": (C.c_int, [vp, vp, _sz, vp]),
            "np_mul_dev": (C.c_int, [vp, vp, vp, vp, _sz, vp]),
            "np_encode_low_dev": (C.c_int, [vp, vp, _sz, vp, _sz, _sz, vp]),
            "np_decode_main_dev": (C.c_int, [vp, vp, _sz, vp, vp, _sz, _sz, vp]),
            "np_debug_bounds_check": (C.c_int, [vp, C.POINTER(C.c_uint32)]),
            "np_pin_registry_stats": (None, [C.POINTER(_sz)]),
        }
        for name, (res, args) in sig.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
        return L


# ----------------------------------------------------------------- errors ----
class Error(Exception):
    """errors.rs:4 `Error`."""

    code = -1

    def __init__(self, *fields):
        self.fields = fields
        super().__init__(self._msg())

    def _msg(self) -> str:
        return f"{type(self).__name__}{self.fields}"

    def __eq__(self, other):
        return type(self) is type(other) and self.fields == other.fields

    def __hash__(self):
        return hash((type(self), self.fields))


class WantedShardCountTooHigh(Error):
    code = 1


class WantedShardCountTooLow(Error):
    code = 2


class WantedPayloadShardCountTooLow(Error):
    code = 3


class PayloadSizeIsZero(Error):
    code = 4


class NeedMoreShards(Error):
    code = 5

    @property
    def have(self):
        return self.fields[0]

    @property
    def min(self):
        return self.fields[1]

    @property
    def all(self):
        return self.fields[2]


class ParamterMustBePowerOf2(Error):
    code = 6


class InconsistentShardLengths(Error):
    code = 7


class EmptyShard(Error):
    code = 8


class InvalidArgument(Error):
    """A case the crate `assert!`s on (the C ABI reports it instead of panicking)."""

    code = 100


class DeviceError(Error):
    code = 101


_BY_CODE = {cls.code: cls for cls in (WantedShardCountTooHigh, WantedShardCountTooLow,
                                      WantedPayloadShardCountTooLow, PayloadSizeIsZero, NeedMoreShards,
                                      ParamterMustBePowerOf2, InconsistentShardLengths, EmptyShard,
                                      InvalidArgument)}
_ARITY = {1: 1, 2: 1, 3: 1, 4: 0, 5: 3, 6: 2, 7: 2, 8: 0}


def _raise(st: int):
    if st == 0:
        return
    det = (_sz * 3)()
    lib().np_last_error_detail(det)
    cls = _BY_CODE.get(st)
    if cls is None:
        msg = lib().np_status_message(st).decode()
        if st in (DeviceError.code, 102):  # NP_ERR_DEVICE / NP_ERR_ALLOC: the failing HIP call
            msg += f" [{lib().np_last_error_site().decode()}]"
        raise DeviceError(st, msg)
    raise cls(*tuple(det)[: _ARITY.get(st, 3)])


# ------------------------------------------------------------------ util ----
def recoverablity_subset_size(n_wanted_shards: int) -> int:
    """util.rs:40 (the crate's spelling)."""
    return int(lib().np_recoverability_subset_size(n_wanted_shards))


recoverability_subset_size = recoverablity_subset_size


def is_power_of_2(x: int) -> bool:
    return x > 0 and (x & (x - 1)) == 0


def next_higher_power_of_2(k: int) -> int:
    return k if is_power_of_2(k) else 1 << k.bit_length()


def next_lower_power_of_2(k: int) -> int:
    return k if is_power_of_2(k) else 1 << (k.bit_length() - 1)


# --------------------------------------------------------------- context ----
class Context:
    """One HIP device + stream + uploaded field tables (np_ctx)."""

    def __init__(self, device: int = -1):
        h = C.c_void_p()
        _raise(lib().np_ctx_create(device, C.byref(h)))
        self.handle = h

    @property
    def stream(self) -> int:
        return lib().np_ctx_stream(self.handle) or 0

    @property
    def device(self) -> int:
        return lib().np_ctx_device(self.handle)

    def synchronize(self):
        _raise(lib().np_ctx_synchronize(self.handle))

    def close(self):
        if self.handle:
            lib().np_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx: dict = {}


def default_context(device: int = -1) -> Context:
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


# ---------------------------------------------------------------- shards ----
class WrappedShard:
    """wrapped_shard.rs:2-78: a byte vector padded to an even length."""

    __slots__ = ("inner",)

    def __init__(self, data: bytes):
        data = bytes(data)
        if len(data) & 1:
            data += b"\x00"
        self.inner = data

    def into_inner(self) -> bytes:
        return self.inner

    def __bytes__(self):
        return self.inner

    def __len__(self):
        return len(self.inner)

    def __eq__(self, other):
        return isinstance(other, WrappedShard) and other.inner == self.inner

    def __repr__(self):
        return f"WrappedShard({self.inner!r})"


def _as_bytes(s) -> bytes:
    if isinstance(s, WrappedShard):
        return s.inner
    return bytes(s)


def _shard_arrays(shards):
    m = len(shards)
    ptrs = (C.c_void_p * max(1, m))()
    lens = (_sz * max(1, m))()
    keep = []
    for i, s in enumerate(shards):
        if s is None:
            ptrs[i] = None
            lens[i] = 0
        else:
            b = _as_bytes(s)
            buf = C.create_string_buffer(b, max(1, len(b)))
            keep.append(buf)
            ptrs[i] = C.cast(buf, C.c_void_p)
            lens[i] = len(b)
    return ptrs, lens, keep


# ---------------------------------------------------------- code params ----
class CodeParams:
    """mod.rs:24-88."""

    __slots__ = ("_n", "_k", "wanted_n")

    def __init__(self, n: int, k: int, wanted_n: int):
        self._n, self._k, self.wanted_n = n, k, wanted_n

    @staticmethod
    def derive_parameters(n: int, k: int) -> "CodeParams":
        p = _Params()
        _raise(lib().np_derive_parameters(n, k, C.byref(p)))
        return CodeParams(p.n, p.k, p.wanted_n)

    def n(self) -> int:
        return self._n

    def k(self) -> int:
        return self._k

    def is_faster8(self) -> bool:
        """True when a specialised gfx950 kernel serves (n, k)."""
        return bool(lib().np_is_fast_path(C.byref(self._c())))

    def make_encoder(self, ctx: Optional[Context] = None) -> "ReedSolomon":
        return ReedSolomon(self._n, self._k, self.wanted_n, ctx=ctx)

    def _c(self) -> _Params:
        return _Params(self._n, self._k, self.wanted_n)

    def __eq__(self, other):
        return isinstance(other, CodeParams) and (self._n, self._k, self.wanted_n) == (
            other._n, other._k, other.wanted_n)

    def __repr__(self):
        return f"CodeParams(n={self._n}, k={self._k}, wanted_n={self.wanted_n})"


# enum np_kernel_family (include/novelpoly.h)
FAMILY_GENERIC, FAMILY_SMALL, FAMILY_FAST, FAMILY_RES, FAMILY_BIG, FAMILY_HUGE = range(6)
FAMILY_NAMES = ("GENERIC", "SMALL", "FAST", "RES", "BIG", "HUGE")


def kernel_family(params: CodeParams, shard_len: int, reconstruct: bool) -> int:
    """np_kernel_family: the kernel family (FAMILY_*) an encode, or with
    `reconstruct` a reconstruct, of rows of `shard_len` bytes runs on in this
    process; -1 for invalid parameters.  Needs no device."""
    return int(lib().np_kernel_family(C.byref(params._c()), shard_len, 1 if reconstruct else 0))


class ReedSolomon:
    """mod.rs:91-285."""

    def __init__(self, n: int, k: int, wanted_n: int, ctx: Optional[Context] = None):
        p = _Params()
        _raise(lib().np_params_new(n, k, wanted_n, C.byref(p)))
        self.n, self.k, self.wanted_n = n, k, wanted_n
        self._p = p
        self.ctx = ctx or default_context()

    def params(self) -> CodeParams:
        return CodeParams(self.n, self.k, self.wanted_n)

    def shard_len(self, payload_size: int) -> int:
        return int(lib().np_shard_len(C.byref(self._p), payload_size))

    def encode(self, data: bytes, shard_type=bytes) -> List:
        data = bytes(data)
        if not data:
            _raise(PayloadSizeIsZero.code)
        sl = self.shard_len(len(data))
        out = C.create_string_buffer(max(1, self.wanted_n * sl))
        _raise(lib().np_rs_encode(self.ctx.handle, C.byref(self._p), data, len(data), out, sl))
        raw = out.raw
        return [shard_type(raw[v * sl:(v + 1) * sl]) for v in range(self.wanted_n)]

    def reconstruct(self, received: Sequence[Optional[bytes]]) -> bytes:
        ptrs, lens, keep = _shard_arrays(received)
        maxsyms = max([(len(_as_bytes(s)) + 1) // 2 for s in received if s is not None] or [0])
        cap = max(1, maxsyms * 2 * self.k)
        out = C.create_string_buffer(cap)
        olen = _sz()
        _raise(lib().np_rs_reconstruct(self.ctx.handle, C.byref(self._p), ptrs, lens, len(received), out, cap,
                                       C.byref(olen)))
        return out.raw[: olen.value]

    def restore_shards(self, received: Sequence[Optional[bytes]]) -> List[bytes]:
        """All ``wanted_n`` shards of ``encode(reconstruct(received))``: the
        received ones as given (padded to an even length), the absent ones
        restored (np_rs_restore_shards)."""
        ptrs, lens, keep = _shard_arrays(received)
        sl = 2 * max([(len(_as_bytes(s)) + 1) // 2 for s in received[: self.n] if s is not None] or [0])
        absent =[i for i in range(self.wanted_n) if i >= len(received) or received[i] is None]
        bufs = {i: C.create_string_buffer(max(1, sl)) for i in absent}
        outs = (C.c_void_p * max(1, self.wanted_n))()
        for i, b in bufs.items():
            outs[i] = C.cast(b, C.c_void_p)
        _raise(lib().np_rs_restore_shards(self.ctx.handle, C.byref(self._p), ptrs, lens, len(received), outs, sl))
        return [bufs[i].raw[:sl] if i in bufs else WrappedShard(_as_bytes(received[i])).inner
                for i in range(self.wanted_n)]

    def mismatched_shards(self, received: Sequence[Optional[bytes]]) -> List[int]:
        """The indices of the received shards that differ from
        ``encode(reconstruct(received))`` (np_rs_verify_shards; odd lengths are
        compared zero padded).  They are the rows that differ from the
        re-encoding, not necessarily the rows that were altered.  Raises as
        :meth:`reconstruct` does."""
        ptrs, lens, keep = _shard_arrays(received)
        bad = _sz(0)
        flags = C.create_string_buffer(max(1, self.n))
        _raise(lib().np_rs_verify_shards(self.ctx.handle, C.byref(self._p), ptrs, lens, len(received), C.byref(bad),
                                         C.cast(flags, C.c_void_p)))
        rows = [i for i, f in enumerate(flags.raw[: self.n]) if f]
        assert len(rows) == bad.value
        return rows

    def verify(self, received: Sequence[Optional[bytes]]) -> bool:
        """True when every received shard equals its row of
        ``encode(reconstruct(received))`` (np_rs_verify_shards).  Always true
        with exactly k shards.  Raises as :meth:`reconstruct` does."""
        ptrs, lens, keep = _shard_arrays(received)
        bad = _sz(0)
        _raise(lib().np_rs_verify_shards(self.ctx.handle, C.byref(self._p), ptrs, lens, len(received), C.byref(bad),
                                         None))
        return bad.value == 0

    def recover(self, received: Sequence[Optional[bytes]]):
        """``(payload, shards, mismatched_rows)`` from one staging and one decode
        of ``received`` (np_rs_recover): what :meth:`reconstruct`,
        :meth:`restore_shards` and :meth:`mismatched_shards` return, each
        exactly.  Raises as :meth:`reconstruct` does."""
        ptrs, lens, keep = _shard_arrays(received)
        syms = max([(len(_as_bytes(s)) + 1) // 2 for s in received[: self.n] if s is not None] or [0])
        sl, cap = 2 * syms, max(1, syms * 2 * self.k)
        out = C.create_string_buffer(cap)
        olen = _sz()
        absent = [i for i in range(self.wanted_n) if i >= len(received) or received[i] is None]
        bufs = {i: C.create_string_buffer(max(1, sl)) for i in absent}
        outs = (C.c_void_p * max(1, self.wanted_n))()
        for i, b in bufs.items():
            outs[i] = C.cast(b, C.c_void_p)
        bad = _sz(0)
        flags = C.create_string_buffer(max(1, self.n))
        _raise(lib().np_rs_recover(self.ctx.handle, C.byref(self._p), ptrs, lens, len(received), C.cast(out, C.c_void_p),
                                   cap, C.byref(olen), outs, sl, C.byref(bad), C.cast(flags, C.c_void_p)))
        shards = [bufs[i].raw[:sl] if i in bufs else WrappedShard(_as_bytes(received[i])).inner
                  for i in range(self.wanted_n)]
        rows = [i for i, f in enumerate(flags.raw[: self.n]) if f]
        assert len(rows) == bad.value
        return out.raw[: olen.value], shards, rows

    def reconstruct_from_systematic(self, chunks: Sequence[bytes]) -> bytes:
        ptrs, lens, keep = _shard_arrays(chunks)
        maxsyms = max([(len(_as_bytes(s)) + 1) // 2 for s in chunks] or [0])
        cap = max(1, maxsyms * 2 * self.k)
        out = C.create_string_buffer(cap)
        olen = _sz()
        _raise(lib().np_rs_reconstruct_from_systematic(self.ctx.handle, C.byref(self._p), ptrs, lens, len(chunks),
                                                       out, cap, C.byref(olen)))
        return out.raw[: olen.value]


def encode(data: bytes, n_min: int, shard_type=bytes, ctx: Optional[Context] = None) -> List:
    """encode.rs:6-11."""
    params = CodeParams.derive_parameters(n_min, recoverablity_subset_size(n_min))
    return params.make_encoder(ctx).encode(data, shard_type=shard_type)


def reconstruct(received: Sequence[Optional[bytes]], validator_count: int, ctx: Optional[Context] = None) -> bytes:
    """reconstruct.rs:4-9."""
    params = CodeParams.derive_parameters(validator_count, recoverablity_subset_size(validator_count))
    return params.make_encoder(ctx).reconstruct(received)


def restore_shards(received: Sequence[Optional[bytes]], validator_count: int,
                   ctx: Optional[Context] = None) -> List[bytes]:
    """All ``validator_count`` shards from the received ones (:meth:`ReedSolomon.restore_shards`),
    with the code :func:`reconstruct` derives."""
    params = CodeParams.derive_parameters(validator_count, recoverablity_subset_size(validator_count))
    return params.make_encoder(ctx).restore_shards(received)


def verify(received: Sequence[Optional[bytes]], validator_count: int, ctx: Optional[Context] = None) -> bool:
    """Whether the received shards are consistent (:meth:`ReedSolomon.verify`), with the code
    :func:`reconstruct` derives."""
    params = CodeParams.derive_parameters(validator_count, recoverablity_subset_size(validator_count))
    return params.make_encoder(ctx).verify(received)


def recover(received: Sequence[Optional[bytes]], validator_count: int, ctx: Optional[Context] = None):
    """``(payload, shards, mismatched_rows)`` of the received shards (:meth:`ReedSolomon.recover`),
    with the code :func:`reconstruct` derives."""
    params = CodeParams.derive_parameters(validator_count, recoverablity_subset_size(validator_count))
    return params.make_encoder(ctx).recover(received)


# -------------------------------------------------- device-resident batch ----
def encode_batch_dev(params: CodeParams, d_payloads: int, payload_len: int, payload_stride: int, batch: int,
                     d_shards: int, batch_stride: int, ctx: Optional[Context] = None, stream: int = 0) -> None:
    ctx = ctx or default_context()
    _raise(lib().np_encode_batch_dev(ctx.handle, C.byref(params._c()), d_payloads, payload_len, payload_stride,
                                     batch, d_shards, batch_stride, stream or None))


def error_locator_dev(n: int, d_present: int, batch: int, d_locators: int, ctx: Optional[Context] = None,
                      stream: int = 0) -> None:
    ctx = ctx or default_context()
    _raise(lib().np_error_locator_dev(ctx.handle, n, d_present, batch, d_locators, stream or None))


def reconstruct_batch_dev2(params: CodeParams, d_shards: int, shard_len: int, batch_stride: int, d_present: int,
                           d_locators: int, batch: int, d_out: int, out_stride: int,
                           ctx: Optional[Context] = None, stream: int = 0, d_status: int = 0) -> None:
    """Device batch reconstruct, bit-exact with the crate for any received bytes.

    d_status: device address of ``batch`` np_payload_status entries (int32 status,
    uint32 have; see :func:`payload_errors`) or 0."""
    ctx = ctx or default_context()
    _raise(lib().np_reconstruct_batch_dev3(ctx.handle, C.byref(params._c()), d_shards, shard_len, batch_stride,
                                           d_present, d_locators or None, batch, d_out, out_stride,
                                           d_status or None, stream or None))


def reconstruct_codewords_batch_dev(params: CodeParams, d_shards: int, shard_len: int, batch_stride: int,
                                    d_present: int, batch: int, d_out: int, out_stride: int,
                                    ctx: Optional[Context] = None, stream: int = 0, d_status: int = 0) -> None:
    """OPT-IN prefix decode for shards known to form a codeword (include/novelpoly.h);
    not crate-equivalent for other bytes."""
    ctx = ctx or default_context()
    _raise(lib().np_reconstruct_codewords_batch_dev(ctx.handle, C.byref(params._c()), d_shards, shard_len,
                                                    batch_stride, d_present, batch, d_out, out_stride,
                                                    d_status or None, stream or None))


def restore_shards_batch_dev(params: CodeParams, d_shards: int, shard_len: int, batch_stride: int, d_present: int,
                             batch: int, ctx: Optional[Context] = None, stream: int = 0, d_status: int = 0) -> None:
    """Writes the absent rows below ``wanted_n`` of every payload with at least k
    present rows into ``d_shards`` (np_restore_shards_batch_dev): the rows of
    ``encode(reconstruct(received))``, bit-exact with the crate for any received
    bytes; nothing else is written.  d_status as :func:`reconstruct_batch_dev2`."""
    ctx = ctx or default_context()
    _raise(lib().np_restore_shards_batch_dev(ctx.handle, C.byref(params._c()), d_shards, shard_len, batch_stride,
                                             d_present, batch, d_status or None, stream or None))


def verify_shards_batch_dev(params: CodeParams, d_shards: int, shard_len: int, batch_stride: int, d_present: int,
                            batch: int, d_bad_rows: int, ctx: Optional[Context] = None, stream: int = 0,
                            d_mismatch: int = 0, d_status: int = 0) -> None:
    """Compares every present row below ``wanted_n`` with its row of
    ``encode(reconstruct(received))`` (np_verify_shards_batch_dev), bit-exact
    with the crate for any received bytes; ``d_shards`` is only read.
    ``d_bad_rows``: one uint32 per payload, the number of mismatching rows, or
    0xFFFFFFFF for a payload with fewer than k present rows.  ``d_mismatch``
    (optional): ``batch x n`` bytes, 1 for a mismatching row.  d_status as
    :func:`reconstruct_batch_dev2`."""
    ctx = ctx or default_context()
    _raise(lib().np_verify_shards_batch_dev(ctx.handle, C.byref(params._c()), d_shards, shard_len, batch_stride,
                                            d_present, batch, d_bad_rows, d_mismatch or None, d_status or None,
                                            stream or None))


def recover_batch_dev(params: CodeParams, d_shards: int, shard_len: int, batch_stride: int, d_present: int,
                      batch: int, ctx: Optional[Context] = None, stream: int = 0, d_out: int = 0, out_stride: int = 0,
                      restore: bool = False, d_bad_rows: int = 0, d_mismatch: int = 0, d_status: int = 0) -> None:
    """The payloads, the absent rows and the verdict from one decode
    (np_recover_batch_dev): ``d_out`` / ``out_stride`` as
    :func:`reconstruct_batch_dev2` without locators, ``restore`` as
    :func:`restore_shards_batch_dev`, ``d_bad_rows`` / ``d_mismatch`` as
    :func:`verify_shards_batch_dev` -- each output bit for bit that call's, for
    any received bytes.  At least one of the three is requested; an output that
    is not requested is never written.  d_status as :func:`reconstruct_batch_dev2`."""
    ctx = ctx or default_context()
    _raise(lib().np_recover_batch_dev(ctx.handle, C.byref(params._c()), d_shards or None, shard_len, batch_stride,
                                      d_present or None, batch, d_out or None, out_stride, 1 if restore else 0,
                                      d_bad_rows or None, d_mismatch or None, d_status or None, stream or None))


NO_ITEM = 0xFFFFFFFF  # block_item of a padding workgroup of ragged_plan


def _ragged_array(items):
    """A ctypes array of RaggedItem from RaggedItem objects or 4-tuples
    (payload_off, payload_len, shards_off, shard_len); an array made by
    :func:`ragged_items` is passed through."""
    if isinstance(items, C.Array) and items._type_ is RaggedItem:
        return items
    arr = (RaggedItem * max(1, len(items)))()
    for i, it in enumerate(items):
        arr[i] = it if isinstance(it, RaggedItem) else RaggedItem(*(int(x) for x in it))
    return arr


def ragged_items(items):
    """The items as the ctypes array the ragged calls take (a caller that makes
    several calls with one batch converts it once)."""
    assert len(items) > 0
    return _ragged_array(items)


def encode_ragged_dev(params: CodeParams, d_payloads: int, payloads_size: int, d_shards: int, shards_size: int,
                      items, ctx: Optional[Context] = None, stream: int = 0) -> None:
    """One encode call for payloads of different lengths (np_encode_ragged_dev):
    item b's payload at ``d_payloads + payload_off``, its row v at ``d_shards +
    shards_off + v * shard_len``; equal to :func:`encode_batch_dev` with batch 1
    per item.  ``items``: RaggedItem objects or 4-tuples, read before the call
    returns."""
    ctx = ctx or default_context()
    _raise(lib().np_encode_ragged_dev(ctx.handle, C.byref(params._c()), d_payloads or None, payloads_size,
                                      d_shards or None, shards_size, _ragged_array(items), len(items),
                                      stream or None))


def reconstruct_ragged_dev(params: CodeParams, d_shards: int, shards_size: int, d_present: int, d_out: int,
                           out_size: int, items, ctx: Optional[Context] = None, stream: int = 0,
                           d_status: int = 0) -> None:
    """One reconstruct call for shards of different lengths
    (np_reconstruct_ragged_dev): item b decodes into ``d_out + payload_off``
    as :func:`reconstruct_batch_dev2` with batch 1 and no caller locators does;
    ``d_present``: ``len(items) x n`` device flags."""
    ctx = ctx or default_context()
    _raise(lib().np_reconstruct_ragged_dev(ctx.handle, C.byref(params._c()), d_shards or None, shards_size,
                                           d_present or None, d_out or None, out_size, _ragged_array(items),
                                           len(items), d_status or None, stream or None))


def restore_shards_ragged_dev(params: CodeParams, d_shards: int, shards_size: int, d_present: int, items,
                              ctx: Optional[Context] = None, stream: int = 0, d_status: int = 0) -> None:
    """:func:`restore_shards_batch_dev` on a ragged buffer
    (np_restore_shards_ragged_dev): item b's absent rows below ``wanted_n`` are
    written at ``d_shards + shards_off + v * shard_len`` as the uniform call
    with batch 1 writes them.  The items of :func:`encode_ragged_dev` serve;
    ``payload_off`` and ``payload_len`` are ignored."""
    ctx = ctx or default_context()
    _raise(lib().np_restore_shards_ragged_dev(ctx.handle, C.byref(params._c()), d_shards or None, shards_size,
                                              d_present or None, _ragged_array(items), len(items), d_status or None,
                                              stream or None))


def verify_shards_ragged_dev(params: CodeParams, d_shards: int, shards_size: int, d_present: int, items,
                             d_bad_rows: int, ctx: Optional[Context] = None, stream: int = 0, d_mismatch: int = 0,
                             d_status: int = 0) -> None:
    """:func:`verify_shards_batch_dev` on a ragged buffer
    (np_verify_shards_ragged_dev): entry b of ``d_bad_rows`` (and row b of
    ``d_mismatch``, ``len(items) x n`` bytes) is what the uniform call with
    batch 1 gives for item b; ``d_shards`` is only read."""
    ctx = ctx or default_context()
    _raise(lib().np_verify_shards_ragged_dev(ctx.handle, C.byref(params._c()), d_shards or None, shards_size,
                                             d_present or None, _ragged_array(items), len(items), d_bad_rows or None,
                                             d_mismatch or None, d_status or None, stream or None))


def recover_ragged_dev(params: CodeParams, d_shards: int, shards_size: int, d_present: int, items, d_out: int = 0,
                       out_size: int = 0, restore: bool = False, d_bad_rows: int = 0, d_mismatch: int = 0,
                       d_status: int = 0, ctx: Optional[Context] = None, stream: int = 0) -> None:
    """:func:`recover_batch_dev` on a ragged buffer (np_recover_ragged_dev):
    from one decode, item b's payload at ``d_out + payload_off`` as
    :func:`reconstruct_ragged_dev`, its absent rows as
    :func:`restore_shards_ragged_dev` (``restore``) and its verdict as
    :func:`verify_shards_ragged_dev` (``d_bad_rows`` / ``d_mismatch``) -- each
    output bit for bit that call's.  At least one of the three is requested; an
    output that is not requested is never written.  Without ``d_out``,
    ``payload_off`` is ignored."""
    ctx = ctx or default_context()
    _raise(lib().np_recover_ragged_dev(ctx.handle, C.byref(params._c()), d_shards or None, shards_size,
                                       d_present or None, d_out or None, out_size, _ragged_array(items), len(items),
                                       1 if restore else 0, d_bad_rows or None, d_mismatch or None, d_status or None,
                                       stream or None))


def ragged_plan(params: CodeParams, items, reconstruct: bool, payloads_size: int, shards_size: int):
    """np_ragged_plan (host only): validates ``items`` as the ragged calls do
    and returns the direct path's launch plan as a list of (item, tile), one
    per workgroup; item == NO_ITEM marks a padding workgroup."""
    arr = _ragged_array(items)
    nb = _sz(0)
    _raise(lib().np_ragged_plan(C.byref(params._c()), arr, len(items), int(bool(reconstruct)), payloads_size,
                                shards_size, None, None, 0, C.byref(nb)))
    bi = (C.c_uint32 * max(1, nb.value))()
    bt = (C.c_uint32 * max(1, nb.value))()
    _raise(lib().np_ragged_plan(C.byref(params._c()), arr, len(items), int(bool(reconstruct)), payloads_size,
                                shards_size, bi, bt, nb.value, C.byref(nb)))
    return [(bi[i], bt[i]) for i in range(nb.value)]


def payload_errors(params: CodeParams, status_pairs) -> List[Optional[Error]]:
    """np_payload_status entries (a sequence of (status, have) pairs, e.g. a
    ``batch x 2`` int array copied to the host) as the crate's per-call result:
    None for a decoded payload, ``NeedMoreShards(have, k, n)`` (mod.rs:178-180)
    otherwise."""
    out: List[Optional[Error]] = []
    for st, have in status_pairs:
        st = int(st)
        if st == 0:
            out.append(None)
        elif st == NeedMoreShards.code:
            out.append(NeedMoreShards(int(have), params.k(), params.n()))
        else:
            out.append(DeviceError(st, "unexpected payload status"))
    return out


def encode_batch_host(params: CodeParams, payloads: int, payload_len: int, payload_stride: int, batch: int,
                      shards: int, batch_stride: int, ctx: Optional[Context] = None) -> None:
    """Host-memory batch encode (addresses of host buffers, e.g. numpy / pinned torch)."""
    ctx = ctx or default_context()
    _raise(lib().np_encode_batch_host(ctx.handle, C.byref(params._c()), payloads, payload_len, payload_stride, batch,
                                      shards, batch_stride))


def reconstruct_batch_host(params: CodeParams, shards: int, shard_len: int, batch_stride: int, present: int,
                           batch: int, out: int, out_stride: int, ctx: Optional[Context] = None) -> None:
    """Host-memory batch reconstruct; present: address of batch*n host flags."""
    ctx = ctx or default_context()
    _raise(lib().np_reconstruct_batch_host(ctx.handle, C.byref(params._c()), shards, shard_len, batch_stride, present,
                                           batch, out, out_stride))


def recover_batch_host(params: CodeParams, shards: int, shard_len: int, batch_stride: int, present: int, batch: int,
                       ctx: Optional[Context] = None, out: int = 0, out_stride: int = 0, restore: bool = False,
                       bad_rows: int = 0, mismatch: int = 0, status: int = 0) -> None:
    """:func:`recover_batch_dev` on host buffers (np_recover_batch_host; addresses
    of host memory, 0 = not given), pipelined like :func:`reconstruct_batch_host`:
    the payloads into ``out``, the absent rows below ``wanted_n`` into ``shards``
    (``restore``) and the verdict into ``bad_rows`` / ``mismatch``, each bit for
    bit the device call's.  With ``status`` (``batch`` np_payload_status entries)
    a payload with fewer than k present rows is reported there and left
    untouched; without it such a payload raises :class:`NeedMoreShards` before
    anything is written.  Returns when every output is in host memory."""
    ctx = ctx or default_context()
    _raise(lib().np_recover_batch_host(ctx.handle, C.byref(params._c()), shards or None, shard_len, batch_stride,
                                       present or None, batch, out or None, out_stride, 1 if restore else 0,
                                       bad_rows or None, mismatch or None, status or None))


def reconstruct_from_systematic_batch_dev(params: CodeParams, d_shards: int, shard_len: int, batch_stride: int,
                                          batch: int, d_out: int, out_stride: int, ctx: Optional[Context] = None,
                                          stream: int = 0) -> None:
    """mod.rs:247-285 for a device batch whose first k shards are present."""
    ctx = ctx or default_context()
    _raise(lib().np_reconstruct_from_systematic_batch_dev(ctx.handle, C.byref(params._c()), d_shards, shard_len,
                                                          batch_stride, batch, d_out, out_stride, stream or None))


def reconstruct_batch_dev(params: CodeParams, d_shards: int, shard_len: int, batch_stride: int, present,
                          batch: int, d_out: int, out_stride: int, ctx: Optional[Context] = None,
                          stream: int = 0) -> None:
    """present: host bytes-like of batch*n flags."""
    ctx = ctx or default_context()
    pres = bytes(present)
    _raise(lib().np_reconstruct_batch_dev(ctx.handle, C.byref(params._c()), d_shards, shard_len, batch_stride,
                                          pres, batch, d_out, out_stride, stream or None))


# ------------------------------------------------------------ multi-GPU ----
def batch_split(batch: int, ndev: int, i: int):
    """np_batch_split: (begin, count) of device i's contiguous payload range."""
    b, c = _sz(), _sz()
    lib().np_batch_split(batch, ndev, i, C.byref(b), C.byref(c))
    return b.value, c.value


def _ptr_array(vals):
    arr = (C.c_void_p * max(1, len(vals)))()
    for i, v in enumerate(vals):
        arr[i] = v or None
    return arr


def _ctx_array(ctxs):
    return _ptr_array([c.handle.value for c in ctxs])


def encode_batch_multi(ctxs, params: CodeParams, d_payloads, payload_len: int, payload_stride: int, batch: int,
                       d_shards, batch_stride: int) -> None:
    """Device-resident batch over several contexts (one per GPU); d_payloads[i] /
    d_shards[i]: device i's buffers for its range (:func:`batch_split`)."""
    _raise(lib().np_encode_batch_multi(_ctx_array(ctxs), len(ctxs), C.byref(params._c()), _ptr_array(d_payloads),
                                       payload_len, payload_stride, batch, _ptr_array(d_shards), batch_stride))


def reconstruct_batch_multi(ctxs, params: CodeParams, d_shards, shard_len: int, batch_stride: int, d_present,
                            batch: int, d_out, out_stride: int, d_status=None) -> None:
    st = _ptr_array(d_status) if d_status else None
    _raise(lib().np_reconstruct_batch_multi(_ctx_array(ctxs), len(ctxs), C.byref(params._c()), _ptr_array(d_shards),
                                            shard_len, batch_stride, _ptr_array(d_present), batch, _ptr_array(d_out),
                                            out_stride, st))


def encode_batch_host_multi(ctxs, params: CodeParams, payloads: int, payload_len: int, payload_stride: int,
                            batch: int, shards: int, batch_stride: int) -> None:
    _raise(lib().np_encode_batch_host_multi(_ctx_array(ctxs), len(ctxs), C.byref(params._c()), payloads, payload_len,
                                            payload_stride, batch, shards, batch_stride))


def reconstruct_batch_host_multi(ctxs, params: CodeParams, shards: int, shard_len: int, batch_stride: int,
                                 present: int, batch: int, out: int, out_stride: int) -> None:
    _raise(lib().np_reconstruct_batch_host_multi(_ctx_array(ctxs), len(ctxs), C.byref(params._c()), shards, shard_len,
                                                 batch_stride, present, batch, out, out_stride))


def recover_batch_multi(ctxs, params: CodeParams, d_shards, shard_len: int, batch_stride: int, d_present, batch: int,
                        d_out=None, out_stride: int = 0, restore: bool = False, d_bad_rows=None, d_mismatch=None,
                        d_status=None) -> None:
    """:func:`recover_batch_dev` over several contexts (np_recover_batch_multi):
    every buffer argument is a list with device i's address for its range
    (:func:`batch_split`); None = that output is not requested."""
    opt = [_ptr_array(a) if a else None for a in (d_out, d_bad_rows, d_mismatch, d_status)]
    _raise(lib().np_recover_batch_multi(_ctx_array(ctxs), len(ctxs), C.byref(params._c()), _ptr_array(d_shards),
                                        shard_len, batch_stride, _ptr_array(d_present), batch, opt[0], out_stride,
                                        1 if restore else 0, opt[1], opt[2], opt[3]))


def recover_batch_host_multi(ctxs, params: CodeParams, shards: int, shard_len: int, batch_stride: int, present: int,
                             batch: int, out: int = 0, out_stride: int = 0, restore: bool = False, bad_rows: int = 0,
                             mismatch: int = 0, status: int = 0) -> None:
    """:func:`recover_batch_host` with the batch split over several contexts
    (np_recover_batch_host_multi): one buffer set, each context its range."""
    _raise(lib().np_recover_batch_host_multi(_ctx_array(ctxs), len(ctxs), C.byref(params._c()), shards or None,
                                             shard_len, batch_stride, present or None, batch, out or None, out_stride,
                                             1 if restore else 0, bad_rows or None, mismatch or None, status or None))


# ---------------------------------------------------- low-level hooks ----
def afft_dev(d_data: int, size: int, index: int, cols: int, inverse: bool = False,
             ctx: Optional[Context] = None, stream: int = 0) -> None:
    ctx = ctx or default_context()
    f = lib().np_inverse_afft_dev if inverse else lib().np_afft_dev
    _raise(f(ctx.handle, d_data, size, index, cols, stream or None))


def walsh_dev(d_data: int, size: int, ctx: Optional[Context] = None, stream: int = 0) -> None:
    ctx = ctx or default_context()
    _raise(lib().np_walsh_dev(ctx.handle, d_data, size, stream or None))


def mul_dev(d_a: int, d_m: int, d_out: int, count: int, ctx: Optional[Context] = None, stream: int = 0) -> None:
    ctx = ctx or default_context()
    _raise(lib().np_mul_dev(ctx.handle, d_a, d_m, d_out, count, stream or None))


def encode_low_dev(d_data: int, k: int, d_codeword: int, n: int, cols: int, ctx: Optional[Context] = None,
                   stream: int = 0) -> None:
    ctx = ctx or default_context()
    _raise(lib().np_encode_low_dev(ctx.handle, d_data, k, d_codeword, n, cols, stream or None))


def decode_main_dev(d_codeword: int, recover_up_to: int, d_present: int, d_locator: int, n: int, cols: int,
                    ctx: Optional[Context] = None, stream: int = 0) -> None:
    ctx = ctx or default_context()
    _raise(lib().np_decode_main_dev(ctx.handle, d_codeword, recover_up_to, d_present, d_locator, n, cols,
                                    stream or None))


def version() -> str:
    return lib().np_version().decode()


# ----------------------------------------------------------- diagnostics ----
BOUNDS_KINDS = ("shards", "present", "locators", "records", "out", "status", "zeros", "payloads", "items", "blocks")


def debug_bounds_check(ctx: Optional[Context] = None) -> Optional[dict]:
    """Checked builds (lib/libnovelpoly_hip_chk.so through NP_LIB_PATH): the
    out-of-extent global accesses of the instrumented kernels since the last
    call, {count, kind, line, workgroup, thread, offset, bytes} (count 0: none);
    None with the product library."""
    ctx = ctx or default_context()
    r = (C.c_uint32 * 8)()
    if lib().np_debug_bounds_check(ctx.handle, r) != 0:
        return None
    kind = BOUNDS_KINDS[r[1]] if r[0] and r[1] < len(BOUNDS_KINDS) else r[1]
    return {"count": r[0], "kind": kind, "line": r[2], "workgroup": r[3], "thread": r[4],
            "offset": r[5] | (r[6] << 32), "bytes": r[7]}


def pin_registry_stats() -> dict:
    """The engine's in-place pin registry: ranges registered now, and
    hipHostUnregister calls the runtime refused (include/novelpoly.h)."""
    o = (_sz * 2)()
    lib().np_pin_registry_stats(o)
    return {"live_ranges": o[0], "failed_unregisters": o[1]}
