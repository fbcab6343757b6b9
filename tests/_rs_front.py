"""The validation that the single-shot host calls share (np_rs_reconstruct,
np_rs_restore_shards, np_rs_verify_shards; np_rs_recover has its own cases in
tests/test_recover_cpu.py): the received set up to `present`, the count and
the symbols per shard (mod.rs:163-214), then the code.  check_front runs the
cases against one entry point; every case returns before the context is
touched, so a zero-filled stand-in serves as one.  No GPU compute here."""
import ctypes as C

import novelpoly_amd as npa

N, K, WN, LEN = 64, 16, 60, 10  # a code, and the bytes of a received shard
NEED = (LEN // 2) * 2 * K

_ctx = C.create_string_buffer(1 << 16)
_row = C.create_string_buffer(b"\x01" * 16)
CTX = C.cast(_ctx, C.c_void_p)


def params(n=N, k=K, wanted_n=WN):
    return npa._Params(n, k, wanted_n)


def detail():
    det = (C.c_size_t * 3)()
    npa.lib().np_last_error_detail(det)
    return tuple(det)


def poison():
    """Leaves a detail that no case below expects, so that (0, 0, 0) is seen to be written."""
    p = params(24, 6, 24)
    assert npa.lib().np_rs_reconstruct(CTX, C.byref(p), None, None, 0, None, 0, None) == npa.ParamterMustBePowerOf2.code
    assert detail() == (24, 6, 0)


def received(count=K, first=0, n=N):
    """Arrays of n + 4 entries: `count` shards of LEN bytes from row `first` on, the rest absent."""
    ptrs, lens = (C.c_void_p * (n + 4))(), (C.c_size_t * (n + 4))()
    for i in range(first, first + count):
        ptrs[i], lens[i] = C.cast(_row, C.c_void_p), LEN
    return ptrs, lens


def outcome(status):
    return status, detail()


def check_front(call):
    """`call(p, ptrs, lens, n_received)` -> status: the entry point with its other
    arguments valid (p is a _Params or None).  The cases are in the order of the
    checks; where two faults are present the earlier check's is reported."""
    inv, pow2, more = 100, npa.ParamterMustBePowerOf2.code, npa.NeedMoreShards.code
    empty, uneq = npa.EmptyShard.code, npa.InconsistentShardLengths.code

    def run(p, ptrs, lens, n_received):
        poison()
        return outcome(call(p, ptrs, lens, n_received))

    ptrs, lens = received()
    # NULL params or arrays: before the code is read
    assert run(None, ptrs, lens, N) == (inv, (0, 0, 0))
    assert run(params(12, 3, 12), None, lens, N) == (inv, (0, 0, 0))
    assert run(params(12, 3, 12), ptrs, None, N) == (inv, (0, 0, 0))
    # neither n nor k a power of two: before the count (nothing received needs no arrays)
    assert run(params(12, 3, 12), None, None, 0) == (pow2, (12, 3, 0))
    assert run(params(12, 3, 12), ptrs, lens, N) == (pow2, (12, 3, 0))
    # fewer than k shards: nothing, k - 1, and k - 1 with more at n and beyond
    assert run(params(), None, None, 0) == (more, (0, K, N))
    assert run(params(), *received(K - 1), N) == (more, (K - 1, K, N))
    assert run(params(), ptrs, lens, K - 1) == (more, (K - 1, K, N))
    ptrs, lens = received(K - 1)
    for i in range(N, N + 4):
        ptrs[i], lens[i] = C.cast(_row, C.c_void_p), LEN
    assert run(params(), ptrs, lens, N + 4) == (more, (K - 1, K, N))
    # ... before the rest of the code is checked (2k > n)
    assert run(params(64, 48, 64), *received(47), N) == (more, (47, 48, 64))
    # the first present shard empty: before unequal lengths
    ptrs, lens = received(K + 1, first=1)
    lens[1], lens[3] = 0, 6
    assert run(params(), ptrs, lens, N) == (empty, (0, 0, 0))
    # unequal lengths: the first row that differs, in symbols; before the code
    lens[1], lens[5] = LEN, 4
    assert run(params(), ptrs, lens, N) == (uneq, (LEN // 2, 3, 0))
    assert run(params(64, 16, 65), ptrs, lens, N) == (uneq, (LEN // 2, 3, 0))
    # LEN - 1 bytes are as many symbols, an absent row's length is not read: the code is next
    ptrs, lens = received(K + 1, first=1)
    lens[2], lens[0], lens[40] = LEN - 1, 3, 7
    assert run(params(64, 16, 65), ptrs, lens, N) == (inv, (64, 16, 65))
    assert run(params(64, 48, 64), *received(48), N) == (inv, (64, 48, 64))
