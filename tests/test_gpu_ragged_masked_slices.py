"""np_restore_shards_ragged_dev / np_verify_shards_ragged_dev in slices: at
n512 k256 a batch of mixed lengths whose decoded payloads sum to more than
twice the context's restore scratch (1/256 of the device's memory, as
include/novelpoly.h documents it), so both calls run in at least three slices
that end at item boundaries.  Generated, erased, altered and compared on the
device.  The reference is the uniform call with batch = 1 per item on a copy of
the buffer, GPU against GPU: the oracle would take minutes at this size, and
the uniform calls are oracle-checked in tests/test_gpu_restore.py and
tests/test_gpu_verify.py."""
import numpy as np
import pytest

import novelpoly_amd as npa

pytestmark = pytest.mark.gpu

FILL = 0x5A
COLS = [3001, 8192, 16385, 24576, 40000, 12288, 47001]  # columns per item, cycled: 1.5 to 23 MiB of payload


def test_restore_and_verify_in_slices(gpu):
    import torch

    p = npa.CodeParams.derive_parameters(512, 256)
    n, k, wn = p.n(), p.k(), p.wanted_n
    assert (n, k, wn) == (512, 256, 512)
    cap = torch.cuda.get_device_properties(0).total_memory // 256
    items, poff, soff, decoded = [], 0, 0, 0
    while decoded <= 2 * cap + (64 << 20):
        i = len(items)
        cols = COLS[i % len(COLS)]
        items.append((poff, cols * 2 * k - (i % 3), soff, 2 * cols))
        poff += cols * 2 * k + 2 * (i % 2)
        soff += n * 2 * cols + 2 * (i % 4)  # some rows at 2 mod 4 addresses
        decoded += (cols * 2 * k + 255) // 256 * 256
    batch = len(items)
    arr = npa.ragged_items(items)
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(11)
    pay = torch.randint(0, 256, (poff,), dtype=torch.uint8, device="cuda", generator=gen)
    code = torch.full((soff,), FILL, dtype=torch.uint8, device="cuda")
    npa.encode_ragged_dev(p, pay.data_ptr(), poff, code.data_ptr(), soff, arr, ctx=gpu, stream=s)
    del pay
    # presence: (n - k) / 2 random rows absent; every 5th item k - 1 rows only, every 7th all systematic rows
    order = torch.rand((batch, n), device="cuda", generator=gen).argsort(dim=1)
    pres = torch.ones((batch, n), dtype=torch.uint8, device="cuda")
    pres.scatter_(1, order[:, : (n - k) // 2], 0)
    for b in range(0, batch, 5):
        pres[b] = 0
        pres[b, order[b, : k - 1]] = 1
    for b in range(3, batch, 7):
        if b % 5:
            pres[b, :k] = 1
    npres = pres.cpu().numpy()
    # absent rows blanked; in every 3rd item one byte of the first present parity row altered
    work = code.clone()
    for b, (_, _, so, sl) in enumerate(items):
        rows = work[so:so + n * sl].view(n, sl)
        rows[pres[b] == 0] = FILL
        if b % 3 == 0:
            v = k + int(np.flatnonzero(npres[b, k:])[0])
            rows[v, (7 * b) % sl] = rows[v, (7 * b) % sl] ^ 0x21
    del code
    received = work.clone()

    # ---- restore
    ref = work.clone()
    st_ref = torch.full((batch, 2), -1, dtype=torch.int32, device="cuda")
    st_got = st_ref.clone()
    for b, (_, _, so, sl) in enumerate(items):
        npa.restore_shards_batch_dev(p, ref.data_ptr() + so, sl, n * sl, pres.data_ptr() + b * n, 1, ctx=gpu, stream=s,
                                     d_status=st_ref.data_ptr() + 8 * b)
    npa.restore_shards_ragged_dev(p, work.data_ptr(), soff, pres.data_ptr(), arr, ctx=gpu, stream=s,
                                  d_status=st_got.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(st_got, st_ref)
    assert int((st_ref[:, 0] != 0).sum()) == len(range(0, batch, 5))
    assert torch.equal(work, ref)
    assert not torch.equal(work, received)  # rows were restored
    del ref, work

    # ---- verify, on the received rows
    cnt_ref = torch.full((batch,), 7, dtype=torch.int32, device="cuda")
    cnt_got = cnt_ref.clone()
    map_ref = torch.full((batch, n), FILL, dtype=torch.uint8, device="cuda")
    map_got = map_ref.clone()
    keep = received.clone()
    for b, (_, _, so, sl) in enumerate(items):
        npa.verify_shards_batch_dev(p, received.data_ptr() + so, sl, n * sl, pres.data_ptr() + b * n, 1,
                                    cnt_ref.data_ptr() + 4 * b, ctx=gpu, stream=s, d_mismatch=map_ref.data_ptr() + b * n)
    npa.verify_shards_ragged_dev(p, received.data_ptr(), soff, pres.data_ptr(), arr, cnt_got.data_ptr(), ctx=gpu,
                                 stream=s, d_mismatch=map_got.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(cnt_got, cnt_ref) and torch.equal(map_got, map_ref)
    assert torch.equal(received, keep)  # only read
    ncnt = cnt_ref.cpu().numpy()
    assert (ncnt[::5] == -1).all()  # undecodable
    clean = [b for b in range(batch) if b % 5 and b % 3]
    altered = [b for b in range(batch) if b % 5 and b % 3 == 0]
    assert clean and altered and not ncnt[clean].any() and (ncnt[altered] > 0).all()
