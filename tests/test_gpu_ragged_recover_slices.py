"""np_recover_ragged_dev in slices: the construction of
tests/test_gpu_ragged_masked_slices.py -- n512 k256, a batch of mixed lengths
whose decoded payloads sum to more than twice the context's restore scratch
(1/256 of the device's memory) -- so the call that restores and verifies
without d_out runs in at least three slices that end at item boundaries, each
with its plan words at the recover plan's stride.  The same request with d_out
keeps no payload in scratch; it must give the same rows, flags and counts, and
the payloads of np_reconstruct_ragged_dev.  Generated, erased, altered and
compared on the device, GPU against GPU: the references are
np_restore_shards_ragged_dev, np_verify_shards_ragged_dev and
np_reconstruct_ragged_dev, which tests/test_gpu_ragged_masked_slices.py and
tests/test_gpu_ragged.py check against the uniform calls and the oracle."""
import numpy as np
import pytest

import novelpoly_amd as npa
from test_gpu_ragged_masked_slices import COLS, FILL

pytestmark = pytest.mark.gpu


def test_recover_in_slices(gpu):
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
        poff += cols * 2 * k + 2 * (i % 2) + (i % 3 == 0)  # odd output offsets too
        soff += n * 2 * cols + 2 * (i % 4)  # some rows at 2 mod 4 addresses
        decoded += (cols * 2 * k + 255) // 256 * 256
    batch = len(items)
    arr = npa.ragged_items(items)
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(13)
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
    received = code
    for b, (_, _, so, sl) in enumerate(items):
        rows = received[so:so + n * sl].view(n, sl)
        rows[pres[b] == 0] = FILL
        if b % 3 == 0:
            v = k + int(np.flatnonzero(npres[b, k:])[0])
            rows[v, (7 * b) % sl] = rows[v, (7 * b) % sl] ^ 0x21

    def results():
        return (torch.full((batch,), 7, dtype=torch.int32, device="cuda"),
                torch.full((batch, n), FILL, dtype=torch.uint8, device="cuda"),
                torch.full((batch, 2), -1, dtype=torch.int32, device="cuda"))

    # ---- the references: the ragged restore and the ragged verify
    ref = received.clone()
    cnt_ref, map_ref, st_ref = results()
    npa.verify_shards_ragged_dev(p, received.data_ptr(), soff, pres.data_ptr(), arr, cnt_ref.data_ptr(), ctx=gpu,
                                 stream=s, d_mismatch=map_ref.data_ptr(), d_status=st_ref.data_ptr())
    npa.restore_shards_ragged_dev(p, ref.data_ptr(), soff, pres.data_ptr(), arr, ctx=gpu, stream=s)

    # ---- restore + verify without d_out: sliced, the recover plan's stride in the scratch layout
    work = received.clone()
    cnt_got, map_got, st_got = results()
    npa.recover_ragged_dev(p, work.data_ptr(), soff, pres.data_ptr(), arr, restore=True, d_bad_rows=cnt_got.data_ptr(),
                           d_mismatch=map_got.data_ptr(), d_status=st_got.data_ptr(), ctx=gpu, stream=s)
    torch.cuda.synchronize()
    assert torch.equal(st_got, st_ref) and torch.equal(cnt_got, cnt_ref) and torch.equal(map_got, map_ref)
    assert torch.equal(work, ref)
    assert not torch.equal(work, received)  # rows were restored
    assert int((st_ref[:, 0] != 0).sum()) == len(range(0, batch, 5))
    ncnt = cnt_ref.cpu().numpy()
    assert (ncnt[::5] == -1).all()  # undecodable
    clean = [b for b in range(batch) if b % 5 and b % 3]
    altered = [b for b in range(batch) if b % 5 and b % 3 == 0]
    assert clean and altered and not ncnt[clean].any() and (ncnt[altered] > 0).all()
    del work

    # ---- the same with d_out, and the map of the call's own: no payload scratch, the same results
    out_ref = torch.full((poff,), FILL, dtype=torch.uint8, device="cuda")
    npa.reconstruct_ragged_dev(p, received.data_ptr(), soff, pres.data_ptr(), out_ref.data_ptr(), poff, arr, ctx=gpu,
                               stream=s)
    out_got = torch.full((poff,), FILL, dtype=torch.uint8, device="cuda")
    work = received.clone()
    cnt_got, _, st_got = results()
    npa.recover_ragged_dev(p, work.data_ptr(), soff, pres.data_ptr(), arr, d_out=out_got.data_ptr(), out_size=poff,
                           restore=True, d_bad_rows=cnt_got.data_ptr(), d_status=st_got.data_ptr(), ctx=gpu, stream=s)
    torch.cuda.synchronize()
    assert torch.equal(st_got, st_ref) and torch.equal(cnt_got, cnt_ref)
    assert torch.equal(work, ref)
    assert torch.equal(out_got, out_ref)
    assert not bool((out_got == FILL).all())
