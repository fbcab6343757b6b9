"""The fast decode's phases between the transforms -- row issue, the layout
exchanges' tile hand-off and the register copy-out (kernels_fast_decode.hip
issue_rows_c, rec_segments, copy_out_cq) -- byte for byte against the oracle.

Instances: NQ = n / k = 2, 4, 8 at K = 256 and NQ = 4 at K = 64 and 128 (they
share rec_segments).  Shard lengths: one full 256-column tile (512 bytes of a
row); four tiles in one workgroup (2048 with NP_REC_TPW = 4: the tile prefetch,
and the tile rotation with a batch of 3, which the tile count does not divide);
a partial last tile (2050, 514: the row loads and the copy-out of partial
tiles).  Every row holds random bytes (no codewords: the decode is a linear map
of every present row), three payloads per call with different erasure masks.
Addresses: the output 16-byte aligned and offset by 8 bytes, the shard base
offset by 2 bytes.  Launches: the same call twice on one stream and once on a
second stream give the same bytes."""
import numpy as np
import pytest

import novelpoly_amd as npa

pytestmark = pytest.mark.gpu

# (n_wanted, k_wanted) -> effective (n, k)
INSTANCES = [((512, 256), (512, 256)), ((1024, 256), (1024, 256)), ((2048, 256), (2048, 256)),
             ((256, 64), (256, 64)), ((512, 128), (512, 128))]
SHARD_LENS = [512, 2048, 2050, 514]
FILL = 0x5A


def _masks(n, k, rng):
    """Six present masks: [random k rows; one systematic row missing; whole
    16-row groups and alternating rows absent in every segment], [one whole
    segment absent; every systematic row present; k - 1 rows (NeedMoreShards)]."""
    nq, groups = n // k, k // 16
    m = []
    p = np.zeros(n, np.uint8)
    p[rng.choice(n, k, replace=False)] = 1
    m.append(p)
    p = np.ones(n, np.uint8)
    p[int(rng.integers(0, k))] = 0
    m.append(p)
    p = np.ones(n, np.uint8)
    for q in range(nq):
        g = (q + 1) % groups
        p[q * k + 16 * g: q * k + 16 * g + 16] = 0
        g2 = (g + 1) % groups
        p[q * k + 16 * g2: q * k + 16 * g2 + 16: 2] = 0
    m.append(p)
    p = np.ones(n, np.uint8)
    if nq == 2:  # the systematic segment absent, the other one complete
        p[:k] = 0
    else:  # the last segment absent (NQ = 8: skipped; NQ = 4: decoded as zeros), a third of the rest erased
        p[(nq - 1) * k:] = 0
        p[rng.choice((nq - 1) * k, (nq - 1) * k // 3, replace=False)] = 0
    m.append(p)
    p = np.ones(n, np.uint8)
    p[k + rng.choice(n - k, (n - k) // 2, replace=False)] = 0
    m.append(p)
    p = np.zeros(n, np.uint8)
    p[rng.choice(n, k - 1, replace=False)] = 1
    m.append(p)
    assert all(int(x.sum()) >= k for x in m[:5]) and int(m[5].sum()) == k - 1
    return [np.stack(m[:3]), np.stack(m[3:])]


@pytest.mark.parametrize("sl", SHARD_LENS)
@pytest.mark.parametrize("want_nk,eff_nk", INSTANCES)
def test_decode_phases(gpu, oracle, monkeypatch, want_nk, eff_nk, sl):
    import torch

    if sl >= 2048:
        monkeypatch.setenv("NP_REC_TPW", "4")
    p = npa.CodeParams.derive_parameters(*want_nk)
    n, k = p.n(), p.k()
    assert (n, k) == eff_nk
    rng = np.random.default_rng(n * 131 + k * 7 + sl)
    batch, olen = 3, (sl // 2) * 2 * k
    cur = torch.cuda.current_stream()
    other = torch.cuda.Stream()

    def run(d_shards, d_pres, stream, out_off=0):
        buf = torch.full((batch * olen + 16,), FILL, dtype=torch.uint8, device="cuda")
        st_d = torch.full((batch, 2), -1, dtype=torch.int32, device="cuda")
        assert buf.data_ptr() % 16 == 0
        npa.reconstruct_batch_dev2(p, d_shards, sl, n * sl, d_pres.data_ptr(), 0, batch, buf.data_ptr() + out_off, olen,
                                   ctx=gpu, stream=stream.cuda_stream, d_status=st_d.data_ptr())
        return buf, st_d, out_off

    for pres in _masks(n, k, rng):
        rows = rng.integers(0, 256, (batch, n, sl), dtype=np.uint8)
        want, have = [], []
        for b in range(batch):
            recv = [rows[b, i].tobytes() if pres[b, i] else None for i in range(n)]
            st, w = oracle.reconstruct(recv, n, k)
            have.append(int(pres[b].sum()))
            if have[b] >= k:
                assert st == 0 and len(w) == olen
                want.append(np.frombuffer(w, np.uint8))
            else:
                assert st == npa.NeedMoreShards.code
                want.append(None)
        flat = torch.from_numpy(rows.reshape(-1))
        ds = flat.cuda()
        ds2 = torch.zeros(flat.numel() + 16, dtype=torch.uint8, device="cuda")  # shard base offset by 2 bytes
        ds2[2:2 + flat.numel()] = ds
        assert ds.data_ptr() % 16 == 0 and ds2.data_ptr() % 16 == 0
        dpres = torch.from_numpy(pres).cuda()
        runs = [("aligned", run(ds.data_ptr(), dpres, cur)),
                ("aligned, again", run(ds.data_ptr(), dpres, cur)),
                ("output + 8", run(ds.data_ptr(), dpres, cur, 8)),
                ("shards + 2", run(ds2.data_ptr() + 2, dpres, cur))]
        other.wait_stream(cur)
        runs.append(("second stream", run(ds.data_ptr(), dpres, other)))
        cur.wait_stream(other)
        torch.cuda.synchronize()
        for name, (buf, st_d, off) in runs:
            o, stat = buf.cpu().numpy(), st_d.cpu().numpy()
            assert (o[:off] == FILL).all() and (o[off + batch * olen:] == FILL).all(), name
            errs = npa.payload_errors(p, stat)
            for b in range(batch):
                got = o[off + b * olen: off + (b + 1) * olen]
                if want[b] is None:
                    assert errs[b] == npa.NeedMoreShards(have[b], k, n), (name, b)
                    assert (got == FILL).all(), (name, b)  # not decoded, output untouched
                else:
                    assert tuple(stat[b]) == (0, have[b]), (name, b, stat[b])  # NP_OK
                    assert np.array_equal(got, want[b]), (name, b)
