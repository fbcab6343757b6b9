"""Checking shards against their re-encoding, device-resident, at config 3
(n1024 k256, 1 MiB payloads, batch 1024): what a caller had to compose before
against np_verify_shards_batch_dev, alternated in one process.

  A  np_reconstruct_batch_dev3 into a payload buffer, np_encode_batch_dev into
     a second full shard buffer, then a compare of the present rows of the two
     shard buffers.  The compare is torch's (8-byte words unequal, any over the
     row, masked by the present flags, summed per payload): the library had no
     kernel for it.
  B  np_verify_shards_batch_dev on the buffer that holds the received rows
     (counts only: d_mismatch NULL).

Three presence patterns per payload, all on codewords: 342 random absent rows
(the bench's), every row present, and every systematic row plus half of the
parity rows.  Device events around each call; prints one JSON line (times in
ms: min / median / max over the repetitions).  Not the bench `value`."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reed-solomon-novelpoly_amd", "python"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import novelpoly_amd as npa  # noqa: E402
from novelpoly_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=3)
ap.add_argument("--batch", type=int, default=0, help="0: the config's batch")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--only", choices=["A", "B"], default=None, help="run one side only (kernel traces)")
args = ap.parse_args()

cfg = synth.CONFIGS[args.config]
p = npa.CodeParams.derive_parameters(cfg["n_wanted"], cfg["k_wanted"])
n, k, wn, plen = p.n(), p.k(), p.wanted_n, cfg["payload"]
B = args.batch or cfg["batch"]
ctx = npa.Context(0)
sl = p.make_encoder(ctx).shard_len(plen)
olen = (sl // 2) * 2 * k
stream = torch.cuda.Stream()
s = stream.cuda_stream

rng = np.random.default_rng(3)


def mask(absent_of):
    m = np.zeros((B, n), np.uint8)
    m[:, :wn] = 1
    for b in range(B):
        m[b, absent_of(b)] = 0
    return torch.from_numpy(m).cuda()


masks = {
    "random_342": mask(lambda b: synth.erasure_indices(b, wn, min(342, wn - k - 1))),
    "all_present": mask(lambda b: np.empty(0, np.int64)),
    "systematic_half_parity": mask(lambda b: k + rng.choice(wn - k, (wn - k) // 2, replace=False)),
}

with torch.cuda.stream(stream):
    pay = synth.payload_batch_dev(0, B, plen, "cuda")
    shards = torch.empty((B, n, sl), dtype=torch.uint8, device="cuda")
    npa.encode_batch_dev(p, pay.data_ptr(), plen, plen, B, shards.data_ptr(), n * sl, ctx=ctx, stream=s)
    del pay
    a_out = torch.empty((B, olen), dtype=torch.uint8, device="cuda")
    a_shards = torch.empty((B, n, sl), dtype=torch.uint8, device="cuda")
    a_counts = torch.zeros((B,), dtype=torch.int64, device="cuda")
    b_counts = torch.zeros((B,), dtype=torch.int32, device="cuda")  # the call's uint32 entries
    words = (sl % 8 == 0)


def run_a(m):
    npa.reconstruct_batch_dev2(p, shards.data_ptr(), sl, n * sl, m.data_ptr(), 0, B, a_out.data_ptr(), olen, ctx=ctx,
                               stream=s)
    npa.encode_batch_dev(p, a_out.data_ptr(), olen, olen, B, a_shards.data_ptr(), n * sl, ctx=ctx, stream=s)
    x, y = (shards.view(torch.int64), a_shards.view(torch.int64)) if words else (shards, a_shards)
    torch.sum((x != y).any(dim=2) & (m != 0), dim=1, out=a_counts)


def run_b(m):
    npa.verify_shards_batch_dev(p, shards.data_ptr(), sl, n * sl, m.data_ptr(), B, b_counts.data_ptr(), ctx=ctx,
                                stream=s)


sides = [("A", run_a), ("B", run_b)]
if args.only:
    sides = [x for x in sides if x[0] == args.only]
calls = [(side + "_" + name, fn, m) for side, fn in sides for name, m in masks.items()]
times = {name: [] for name, _, _ in calls}
ok = True
with torch.cuda.stream(stream):
    # results first: codewords are consistent; one altered byte in a present parity row of payload 0 shows
    row = int(torch.nonzero(masks["random_342"][0, k:])[0]) + k
    for name, fn, m in calls:
        fn(m)
        got = a_counts if fn is run_a else b_counts
        ok = ok and bool((got == 0).all())
    shards[0, row, sl - 1] ^= 0x20
    for name, fn, m in calls:
        if not name.endswith("random_342"):
            continue
        fn(m)
        got = a_counts if fn is run_a else b_counts
        ok = ok and int(got[0]) > 0 and bool((got[1:] == 0).all())
    shards[0, row, sl - 1] ^= 0x20
    for rep in range(args.warmup + args.reps):
        for name, fn, m in calls:  # alternated: every repetition runs each call once
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            fn(m)
            t1.record(stream)
            t1.synchronize()
            if rep >= args.warmup:
                times[name].append(t0.elapsed_time(t1))


def summary(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


res = {"config": args.config, "n": n, "k": k, "wanted_n": wn, "payload_bytes": plen, "batch": B, "shard_len": sl,
       "reps": args.reps, "warmup": args.warmup, "unit": "ms per call", "compare_of_A": "torch",
       "calls": {name: summary(v) for name, v in times.items()}, "results_ok": bool(ok)}
if not args.only:
    res["B_over_A_median"] = {name: round(res["calls"]["B_" + name]["median"] / res["calls"]["A_" + name]["median"], 3)
                              for name in masks}
print(json.dumps(res))
