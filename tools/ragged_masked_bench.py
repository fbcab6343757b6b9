"""Restore and verify on a mixed-size batch, device-resident, at config 3
(n1024 k256, batch 1024): what a caller had to do before the ragged restore and
verify against them, alternated in one process.

  A  np_restore_shards_batch_dev / np_verify_shards_batch_dev on a shard buffer
     padded to the longest item (1 MiB payloads).  The padding copy is not timed.
  B  np_restore_shards_ragged_dev / np_verify_shards_ragged_dev on the packed
     buffer.

Two cases: `mixed`, lengths 1 MiB * ((i % 8) + 1) / 8 permuted by a fixed seed
(tools/ragged_bench.py's mix: B does 0.5625 of A's tiles), and `equal`, every
length 1 MiB.  Restore patterns: the bench's 342 random absent rows, and one
absent row.  Verify patterns: all but those 342 rows present, and every row
present.  Device events around each call; prints one JSON line (times in ms:
min / median / max over the repetitions) and writes it to --out when given.
Not the bench `value`."""
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
ap.add_argument("--cases", default="mixed,equal")
ap.add_argument("--out", default="", help="also write the JSON line to this file")
args = ap.parse_args()

cfg = synth.CONFIGS[args.config]
p = npa.CodeParams.derive_parameters(cfg["n_wanted"], cfg["k_wanted"])
n, k, wn, pmax = p.n(), p.k(), p.wanted_n, cfg["payload"]
B = args.batch or cfg["batch"]
ctx = npa.Context(0)
rs = p.make_encoder(ctx)
slmax = rs.shard_len(pmax)
stream = torch.cuda.Stream()
s = stream.cuda_stream
rng = np.random.default_rng(3)


def mask(absent_of):
    m = np.zeros((B, n), np.uint8)
    m[:, :wn] = 1
    for b in range(B):
        m[b, absent_of(b)] = 0
    return torch.from_numpy(m).cuda()


with torch.cuda.stream(stream):
    masks = {
        "random_342": mask(lambda b: synth.erasure_indices(b, wn, min(342, wn - k))),
        "one_row": mask(lambda b: rng.integers(0, wn, 1)),
        "all_present": mask(lambda b: []),
    }
RESTORE = ["random_342", "one_row"]
VERIFY = ["random_342", "all_present"]


def summary(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def run_case(name):
    if name == "mixed":
        lens = [pmax * ((i % 8) + 1) // 8 for i in range(B)]
        lens = [lens[i] for i in np.random.default_rng(3).permutation(B)]
    else:
        lens = [pmax] * B
    sls = [rs.shard_len(x) for x in lens]
    items, poff, soff = [], 0, 0
    for x, sl in zip(lens, sls):
        items.append((poff, x, soff, sl))
        poff += x
        soff += n * sl
    items_c = npa.ragged_items(items)  # the array a C caller holds: not converted per call
    with torch.cuda.stream(stream):
        padded = synth.payload_batch_dev(0, B, pmax, "cuda")
        packed = torch.empty(poff, dtype=torch.uint8, device="cuda")
        for b, (po, x, _, _) in enumerate(items):
            packed[po:po + x] = padded[b, :x]
            padded[b, x:] = 0  # A pads with zeros: zero columns encode to zero columns
        a_ref = torch.zeros((B, n, slmax), dtype=torch.uint8, device="cuda")
        b_ref = torch.zeros(soff, dtype=torch.uint8, device="cuda")
        npa.encode_batch_dev(p, padded.data_ptr(), pmax, pmax, B, a_ref.data_ptr(), n * slmax, ctx=ctx, stream=s)
        npa.encode_ragged_dev(p, packed.data_ptr(), poff, b_ref.data_ptr(), soff, items_c, ctx=ctx, stream=s)
        del padded, packed
        a_shards, b_shards = a_ref.clone(), b_ref.clone()
        a_cnt = torch.empty(B, dtype=torch.int32, device="cuda")
        b_cnt = torch.empty(B, dtype=torch.int32, device="cuda")

    def restore_a(m):
        npa.restore_shards_batch_dev(p, a_shards.data_ptr(), slmax, n * slmax, m.data_ptr(), B, ctx=ctx, stream=s)

    def restore_b(m):
        npa.restore_shards_ragged_dev(p, b_shards.data_ptr(), soff, m.data_ptr(), items_c, ctx=ctx, stream=s)

    def verify_a(m):
        npa.verify_shards_batch_dev(p, a_shards.data_ptr(), slmax, n * slmax, m.data_ptr(), B, a_cnt.data_ptr(), ctx=ctx,
                                    stream=s)

    def verify_b(m):
        npa.verify_shards_ragged_dev(p, b_shards.data_ptr(), soff, m.data_ptr(), items_c, b_cnt.data_ptr(), ctx=ctx,
                                     stream=s)

    calls = []
    for pat in RESTORE:
        calls += [(f"restore_{pat}_A", restore_a, masks[pat]), (f"restore_{pat}_B", restore_b, masks[pat])]
    for pat in VERIFY:
        calls += [(f"verify_{pat}_A", verify_a, masks[pat]), (f"verify_{pat}_B", verify_b, masks[pat])]
    times = {c: [] for c, _, _ in calls}
    ok = True
    with torch.cuda.stream(stream):
        # results first: both restore the blanked rows of their buffers, and both find a codeword consistent
        for pat in RESTORE:
            m = masks[pat]
            a_shards[m == 0] = 0x5A
            for b, (_, _, so, sl) in enumerate(items):
                b_shards[so:so + n * sl].view(n, sl)[m[b] == 0] = 0x5A
            restore_a(m)
            restore_b(m)
            # (A's padding columns of an absent row come back as the zero columns they were)
            ok = ok and bool(torch.equal(a_shards, a_ref)) and bool(torch.equal(b_shards, b_ref))
        for pat in VERIFY:
            verify_a(masks[pat])
            verify_b(masks[pat])
            ok = ok and not bool(a_cnt.any()) and not bool(b_cnt.any())
        for rep in range(args.warmup + args.reps):
            for c, fn, m in calls:  # alternated: every repetition runs each call once
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                fn(m)
                t1.record(stream)
                t1.synchronize()
                if rep >= args.warmup:
                    times[c].append(t0.elapsed_time(t1))
    tiles_a = B * ((slmax // 2 + 255) // 256)
    tiles_b = sum((sl // 2 + 255) // 256 for sl in sls)
    res = {"payload_bytes_total": sum(lens), "tiles_A": tiles_a, "tiles_B": tiles_b,
           "tiles_B_over_A": round(tiles_b / tiles_a, 4),
           "calls": {c: summary(v) for c, v in times.items()}, "results_ok": bool(ok)}
    names = [f"restore_{pat}" for pat in RESTORE] + [f"verify_{pat}" for pat in VERIFY]
    res["B_over_A_median"] = {d: round(res["calls"][d + "_B"]["median"] / res["calls"][d + "_A"]["median"], 3)
                              for d in names}
    res["B_median_below_A_min"] = {d: bool(res["calls"][d + "_B"]["median"] <= res["calls"][d + "_A"]["min"])
                                   for d in names}
    return res


out = {"config": args.config, "n": n, "k": k, "wanted_n": wn, "max_payload_bytes": pmax, "batch": B,
       "reps": args.reps, "warmup": args.warmup, "unit": "ms per call",
       "cases": {c: run_case(c) for c in args.cases.split(",")}}
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
