"""The payload, the missing shards and the verdict of a HOST-memory batch at
config 3 (n1024 k256, 1 MiB payloads; batch 256): what a host caller composed
before against np_recover_batch_host, alternated in one process.

  A      np_reconstruct_batch_host, then np_encode_batch_host of the decoded
         payloads, then a numpy compare of the present parity rows with the
         re-encoding (A_compare: that part alone, included in A)
  B      np_recover_batch_host: payload + restore + verify (counts and map)
  B_p / B_r / B_v   np_recover_batch_host with one request

Three presence patterns per payload: 342 random absent rows (the bench's), one
absent row, every row present; pageable (numpy) and caller-pinned (torch
pin_memory) buffers.  Wall clock around the calls; prints one JSON line and
writes it to --out: ms as min / median / max over the repetitions, B / A of the
medians, and the PCIe bytes each side moves per payload, computed from the
masks.  results_ok: B's payloads, restored rows and verdict equal A's.
--stats: one more A and B per pattern with NP_PIPE_STATS=1 (the pipeline's time
split on stderr).  Not the bench `value`."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reed-solomon-novelpoly_amd", "python"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import novelpoly_amd as npa  # noqa: E402
from novelpoly_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=3)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recover_host", "config3.json"))
ap.add_argument("--stats", action="store_true")
args = ap.parse_args()

cfg = synth.CONFIGS[args.config]
p = npa.CodeParams.derive_parameters(cfg["n_wanted"], cfg["k_wanted"])
n, k, wn, plen = p.n(), p.k(), p.wanted_n, cfg["payload"]
B = args.batch
ctx = npa.Context(0)
sl = p.make_encoder(ctx).shard_len(plen)
olen = (sl // 2) * 2 * k
rng = np.random.default_rng(3)


def mask(absent_of):
    m = np.zeros((B, n), np.uint8)
    m[:, :wn] = 1
    for b in range(B):
        m[b, absent_of(b)] = 0
    return m


MASKS = {
    "random_342": mask(lambda b: synth.erasure_indices(b, wn, min(342, wn - k))),
    "one_row": mask(lambda b: rng.integers(0, wn, 1)),
    "all_present": mask(lambda b: []),
}


def codewords():
    """B codewords in host memory, one byte of a parity row of each altered."""
    pay = synth.payload_batch_dev(0, B, plen, "cuda")
    d = torch.empty((B, n, sl), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    npa.encode_batch_dev(p, pay.data_ptr(), plen, plen, B, d.data_ptr(), n * sl, ctx=ctx, stream=s)
    torch.cuda.synchronize()
    h = d.cpu().numpy()
    for b in range(B):
        h[b, k + b % (wn - k), 7] ^= 0x40
    return h


def host(shape, dtype, pinned):
    if pinned:
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True).numpy().view(dtype).reshape(shape)
    return np.empty(shape, dtype)


def moved(m):
    """PCIe bytes per payload, averaged over the batch: (A in, A out, B in, B out)."""
    systematic = bool(m[:, :k].all())
    rec_rows = m[:, :k].sum() if systematic else m.sum()  # what the reconstruct ships
    absent = (m[:, :wn] == 0).sum()
    a_in = rec_rows * sl / B + olen  # present rows, then the payload for the encode
    a_out = olen + wn * sl  # the payload, then every row of the re-encoding
    b_in = m.sum() * sl / B  # every present row: the compare reads the parity rows
    b_out = olen + absent * sl / B + 4 + n  # the payload, the restored rows, the count and the map
    return [int(round(x)) for x in (a_in, a_out, b_in, b_out)]


def summary(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def measure(kind, source):
    pinned = kind == "pinned"
    shards = host((B, n, sl), np.uint8, pinned)
    enc = host((B, wn, sl), np.uint8, pinned)
    out_a, out_b = host((B, olen), np.uint8, pinned), host((B, olen), np.uint8, pinned)
    cnt, flags = host((B,), np.uint32, pinned), host((B, n), np.uint8, pinned)
    pres = host((B, n), np.uint8, pinned)
    verdict = {}

    def run_a():
        npa.reconstruct_batch_host(p, shards.ctypes.data, sl, n * sl, pres.ctypes.data, B, out_a.ctypes.data, olen,
                                   ctx=ctx)
        npa.encode_batch_host(p, out_a.ctypes.data, olen, olen, B, enc.ctypes.data, wn * sl, ctx=ctx)
        t = time.perf_counter()
        bad = np.zeros((B, n), np.uint8)
        for b in range(B):
            rows = np.flatnonzero(pres[b, k:wn]) + k
            bad[b, rows] = (shards[b, rows] != enc[b, rows]).any(axis=1)
        verdict["map"], verdict["compare_ms"] = bad, (time.perf_counter() - t) * 1e3

    def recover(with_out, restore, verify):
        def run():
            npa.recover_batch_host(p, shards.ctypes.data, sl, n * sl, pres.ctypes.data, B, ctx=ctx,
                                   out=out_b.ctypes.data if with_out else 0, out_stride=olen if with_out else 0,
                                   restore=restore, bad_rows=cnt.ctypes.data if verify else 0,
                                   mismatch=flags.ctypes.data if verify else 0)
        return run

    sides = [("A", run_a), ("B", recover(True, True, True)), ("B_p", recover(True, False, False)),
             ("B_r", recover(False, True, False)), ("B_v", recover(False, False, True))]
    res, ok = {}, True
    for name, m in MASKS.items():
        pres[...] = m
        shards[...] = source
        shards[m == 0] = 0x5A  # the absent rows: never read, restored by B
        times = {side: [] for side, _ in sides}
        times["A_compare"] = []
        for rep in range(args.warmup + args.reps):
            for side, fn in sides:  # alternated: every repetition runs each side once
                t = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t) * 1e3
                if rep >= args.warmup:
                    times[side].append(dt)
                    if side == "A":
                        times["A_compare"].append(verdict["compare_ms"])
        # B's answers against A's: the payloads, the verdict, the restored rows
        ok = ok and np.array_equal(out_a, out_b) and np.array_equal(flags, verdict["map"])
        ok = ok and np.array_equal(cnt, verdict["map"].sum(axis=1)) and bool(cnt.any())
        ok = ok and all(np.array_equal(shards[b, :wn][m[b, :wn] == 0], enc[b][m[b, :wn] == 0]) for b in range(0, B, 16))
        calls = {side: summary(v) for side, v in times.items()}
        a_in, a_out, b_in, b_out = moved(m)
        res[name] = {"calls": calls, "B_over_A": round(calls["B"]["median"] / calls["A"]["median"], 3),
                     "B_below_A_minus_spread": calls["B"]["median"] < calls["A"]["median"] - (calls["A"]["max"] -
                                                                                             calls["A"]["min"]),
                     "pcie_bytes_per_payload": {"A_in": a_in, "A_out": a_out, "B_in": b_in, "B_out": b_out,
                                                "B_over_A": round((b_in + b_out) / (a_in + a_out), 3)}}
        if args.stats:
            os.environ["NP_PIPE_STATS"] = "1"
            print(f"-- {kind} {name}: A (reconstruct, encode), then B", file=sys.stderr, flush=True)
            run_a()
            sides[1][1]()
            del os.environ["NP_PIPE_STATS"]
    return res, ok


source = codewords()
result = {"config": args.config, "n": n, "k": k, "wanted_n": wn, "payload_bytes": plen, "batch": B, "shard_len": sl,
          "reps": args.reps, "warmup": args.warmup, "unit": "ms per call, wall clock", "buffers": {}}
all_ok = True
for kind in ("pageable", "pinned"):
    result["buffers"][kind], ok = measure(kind, source)
    all_ok = all_ok and ok
result["results_ok"] = bool(all_ok)
line = json.dumps(result)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(line + "\n")
