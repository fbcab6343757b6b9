"""The payload, the missing shards and the verdict from one decode, device-
resident, at config 3 (n1024 k256, 1 MiB payloads, batch 1024): the three calls
a node composed before against np_recover_batch_dev, alternated in one process.

  R      np_reconstruct_batch_dev3 alone
  S      np_restore_shards_batch_dev alone
  V      np_verify_shards_batch_dev alone
  B_pr   np_recover_batch_dev: payload + restore
  B_pv   np_recover_batch_dev: payload + verify
  B_prv  np_recover_batch_dev: payload + restore + verify

Three presence patterns per payload: 342 random absent rows (the bench's), one
absent row, every row present.  Device events around each call; prints one JSON
line (times in ms: min / median / max over the repetitions) with the two
conditions of DESIGN.md §4.17 evaluated per pattern:

  in_band   median(B_pr) inside S's band and median(B_pv) inside V's -- the
            band is the call's own min..max widened by its width on each side;
  one_pass  median(B_prv) < median(S) + median(V) - median(R), one decode and
            the two existing encodes as separate launches.

results_ok: on a copy of the buffer with one byte of a present parity row of
every payload altered, each request combination gives exactly the outputs of
R, S and V.  Not the bench `value`."""
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
    "random_342": mask(lambda b: synth.erasure_indices(b, wn, min(342, wn - k))),
    "one_row": mask(lambda b: rng.integers(0, wn, 1)),
    "all_present": mask(lambda b: []),
}

with torch.cuda.stream(stream):
    pay = synth.payload_batch_dev(0, B, plen, "cuda")
    shards = torch.empty((B, n, sl), dtype=torch.uint8, device="cuda")
    npa.encode_batch_dev(p, pay.data_ptr(), plen, plen, B, shards.data_ptr(), n * sl, ctx=ctx, stream=s)
    del pay
    ref = shards.clone()
    out = torch.empty((B, olen), dtype=torch.uint8, device="cuda")
    cnt = torch.empty((B,), dtype=torch.int32, device="cuda")
    flags = torch.empty((B, n), dtype=torch.uint8, device="cuda")


def run_r(m, buf=None):
    npa.reconstruct_batch_dev2(p, (buf if buf is not None else shards).data_ptr(), sl, n * sl, m.data_ptr(), 0, B,
                               out.data_ptr(), olen, ctx=ctx, stream=s)


def run_s(m, buf=None):
    npa.restore_shards_batch_dev(p, (buf if buf is not None else shards).data_ptr(), sl, n * sl, m.data_ptr(), B,
                                 ctx=ctx, stream=s)


def run_v(m, buf=None):
    npa.verify_shards_batch_dev(p, (buf if buf is not None else shards).data_ptr(), sl, n * sl, m.data_ptr(), B,
                                cnt.data_ptr(), ctx=ctx, stream=s, d_mismatch=flags.data_ptr())


def recover(restore, verify):
    def run(m, buf=None):
        npa.recover_batch_dev(p, (buf if buf is not None else shards).data_ptr(), sl, n * sl, m.data_ptr(), B, ctx=ctx,
                              stream=s, d_out=out.data_ptr(), out_stride=olen, restore=restore,
                              d_bad_rows=cnt.data_ptr() if verify else 0, d_mismatch=flags.data_ptr() if verify else 0)
    return run


SIDES = [("R", run_r), ("S", run_s), ("V", run_v), ("B_pr", recover(True, False)), ("B_pv", recover(False, True)),
         ("B_prv", recover(True, True))]


def check(m):
    """Every side on `ref` with one byte of the first present parity row of each
    payload altered and the absent rows blanked: the new call's outputs against
    those of R, S and V."""
    work = ref.clone()
    first = (m[:, k:wn] != 0).to(torch.uint8).argmax(dim=1) + k
    work[torch.arange(B, device="cuda"), first, 7] ^= 0x40
    work[m == 0] = 0x5A
    got = {}
    for name, fn in SIDES:
        buf = work.clone()
        out.fill_(0xA5), cnt.fill_(7), flags.fill_(0xA5)
        fn(m, buf)
        got[name] = (out.clone(), buf, cnt.clone(), flags.clone())
    pay_r, rows_s, (cnt_v, map_v) = got["R"][0], got["S"][1], got["V"][2:]
    ok = bool((cnt_v > 0).all())  # the altered row shows
    for name, restore, verify in (("B_pr", True, False), ("B_pv", False, True), ("B_prv", True, True)):
        o, buf, c, f = got[name]
        ok = ok and bool(torch.equal(o, pay_r)) and bool(torch.equal(buf, rows_s if restore else work))
        if verify:
            ok = ok and bool(torch.equal(c, cnt_v)) and bool(torch.equal(f, map_v))
        else:
            ok = ok and bool((c == 7).all()) and bool((f == 0xA5).all())
    return ok


calls = [(side + "_" + name, fn, m) for name, m in masks.items() for side, fn in SIDES]
times = {name: [] for name, _, _ in calls}
ok = True
with torch.cuda.stream(stream):
    for name, m in masks.items():
        ok = check(m) and ok
    for rep in range(args.warmup + args.reps):
        for name, fn, m in calls:  # alternated: every repetition runs each call once
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            fn(m)
            t1.record(stream)
            t1.synchronize()
            if rep >= args.warmup:
                times[name].append(t0.elapsed_time(t1))
    ok = ok and bool(torch.equal(shards[:, :wn], ref[:, :wn]))  # the timed restores wrote the rows that were there


def summary(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


res = {"config": args.config, "n": n, "k": k, "wanted_n": wn, "payload_bytes": plen, "batch": B, "shard_len": sl,
       "reps": args.reps, "warmup": args.warmup, "unit": "ms per call",
       "calls": {name: summary(v) for name, v in times.items()}, "results_ok": bool(ok)}


def in_band(x, of):
    w = of["max"] - of["min"]
    return of["min"] - w <= x["median"] <= of["max"] + w


res["conditions"] = {}
for name in masks:
    c = {side: res["calls"][side + "_" + name] for side, _ in SIDES}
    bound = round(c["S"]["median"] + c["V"]["median"] - c["R"]["median"], 3)
    res["conditions"][name] = {
        "B_pr_in_S_band": in_band(c["B_pr"], c["S"]), "B_pv_in_V_band": in_band(c["B_pv"], c["V"]),
        "S_plus_V_minus_R": bound, "B_prv_below_it": c["B_prv"]["median"] < bound,
        "three_calls": round(c["R"]["median"] + c["S"]["median"] + c["V"]["median"], 3),
    }
print(json.dumps(res))
