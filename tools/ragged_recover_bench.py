"""The payload, the missing shards and the verdict of a mixed-size batch from
one decode, device-resident, at config 3 (n1024 k256, batch 1024): what a node
had to do before np_recover_ragged_dev against it, alternated in one process.

  A_pr / A_pv / A_prv   np_recover_batch_dev on buffers padded to the longest
                        item (1 MiB payloads).  The padding copy is not timed.
  A_S / A_V             np_restore_shards_batch_dev / np_verify_shards_batch_dev
                        on the padded buffer (for the `equal` ratios)
  R / S / V             np_reconstruct_ragged_dev / np_restore_shards_ragged_dev /
                        np_verify_shards_ragged_dev alone on the packed buffer
  B_pr / B_pv / B_prv   np_recover_ragged_dev: payload + restore, payload +
                        verify, all three

Two cases: `mixed`, lengths 1 MiB * ((i % 8) + 1) / 8 permuted by a fixed seed
(tools/ragged_bench.py's mix: B does 0.5625 of A's tiles), and `equal`, every
length 1 MiB.  Three presence patterns per item: 342 random absent rows (the
bench's), one absent row, every row present.  Device events around each call;
prints one JSON line (times in ms: min / median / max over the repetitions) and
writes it to --out, with the conditions of DESIGN.md §4.18 per case and pattern:

  in_band     median(B_pr) inside or below S's band and median(B_pv) inside or
              below V's -- the band is the call's own min..max widened by its
              width on each side;
  one_pass    median(B_prv) < median(S) + median(V) - median(R): one decode and
              the two existing ragged encodes as separate launches;
  padded      median(B_prv) < min(A_prv) (asked of `mixed`; on `equal` the ratio
              is reported next to S / A_S and V / A_V).

results_ok: on a copy of the packed buffer with one byte of a present parity row
of every item altered and the absent rows blanked, each request combination of
B gives exactly the outputs of R, S and V.  Not the bench `value`."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_recover", "config3.json"))
args = ap.parse_args()

cfg = synth.CONFIGS[args.config]
p = npa.CodeParams.derive_parameters(cfg["n_wanted"], cfg["k_wanted"])
n, k, wn, pmax = p.n(), p.k(), p.wanted_n, cfg["payload"]
B = args.batch or cfg["batch"]
ctx = npa.Context(0)
rs = p.make_encoder(ctx)
slmax = rs.shard_len(pmax)
omax = (slmax // 2) * 2 * k
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


def summary(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def in_or_below_band(x, of):
    return x["median"] <= of["max"] + (of["max"] - of["min"])


def run_case(name):
    if name == "mixed":
        lens = [pmax * ((i % 8) + 1) // 8 for i in range(B)]
        lens = [lens[i] for i in np.random.default_rng(3).permutation(B)]
    else:
        lens = [pmax] * B
    sls = [rs.shard_len(x) for x in lens]
    items, poff, ooff, soff = [], 0, 0, 0
    for x, sl in zip(lens, sls):
        items.append((poff, x, soff, sl))
        poff += x
        soff += n * sl
    # the decode's items: the outputs padded to whole columns, packed
    rec_items = []
    for (_, x, so, sl) in items:
        rec_items.append((ooff, x, so, sl))
        ooff += (sl // 2) * 2 * k
    items_c = npa.ragged_items(items)  # the arrays a C caller holds: not converted per call
    rec_c = npa.ragged_items(rec_items)
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
        a_out = torch.empty((B, omax), dtype=torch.uint8, device="cuda")
        b_out = torch.empty(ooff, dtype=torch.uint8, device="cuda")
        cnt = torch.empty(B, dtype=torch.int32, device="cuda")
        flags = torch.empty((B, n), dtype=torch.uint8, device="cuda")

    def a_recover(restore, verify):
        def run(m, buf=None):
            npa.recover_batch_dev(p, a_shards.data_ptr(), slmax, n * slmax, m.data_ptr(), B, ctx=ctx, stream=s,
                                  d_out=a_out.data_ptr(), out_stride=omax, restore=restore,
                                  d_bad_rows=cnt.data_ptr() if verify else 0,
                                  d_mismatch=flags.data_ptr() if verify else 0)
        return run

    def a_s(m, buf=None):
        npa.restore_shards_batch_dev(p, a_shards.data_ptr(), slmax, n * slmax, m.data_ptr(), B, ctx=ctx, stream=s)

    def a_v(m, buf=None):
        npa.verify_shards_batch_dev(p, a_shards.data_ptr(), slmax, n * slmax, m.data_ptr(), B, cnt.data_ptr(), ctx=ctx,
                                    stream=s, d_mismatch=flags.data_ptr())

    def run_r(m, buf=None):
        npa.reconstruct_ragged_dev(p, (b_shards if buf is None else buf).data_ptr(), soff, m.data_ptr(),
                                   b_out.data_ptr(), ooff, rec_c, ctx=ctx, stream=s)

    def run_s(m, buf=None):
        npa.restore_shards_ragged_dev(p, (b_shards if buf is None else buf).data_ptr(), soff, m.data_ptr(), items_c,
                                      ctx=ctx, stream=s)

    def run_v(m, buf=None):
        npa.verify_shards_ragged_dev(p, (b_shards if buf is None else buf).data_ptr(), soff, m.data_ptr(), items_c,
                                     cnt.data_ptr(), ctx=ctx, stream=s, d_mismatch=flags.data_ptr())

    def b_recover(restore, verify):
        def run(m, buf=None):
            npa.recover_ragged_dev(p, (b_shards if buf is None else buf).data_ptr(), soff, m.data_ptr(), rec_c,
                                   d_out=b_out.data_ptr(), out_size=ooff, restore=restore,
                                   d_bad_rows=cnt.data_ptr() if verify else 0,
                                   d_mismatch=flags.data_ptr() if verify else 0, ctx=ctx, stream=s)
        return run

    ragged = [("R", run_r), ("S", run_s), ("V", run_v), ("B_pr", b_recover(True, False)),
              ("B_pv", b_recover(False, True)), ("B_prv", b_recover(True, True))]
    sides = [("A_pr", a_recover(True, False)), ("A_pv", a_recover(False, True)), ("A_prv", a_recover(True, True)),
             ("A_S", a_s), ("A_V", a_v)] + ragged

    def check(m):
        """Every ragged side on the packed codewords with one byte of the first
        present parity row of each item altered and the absent rows blanked:
        the new call's outputs against those of R, S and V."""
        work = b_ref.clone()
        first = ((m[:, k:wn] != 0).to(torch.uint8).argmax(dim=1) + k).tolist()
        for b, (_, _, so, sl) in enumerate(items):
            rows = work[so:so + n * sl].view(n, sl)
            rows[first[b], 7 % sl] ^= 0x40
            rows[m[b] == 0] = 0x5A
        got = {}
        for side, fn in ragged:
            buf = work.clone()
            b_out.fill_(0xA5), cnt.fill_(7), flags.fill_(0xA5)
            fn(m, buf)
            got[side] = (b_out.clone(), buf, cnt.clone(), flags.clone())
        pay_r, rows_s, (cnt_v, map_v) = got["R"][0], got["S"][1], got["V"][2:]
        good = bool((cnt_v > 0).all())  # the altered row shows
        for side, restore, verify in (("B_pr", True, False), ("B_pv", False, True), ("B_prv", True, True)):
            o, buf, c, f = got[side]
            good = good and bool(torch.equal(o, pay_r)) and bool(torch.equal(buf, rows_s if restore else work))
            if verify:
                good = good and bool(torch.equal(c, cnt_v)) and bool(torch.equal(f, map_v))
            else:
                good = good and bool((c == 7).all()) and bool((f == 0xA5).all())
        return good

    calls = [(side + "_" + pat, fn, m) for pat, m in masks.items() for side, fn in sides]
    times = {c: [] for c, _, _ in calls}
    ok = True
    with torch.cuda.stream(stream):
        for pat, m in masks.items():
            ok = check(m) and ok
        for rep in range(args.warmup + args.reps):
            for c, fn, m in calls:  # alternated: every repetition runs each call once
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                fn(m)
                t1.record(stream)
                t1.synchronize()
                if rep >= args.warmup:
                    times[c].append(t0.elapsed_time(t1))
        # the timed restores wrote the rows that were there
        ok = ok and bool(torch.equal(b_shards, b_ref)) and bool(torch.equal(a_shards, a_ref))
    tiles_a = B * ((slmax // 2 + 255) // 256)
    tiles_b = sum((sl // 2 + 255) // 256 for sl in sls)
    res = {"payload_bytes_total": sum(lens), "tiles_A": tiles_a, "tiles_B": tiles_b,
           "tiles_B_over_A": round(tiles_b / tiles_a, 4),
           "calls": {c: summary(v) for c, v in times.items()}, "results_ok": bool(ok), "conditions": {}}
    for pat in masks:
        c = {side: res["calls"][side + "_" + pat] for side, _ in sides}
        bound = round(c["S"]["median"] + c["V"]["median"] - c["R"]["median"], 3)
        res["conditions"][pat] = {
            "B_pr_in_or_below_S_band": in_or_below_band(c["B_pr"], c["S"]),
            "B_pv_in_or_below_V_band": in_or_below_band(c["B_pv"], c["V"]),
            "S_plus_V_minus_R": bound, "B_prv_below_it": c["B_prv"]["median"] < bound,
            "three_calls": round(c["R"]["median"] + c["S"]["median"] + c["V"]["median"], 3),
            "B_prv_below_A_prv_min": c["B_prv"]["median"] < c["A_prv"]["min"],
            "B_prv_over_A_prv": round(c["B_prv"]["median"] / c["A_prv"]["median"], 3),
            "B_pr_over_A_pr": round(c["B_pr"]["median"] / c["A_pr"]["median"], 3),
            "B_pv_over_A_pv": round(c["B_pv"]["median"] / c["A_pv"]["median"], 3),
            "S_over_A_S": round(c["S"]["median"] / c["A_S"]["median"], 3),
            "V_over_A_V": round(c["V"]["median"] / c["A_V"]["median"], 3),
        }
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
