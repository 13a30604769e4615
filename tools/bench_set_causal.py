#!/usr/bin/env python3
"""The causal OR-Set merge on the configs[3] sorted set shape
(crdt_orset_merge_causal), timed with HIP events after a warm-up beside the
sibling calls over the same merged order, in one process on the same inputs.

    python tools/bench_set_causal.py [--steps K] [--warmup W] [--out FILE]

Input: synth_set_tuples(2024, side, 10M, key space 8M) for both sides A
(side 0) and B (side 1), sorted; contexts of 64 uniform values below 2^20, so
about half of the one-sided tags are covered.  Legs, alternating inside every
timed step:
  causal_count  out = NULL (the count alone)
  causal        tuples + merged context
  causal_src    tuples + source indices + merged context
  merge_src     crdt_orset_merge_src(A, B): the tombstone-form merge with
                source indices -- yardstick
  delta         crdt_set_delta(OR-Set, B, A): the two-sided sibling whose
                kernel form the causal merge copies -- yardstick
One JSON line per leg: the median, mean and minimum ms, the ratio of the
medians to each yardstick, algorithmic bytes, and the fraction of this run's
crdt_stream_read peak those bytes over the median come to.  Needs a GPU: there
is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import measure_peaks                      # noqa: E402
from crdt_amd.engine import Engine, TupleSet, u64_tensor   # noqa: E402


def timed(stream, steps, warmup, *fns):
    """ms of each fn per step [steps, len(fns)], the fns alternating inside every step."""
    for _ in range(warmup):
        for f in fns:
            f()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)] for _ in range(steps)]
    for row in evs:
        row[0].record(stream)
        for i, f in enumerate(fns):
            f()
            row[i + 1].record(stream)
    torch.cuda.synchronize()
    return np.array([[row[i].elapsed_time(row[i + 1]) for i in range(len(fns))] for row in evs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    eng = Engine(0)
    dev = eng.device
    stream = torch.cuda.current_stream(dev)
    peak = measure_peaks(eng)["read"]                   # GB/s
    n_side, ks = 10_000_000, 8_000_000
    A = eng.synth_set_tuples(2024, 0, n_side, ks)
    B = eng.synth_set_tuples(2024, 1, n_side, ks)
    rng = np.random.default_rng(2024)
    ca = u64_tensor(rng.integers(0, 2**20, 64).astype(np.uint64), dev)
    cb = u64_tensor(rng.integers(0, 2**20, 64).astype(np.uint64), dev)
    eng.reserve(256 << 20)
    na, nb = len(A), len(B)
    out, src = TupleSet.empty(na + nb, dev), torch.empty(na + nb, dtype=torch.int64, device=dev)
    ctx_out = torch.empty(64, dtype=torch.int64, device=dev)
    cnt, ccnt, mcnt, dcnt = (torch.empty(1, dtype=torch.int64, device=dev) for _ in range(4))
    mout, msrc = TupleSet.empty(na + nb, dev), torch.empty(na + nb, dtype=torch.int64, device=dev)
    dout = TupleSet.empty(nb, dev)
    legs = {
        "causal_count": lambda: eng.causal_merge_count(A, ca, B, cb, count=ccnt),
        "causal": lambda: eng.causal_merge(A, ca, B, cb, out=out, ctx_out=ctx_out, count=cnt),
        "causal_src": lambda: eng.causal_merge(A, ca, B, cb, out=out, src=src, ctx_out=ctx_out, count=cnt),
        "merge_src": lambda: mcnt.copy_(eng.orset_merge_src(A, B, out=mout, src=msrc)[1]),
        "delta": lambda: eng.set_delta(B, A, False, out=dout, count=dcnt),
    }
    names = list(legs)
    ms = timed(stream, args.steps, args.warmup, *legs.values())
    flags = eng.device_status(clear=True)
    if flags:
        raise SystemExit(f"device-side failure flags 0x{flags:x}: no valid figures")
    k, km, kd = int(cnt.item()), int(mcnt.item()), int(dcnt.item())
    if int(ccnt.item()) != k:
        raise SystemExit(f"the count-only call gives {int(ccnt.item())}, the full call {k}")
    med = dict(zip(names, np.median(ms, axis=0)))
    read = 21 * (na + nb)                               # the count pass: every field of both sides once
    nbytes = {
        "causal_count": read,
        "causal": read + 20 * k + 21 * k,               # + the write pass: key / ts / rep of each survivor read, 4 fields written
        "causal_src": read + 20 * k + 29 * k,           # + its source index
        "merge_src": read + 29 * km,
        "delta": read + 21 * kd,
    }
    notes = {
        "causal_count": "bytes: every field of both sides read once",
        "causal": "bytes: the count's reads + key / ts / rep of each surviving tag re-read + its 4 fields written",
        "causal_src": "bytes: as causal + 8 per surviving tag (the walk back to the first copy not counted)",
        "merge_src": "bytes: every field of both sides read once + the merged tuples and source indices written",
        "delta": "bytes: every field of both sides read once + the shipped tuples written",
    }
    lines = []
    for i, name in enumerate(names):
        m = float(med[name])
        d = {"leg": name, "ms_median": round(m, 4), "ms_mean": round(float(ms[:, i].mean()), 4),
             "ms_min": round(float(ms[:, i].min()), 4), "steps": args.steps, "warmup": args.warmup,
             "a": na, "b": nb, "n_ctx": 64, "survivors": k, "merged": km, "shipped": kd,
             "algorithmic_bytes": int(nbytes[name]), "GBps": round(nbytes[name] / m / 1e6, 1),
             "frac_stream_read_peak": round(nbytes[name] / m / 1e6 / peak, 3), "stream_read_peak_GBps": peak,
             "ratio_to_merge_src": round(m / float(med["merge_src"]), 3),
             "ratio_to_delta": round(m / float(med["delta"]), 3),
             "ratio_to_merge_src_plus_delta": round(m / float(med["merge_src"] + med["delta"]), 3),
             "note": notes[name]}
        lines.append(d)
        print(json.dumps(d), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
