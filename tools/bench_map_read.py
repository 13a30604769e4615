#!/usr/bin/env python3
"""The map reads on the configs[3] shape (crdt_map_read, crdt_map_lookup), timed
with HIP events after a warm-up as bench.py times its steps.

    python tools/bench_map_read.py [--steps K] [--warmup W] [--m M ...] [--out FILE]

State: orset_merge of synth_set_tuples(2024, side, 10M, key space 8M) for both
sides, merged once outside the timed loops, with an 8-byte value column.  Every
leg of the read and both yardsticks alternate inside every step of ONE loop, so
each ratio is of two times from the same loop; the spread given beside a time
is the standard deviation over that loop's steps.  One JSON line per leg, with
this run's crdt_stream_read peak.  Legs:
  read          crdt_map_read with keys, per mode, without / with nsib
  map_values    the OR-Set read, then one crdt_src_gather of the value column
                chained off the device count
  lookup        crdt_map_lookup of m seeded probe keys (about 5 in 8 present),
                per mode, without / with nsib
Yardsticks, existing calls only:
  compose       what a caller composes without the read: crdt_set_compact in
                OR-Set mode under a 64-entry cut of 2^64-1 with source indices,
                an LWW crdt_set_compact of the result with source indices, one
                crdt_src_gather composing the two index arrays
  set_elements  crdt_set_elements with keys written (the same member keys,
                no winner)
Needs a GPU: there is no fallback."""
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


def timed(stream, steps, warmup, fns):
    """Per-step ms of each fn ([steps, len(fns)]), the fns alternating inside every step."""
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
    ap.add_argument("--m", type=int, nargs="+", default=[10**4, 10**5, 10**6], help="probes per lookup")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    eng = Engine(0)
    dev = eng.device
    stream = torch.cuda.current_stream(dev)
    peak = measure_peaks(eng)["read"]                   # GB/s
    lines = []

    def emit(d):
        d["stream_read_peak_GBps"] = peak
        lines.append(d)
        print(json.dumps(d), flush=True)

    n_side, ks = 10_000_000, 8_000_000
    t = eng.orset_merge(eng.synth_set_tuples(2024, 0, n_side, ks), eng.synth_set_tuples(2024, 1, n_side, ks))
    n = len(t)
    torch.cuda.empty_cache()
    i64 = lambda k: torch.empty(k, dtype=torch.int64, device=dev)
    val = torch.arange(n, dtype=torch.int64, device=dev)
    keys, win, oval = i64(n), i64(n), i64(n)
    nsib = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = {k: i64(1) for k in ("or", "or_nsib", "lww", "lww_nsib", "mv", "c1", "c2", "el")}
    cut = u64_tensor(np.full(64, 2**64 - 1, np.uint64), dev)
    c1, src1 = TupleSet.empty(n, dev), i64(n)
    c2, src2 = TupleSet.empty(n, dev), i64(n)
    ywin, ykeys = i64(n), i64(n)
    eng.reserve(256 << 20)

    def read(lww, sib, c):
        return lambda: eng.map_read(t, lww, keys=keys, win=win, nsib=nsib if sib else None, with_keys=True, count=c)

    def map_values():
        eng.map_read(t, False, keys=keys, win=win, count=cnt["mv"])
        eng.gather_src(win, val, val[:0], n_dev=cnt["mv"], out=oval)

    def compose():
        eng.set_compact(t, False, cut, out=c1, src=src1, count=cnt["c1"])
        eng.set_compact(c1, True, None, n_dev=cnt["c1"], out=c2, src=src2, count=cnt["c2"])
        eng.gather_src(src2, src1, src1[:0], n_dev=cnt["c2"], out=ywin)

    def set_elements():
        eng.set_elements(t, False, out=ykeys, count=cnt["el"])

    legs = [("read", "orset", False, read(False, False, cnt["or"])), ("read", "orset", True, read(False, True, cnt["or_nsib"])),
            ("read", "lww", False, read(True, False, cnt["lww"])), ("read", "lww", True, read(True, True, cnt["lww_nsib"])),
            ("map_values", "orset", False, map_values), ("yardstick_compose", "orset", False, compose),
            ("yardstick_set_elements", "orset", False, set_elements)]
    ms = timed(stream, args.steps, args.warmup, [f for *_, f in legs])
    rows = int(cnt["or"].item())
    if not (rows == int(cnt["c2"].item()) == int(cnt["el"].item()) == int(cnt["or_nsib"].item())):
        raise SystemExit("the read and its yardsticks disagree on the member count: no valid figures")
    if not torch.equal(win[:rows], ywin[:rows]):         # (win: the last leg that wrote it is the OR-Set map_values)
        raise SystemExit("the read's win differs from the composition's: no valid figures")
    mean, sd, mn = ms.mean(axis=0), ms.std(axis=0), ms.min(axis=0)
    yc, ye = 5, 6
    for j, (leg, mode, sib, _) in enumerate(legs):
        d = {"leg": leg, "mode": mode, "nsib": sib, "tuples": n, "rows": rows if mode == "orset" else int(cnt["lww"].item()),
             "ms": round(float(mean[j]), 4), "ms_sd": round(float(sd[j]), 4), "ms_min": round(float(mn[j]), 4),
             "spread": round(float(sd[j] / mean[j]), 4)}
        if j < yc:
            ratio = ms[:, j] / ms[:, yc]
            d.update({"time_over_compose": round(float(mean[j] / mean[yc]), 4),
                      "time_over_compose_per_step_min_max": [round(float(ratio.min()), 4), round(float(ratio.max()), 4)],
                      "time_over_set_elements": round(float(mean[j] / mean[ye]), 4)})
            nbytes = 21 * n + (16 + (4 if sib else 0)) * d["rows"] + (16 * d["rows"] if leg == "map_values" else 0)
            d.update({"algorithmic_bytes": int(nbytes), "frac_stream_read_peak": round(nbytes / mean[j] / 1e6 / peak, 3)})
        emit(d)
    flags = eng.device_status(clear=True)
    if flags:
        raise SystemExit(f"device-side failure flags 0x{flags:x}: no valid figures")

    rng = np.random.default_rng(2024)
    for m in args.m:
        probes = u64_tensor(rng.integers(0, ks, m).astype(np.uint64), dev)
        lw, ls = i64(m), torch.empty(m, dtype=torch.int32, device=dev)
        sorted_keys, hit = ykeys, None
        look = [("orset", False), ("orset", True), ("lww", False), ("lww", True)]
        fns = [(lambda lww=(mode == "lww"), sib=sib: eng.map_lookup(t, probes, lww, win=lw, nsib=ls if sib else None))
               for mode, sib in look]
        fns.append(lambda: eng.keys_contain(sorted_keys, probes, n_dev=cnt["el"]))
        ms = timed(stream, args.steps, args.warmup, fns)
        mean, sd, mn = ms.mean(axis=0), ms.std(axis=0), ms.min(axis=0)
        hit = int((lw >= 0).sum().item())
        for j, (mode, sib) in enumerate(look):
            emit({"leg": "lookup", "mode": mode, "nsib": sib, "m": m, "tuples": n, "ms": round(float(mean[j]), 4),
                  "ms_sd": round(float(sd[j]), 4), "ms_min": round(float(mn[j]), 4),
                  "Mprobes_per_s": round(m / mean[j] / 1e3, 1),
                  "time_over_keys_contain": round(float(mean[j] / mean[-1]), 3)})
        emit({"leg": "yardstick_keys_contain", "m": m, "keys": rows, "ms": round(float(mean[-1]), 4),
              "ms_sd": round(float(sd[-1]), 4), "ms_min": round(float(mn[-1]), 4), "lww_hits_last_lookup": hit})
        flags = eng.device_status(clear=True)
        if flags:
            raise SystemExit(f"device-side failure flags 0x{flags:x}: no valid figures")
    if args.out:
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
