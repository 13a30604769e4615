#!/usr/bin/env python3
"""The OR-Set mutators on the configs[3] shape (crdt_set_apply), timed with HIP
events after a warm-up as bench.py times its steps.

    python tools/bench_set_apply.py [--steps K] [--warmup W] [--m M ...] [--batch adds removes mixed] [--out FILE]

State: orset_merge of synth_set_tuples(2024, side, 10M, key space 8M) for both
sides, merged once outside the timed loops (ts < 2^20, rep < 64); the clock
holds 2^20 in every column, so every tag of the applying replica is covered.
Batches: seeded keys over the state's key space, sorted on the host, m = 10^4,
10^5 and 10^6, adds only / removes only / mixed, in both forms.  One JSON line
per leg: ms beside the yardstick's ms FROM THE SAME LOOP (the two calls
alternate inside every step), algorithmic bytes (21 B per tuple read, 21 B per
tuple written, 9 B per operation, plus source indices and the gather), and the
fraction of this run's crdt_stream_read peak those bytes over that time come
to.  Legs:
  tuples        the new state written out
  map           tuples + source indices + one crdt_src_gather of an 8-byte
                value column chained off the device count
  yardstick     existing code, never the code under test: for the adds-only
                tombstone legs crdt_orset_merge(t, the same tags built
                beforehand), which produces the same bytes; for every other leg
                crdt_set_compact(t, no cut), the one-pass normalisation of the
                same state.
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


def timed(stream, steps, warmup, *fns):
    """Mean / min ms of each fn, the fns alternating inside every step."""
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
    ms = np.array([[row[i].elapsed_time(row[i + 1]) for i in range(len(fns))] for row in evs])
    return ms.mean(axis=0), ms.min(axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--m", type=int, nargs="+", default=[10**4, 10**5, 10**6], help="batch sizes")
    ap.add_argument("--batch", nargs="+", default=["adds", "removes", "mixed"], choices=["adds", "removes", "mixed"])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    eng = Engine(0)
    dev = eng.device
    stream = torch.cuda.current_stream(dev)
    peak = measure_peaks(eng)["read"]                   # GB/s
    lines = []
    n_side, ks, rep = 10_000_000, 8_000_000, 7
    t = eng.orset_merge(eng.synth_set_tuples(2024, 0, n_side, ks), eng.synth_set_tuples(2024, 1, n_side, ks))
    n = len(t)
    torch.cuda.empty_cache()
    clock = u64_tensor(np.full(64, 2**20, np.uint64), dev)
    clock_out = torch.empty(64, dtype=torch.int64, device=dev)
    val = torch.arange(n, dtype=torch.int64, device=dev)
    m_max = max(args.m)
    cap = n + m_max
    out, src = TupleSet.empty(cap, dev), torch.empty(cap, dtype=torch.int64, device=dev)
    oval = torch.empty(cap, dtype=torch.int64, device=dev)
    yout = TupleSet.empty(cap, dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    ycnt = torch.empty(1, dtype=torch.int64, device=dev)
    eng.reserve(256 << 20)
    rng = np.random.default_rng(2024)
    for m in args.m:
        keys_h = np.sort(rng.integers(0, ks, m).astype(np.uint64))
        keys = u64_tensor(keys_h, dev)
        opv = torch.arange(m, dtype=torch.int64, device=dev)
        ts = np.uint64(2**20 + 1) + np.arange(m, dtype=np.uint64)
        tags = TupleSet.from_numpy(keys_h, ts, np.full(m, rep, np.uint32), np.zeros(m, np.uint8), dev)
        for kname, kinds_h in (("adds", np.zeros(m, np.uint8)), ("removes", np.ones(m, np.uint8)),
                               ("mixed", (rng.random(m) < 0.5).astype(np.uint8))):
            if kname not in args.batch:
                continue
            kinds = torch.from_numpy(kinds_h).to(dev)
            for causal in (False, True):
                form = "causal" if causal else "tombstone"
                if kname == "adds" and not causal:
                    yname, yard = "orset_merge_tags", lambda: eng.orset_merge(t, tags, out=yout, count=ycnt, trim=False)
                else:
                    yname, yard = "set_compact_no_cut", lambda: eng.set_compact(t, False, None, out=yout, count=ycnt)
                tup = lambda: eng.set_apply(t, clock, rep, keys, kinds, causal, out=out, clock_out=clock_out,
                                            count=cnt, trim=False)

                def mapc():
                    eng.set_apply(t, clock, rep, keys, kinds, causal, out=out, src=src, clock_out=clock_out, count=cnt,
                                  trim=False)
                    eng.gather_src(src, val, opv, n_dev=cnt, out=oval)

                for leg, fn in (("tuples", tup), ("map", mapc)):
                    (a_ms, y_ms), (a_mn, y_mn) = timed(stream, args.steps, args.warmup, fn, yard)
                    k, yk = int(cnt.item()), int(ycnt.item())
                    nbytes = 21 * n + 21 * k + 9 * m + (32 * k if leg == "map" else 0)
                    ybytes = 21 * n + 21 * yk + (21 * m if yname == "orset_merge_tags" else 0)
                    d = {"leg": leg, "form": form, "batch": kname, "m": m, "tuples": n, "out": k,
                         "ms": round(float(a_ms), 4), "ms_min": round(float(a_mn), 4), "algorithmic_bytes": int(nbytes),
                         "GBps": round(nbytes / a_ms / 1e6, 1),
                         "frac_stream_read_peak": round(nbytes / a_ms / 1e6 / peak, 3), "yardstick": yname,
                         "yardstick_ms_same_loop": round(float(y_ms), 4), "yardstick_ms_min": round(float(y_mn), 4),
                         "yardstick_frac_stream_read_peak": round(ybytes / y_ms / 1e6 / peak, 3),
                         "time_over_yardstick": round(float(a_ms / y_ms), 3), "stream_read_peak_GBps": peak}
                    lines.append(d)
                    print(json.dumps(d), flush=True)
                flags = eng.device_status(clear=True)
                if flags:
                    raise SystemExit(f"device-side failure flags 0x{flags:x}: no valid figures")
    if args.out:
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
