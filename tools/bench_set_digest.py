#!/usr/bin/env python3
"""Range digests and the selection of flagged ranges on the configs[3] shape
(crdt_set_digest, crdt_set_select), timed with HIP events after a warm-up as
bench.py times its steps.

    python tools/bench_set_digest.py [--steps K] [--warmup W] [--out FILE]

Input: synth_set_tuples(2024, side, 10M, key space 8M) for both sides, merged
once outside the timed loop with lww_merge / orset_merge.  One JSON line per
leg: ms beside the yardstick's ms FROM THE SAME LOOP (all the calls alternate
inside every step), algorithmic bytes, and the fraction of this run's
crdt_stream_read peak those bytes over that time come to.  Legs, per mode:
  digest        m = 0, 255 and 65535 splitters (every ceil(n / (m + 1))-th key)
  select        over the 256 buckets, every 16th flagged, and all flagged
  yardstick     crdt_set_compact with no cut and no output (count only): the
                existing one-pass normaliser over the same tuples
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
from crdt_amd.engine import Engine, TupleSet         # noqa: E402
from crdt_amd.reconcile import key_splitters         # noqa: E402


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
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    eng = Engine(0)
    dev = eng.device
    stream = torch.cuda.current_stream(dev)
    peak = measure_peaks(eng)["read"]                   # GB/s
    lines = []

    def emit(leg, mode, mean, mn, nbytes, y_mean, y_bytes, **kw):
        d = {"leg": leg, "mode": mode, "ms": round(float(mean), 4), "ms_min": round(float(mn), 4),
             "algorithmic_bytes": int(nbytes), "GBps": round(nbytes / mean / 1e6, 1),
             "frac_stream_read_peak": round(nbytes / mean / 1e6 / peak, 3),
             "yardstick_ms_same_loop": round(float(y_mean), 4),
             "yardstick_frac_stream_read_peak": round(y_bytes / y_mean / 1e6 / peak, 3),
             "time_over_yardstick": round(float(mean / y_mean), 3), "stream_read_peak_GBps": peak,
             "yardstick": "set_compact_count_no_cut"}
        d.update(kw)
        lines.append(d)
        print(json.dumps(d), flush=True)

    n_side, ks = 10_000_000, 8_000_000
    A = eng.synth_set_tuples(2024, 0, n_side, ks)
    B = eng.synth_set_tuples(2024, 1, n_side, ks)
    for lww in (True, False):
        mode = "lww" if lww else "orset"
        t = (eng.lww_merge if lww else eng.orset_merge)(A, B)
        n = len(t)
        sps = {m: key_splitters(t, m) for m in (0, 255, 65535)}
        dig = {m: (torch.empty(m + 1, dtype=torch.int64, device=dev), torch.empty(m + 1, dtype=torch.int64, device=dev))
               for m in sps}
        some = (torch.arange(256, device=dev) % 16 == 0).to(torch.uint8)
        every = torch.ones(256, dtype=torch.uint8, device=dev)
        out = TupleSet.empty(n, dev)
        cnt, scnt, acnt = (torch.empty(1, dtype=torch.int64, device=dev) for _ in range(3))
        eng.reserve(64 << 20)
        fns = [lambda m=m: eng.set_digest(t, lww, sps[m] if m else None, hash_out=dig[m][0], count_out=dig[m][1])
               for m in sps]
        fns.append(lambda: eng.set_select(t, lww, sps[255], some, out=out, count=scnt))
        fns.append(lambda: eng.set_select(t, lww, sps[255], every, out=out, count=acnt))
        fns.append(lambda: eng.set_compact_count(t, lww, None, count=cnt))
        mean, mn = timed(stream, args.steps, args.warmup, *fns)
        y_ms, y_bytes = mean[-1], n * (9 if lww else 21)    # the count pass: LWW key + tomb; OR-Set all four fields
        assert int(cnt.item()) == n == int(acnt.item()) and int(dig[0][1].item()) == n
        for i, m in enumerate(sps):                         # a digest hashes all four fields of every canonical tuple
            emit("digest", mode, mean[i], mn[i], 21 * n + 16 * (m + 1) + 8 * m, y_ms, y_bytes, m=m, tuples=n,
                 nonempty_buckets=int((dig[m][1] != 0).sum().item()))
        for i, (name, c) in enumerate((("select_1_of_16", scnt), ("select_all", acnt))):
            k = int(c.item())
            emit(name, mode, mean[3 + i], mn[3 + i], 21 * n + 21 * k, y_ms, y_bytes, m=255, tuples=n, selected=k)
        flags = eng.device_status(clear=True)
        if flags:
            raise SystemExit(f"device-side failure flags 0x{flags:x}: no valid figures")
        del t, out, sps, dig
    if args.out:
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
