#!/usr/bin/env python3
"""Tombstone compaction on the configs[3] shape and the stability cut on the
flagship population (crdt_set_compact, crdt_vclock_stable_cut), timed with HIP
events after a warm-up as bench.py times its steps.

    python tools/bench_set_compact.py [--steps K] [--warmup W] [--rows R] [--out FILE]

Input: synth_set_tuples(2024, side, 10M, key space 8M) for both sides, merged
once outside the timed loops with lww_merge / orset_merge (ts < 2^20, rep < 64,
a tenth of the tuples dead).  One JSON line per leg: ms beside the yardstick's
ms FROM THE SAME LOOP (the two calls alternate inside every step), algorithmic
bytes, and the fraction of this run's crdt_stream_read peak those bytes over
that time come to.  Legs, per mode and per cut (none; 2^19 - 1 in every
column: about half the dead tuples go; 2^20: all of them go):
  count         out = NULL (one pass over the tuples)
  tuples        the kept tuples written out
  map           tuples + source indices + one crdt_src_gather of an 8-byte
                value column chained off the device count
  yardstick     crdt_*_merge(t, {}) of the same state -- the only device pass
                that normalised a state before this one
Then crdt_vclock_stable_cut of a [rows x 128] population against
crdt_gcounter_fold of the same tensor in the same loop (same bytes, same
access pattern).  Needs a GPU: there is no fallback."""
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
    ap.add_argument("--rows", type=int, default=10_000_000, help="replicas of the stable-cut population (x 128 nodes)")
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
             "time_over_yardstick": round(float(mean / y_mean), 3), "stream_read_peak_GBps": peak}
        d.update(kw)
        lines.append(d)
        print(json.dumps(d), flush=True)

    n_side, ks = 10_000_000, 8_000_000
    A = eng.synth_set_tuples(2024, 0, n_side, ks)
    B = eng.synth_set_tuples(2024, 1, n_side, ks)
    empty = TupleSet.empty(0, dev)
    cuts = {"none": None, "half": u64_tensor(np.full(64, 2**19 - 1, np.uint64), dev),
            "all": u64_tensor(np.full(64, 2**20, np.uint64), dev)}
    for lww in (True, False):
        mode = "lww" if lww else "orset"
        merge = eng.lww_merge if lww else eng.orset_merge
        t = merge(A, B)
        n = len(t)
        dead = int(t.tomb.sum().item())
        val = torch.arange(n, dtype=torch.int64, device=dev)
        out, src = TupleSet.empty(n, dev), torch.empty(n, dtype=torch.int64, device=dev)
        oval = torch.empty(n, dtype=torch.int64, device=dev)
        cnt = torch.empty(1, dtype=torch.int64, device=dev)
        mout = TupleSet.empty(n, dev)
        mcnt = torch.empty(1, dtype=torch.int64, device=dev)
        eng.reserve(64 << 20)
        mrg = lambda: merge(t, empty, out=mout, count=mcnt, trim=False)
        read = n * (9 if lww else 21)                   # one pass: LWW key + tomb; OR-Set all four fields
        for cname, cut in cuts.items():
            count = lambda: eng.set_compact_count(t, lww, cut, count=cnt)
            tup = lambda: eng.set_compact(t, lww, cut, out=out, count=cnt)

            def mapc():
                eng.set_compact(t, lww, cut, out=out, src=src, count=cnt)
                eng.gather_src(src, val, val[:0], n_dev=cnt, out=oval)

            for leg, fn in (("count", count), ("tuples", tup), ("map", mapc)):
                (c_ms, m_ms), (c_mn, _) = timed(stream, args.steps, args.warmup, fn, mrg)
                k, mk = int(cnt.item()), int(mcnt.item())
                nbytes = {"count": read, "tuples": 21 * n + 21 * k, "map": 21 * n + 21 * k + 8 * k + 24 * k}[leg]
                emit(leg, mode, c_ms, c_mn, nbytes, m_ms, 21 * n + 21 * mk, cut=cname, tuples=n, dead=dead, kept=k,
                     dropped=mk - k, yardstick="merge_empty")
        flags = eng.device_status(clear=True)
        if flags:
            raise SystemExit(f"device-side failure flags 0x{flags:x}: no valid figures")
        del t, out, src, oval, mout, val
    del A, B
    torch.cuda.empty_cache()
    rows, nodes = args.rows, 128
    pop = eng.synth_counters(5, 4, rows, nodes)
    o1 = torch.empty(nodes, dtype=torch.int64, device=dev)
    o2 = torch.empty(nodes, dtype=torch.int64, device=dev)
    eng.reserve(64 << 20)
    (s_ms, f_ms), (s_mn, f_mn) = timed(stream, args.steps, args.warmup, lambda: eng.vclock_stable_cut(pop, out=o1),
                                       lambda: eng.gcounter_fold(pop, out=o2))
    nbytes = rows * nodes * 8
    emit("stable_cut", "vclock", s_ms, s_mn, nbytes, f_ms, nbytes, rows=rows, nodes=nodes, yardstick="gcounter_fold",
         yardstick_ms_min=round(float(f_mn), 4))
    if args.out:
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
