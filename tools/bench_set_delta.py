#!/usr/bin/env python3
"""Set deltas on the configs[3] shape: the tuples of one LWW / OR-Set state
another lacks (crdt_set_delta), timed with HIP events after a warm-up as
bench.py times its steps.

    python tools/bench_set_delta.py [--steps K] [--warmup W] [--out FILE]

Input: synth_set_tuples(2024, side, 10M, key space 8M) for both sides A
(side 0) and B (side 1).  Cases, per mode:
  b_vs_a      delta(B, A): what A still needs of B
  in_sync     delta(B, merge(A, B)): the in-sync test, an empty result
Legs per case, alternating inside every timed step:
  delta_count   out = NULL (the count alone)
  delta         the delta written out
  merge         crdt_*_merge(dst, src) of the same operands -- what a caller
                had to run before this call existed; the yardstick
One JSON line per leg: ms, the ratio to the same loop's merge, algorithmic
bytes, and the fraction of this run's crdt_stream_read peak those bytes over
that time come to.  Needs a GPU: there is no fallback."""
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

    def emit(leg, case, mode, mean, mn, nbytes, **kw):
        d = {"leg": leg, "case": case, "mode": mode, "ms": round(float(mean), 4), "ms_min": round(float(mn), 4),
             "algorithmic_bytes": int(nbytes), "GBps": round(nbytes / mean / 1e6, 1),
             "frac_stream_read_peak": round(nbytes / mean / 1e6 / peak, 3), "stream_read_peak_GBps": peak}
        d.update(kw)
        lines.append(d)
        print(json.dumps(d), flush=True)

    n_side, ks = 10_000_000, 8_000_000
    A = eng.synth_set_tuples(2024, 0, n_side, ks)
    B = eng.synth_set_tuples(2024, 1, n_side, ks)
    empty = TupleSet.empty(0, dev)
    eng.reserve(256 << 20)
    for lww in (True, False):
        mode = "lww" if lww else "orset"
        merge = eng.lww_merge if lww else eng.orset_merge
        src_keys = len(eng.lww_merge(B, empty))         # distinct keys of src: LWW reads ts / rep at their run ends
        AB = merge(A, B)
        for case, dst in (("b_vs_a", A), ("in_sync", AB)):
            ns, nd = len(B), len(dst)
            out = TupleSet.empty(ns, dev)
            cnt = torch.empty(1, dtype=torch.int64, device=dev)
            mout = TupleSet.empty(ns + nd, dev)
            mcnt = torch.empty(1, dtype=torch.int64, device=dev)
            count = lambda: eng.set_delta_count(B, dst, lww, count=cnt)
            full = lambda: eng.set_delta(B, dst, lww, out=out, count=cnt)
            mrg = lambda: merge(dst, B, out=mout, count=mcnt, trim=False)
            (c_ms, f_ms, m_ms), (c_mn, f_mn, m_mn) = timed(stream, args.steps, args.warmup, count, full, mrg)
            nship, nm = int(cnt.item()), int(mcnt.item())
            # the count: LWW every key + ts / rep of each src key's run end and of dst's; OR-Set every field
            read = 8 * (ns + nd) + 24 * src_keys if lww else 21 * (ns + nd)
            kw = dict(src=ns, dst=nd, shipped=nship, merge_ms_same_loop=round(float(m_ms), 4))
            emit("delta_count", case, mode, c_ms, c_mn, read, ratio_to_merge=round(float(c_ms / m_ms), 3), **kw)
            emit("delta", case, mode, f_ms, f_mn, read + 21 * nship, ratio_to_merge=round(float(f_ms / m_ms), 3),
                 note="bytes: the count's reads + the shipped tuples written", **kw)
            emit("merge", case, mode, m_ms, m_mn, 21 * (ns + nd) + 21 * nm, merged=nm, src=ns, dst=nd,
                 note="bytes: every field of both sides read once + the merged tuples written")
            if case == "in_sync" and nship != 0:
                raise SystemExit(f"delta(B, merge(A, B)) holds {nship} tuples, not 0")
            flags = eng.device_status(clear=True)
            if flags:
                raise SystemExit(f"device-side failure flags 0x{flags:x}: no valid figures")
            del out, mout
        del AB
    if args.out:
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
