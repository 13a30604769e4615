#!/usr/bin/env python3
"""Set reads on the configs[3] shape: cardinality, elements and membership of
the merged LWW / OR-Set state (crdt_set_elements, crdt_u64_contains), timed
with HIP events after a warm-up as bench.py times its steps.

    python tools/bench_set_read.py [--steps K] [--warmup W] [--out FILE]

Input: synth_set_tuples(2024, side, 10M, key space 8M) for both sides, merged
once outside the timed loops with lww_merge / orset_merge.  One JSON line per
leg: ms, algorithmic bytes, and the fraction of this run's crdt_stream_read
peak those bytes over that time come to.  Legs, per mode:
  cardinality   keys_out = NULL (one pass over the tuples)
  elements      the live keys written out
  contains      1M probes into the element keys
  merge_empty   crdt_*_merge(t, {}) -- the one device pass over a set state
                there was before the reads; timed alternating with
                cardinality, the yardstick of DESIGN.md §5.9
  degenerate    cardinality / elements of 20M tuples of ONE key against 20M
                tuples over 8M keys (the carry scan must stay linear)
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
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    eng = Engine(0)
    dev = eng.device
    stream = torch.cuda.current_stream(dev)
    peak = measure_peaks(eng)["read"]                   # GB/s
    lines = []

    def emit(leg, mode, mean, mn, nbytes, **kw):
        d = {"leg": leg, "mode": mode, "ms": round(float(mean), 4), "ms_min": round(float(mn), 4),
             "algorithmic_bytes": int(nbytes), "GBps": round(nbytes / mean / 1e6, 1),
             "frac_stream_read_peak": round(nbytes / mean / 1e6 / peak, 3), "stream_read_peak_GBps": peak}
        d.update(kw)
        lines.append(d)
        print(json.dumps(d), flush=True)

    def tuple_bytes(n, lww):                            # what one pass over the state has to read
        return n * (9 if lww else 21)                   # LWW: key + tomb; OR-Set: key, ts, rep, tomb

    n_side, ks = 10_000_000, 8_000_000
    A = eng.synth_set_tuples(2024, 0, n_side, ks)
    B = eng.synth_set_tuples(2024, 1, n_side, ks)
    empty = TupleSet.empty(0, dev)
    rng = np.random.default_rng(2024)
    for lww in (True, False):
        mode = "lww" if lww else "orset"
        merge = eng.lww_merge if lww else eng.orset_merge
        t = merge(A, B)
        n = len(t)
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        cnt = torch.empty(1, dtype=torch.int64, device=dev)
        mout = TupleSet.empty(n, dev)
        mcnt = torch.empty(1, dtype=torch.int64, device=dev)
        eng.reserve(64 << 20)
        card = lambda: eng.set_cardinality(t, lww, count=cnt)
        elem = lambda: eng.set_elements(t, lww, out=keys, count=cnt)
        mrg = lambda: merge(t, empty, out=mout, count=mcnt, trim=False)
        (c_ms, m_ms), (c_mn, m_mn) = timed(stream, args.steps, args.warmup, card, mrg)
        (e_ms, m2_ms), (e_mn, m2_mn) = timed(stream, args.steps, args.warmup, elem, mrg)
        live = int(cnt.item())
        emit("cardinality", mode, c_ms, c_mn, tuple_bytes(n, lww), tuples=n, live=live)
        emit("merge_empty", mode, m_ms, m_mn, tuple_bytes(n, lww) + 21 * int(mcnt.item()), tuples=n,
             note="bytes: the state read once + the merged tuples written; alternating with cardinality")
        emit("elements", mode, e_ms, e_mn, tuple_bytes(n, lww) + 8 * n + n // 8 + 8 * live, tuples=n, live=live,
             merge_empty_ms_same_loop=round(float(m2_ms), 4))
        m = 1_000_000
        probes = u64_tensor(rng.integers(0, ks + ks // 4, m, dtype=np.uint64), dev)
        (p_ms,), (p_mn,) = timed(stream, args.steps, args.warmup,
                                 lambda: eng.keys_contain(keys, probes, n_dev=cnt))
        emit("contains", mode, p_ms, p_mn, 9 * m, probes=m, keys=live,
             note="bytes: the probes read + the flags written (the searches hit cache)")
        flags = eng.device_status(clear=True)
        if flags:
            raise SystemExit(f"device-side failure flags 0x{flags:x}: no valid figures")
        del t, keys, mout
    del A, B
    # one key over 20M tuples against 8M keys over 20M tuples, the same calls
    n20 = 20_000_000
    res = {}
    for ks1 in (8_000_000, 1):
        t = eng.synth_set_tuples(2024, 0, n20, ks1)
        keys = torch.empty(n20, dtype=torch.int64, device=dev)
        cnt = torch.empty(1, dtype=torch.int64, device=dev)
        for lww in (True, False):
            (c_ms, e_ms), _ = timed(stream, args.steps, args.warmup,
                                    lambda: eng.set_cardinality(t, lww, count=cnt),
                                    lambda: eng.set_elements(t, lww, out=keys, count=cnt))
            res[(ks1, lww)] = (float(c_ms), float(e_ms))
        del t, keys
    for lww in (True, False):
        mode = "lww" if lww else "orset"
        for i, leg in enumerate(("cardinality", "elements")):
            one, many = res[(1, lww)][i], res[(8_000_000, lww)][i]
            emit("degenerate_" + leg, mode, one, one, tuple_bytes(n20, lww), tuples=n20, key_space=1,
                 ms_key_space_8M=round(many, 4), ratio=round(one / many, 3))
    if args.out:
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
