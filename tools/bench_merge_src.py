#!/usr/bin/env python3
"""The payload-carrying set merges on the configs[3] shape: what the source
indices (crdt_*_merge_src) and the gather of one value column by them
(crdt_src_gather) cost beside the plain merge, timed with HIP events after a
warm-up as bench.py times its steps.

    python tools/bench_merge_src.py [--steps K] [--warmup W] [--out FILE]

Input: bench.py's lww_merge / orset_merge sides -- synth_set_tuples(2024, side,
10M, key space 8M), sorted.  Legs per mode, alternating inside every timed
step (one process, one loop: the ratios do not carry run-to-run drift):
  merge        crdt_*_merge -- the yardstick
  merge_src    crdt_*_merge_src: the same passes, 8 more bytes stored per
               output tuple beside its 21, no byte more read
  map_merge    merge_src, then crdt_src_gather of an 8-byte value column by
               the merge's device count (Engine.*_map_merge's two calls)
One JSON line per leg: ms, the ratio to the same loop's merge, algorithmic
bytes, the ratio of those bytes to the merge's (the traffic ratio), GB/s.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
    ap.add_argument("--set-n", type=int, default=10_000_000)
    ap.add_argument("--key-space", type=int, default=8_000_000)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    eng = Engine(0)
    dev = eng.device
    stream = torch.cuda.current_stream(dev)
    lines = []
    n = args.set_n
    A = eng.synth_set_tuples(2024, 0, n, args.key_space)
    B = eng.synth_set_tuples(2024, 1, n, args.key_space)
    va = torch.arange(n, dtype=torch.int64, device=dev)
    vb = torch.arange(n, dtype=torch.int64, device=dev) | (-(1 << 63))
    eng.reserve(256 << 20)
    for lww in (True, False):
        mode = "lww" if lww else "orset"
        merge = eng.lww_merge if lww else eng.orset_merge
        merge_src = eng.lww_merge_src if lww else eng.orset_merge_src
        out = TupleSet.empty(2 * n, dev)
        cnt = torch.empty(1, dtype=torch.int64, device=dev)
        src = torch.empty(2 * n, dtype=torch.int64, device=dev)
        val = torch.empty(2 * n, dtype=torch.int64, device=dev)
        got = {}

        def plain():
            merge(A, B, out=out, count=cnt, trim=False)

        def with_src():
            got["cnt"] = merge_src(A, B, out=out, src=src)[1]

        def map_merge():
            _, c, s = merge_src(A, B, out=out, src=src)
            eng.gather_src(s, va, vb, n_dev=c, out=val)

        (p_ms, s_ms, m_ms), (p_mn, s_mn, m_mn) = timed(stream, args.steps, args.warmup, plain, with_src, map_merge)
        n_out = int(cnt.item())
        if int(got["cnt"].item()) != n_out:
            raise SystemExit("merge_src and the plain merge disagree on the count")
        v = val[:n_out]
        s = src[:n_out]
        ok = torch.equal(torch.where(v >= 0, v, -(v & ((1 << 63) - 1)) - 1), s)
        flags = eng.device_status(clear=True)
        if flags or not ok:
            raise SystemExit(f"device flags 0x{flags:x}, values decode to src: {ok}: no valid figures")
        rd, st = 21 * 2 * n, 21 * n_out                      # every field of both sides read once; the tuples stored
        legs = (("merge", p_ms, p_mn, rd, st, "both sides read once, the merged tuples stored"),
                ("merge_src", s_ms, s_mn, rd, st + 8 * n_out, "the merge's, + 8 bytes stored per output (src)"),
                ("map_merge", m_ms, m_mn, rd + 16 * n_out, st + 16 * n_out,
                 "merge_src's, + per output src and one 8-byte value read, the value stored"))
        for leg, mean, mn, rbytes, sbytes, note in legs:
            nbytes = rbytes + sbytes
            d = {"leg": leg, "mode": mode, "ms": round(float(mean), 4), "ms_min": round(float(mn), 4),
                 "ratio_to_merge": round(float(mean / p_ms), 4), "algorithmic_bytes": int(nbytes),
                 "traffic_ratio_to_merge": round(nbytes / (rd + st), 4),
                 "store_ratio_to_merge": round(sbytes / st, 4),
                 "GBps": round(nbytes / mean / 1e6, 1), "tuples_per_side": n, "n_out": n_out, "note": note}
            lines.append(d)
            print(json.dumps(d), flush=True)
        del out, src, val
    if args.out:
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
