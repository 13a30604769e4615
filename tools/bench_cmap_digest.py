#!/usr/bin/env python3
"""Range digests of a counter map and the selection of flagged ranges
(crdt_cmap_digest, crdt_cmap_select) on the state tools/bench_cmap.py builds,
timed with HIP events after a warm-up as bench.py times its steps.

    python tools/bench_cmap_digest.py [--n N] [--steps K] [--warmup W] [--out FILE]

Input: bench_cmap's two seeded states of n cells (8 replicas a key, about half
the cells shared) and the same cells as an OR-Set of unique tags.  One JSON
line per leg: ms, algorithmic bytes, the fraction of this run's
crdt_stream_read peak those bytes over that time come to, and picoseconds per
byte beside the comparison leg's FROM THE SAME LOOP (all the calls alternate
inside every step).  Legs:
  digest        m = 0, 255 and 65535 splitters (every ceil(n / (m + 1))-th key),
                28 B a cell read; compared per byte read with crdt_set_digest
                (OR-Set mode, 21 B a tuple) at the same m
  select        over the 256 buckets, every 16th flagged, and all flagged: 8 B a
                cell read by the count pass, 28 B read and 28 B written a shipped
                cell; compared per byte moved with crdt_cmap_delta of the pair
  cmap_merge    of the same pair, the loop's yardstick
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench import measure_peaks                      # noqa: E402
from bench_cmap import _cmap, _ids, _tuples          # noqa: E402
from bench_set_digest import timed                   # noqa: E402
from crdt_amd.engine import CounterMap, Engine       # noqa: E402
from crdt_amd.reconcile import key_splitters         # noqa: E402

MS = (0, 255, 65535)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    eng = Engine(0)
    dev = eng.device
    stream = torch.cuda.current_stream(dev)
    peak = measure_peaks(eng)["read"]                   # GB/s
    n = args.n
    ia, ib = _ids(n, 1, dev)
    A, B = _cmap(ia, 2, dev), _cmap(ib, 3, dev)
    S = _tuples(ia, 4, dev)
    sps = {m: key_splitters(A, m) for m in MS}
    i64 = lambda k: torch.empty(k, dtype=torch.int64, device=dev)   # noqa: E731
    dig = {m: (i64(m + 1), i64(m + 1)) for m in MS}
    sdig = {m: (i64(m + 1), i64(m + 1)) for m in MS}
    some = (torch.arange(256, device=dev) % 16 == 0).to(torch.uint8)
    every = torch.ones(256, dtype=torch.uint8, device=dev)
    out, big = CounterMap.empty(n, dev), CounterMap.empty(2 * n, dev)
    scnt, acnt, dcnt, mcnt = (i64(1) for _ in range(4))
    eng.reserve(256 << 20)

    names, fns = [], []
    for m in MS:
        names.append(("digest", m))
        fns.append(lambda m=m: eng.cmap_digest(A, sps[m] if m else None, hash_out=dig[m][0], count_out=dig[m][1]))
    for m in MS:
        names.append(("set_digest_orset", m))
        fns.append(lambda m=m: eng.set_digest(S, False, sps[m] if m else None, hash_out=sdig[m][0], count_out=sdig[m][1]))
    names += [("select_1_of_16", 255), ("select_all", 255), ("cmap_delta", None), ("cmap_merge", None)]
    fns.append(lambda: eng.cmap_select(A, sps[255], some, out=out, count=scnt))
    fns.append(lambda: eng.cmap_select(A, sps[255], every, out=out, count=acnt))
    fns.append(lambda: eng.cmap_delta(A, B, out=out, count=dcnt))
    fns.append(lambda: eng.cmap_merge(A, B, out=big, count=mcnt))
    mean, mn = timed(stream, args.steps, args.warmup, *fns)
    flags = eng.device_status(clear=True)
    if flags:
        raise SystemExit(f"device-side failure flags 0x{flags:x}: no valid figures")
    at = {k: i for i, k in enumerate(names)}
    assert int(acnt.item()) == n == int(dig[0][1].item()) == int(sdig[0][1].item())
    merged, shipped = int(mcnt.item()), int(dcnt.item())
    shared = 2 * n - merged
    bitmaps = 8 * (n // 64) * 2                          # the emit words: written by the count pass, read by the write pass
    nbytes = {("cmap_merge", None): 28 * 2 * n + 28 * merged + 3 * 8 * (2 * n // 64) * 2,
              # delta: key and rep of both sides, p and n of both copies at the shared cells, the shipped cells in and out
              ("cmap_delta", None): 12 * 2 * n + 32 * shared + 56 * shipped + 2 * 8 * (2 * n // 64) * 2,
              ("select_1_of_16", 255): 8 * n + 56 * int(scnt.item()) + bitmaps,
              ("select_all", 255): 8 * n + 56 * n + bitmaps}
    for m in MS:
        nbytes[("digest", m)] = 28 * n + 16 * (m + 1) + 8 * m
        nbytes[("set_digest_orset", m)] = 21 * n + 16 * (m + 1) + 8 * m
    versus = {("select_1_of_16", 255): ("cmap_delta", None), ("select_all", 255): ("cmap_delta", None)}
    for m in MS:
        versus[("digest", m)] = ("set_digest_orset", m)
    lines = []
    for k in names:
        i, b = at[k], nbytes[k]
        d = {"leg": k[0], "m": k[1], "cells": n, "ms": round(float(mean[i]), 4), "ms_min": round(float(mn[i]), 4),
             "algorithmic_bytes": int(b), "GBps": round(b / mean[i] / 1e6, 1), "ps_per_byte": round(mean[i] * 1e9 / b, 4),
             "frac_stream_read_peak": round(b / mean[i] / 1e6 / peak, 3), "stream_read_peak_GBps": peak,
             "cmap_merge_ms_same_loop": round(float(mean[at[("cmap_merge", None)]]), 4)}
        if k in versus:
            j, vb = at[versus[k]], nbytes[versus[k]]
            d.update(versus=versus[k][0], versus_ms_same_loop=round(float(mean[j]), 4),
                     versus_ps_per_byte=round(mean[j] * 1e9 / vb, 4),
                     ps_per_byte_over_versus=round((mean[i] / b) / (mean[j] / vb), 3))
        if k[0] == "digest":
            d["nonempty_buckets"] = int((dig[k[1]][1] != 0).sum().item())
        if k[0].startswith("select"):
            d["selected"] = int((scnt if k[0] == "select_1_of_16" else acnt).item())
        if k[0] == "cmap_delta":
            d["shipped"] = shipped
        lines.append(d)
        print(json.dumps(d), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
