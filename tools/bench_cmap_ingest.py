#!/usr/bin/env python3
"""Counter-map state from increment logs (crdt_cmap_combine, crdt_cmap_add,
crdt_cmap_from_ops, Engine.cmap_ingest) on the state tools/bench_cmap.py
builds, timed with HIP events after a warm-up as bench.py times its steps.

    python tools/bench_cmap_ingest.py [--n N] [--steps K] [--warmup W] [--out FILE]

Input: bench_cmap's seeded state of n cells, expanded to a log of 3 n
operations (3 a cell), once sorted by (key, rep) and once shuffled with a fixed
seed; a second seeded state of n cells (about half shared) as the state the
log is added to.  One JSON line per leg: ms, algorithmic bytes, picoseconds
per byte, and the ratio of that to the yardstick's FROM THE SAME LOOP (all the
calls alternate inside every step).  Legs and what their bytes count (k = the
distinct cells, M = the merged cells):
  combine        28 B a cell read (key, rep by the heads pass, p, n by the sums),
                 40 B a distinct cell (key, rep read again at the head, the cell
                 written); yardstick cmap_values
  combine_idx    the same with 4 B of index a cell, the p / n reads gathers
  cmap_values    on the same cells, all four outputs: 24 B a cell, 40 B a key
  tuples_sort    the view (key, rep widened, index, tomb) alone: 21 B a tuple in
                 and out, whatever the passes in between move
  from_ops       the view's three columns (4 B read, 13 B written an operation),
                 the sort, the combine over (key, widened rep, index): 36 B an
                 operation, 40 B a cell; yardstick tuples_sort
  cmap_add       of the second state and the combined log; yardstick cmap_merge
                 of the same pair (28 B a cell in and out)
  cmap_ingest    from_ops, then cmap_add off its device count
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
from bench_cmap import _cmap, _ids                   # noqa: E402
from bench_set_digest import timed                   # noqa: E402
from crdt_amd.engine import CounterMap, Engine, TupleSet   # noqa: E402

COPIES = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    eng = Engine(0)
    dev = eng.device
    stream = torch.cuda.current_stream(dev)
    peak = measure_peaks(eng)["read"]                   # GB/s
    n = args.n
    m = COPIES * n
    ia, ib = _ids(n, 1, dev)
    A, B = _cmap(ia, 2, dev), _cmap(ib, 3, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    # the sorted log: each cell of A three times in a row, amounts of its own
    log = CounterMap(A.key.repeat_interleave(COPIES), A.rep.repeat_interleave(COPIES),
                     torch.randint(0, 1 << 40, (m,), generator=g, dtype=torch.int64, device=dev),
                     torch.randint(0, 1 << 40, (m,), generator=g, dtype=torch.int64, device=dev))
    order = torch.randperm(m, generator=g, device=dev)
    shuf = CounterMap(log.key[order].contiguous(), log.rep[order].contiguous(), log.p[order].contiguous(),
                      log.n[order].contiguous())
    # the indexed form: sorted key / rep, the shuffled amounts, idx = where each sorted operation's amounts are
    idx = torch.empty(m, dtype=torch.int64, device=dev)
    idx[order] = torch.arange(m, device=dev)
    idx = idx.to(torch.int32).contiguous()
    by_idx = CounterMap(log.key, log.rep, shuf.p, shuf.n)
    view = TupleSet(shuf.key, shuf.rep.to(torch.int64).contiguous(), torch.arange(m, dtype=torch.int32, device=dev),
                    torch.zeros(m, dtype=torch.uint8, device=dev))
    del order
    i64 = lambda k: torch.empty(k, dtype=torch.int64, device=dev)   # noqa: E731
    out_m, out_m2 = CounterMap.empty(m, dev), CounterMap.empty(m, dev)
    out_2n, sorted_view = CounterMap.empty(n + m, dev), TupleSet.empty(m, dev)
    vals = [i64(m) for _ in range(4)]
    c_comb, c_idx, c_val, c_ops, c_add, c_mrg, c_ing = (i64(1) for _ in range(7))
    D, c_d = eng.cmap_combine(log)                       # the combined log: the batch of the add / merge legs
    D = D.slice(n)

    names = ["combine", "combine_idx", "cmap_values", "tuples_sort", "from_ops", "cmap_add", "cmap_merge", "cmap_ingest"]
    fns = [lambda: eng.cmap_combine(log, out=out_m, count=c_comb),
           lambda: eng.cmap_combine(by_idx, idx=idx, out=out_m, count=c_idx),
           lambda: eng.cmap_values(log, keys=vals[0], p=vals[1], n=vals[2], value=vals[3], count=c_val),
           lambda: eng.sort_tuples(view, out=sorted_view),
           lambda: eng.cmap_from_ops(shuf.key, shuf.rep, shuf.p, shuf.n, out=out_m2, count=c_ops),
           lambda: eng.cmap_add(B, D, out=out_2n, count=c_add),
           lambda: eng.cmap_merge(B, D, out=out_2n, count=c_mrg),
           lambda: eng.cmap_ingest(B, shuf.key, shuf.rep, shuf.p, shuf.n, out=out_2n, count=c_ing)]
    mean, mn = timed(stream, args.steps, args.warmup, *fns)
    flags = eng.device_status(clear=True)
    if flags:
        raise SystemExit(f"device-side failure flags 0x{flags:x}: no valid figures")
    k, keys, merged = int(c_comb.item()), int(c_val.item()), int(c_add.item())
    assert int(c_d.item()) == n == k == int(c_idx.item()) == int(c_ops.item()), "the log's distinct cells"
    assert merged == int(c_mrg.item()) == int(c_ing.item())
    assert all(torch.equal(a, b) for a, b in zip((out_m.key[:k], out_m.rep[:k], out_m.p[:k], out_m.n[:k]),
                                                 (out_m2.key[:k], out_m2.rep[:k], out_m2.p[:k], out_m2.n[:k])))
    bm = 8 * (m // 64)                                   # one tile bitmap over the log
    two = 28 * 2 * n + 28 * merged + 3 * 8 * (2 * n // 64) * 2
    b_sort = 42 * m
    b_ops = 17 * m + b_sort + 36 * m + 40 * k + 2 * bm
    nbytes = {"combine": 28 * m + 40 * k + 2 * bm, "combine_idx": 32 * m + 40 * k + 2 * bm,
              "cmap_values": 24 * m + 40 * keys + 3 * bm, "tuples_sort": b_sort, "from_ops": b_ops,
              "cmap_add": two, "cmap_merge": two, "cmap_ingest": b_ops + two}
    versus = {"combine": "cmap_values", "combine_idx": "cmap_values", "from_ops": "tuples_sort",
              "cmap_add": "cmap_merge", "cmap_ingest": "tuples_sort"}
    at = {name: i for i, name in enumerate(names)}
    lines = []
    for name in names:
        i, b = at[name], nbytes[name]
        d = {"leg": name, "cells": n, "operations": m, "ms": round(float(mean[i]), 4), "ms_min": round(float(mn[i]), 4),
             "algorithmic_bytes": int(b), "GBps": round(b / mean[i] / 1e6, 1), "ps_per_byte": round(mean[i] * 1e9 / b, 4),
             "frac_stream_read_peak": round(b / mean[i] / 1e6 / peak, 3), "stream_read_peak_GBps": peak}
        if name in versus:
            j, vb = at[versus[name]], nbytes[versus[name]]
            d.update(versus=versus[name], versus_ms_same_loop=round(float(mean[j]), 4),
                     versus_ps_per_byte=round(mean[j] * 1e9 / vb, 4),
                     ps_per_byte_over_versus=round((mean[i] / b) / (mean[j] / vb), 3))
        lines.append(d)
        print(json.dumps(d), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
