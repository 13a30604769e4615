#!/usr/bin/env python3
"""The range-restricted causal OR-Set merge (crdt_orset_merge_causal_ranges)
and the digest round built on it (crdt_amd.reconcile.causal_round) on the
configs[3] sorted set shape, timed with HIP events after a warm-up beside
crdt_orset_merge_causal(A, B) -- what a replica runs without it -- in one
process, the legs alternating inside every timed step on the same inputs.

    python tools/bench_set_causal_ranges.py [--steps K] [--warmup W] [--out FILE]

Input: tools/bench_set_causal.py's -- synth_set_tuples(2024, side, 10M, key
space 8M) for the sides A (side 0) and B (side 1), sorted; contexts of 64
uniform values below 2^20 -- and 255 splitters at the quantiles of A's keys.
For "d of 256 buckets differ" the peer is B_d: A's tuples in the other buckets,
B's in d evenly spread ones, so its digests differ from A's in exactly those.
Legs:
  causal            crdt_orset_merge_causal(A, B): the yardstick
  ranged_all_B      ranged, every flag set, b = B: the same work + the lookup
  ranged_all_B_m16383
                    the same with 16383 splitters: a bucket is shorter than a
                    tile, so every tile straddles buckets and searches per item
  ranged_1          ranged, 1 bucket differing, b = select(B_1)
  ranged_16         ranged, 16 buckets differing, b = select(B_16)
  ranged_256        ranged, all 256 differing, b = select(B)
  round_1, round_16, round_256
                    the whole round in one direction: two digests, the diff,
                    one select and one ranged merge (the peer's digest and
                    select run on this GPU too)
One JSON line per leg: the median, mean and minimum ms, the ratio of the
medians to the yardstick, the tuples and bytes shipped against the whole
state, algorithmic bytes, and the fraction of this run's crdt_stream_read peak
those bytes over the median come to.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import measure_peaks                      # noqa: E402
from crdt_amd import reconcile                       # noqa: E402
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


def peer(eng, A, B, sp, d):
    """(B_d, flags): A's tuples outside d evenly spread buckets of 256, B's
    inside them (both selections are canonical and ascending, so their
    tombstone-form merge is their sorted union)."""
    dev = eng.device
    hot = torch.zeros(256, dtype=torch.uint8, device=dev)
    hot[torch.arange(d, device=dev) * (256 // d) + (256 // d) // 2] = 1
    if d == 256:
        return B, hot
    pa, _ = eng.set_select(A, False, sp, 1 - hot, trim=True)
    pb, _ = eng.set_select(B, False, sp, hot, trim=True)
    return eng.orset_merge(pa, pb), hot


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
    sp = reconcile.key_splitters(A, 255)
    eng.reserve(256 << 20)
    na = len(A)
    ones = torch.ones(256, dtype=torch.uint8, device=dev)
    ctx_out = torch.empty(64, dtype=torch.int64, device=dev)
    out = TupleSet.empty(2 * n_side + (n_side >> 2), dev)      # (a B_d may hold a few more tuples than B)
    legs, meta = {}, {}

    ycnt = torch.empty(1, dtype=torch.int64, device=dev)
    legs["causal"] = lambda: eng.causal_merge(A, ca, B, cb, out=out, ctx_out=ctx_out, count=ycnt)
    meta["causal"] = dict(differing=None, b=len(B), count=ycnt, shipped=len(B))
    acnt = torch.empty(1, dtype=torch.int64, device=dev)
    legs["ranged_all_B"] = lambda: eng.causal_merge_ranges(A, ca, B, cb, sp, ones, out=out, ctx_out=ctx_out, count=acnt)
    meta["ranged_all_B"] = dict(differing=256, b=len(B), count=acnt, shipped=len(B))
    sp_fine = reconcile.key_splitters(A, 16383)
    ones_fine = torch.ones(16384, dtype=torch.uint8, device=dev)
    fcnt = torch.empty(1, dtype=torch.int64, device=dev)
    legs["ranged_all_B_m16383"] = lambda: eng.causal_merge_ranges(A, ca, B, cb, sp_fine, ones_fine, out=out,
                                                                  ctx_out=ctx_out, count=fcnt)
    meta["ranged_all_B_m16383"] = dict(differing=16384, b=len(B), count=fcnt, shipped=len(B), splitters=16383)

    for d in (1, 16, 256):
        Bd, _ = peer(eng, A, B, sp, d)
        flags, n_diff = eng.digest_diff(eng.set_digest(A, False, sp), eng.set_digest(Bd, False, sp))
        if int(n_diff.item()) != d:
            raise SystemExit(f"{int(n_diff.item())} buckets differ, {d} wanted")
        sel, ship = eng.set_select(Bd, False, sp, flags)
        shipped = int(ship.item())
        rcnt, qcnt = (torch.empty(1, dtype=torch.int64, device=dev) for _ in range(2))
        legs[f"ranged_{d}"] = (lambda sel=sel, ship=ship, flags=flags, rcnt=rcnt:
                               eng.causal_merge_ranges(A, ca, sel, cb, sp, flags, n_b_dev=ship, out=out, ctx_out=ctx_out,
                                                       count=rcnt))
        meta[f"ranged_{d}"] = dict(differing=d, b=len(Bd), count=rcnt, shipped=shipped,
                                   whole=eng.causal_merge_count(A, ca, Bd, cb))
        # the round, one direction, every buffer preallocated
        ha, hb = (torch.empty(256, dtype=torch.int64, device=dev) for _ in range(2))
        ka, kb = (torch.empty(256, dtype=torch.int64, device=dev) for _ in range(2))
        fl, nd = torch.empty(256, dtype=torch.uint8, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
        sbuf, scnt = TupleSet.empty(len(Bd), dev), torch.empty(1, dtype=torch.int64, device=dev)

        def round_(Bd=Bd, ha=ha, hb=hb, ka=ka, kb=kb, fl=fl, nd=nd, sbuf=sbuf, scnt=scnt, qcnt=qcnt):
            da = eng.set_digest(A, False, sp, hash_out=ha, count_out=ka)
            db = eng.set_digest(Bd, False, sp, hash_out=hb, count_out=kb)
            eng.digest_diff(da, db, flags=fl, n_diff=nd)
            eng.set_select(Bd, False, sp, fl, out=sbuf, count=scnt)
            eng.causal_merge_ranges(A, ca, sbuf, cb, sp, fl, n_b_dev=scnt, out=out, ctx_out=ctx_out, count=qcnt)

        legs[f"round_{d}"] = round_
        meta[f"round_{d}"] = dict(differing=d, b=len(Bd), count=qcnt, shipped=shipped)

    names = list(legs)
    ms = timed(stream, args.steps, args.warmup, *legs.values())
    status = eng.device_status(clear=True)
    if status:
        raise SystemExit(f"device-side failure flags 0x{status:x}: no valid figures")
    if int(acnt.item()) != int(ycnt.item()) or int(fcnt.item()) != int(ycnt.item()):
        raise SystemExit(f"every flag set gives {int(acnt.item())} / {int(fcnt.item())} tuples, the plain merge {int(ycnt.item())}")
    for d in (1, 16, 256):
        k = int(meta[f"ranged_{d}"]["count"].item())
        if k != int(meta[f"round_{d}"]["count"].item()) or k != int(meta[f"ranged_{d}"]["whole"].item()):
            raise SystemExit(f"ranged_{d}, round_{d} and the merge with the whole peer state disagree")
    med = dict(zip(names, np.median(ms, axis=0)))
    lines = []
    for i, name in enumerate(names):
        m, mt = float(med[name]), meta[name]
        k, nb, shipped = int(mt["count"].item()), mt["b"], mt["shipped"]
        merge_bytes = 21 * (na + shipped) + 41 * k       # the count pass: every field of both operands once; the write pass
        nbytes = merge_bytes
        note = "bytes: every field of a and of the shipped b read once + 41 per surviving tag (20 re-read, 21 written)"
        if name.startswith("round_"):
            # + two digests (21 a tuple), the select's count pass (21 a tuple) and write (41 a shipped tuple)
            nbytes += 21 * na + 21 * nb + 21 * nb + 41 * shipped
            note = "bytes: as ranged + two digests and the select's count pass at 21 a tuple + 41 per shipped tuple"
        d = {"leg": name, "ms_median": round(m, 4), "ms_mean": round(float(ms[:, i].mean()), 4),
             "ms_min": round(float(ms[:, i].min()), 4), "steps": args.steps, "warmup": args.warmup,
             "a": na, "b_state": nb, "n_ctx": 64, "splitters": mt.get("splitters", 255), "buckets_differing": mt["differing"],
             "survivors": k, "shipped_tuples": shipped, "shipped_bytes": 21 * shipped + ((mt.get("splitters", 255) + 1) * 16 + 64 * 8 if mt["differing"] else 64 * 8),
             "whole_state_bytes": 21 * nb + 64 * 8, "shipped_fraction": round(shipped / nb, 5),
             "algorithmic_bytes": int(nbytes), "GBps": round(nbytes / m / 1e6, 1),
             "frac_stream_read_peak": round(nbytes / m / 1e6 / peak, 3), "stream_read_peak_GBps": peak,
             "ratio_to_causal": round(m / float(med["causal"]), 3), "note": note}
        lines.append(d)
        print(json.dumps(d), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
