"""Micro-timing of the keyed PN-Counter map (crdt_cmap_*) beside its yardstick,
this repository's own sorted OR-Set merge at the same merged item count.

Inputs (seeded, built on the device): two states of n cells with about half
the cells shared; the OR-Set sides are the same cells as unique tags.  Timed by
HIP events around ``steps`` calls after ``warmup`` calls: merge, delta, values,
apply of n / 10 operations, a million point lookups, and the OR-Set merge.
``values`` is also timed on the two extreme key shapes: every key one cell
(every run inside a tile, plain stores alone) and 6161 replicas a key (every
run piece crosses a tile boundary: the atomic path's worst case), the lookups
on the latter too (every run is finished by its whole wave).

Prints microseconds per call and, from the bytes the algorithm moves (DESIGN.md
§5.23: 28 B a cell in and at most 28 B out, 21 B a tuple), picoseconds per byte
moved: the figure the counter-map merge and the OR-Set merge are compared by.
"""
import json
import sys

import torch

from crdt_amd.engine import CounterMap, Engine, TupleSet

REPS = 8                       # replicas a key in the mixed states


def _ids(n, seed, dev):
    """Two sorted id lists of n cells out of 3n / 2, the middle n / 2 of a random order shared."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    perm = torch.randperm(n + n // 2, generator=g, device=dev)
    return torch.sort(perm[:n]).values, torch.sort(perm[n // 2:]).values


def _cmap(ids, seed, dev, reps=REPS):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    p = torch.randint(0, 1 << 40, (ids.numel(),), generator=g, dtype=torch.int64, device=dev)
    q = torch.randint(0, 1 << 40, (ids.numel(),), generator=g, dtype=torch.int64, device=dev)
    return CounterMap((ids // reps).contiguous(), (ids % reps).to(torch.int32).contiguous(), p, q)


def _tuples(ids, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    tomb = (torch.rand(ids.numel(), generator=g, device=dev) < 0.1).to(torch.uint8)
    rep = torch.zeros_like(ids, dtype=torch.int32)
    return TupleSet((ids // REPS).contiguous(), (ids % REPS).contiguous(), rep, tomb)


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps * 1000.0            # us per call


def main(n=10_000_000, steps=20, warmup=3):
    eng = Engine(0)
    dev = eng.device
    ia, ib = _ids(n, 1, dev)
    A, B = _cmap(ia, 2, dev), _cmap(ib, 3, dev)
    SA, SB = _tuples(ia, 4, dev), _tuples(ib, 5, dev)
    out, cnt = CounterMap.empty(2 * n, dev), torch.zeros(1, dtype=torch.int64, device=dev)
    sout = TupleSet.empty(2 * n, dev)
    m = n // 10
    g = torch.Generator(device=dev)
    g.manual_seed(6)
    op_keys = torch.sort(torch.randperm((n + n // 2) // REPS, generator=g, device=dev)[:m]).values.contiguous()
    op_dp = torch.randint(0, 1 << 20, (m,), generator=g, dtype=torch.int64, device=dev)
    op_dn = torch.randint(0, 1 << 20, (m,), generator=g, dtype=torch.int64, device=dev)
    cols = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(4)]
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    singles = CounterMap(idx, torch.zeros(n, dtype=torch.int32, device=dev), A.p, A.n)
    long_runs = CounterMap((idx // 6161).contiguous(), (idx % 6161).to(torch.int32).contiguous(), A.p, A.n)
    probes = torch.randint(0, (n + n // 2) // REPS, (1_000_000,), generator=g, dtype=torch.int64, device=dev)
    long_probes = torch.randint(0, n // 6161 + 1, (1_000_000,), generator=g, dtype=torch.int64, device=dev)
    val = torch.empty(1_000_000, dtype=torch.int64, device=dev)
    found = torch.empty(1_000_000, dtype=torch.uint8, device=dev)
    eng.reserve(256 << 20)

    def values(t):
        return lambda: eng.cmap_values(t, keys=cols[0], p=cols[1], n=cols[2], value=cols[3], count=cnt)

    calls = {
        "cmap_merge": lambda: eng.cmap_merge(A, B, out=out, count=cnt),
        "cmap_merge_count": lambda: eng.cmap_merge_count(A, B, count=cnt),
        "cmap_delta": lambda: eng.cmap_delta(A, B, out=out, count=cnt),
        "cmap_delta_count": lambda: eng.cmap_delta_count(A, B, count=cnt),
        "cmap_apply": lambda: eng.cmap_apply(A, 3, op_keys, op_dp, op_dn, out=out, count=cnt),
        "cmap_values": values(A),
        "cmap_values_single_cell_keys": values(singles),
        "cmap_values_6161_replicas_a_key": values(long_runs),
        "cmap_get_1M_probes": lambda: eng.cmap_get(A, probes, value=val, found=found),
        "cmap_get_1M_probes_6161_replicas_a_key": lambda: eng.cmap_get(long_runs, long_probes, value=val, found=found),
        "orset_merge": lambda: eng.orset_merge(SA, SB, out=sout, count=cnt, trim=False),
    }
    res = {"n": n, "steps": steps, "warmup": warmup}
    counts = {}
    for name, fn in calls.items():
        us = timed(fn, warmup, steps)
        counts[name] = int(cnt.item())
        res[name + "_us"] = round(us, 1)
        print(f"{name:36s} {us:10.1f} us   count {counts[name]}", flush=True)
    assert eng.device_status() == 0
    # bytes moved by the merges: every input item read once, every output item written once, 3 bitmap words a 64 items
    items = 2 * n
    cm_bytes = 28 * items + 28 * counts["cmap_merge"] + 3 * 8 * items // 64 * 2
    or_bytes = 21 * items + 21 * counts["orset_merge"] + 3 * 8 * items // 64 * 2
    res["cmap_merge_ps_per_byte"] = round(res["cmap_merge_us"] * 1e6 / cm_bytes, 3)
    res["orset_merge_ps_per_byte"] = round(res["orset_merge_us"] * 1e6 / or_bytes, 3)
    res["cmap_merge_gb_s"] = round(cm_bytes / res["cmap_merge_us"] / 1e3, 1)
    res["orset_merge_gb_s"] = round(or_bytes / res["orset_merge_us"] / 1e3, 1)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main(*[int(x) for x in sys.argv[1:]])
