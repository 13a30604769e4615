#!/usr/bin/env python3
"""bench.py -- batched CRDT merge throughput on MI355X (driver contract).

    python bench.py --gpus N --steps K --warmup W [--workload NAME] [--dump-outputs DIR] [--full]

Default workload = BASELINE.json configs[4] (the north_star's scaling
config): a 100M-replica x 64-node uint64 G-Counter population sharded by
contiguous rows over the N GPUs; one step = every rank folds its shard
(crdt_gcounter_fold) and ONE RCCL ncclAllReduce(ncclUint64, ncclMax) of the
512-B fold joins the shards (crdt_shard_fold_max_u64, the library's own
communicator).  At N=1 the whole 51.2-GB population is on one GPU.  Total
work is fixed as N grows ("strong").  configs[1] (pairwise join of 1M x 64)
is --workload gcounter_join.

N>1: one process per GPU.  Under torchrun the ranks come from the env; a
plain `python bench.py --gpus N` spawns its own N rank processes before the
parent touches the GPU and exits with their status.

Prints ONE JSON line (rank 0) with value = whole-job units/s, ms_per_step and
a roofline object for the dominant kernel (HIP-event-timed on the launch
stream).  A plain run does only that: set up, warm up, time the K steps, print.

--dump-outputs DIR: after the timed steps, what the last step computed (the
arrays its caller receives) goes to DIR/<name>.npy (dump_outputs below).

--full adds the measurements that take runs of their own: the self-measured
streaming peaks (roofline.measured_peak), the PCIe-inclusive e2e_pcie time and
the cpu_baseline object (the oracle restatement on this host's cores, rank 0
at N=1 only, bounded sample, with its parity spot-check of the device
outputs).  --no-peaks / --no-e2e / --no-cpu-baseline drop one of them.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from crdt_amd import engine as E  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md, chip table)
METRIC = "replica-merges/sec + achieved HBM GB/s vs peak, 1/2/4/8 MI355X"


def dist_init():
    """One process per GPU.  Backend "nccl" (= RCCL over xGMI on ROCm).
    CRDT_BENCH_BACKEND=gloo lets several ranks share one GPU to rehearse the
    multi-rank path on a 1-GPU box (never used for reported numbers)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("CRDT_BENCH_BACKEND", "nccl")
    dev = local % max(torch.cuda.device_count(), 1) if backend == "gloo" else local
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev))
        else:
            dist.init_process_group(backend)
    return world, rank, dev


def spawn_ranks(n: int) -> int:
    """`--gpus N` without a launcher: start N rank processes of this script
    (RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* in their env) and return the first
    failing exit status (0 if all succeed).  Runs before this process makes
    any GPU call; if a rank fails the others are stopped (a peer blocked in a
    collective would never return)."""
    import signal
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    while procs:
        for p in list(procs):
            code = p.poll()
            if code is None:
                continue
            procs.remove(p)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 128 - code
                for q in procs:
                    q.send_signal(signal.SIGTERM)
        time.sleep(0.05)
    return rc


E2E_MAX_BYTES = 4 << 30      # bounded: larger populations (vclock, configs[4]) are not staged through pinned memory


def measure_e2e(wl, reps=3):
    """SURVEY §8(d) "also report end-to-end time including H2D/D2H": the
    step's inputs copied from pinned host memory into its device buffers
    (same contents, so the outputs are unchanged), the step, and its outputs
    copied back to pinned host memory, serialised on the launch stream and
    timed by HIP events; median of `reps`.  Never the reported `value`."""
    if getattr(wl, "e2e_stream", None) is not None:     # a population larger than the staging bound
        return wl.e2e_stream()
    if getattr(wl, "io", None) is None:
        return {"skipped": getattr(wl, "e2e_skip", "this step has no host-staged form")}
    ins, outs = wl.io()
    nbytes = lambda ts: sum(t.numel() * t.element_size() for t in ts)
    n_in, n_out = nbytes(ins), nbytes(outs)
    if n_in + n_out > E2E_MAX_BYTES:
        return {"skipped": f"{(n_in + n_out) / 1e9:.1f} GB of inputs + outputs exceed the {E2E_MAX_BYTES >> 30} GiB "
                           "pinned-staging bound of this measurement"}
    stream = torch.cuda.current_stream()
    h_in = [t.cpu().pin_memory() for t in ins]
    h_out = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in outs]
    ms = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for d, h in zip(ins, h_in):
            d.copy_(h, non_blocking=True)
        wl.step()
        for h, d in zip(h_out, wl.io()[1]):
            h.copy_(d, non_blocking=True)
        e1.record(stream)
        torch.cuda.synchronize()
        if r:
            ms.append(e0.elapsed_time(e1))
    med = float(np.median(ms))
    return {"ms": round(med, 4), "value": round(wl.units() / (med / 1e3), 1), "unit": wl.unit,
            "h2d_bytes": n_in, "d2h_bytes": n_out,
            "timing": f"H2D of the step's inputs (pinned) + step + D2H of its outputs (pinned), one stream, "
                      f"HIP events, median of {reps}"}


def cpu_share() -> tuple[int, int]:
    """(threads for the CPU baseline, CPUs in this process's affinity mask).
    The box grants each GPU a CPU share that OMP_NUM_THREADS states while the
    affinity mask may show the whole machine: use the smaller of the two."""
    aff = len(os.sched_getaffinity(0))
    env = os.environ.get("OMP_NUM_THREADS", "")
    share = int(env) if env.isdigit() and int(env) > 0 else aff
    return max(1, min(aff, share)), aff


def measure_peaks(eng, gib=1):
    """the self-measured streaming peaks the roofline is also
    read against -- the library's copy kernel (bytes read + written) and its
    read-only sweep, best of an unroll x workgroups-per-CU sweep over a
    `gib`-GiB buffer, HIP events on the launch stream."""
    dev = eng.device
    n = gib << 30
    src = torch.empty(n // 8, dtype=torch.int64, device=dev)
    dst = torch.empty_like(src)
    sink = torch.empty(eng.num_cus * 64 if hasattr(eng, "num_cus") else 1 << 16, dtype=torch.int64, device=dev)
    src.fill_(1)
    stream = torch.cuda.current_stream(dev)
    best = {"copy": (0.0, None), "read": (0.0, None)}
    for unroll in (1, 2, 4, 8):
        for bpc in (1, 2, 4, 8):
            for kind in ("copy", "read"):
                def run():
                    if kind == "copy":
                        eng.stream_copy(src, dst, unroll, bpc)
                    else:
                        eng.stream_read(src, sink, unroll, bpc)
                run()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(5):
                    run()
                e1.record(stream)
                e1.synchronize()
                t = e0.elapsed_time(e1) / 5 / 1e3
                gbs = (2 * n if kind == "copy" else n) / t / 1e9
                if gbs > best[kind][0]:
                    best[kind] = (gbs, f"unroll {unroll}, {bpc} workgroups/CU")
    del src, dst, sink
    return {"copy": round(best["copy"][0], 1), "copy_shape": best["copy"][1],
            "read": round(best["read"][0], 1), "read_shape": best["read"][1], "unit": "GB/s",
            "kernels": f"crdt_stream_copy (read + write bytes) / crdt_stream_read, {gib} GiB, 16-B nontemporal "
                       "accesses, best of unroll {1,2,4,8} x {1,2,4,8} workgroups/CU"}


def barrier(world):
    if world > 1:
        import torch.distributed as dist
        dist.barrier()


def max_over_ranks(x: float, world: int, dev) -> float:
    if world == 1:
        return x
    import torch.distributed as dist
    t = torch.tensor([x], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def sum_over_ranks(x: int, world: int, dev) -> int:
    if world == 1:
        return x
    import torch.distributed as dist
    t = torch.tensor([x], dtype=torch.int64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return int(t.item())


DUMP_MAX_BYTES = 64_000_000   # --dump-outputs: bound on the float forms of all arrays together
DUMP_SEED = 2024


def dump_outputs(outdir, arrays, prefix=""):
    """--dump-outputs: every array of `arrays` (name -> tensor or ndarray) as
    outdir/<prefix><name>.npy.  The outputs are integers, so each is stored
    in a float form that holds them exactly: 8-byte integers as float64
    [..., 2] = (high, low) 32-bit halves of the bit pattern, 4-byte integers
    as float64, narrower ones as float32.  When the float forms exceed
    DUMP_MAX_BYTES together, every array keeps the same fraction of its rows
    (first axis): a sorted sample drawn from DUMP_SEED, the same rows for
    arrays of the same length, so runs with the same arguments store the
    same elements."""
    os.makedirs(outdir, exist_ok=True)
    form = lambda x: 16 if x.element_size() == 8 else 8 if x.element_size() == 4 else 4
    arrays = {k: (v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))) for k, v in arrays.items()}
    total = sum(v.numel() * form(v) for v in arrays.values())
    frac = min(1.0, (DUMP_MAX_BYTES - 1024 * len(arrays)) / max(total, 1))
    rng, picks = np.random.default_rng(DUMP_SEED), {}
    for name, x in arrays.items():
        rows = x.shape[0] if x.dim() else 1
        if frac < 1.0 and rows > 1:
            if rows not in picks:
                picks[rows] = torch.from_numpy(np.sort(rng.choice(rows, max(1, int(rows * frac)), replace=False)))
            x = x[picks[rows].to(x.device)]
        a = x.detach().cpu().contiguous().numpy()
        if a.dtype.kind == "f":
            f = a.astype(np.float64 if a.itemsize == 8 else np.float32)
        elif a.itemsize == 8:
            u = a.view(np.uint64)
            f = np.stack([(u >> np.uint64(32)).astype(np.float64), (u & np.uint64(0xFFFFFFFF)).astype(np.float64)], -1)
        else:
            f = a.astype(np.float64 if a.itemsize == 4 else np.float32)
        np.save(os.path.join(outdir, f"{prefix}{name}.npy"), f)


def _tuple_arrays(t, prefix=""):
    return {prefix + "key": t.key, prefix + "ts": t.ts, prefix + "rep": t.rep, prefix + "tomb": t.tomb}


def _refmerge_arrays(o):
    """A refmerge output's defined part: the new Diffs up to off[-1], a
    slot's string id only where it holds a string, its sum only where it
    holds a sum (the rest of those buffers is never written)."""
    n = int(o["off"][-1].item())
    kind = o["st_kind"]
    return {"off": o["off"], "ts": o["ts"][:n], "origin": o["origin"][:n], "src": o["src"][:n], "st_kind": kind,
            "st_str": torch.where(kind == 1, o["st_str"], torch.zeros_like(o["st_str"])),
            "st_sum": torch.where(kind == 2, o["st_sum"], torch.zeros_like(o["st_sum"]))}


def _population_arrays(h, prefix=""):
    """NativePopulation.read() with the undefined state fields zeroed (as _refmerge_arrays)."""
    h = dict(h)
    h["st_str"] = np.where(h["st_kind"] == 1, h["st_str"], 0).astype(np.uint32)
    h["st_sum"] = np.where(h["st_kind"] == 2, h["st_sum"], 0).astype(np.int64)
    return {prefix + k: v for k, v in h.items()}


# --------------------------------------------------------------------------- workloads
class Workload:
    """setup() allocates device inputs; step() enqueues one pass of the hot path;
    outputs() names the arrays the last step's caller received (--dump-outputs)."""
    name = ""
    unit = "replica-merges/s"
    dtype = "u64"
    kernel = ""           # dominant kernel name (for the rocprof cross-check)
    config: dict = {}

    def units(self) -> int: ...
    def bytes_per_launch(self) -> int: ...
    def step(self): ...
    def outputs(self) -> dict: ...


class GCounterJoin(Workload):
    name = "gcounter_join"
    kernel = "k_join"

    def __init__(self, eng, rank, world, rows, nodes, seed=2024):
        self.eng, self.rows, self.nodes = eng, rows, nodes
        base = rank * rows                       # weak scaling: each rank its own replicas
        self.a = eng.synth_counters(seed, 1, rows, nodes, row_base=base)
        self.b = eng.synth_counters(seed, 2, rows, nodes, row_base=base)
        self.out = torch.empty_like(self.a)
        self.config = {"workload": f"G-Counter join, {rows} replicas x {nodes} nodes uint64 per GPU "
                                   "(BASELINE configs[1])", "rows_per_gpu": rows, "nodes": nodes,
                       "parallelism": f"replica-shard x{world}"}

    def units(self):
        return self.rows

    def bytes_per_launch(self):
        return 3 * self.rows * self.nodes * 8    # read A, read B, write out once

    def step(self):
        self.eng.gcounter_join(self.a, self.b, out=self.out)

    def io(self):
        return [self.a, self.b], [self.out]

    def outputs(self):
        return {"out": self.out}

    def cpu_baseline(self, seconds, threads):
        from oracle import oracle
        rows = min(self.rows, 250_000)
        a = E.as_u64(self.a[:rows]).reshape(rows, self.nodes)
        b = E.as_u64(self.b[:rows]).reshape(rows, self.nodes)
        # parity spot-check of the sample before timing it
        assert np.array_equal(oracle.gcounter_join(a, b, threads), E.as_u64(self.out[:rows]).reshape(rows, self.nodes))
        done, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            oracle.gcounter_join(a, b, threads)
            done += rows
        dt = time.perf_counter() - t0
        return {"value": done / dt, "unit": self.unit, "cores": threads, "kind": "port",
                "sample": f"oracle/crdt_oracle.c oc_gcounter_join (C restatement, not the Go reference: no Go "
                          f"toolchain), {rows} replicas x {self.nodes} nodes from the same device inputs, "
                          f"repeated {done // rows}x over {dt:.1f}s, {threads} pthreads"}


class PNCounterJoin(GCounterJoin):
    name = "pncounter_join"
    kernel = "k_join (P pass, N pass)"

    def __init__(self, eng, rank, world, rows, nodes, seed=2024):
        super().__init__(eng, rank, world, rows, nodes, seed)
        base = rank * rows
        self.na = eng.synth_counters(seed, 3, rows, nodes, row_base=base)
        self.nb = eng.synth_counters(seed, 4, rows, nodes, row_base=base)
        self.nout = torch.empty_like(self.na)
        self.config = dict(self.config, workload=f"PN-Counter join, {rows} replicas x {nodes} nodes (P,N) uint64")

    def bytes_per_launch(self):
        return 6 * self.rows * self.nodes * 8

    def step(self):
        self.eng.pncounter_join(self.a, self.na, self.b, self.nb, self.out, self.nout)

    def io(self):
        return [self.a, self.na, self.b, self.nb], [self.out, self.nout]

    def outputs(self):
        return {"p_out": self.out, "n_out": self.nout}

    def cpu_baseline(self, seconds, threads):
        return None


class VClockClassify(Workload):
    name = "vclock_classify"
    unit = "pairs/s"
    kernel = "k_vclock"
    read_dominated = True

    def __init__(self, eng, rank, world, pairs, nodes, seed=2024):
        self.eng, self.pairs, self.nodes = eng, pairs, nodes
        self.a, self.b = eng.synth_vclock_pairs(seed, pairs, nodes, pair_base=rank * pairs)
        self.cls = torch.empty(pairs, dtype=torch.uint8, device=eng.device)
        self.config = {"workload": f"vector-clock classify, {pairs} pairs x {nodes} nodes (BASELINE configs[2])",
                       "pairs_per_gpu": pairs, "nodes": nodes, "parallelism": f"replicas x{world}"}

    def units(self):
        return self.pairs

    def bytes_per_launch(self):
        return self.pairs * (2 * self.nodes * 8 + 1)

    def step(self):
        self.eng.vclock_classify(self.a, self.b, out=self.cls)

    def io(self):
        return [self.a, self.b], [self.cls]

    def outputs(self):
        return {"cls": self.cls}

    def cpu_baseline(self, seconds, threads):
        from oracle import oracle
        n = min(self.pairs, 200_000)
        a, b = E.as_u64(self.a[:n]), E.as_u64(self.b[:n])
        assert np.array_equal(oracle.vclock_classify(a, b, threads), self.cls[:n].cpu().numpy())
        done, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            oracle.vclock_classify(a, b, threads)
            done += n
        dt = time.perf_counter() - t0
        return {"value": done / dt, "unit": self.unit, "cores": threads, "kind": "port",
                "sample": f"oc_vclock_classify, {n} pairs x {self.nodes} nodes, {dt:.1f}s, {threads} pthreads"}


class SetMerge(Workload):
    unit = "input-tuples/s"
    kernel = "whole op: k_{lww,or}_split + k_{lww,or}_count + k_lww_scan + k_{lww,or}_write"

    def __init__(self, eng, rank, world, n, key_space, lww=True, seed=2024):
        self.eng, self.n, self.lww = eng, n, lww
        self.name = "lww_merge" if lww else "orset_merge"
        s = seed + 7919 * rank
        self.A = eng.synth_set_tuples(s, 0, n, key_space)
        self.B = eng.synth_set_tuples(s, 1, n, key_space)
        self.out = E.TupleSet.empty(2 * n, eng.device)
        self.count = torch.zeros(1, dtype=torch.int64, device=eng.device)
        fn = eng.lww_merge if lww else eng.orset_merge
        fn(self.A, self.B, out=self.out, count=self.count, trim=False)
        torch.cuda.synchronize()
        self.n_out = int(self.count.item())
        self.config = {"workload": f"{'LWW-Element-Set' if lww else 'OR-Set'} merge, {n} tuples per side, "
                                   f"key space {key_space}, pre-sorted (BASELINE configs[3], D1)",
                       "tuples_per_side": n, "key_space": key_space, "n_out": self.n_out,
                       "parallelism": f"replicas x{world}"}
        self._fn = fn

    def units(self):
        return 2 * self.n

    def bytes_per_launch(self):
        return 21 * 2 * self.n + 21 * self.n_out

    def step(self):
        self._fn(self.A, self.B, out=self.out, count=self.count, trim=False)

    def _sides(self):
        return self.A, self.B

    def io(self):
        o = self.out.slice(self.n_out)
        ins = [t for side in self._sides() for t in (side.key, side.ts, side.rep, side.tomb)]
        return ins, [o.key, o.ts, o.rep, o.tomb, self.count]

    def outputs(self):
        return dict(_tuple_arrays(self.out.slice(int(self.count.item()))), count=self.count)

    def cpu_baseline(self, seconds, threads):
        """The oracle's serial merge run on `threads` host threads, each over
        one key range of both sorted inputs (a key's output depends only on
        its own tuples, so key-range pieces concatenate to the whole merge --
        the same split the multi-GPU path uses)."""
        from concurrent.futures import ThreadPoolExecutor
        from oracle import oracle
        a = self.A.to_numpy()
        b = self.B.to_numpy()
        fn = oracle.lww_merge if self.lww else oracle.orset_merge
        pieces = _key_range_pieces(a, b, threads)
        with ThreadPoolExecutor(threads) as ex:
            got = list(ex.map(lambda ab: fn(*ab), pieces))
            n_cpu = sum(len(g[0]) for g in got)
            assert n_cpu == self.n_out, f"cpu merge length {n_cpu} != device {self.n_out}"
            done, t0 = 0, time.perf_counter()
            while True:
                list(ex.map(lambda ab: fn(*ab), pieces))
                done += 2 * self.n
                if time.perf_counter() - t0 > seconds:
                    break
            dt = time.perf_counter() - t0
        return {"value": done / dt, "unit": self.unit, "cores": threads, "kind": "port",
                "sample": f"oc_{self.name} (C restatement) on {threads} threads, one key range of both sorted "
                          f"sides each, {self.n} tuples per side, {done // (2 * self.n)} reps in {dt:.1f}s"}


def _key_range_pieces(a, b, parts):
    """Split two key-sorted SoA tuple sets into `parts` aligned key ranges."""
    keys = np.concatenate([a[0], b[0]])
    if len(keys) == 0:
        return [(a, b)]
    qs = np.unique(np.quantile(keys, np.linspace(0, 1, parts + 1)[1:-1], method="nearest").astype(np.uint64))
    ia = [0] + list(np.searchsorted(a[0], qs)) + [len(a[0])]
    ib = [0] + list(np.searchsorted(b[0], qs)) + [len(b[0])]
    return [(tuple(x[ia[i]:ia[i + 1]] for x in a), tuple(x[ib[i]:ib[i + 1]] for x in b))
            for i in range(len(ia) - 1)]


class SetMergeUnsorted(SetMerge):
    """configs[3] D2: both sides arrive UNSORTED; a step is ONE call of
    crdt_*_merge_unsorted over both sides together (a packed (key, ts, rep,
    side, tomb) composite, whose order is the stable merge of the sorted
    sides).  On config D's dense keys no radix pass runs: the composing pass
    groups each tile by the key's top byte (k_lww_up_tiled); LWW gathers each
    byte's runs into an LDS table of per-key winners (k_lww_table_g), OR-Set
    gathers them into 2^9-key chunk ranges (k_or_bucket), each chunk sorted
    and deduplicated in LDS (k_or_chunk); both planned from a sample of the
    inputs, launched from the context's cached plan.  Algorithmic bytes
    are those of the merge itself (inputs read once, output written once);
    the sort's passes are the price of unsorted input, so frac reads against
    that."""

    @property
    def kernel(self):
        return ("k_sample_minmax + k_plan_match + k_lww_up_tiled + k_lww_table_g" if self.lww else
                "k_sample_minmax + k_plan_match + k_lww_up_tiled + k_or_bucket + k_or_chunk")

    def __init__(self, eng, rank, world, n, key_space, lww=True, seed=2024):
        self.eng, self.n, self.lww = eng, n, lww
        self.name = ("lww_merge" if lww else "orset_merge") + "_d2"
        s = seed + 7919 * rank
        self.UA = eng.synth_set_tuples(s, 0, n, key_space, sort=False)
        self.UB = eng.synth_set_tuples(s, 1, n, key_space, sort=False)
        self.out = E.TupleSet.empty(2 * n, eng.device)
        self.count = torch.zeros(1, dtype=torch.int64, device=eng.device)
        self._fn = eng.lww_merge_unsorted if lww else eng.orset_merge_unsorted
        self.step()
        torch.cuda.synchronize()
        self.n_out = int(self.count.item())
        self.config = {"workload": f"{'LWW-Element-Set' if lww else 'OR-Set'} merge, {n} tuples per side, "
                                   f"key space {key_space}, UNSORTED inputs: one device sort of both sides + dedup "
                                   "(BASELINE configs[3], D2)",
                       "tuples_per_side": n, "key_space": key_space, "n_out": self.n_out,
                       "parallelism": f"replicas x{world}"}

    def step(self):
        self._fn(self.UA, self.UB, out=self.out, count=self.count, trim=False)

    def _sides(self):
        return self.UA, self.UB

    def cpu_baseline(self, seconds, threads):
        """numpy lexsort of each unsorted side (the oracle's sort order) then
        the oracle's serial merge, one thread, on a 1M-tuple-per-side slice
        of the same device inputs (a full-size rep would take too long)."""
        from oracle import oracle
        m = min(self.n, 1_000_000)
        ua = [x[:m] for x in self.UA.to_numpy()]
        ub = [x[:m] for x in self.UB.to_numpy()]
        fn = oracle.lww_merge if self.lww else oracle.orset_merge

        def srt(t):
            o = np.lexsort((t[3], t[2], t[1], t[0]))
            return tuple(np.ascontiguousarray(x[o]) for x in t)

        from concurrent.futures import ThreadPoolExecutor
        done, t0 = 0, time.perf_counter()
        with ThreadPoolExecutor(threads) as ex:
            while True:
                sa, sb = ex.map(srt, (ua, ub))
                list(ex.map(lambda ab: fn(*ab), _key_range_pieces(sa, sb, threads)))
                done += 2 * m
                if time.perf_counter() - t0 > seconds:
                    break
        dt = time.perf_counter() - t0
        return {"value": done / dt, "unit": self.unit, "cores": threads, "kind": "port",
                "sample": f"numpy lexsort of both unsorted sides (one thread each) + oc_{self.name[:-3]} on {threads} "
                          f"threads over key ranges, {m} tuples per side (slice of the device inputs), "
                          f"{done // (2 * m)} reps"}


def native_comm(eng, world):
    """The library's own RCCL communicator (crdt_shard_comm_init_rank), one
    rank per process; None in the gloo rehearsal (ranks sharing one GPU,
    which RCCL refuses): the exchange then goes through torch.distributed."""
    if os.environ.get("CRDT_BENCH_BACKEND", "nccl") != "nccl":
        return None
    from crdt_amd import shard
    return shard.Comm.init_rank(eng)


class ShardFold(Workload):
    """configs[4] E1: `total_rows` replicas sharded by contiguous rows over
    the ranks; a step = each rank folds its [rows, 64] shard on its GPU, then
    ONE ncclAllReduce(ncclUint64, ncclMax) of the 512-B folds
    (crdt_shard_fold_max_u64).  Rows processed per step summed over ranks =
    total_rows (strong scaling)."""
    name = "shard_fold"
    unit = "replica-merges/s"
    kernel = "k_fold_pow2"
    scaling = "strong"
    read_dominated = True

    def __init__(self, eng, rank, world, total_rows, nodes, seed=2024):
        from crdt_amd import shard
        self.eng, self.world, self.nodes, self.total = eng, world, nodes, total_rows
        b, e = shard.shard_range(total_rows, world, rank)
        self.row0, self.rows = b, e - b
        self.a = eng.synth_counters(seed, 1, self.rows, nodes, row_base=b)
        self.fold = torch.empty(nodes, dtype=torch.int64, device=eng.device)
        self.comm = native_comm(eng, world)
        xchg = "RCCL ncclAllReduce(ncclUint64, ncclMax) via crdt_shard_fold_max_u64" if self.comm else \
            "gloo all-reduce(max) rehearsal (ranks share one GPU)"
        self.config = {"workload": f"sharded fold, {total_rows} replicas x {nodes} nodes uint64 total "
                                   f"({total_rows * nodes * 8 / 1e9:.1f} GB), per-GPU fold + all-reduce(max) "
                                   "(BASELINE configs[4], E1)",
                       "total_rows": total_rows, "rows_per_gpu": self.rows, "nodes": nodes,
                       "parallelism": f"row-shard x{world} + {xchg}"}

    def units(self):
        return self.rows

    def bytes_per_launch(self):
        return self.rows * self.nodes * 8

    def step(self):
        if self.comm is not None:
            self.comm.fold_max([self.a], [self.fold])
        else:
            from crdt_amd import shard
            self.eng.gcounter_fold(self.a, out=self.fold)
            if self.world > 1:
                shard.allreduce_max_u64(self.fold, self.eng)

    def outputs(self):
        return {"fold": self.fold}

    def e2e_stream(self, chunk_bytes=1 << 30):
        """VERDICT r05 missing #4: the PCIe-inclusive time of the whole
        configs[4] population.  It streams from pinned host memory into HBM
        in 1-GiB chunks on a copy stream.  Each chunk folds on the launch
        stream as soon as it has landed, while the next chunk is in flight.
        Then the chunk folds are folded, and the 512-B result is copied to
        pinned host memory.  The timing covers that whole pipeline (HIP
        events, one run).  The host source is a 2-GiB pinned slice (the
        population's first 4M rows) sent over and over: 51.2 GB cross PCIe,
        but the population becomes periodic, so the fold result is not
        checked here.  (The fold's parity is the tests' job; the cpu_baseline
        parity check runs on the same device rows.)  Never `value`."""
        if self.world > 1:
            return {"skipped": "rank 0 of one GPU only"}
        dev = self.eng.device
        crows = max(1, chunk_bytes // (self.nodes * 8))
        nch = (self.rows + crows - 1) // crows
        src_rows = min(self.rows, 2 * crows)
        host = self.a[:src_rows].cpu().pin_memory()
        folds = torch.empty((nch, self.nodes), dtype=torch.int64, device=dev)
        out_h = torch.empty(self.nodes, dtype=torch.int64, pin_memory=True)
        main, cs = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
        landed = [torch.cuda.Event() for _ in range(nch)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record(main)
        cs.wait_event(e0)
        for c in range(nch):
            r0, r1 = c * crows, min(self.rows, (c + 1) * crows)
            h0 = (c * crows) % src_rows
            n = min(r1 - r0, src_rows - h0)
            with torch.cuda.stream(cs):
                self.a[r0:r0 + n].copy_(host[h0:h0 + n], non_blocking=True)
                if n < r1 - r0:
                    self.a[r0 + n:r1].copy_(host[:r1 - r0 - n], non_blocking=True)
                landed[c].record(cs)
            main.wait_event(landed[c])
            self.eng.gcounter_fold(self.a[r0:r1], out=folds[c])
        self.eng.gcounter_fold(folds, out=self.fold)
        out_h.copy_(self.fold, non_blocking=True)
        e1.record(main)
        torch.cuda.synchronize(dev)
        ms = e0.elapsed_time(e1)
        nb = self.rows * self.nodes * 8
        return {"ms": round(ms, 3), "value": round(self.rows / (ms / 1e3), 1), "unit": self.unit,
                "h2d_bytes": nb, "d2h_bytes": self.nodes * 8, "h2d_GBps": round(nb / (ms / 1e3) / 1e9, 2),
                "timing": f"{nb / 1e9:.1f} GB streamed from pinned host memory in {nch} chunks of "
                          f"{crows * self.nodes * 8 >> 20} MiB (copy stream), each folded on arrival while the "
                          "next is in flight, the chunk folds folded, the 512-B fold copied back; HIP events, "
                          f"one run.  Source: a {src_rows * self.nodes * 8 >> 20}-MiB pinned slice of the "
                          "population, repeated (timing only)"}

    def cpu_baseline(self, seconds, threads):
        """oc_gcounter_fold over `threads` row ranges of a 2M-row (1 GB)
        slice of the same device population, max-combined (the same
        associative join), repeated for ~`seconds`."""
        from concurrent.futures import ThreadPoolExecutor
        from oracle import oracle
        rows = min(self.rows, 2_000_000)
        a = E.as_u64(self.a[:rows]).reshape(rows, self.nodes)
        parts = [a[i * rows // threads:(i + 1) * rows // threads] for i in range(threads)]

        def fold(ex):
            return np.maximum.reduce(list(ex.map(oracle.gcounter_fold, parts)))

        with ThreadPoolExecutor(threads) as ex:
            got = fold(ex)
            assert np.array_equal(got, E.as_u64(self.eng.gcounter_fold(self.a[:rows]))), "fold parity"
            done, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < seconds:
                fold(ex)
                done += rows
            dt = time.perf_counter() - t0
        return {"value": done / dt, "unit": self.unit, "cores": threads, "kind": "port",
                "sample": f"oracle/crdt_oracle.c oc_gcounter_fold (C restatement; no Go toolchain) over {threads} "
                          f"row ranges of {rows} replicas x {self.nodes} nodes copied from the device population, "
                          f"max-combined, {done // rows} reps in {dt:.1f}s"}


class ShardSetMerge(SetMerge):
    """configs[3] as a DISTRIBUTED population (north_star (3): "all-gather
    and final merge for keyed sets"): every rank holds only its own sorted
    10M + 10M tuples (A and B); a step = crdt_shard_{lww,orset}_merge_local
    -- sampled splitters (one all-gather), every rank's tuples sent to their
    key-range owner (all-to-all-v over xGMI), the owner's merge of the
    received runs, then the all-gather-v of the merged state to every rank.
    Units = input tuples of all ranks; per-GPU work fixed (weak scaling).  At
    N=1 the library skips the exchange (one rank owns every key): the line is
    the D1 merge's, through this entry point."""
    kernel = "whole op: crdt_shard_*_merge_local (N=1: the D1 merge passes)"

    def __init__(self, eng, rank, world, n, key_space, lww=True, seed=2024):
        super().__init__(eng, rank, world, n, key_space, lww, seed)
        self.name = "shard_set_merge" if lww else "shard_orset_merge"
        self.world = world
        self.comm = native_comm(eng, world)
        if self.comm is None:
            raise SystemExit("shard_set_merge needs the native RCCL communicator (CRDT_BENCH_BACKEND=nccl)")
        self.cap = 2 * n * world
        self.gout = E.TupleSet.empty(self.cap, eng.device)
        self.step()
        torch.cuda.synchronize()
        self.n_total = len(self.last) if self.last_count is None else int(self.last_count.item())
        self.config = dict(self.config, workload=(
            f"{'LWW-Element-Set' if lww else 'OR-Set'} merge of a distributed population: {n} tuples per side "
            f"per GPU (sorted), key space {key_space}, key-range all-to-all + local merge + all-gather-v "
            "(BASELINE configs[3] sharded, north_star (3))"),
            n_out_total=self.n_total, parallelism=f"key-range shard x{world} (RCCL all-to-all-v + all-gather-v)")

    io = None
    e2e_skip = "the step's outputs are the whole population's merged state on every rank: no host-staged form"

    def step(self):
        if self.world == 1:
            # one rank: the whole merged state IS the rank's own key range, so
            # the count-on-device form returns the same state without the
            # trailing read-back (crdt_shard_*_merge_local_dev)
            outs, cnt = self.comm.set_merge_local_dev([self.A], [self.B], lww=self.lww, cap=self.cap,
                                                      outs=[self.gout])
            self.last, self.last_count = outs[0], cnt[0]
            return
        self.last = self.comm.set_merge_local([self.A], [self.B], lww=self.lww, gather=True, cap=self.cap,
                                              outs=[self.gout])[0]
        self.last_count = None

    def outputs(self):
        n = len(self.last) if self.last_count is None else int(self.last_count.item())
        return dict(_tuple_arrays(self.last.slice(n)), count=np.array([n], np.int64))

    def extra(self, avg_ms):
        return {"exchange": {"n_out_total": self.n_total, "ranks": self.world,
                             "note": "N>1: each rank sends every tuple to its key-range owner and receives the "
                                     "whole merged state; roofline.bytes_per_launch counts this rank's merge only"}}


class LoopbackSetMerge(Workload):
    """configs[3] as a distributed population over R LOOPBACK ranks on this
    one GPU (crdt_shard_comm_create_loopback): rank r holds its own sorted
    share of the 10M + 10M tuples; a step = crdt_shard_{lww,orset}_merge_local
    with the final all-gather -- weighted splitters from pooled samples (one
    all-gather), the count matrix (one all-gather), every tuple sent to its
    key-range owner (ONE point-to-point group), the owner's rank-order merge
    tree and set merge, the all-gather-v of the merged state to every rank.
    The R ranks share one GPU's HBM, so the line prices the protocol itself
    (planning, host round trips, the exchange's device copies, R-fold output)
    before the first multi-GPU run, not xGMI.  Algorithmic bytes are the
    merge's (inputs once, output once)."""
    unit = "input-tuples/s"
    scaling = "weak"

    def __init__(self, eng, rank, world, n, key_space, ranks, lww=True, seed=2024):
        from crdt_amd import shard
        if world != 1:
            raise SystemExit("loopback_* workloads run R ranks on ONE GPU: use --gpus 1")
        self.eng, self.n, self.lww, self.R = eng, n, lww, ranks
        self.name = "loopback_set_merge" if lww else "loopback_orset_merge"
        self.kernel = f"whole op: crdt_shard_{'lww' if lww else 'orset'}_merge_local over {ranks} loopback ranks"
        self.comm = shard.Comm.loopback(torch.device(eng.device).index or 0, ranks)
        self.A, self.B = [], []
        for r in range(ranks):
            b, e = shard.shard_range(n, ranks, r)
            self.A.append(eng.synth_set_tuples(seed * 100 + r, 0, e - b, key_space))
            self.B.append(eng.synth_set_tuples(seed * 100 + r, 1, e - b, key_space))
        self.cap = 2 * n
        self.outs = [E.TupleSet.empty(self.cap, eng.device) for _ in range(ranks)]
        self.step()
        torch.cuda.synchronize()
        self.n_out = len(self.last[0])
        self.config = {"workload": f"{'LWW-Element-Set' if lww else 'OR-Set'} merge of a distributed population, "
                                   f"{n} tuples per side split over {ranks} loopback ranks on one GPU, key space "
                                   f"{key_space}: splitters + count matrix + one p2p group + owner merge + "
                                   "all-gather-v (BASELINE configs[3] sharded; the protocol's cost before xGMI)",
                       "tuples_per_side": n, "key_space": key_space, "loopback_ranks": ranks, "n_out": self.n_out,
                       "parallelism": f"key-range shard x{ranks} loopback ranks on 1 GPU"}

    def units(self):
        return 2 * self.n

    def bytes_per_launch(self):
        return 21 * 2 * self.n + 21 * self.n_out

    def step(self):
        self.last = self.comm.set_merge_local(self.A, self.B, lww=self.lww, gather=True, cap=self.cap,
                                              outs=self.outs)

    def outputs(self):
        out = {}
        for r, t in enumerate(self.last):            # every rank's copy of the merged state
            out.update(_tuple_arrays(t, f"r{r}_"))
        return out

    def extra(self, avg_ms):
        return {"exchange": {"transport": "loopback", "ranks": self.R, "n_out_total": self.n_out,
                             "note": "R ranks on one GPU: every rank receives the whole merged state (R-fold "
                                     "output writes); roofline.bytes_per_launch counts the merge once"}}


class LoopbackGossipRound(Workload):
    """crdt_population_round_sharded at the gossip_round bench's population
    (1000 replicas x 10k entries) over R LOOPBACK ranks on this one GPU: the
    per-replica counts all-gathered, the round's global draw planned on every
    rank, each rank's pulled Diffs packed and delivered by ONE point-to-point
    group, the merge over the received Diffs in place; each step the same
    draw, undone after (as gossip_round).  Prices the sharded protocol before
    the first multi-GPU run."""
    unit = "remote-entries/s"
    dtype = "int64"
    name = "loopback_gossip_round"
    scaling = "weak"

    def __init__(self, eng, rank, world, replicas, entries, ranks, seed=2024):
        from crdt_amd import gossip, shard, synth
        if world != 1:
            raise SystemExit("loopback_* workloads run R ranks on ONE GPU: use --gpus 1")
        self.kernel = f"gossip round through crdt_population_round_sharded over {ranks} loopback ranks"
        h = synth.refmerge_packed(seed, replicas, entries)
        n_l = len(h["l_ts"])
        kvk, kvv = h["kv_key"].view(np.uint32)[:n_l], h["kv_val"].view(np.uint32)[:n_l]
        self.comm = shard.Comm.loopback(torch.device(eng.device).index or 0, ranks)
        self.pops, self.R, self.P, self.n_l = [], ranks, replicas, n_l
        for i in range(ranks):
            b, e = shard.shard_range(replicas, ranks, i)
            lb, le = int(h["l_off"][b]), int(h["l_off"][e])
            kb, ke = int(h["l_kv"][lb]), int(h["l_kv"][le])
            host = {"replicas": e - b, "l_off": h["l_off"][b:e + 1] - lb, "l_ts": h["l_ts"][lb:le],
                    "l_origin": h["l_origin"][lb:le], "l_kv": h["l_kv"][lb:le + 1] - kb,
                    "kv_key": (kvk[kb:ke].astype(np.int64) - b * 62).astype(np.uint32), "kv_val": kvv[kb:ke],
                    "str_bytes": h["str_bytes"], "str_off": h["str_off"]}
            self.pops.append(gossip.NativePopulation.on_member(self.comm, i, host, 62, b))
        self.gossip = gossip
        self.peers = gossip.random_peers(np.random.default_rng(seed), replicas, 0, replicas)
        gossip.NativePopulation.round_sharded(self.comm, self.pops, self.peers)
        self.n_out = sum(p.sizes()[1] for p in self.pops)
        for p in self.pops:
            p.undo()
        self.config = {"workload": f"sharded gossip round: {replicas} replicas x {entries} Diff entries over "
                                   f"{ranks} loopback ranks on one GPU, each replica pulls a random peer's Diff "
                                   "(count all-gather + one p2p group of the pulled Diffs + in-place merge)",
                       "replicas": replicas, "entries": entries, "loopback_ranks": ranks,
                       "parallelism": f"replica shard x{ranks} loopback ranks on 1 GPU"}

    def units(self):
        return self.n_l

    def bytes_per_launch(self):
        # as gossip_round: the merge's compulsory bytes + the new Diffs' kv pairs
        n_r, n_out = self.n_l, self.n_out
        return self.n_l * 17 + n_r * 16 + n_r * 8 + n_out * 17 + n_out * 24

    def step(self):
        self.gossip.NativePopulation.round_sharded(self.comm, self.pops, self.peers)
        for p in self.pops:
            p.undo()

    def outputs(self):
        """Every step is the same round, undone after: the round once more,
        every rank's population read before it is undone."""
        self.gossip.NativePopulation.round_sharded(self.comm, self.pops, self.peers)
        out = {}
        for r, p in enumerate(self.pops):
            out.update(_population_arrays(p.read(), f"r{r}_"))
            p.undo()
        return out

    def extra(self, avg_ms):
        return {"exchange": {"transport": "loopback", "ranks": self.R,
                             "note": "the pulled Diffs of other ranks' replicas move as device copies on the one "
                                     "GPU; roofline.bytes_per_launch counts the merge once, not the exchange"}}


class ShardJoin(Workload):
    """configs[4] E2: every rank holds a DIVERGENT full copy of the
    [rows, nodes] counter state; the join is one in-place
    ncclAllReduce(ncclUint64, ncclMax) over xGMI
    (crdt_shard_allreduce_max_u64).  The bound is xGMI, reported as bus
    bandwidth 2(G-1)/G * S / t."""
    name = "shard_join"
    unit = "replica-merges/s"
    kernel = "RCCL ncclAllReduce(ncclUint64, ncclMax)"

    def __init__(self, eng, rank, world, rows, nodes, seed=2024):
        if world < 2:
            # one rank's in-place all-reduce moves nothing: a line would
            # report bytes that were never touched
            raise SystemExit("shard_join is the cross-GPU exchange of configs[4] E2: run it with --gpus >= 2")
        self.eng, self.world, self.rows, self.nodes = eng, world, rows, nodes
        self.state = eng.synth_counters(seed, 100 + rank, rows, nodes)    # divergent per rank
        self.comm = native_comm(eng, world)
        if self.comm is None:
            self.buf = torch.empty_like(self.state)
        self.config = {"workload": f"divergent full-state join, {rows} replicas x {nodes} nodes uint64 "
                                   f"({rows * nodes * 8 / 1e9:.3f} GB) per rank, all-reduce(max) "
                                   "(BASELINE configs[4], E2)",
                       "rows": rows, "nodes": nodes, "parallelism": f"state-replica x{world} + RCCL all-reduce(max)"}

    def units(self):
        return self.rows            # each rank's copy of every replica row merged once per step

    def bytes_per_launch(self):
        return self.rows * self.nodes * 8 * 2     # each rank reads its copy and writes the joined state

    def step(self):
        if self.comm is not None:
            self.comm.allreduce_max_u64([self.state])
            return
        self.eng.u64_to_ordered_i64(self.state, out=self.buf)
        if self.world > 1:
            import torch.distributed as dist
            dist.all_reduce(self.buf, op=dist.ReduceOp.MAX)
        self.eng.ordered_i64_to_u64(self.buf, out=self.state)

    def outputs(self):
        return {"state": self.state}

    def extra(self, avg_ms):
        S = self.rows * self.nodes * 8
        g = self.world
        bus = 2 * (g - 1) / g * S / (avg_ms / 1e3) / 1e9 if g > 1 else 0.0
        return {"xgmi": {"bus_bw": round(bus, 1), "unit": "GB/s", "bytes_per_rank": S,
                         "link_peak": 153.0, "links_per_gpu": 7,
                         "note": "ring all-reduce busBW = 2(G-1)/G * S / t; per-link bound"}}

    def cpu_baseline(self, seconds, threads):
        return None


class RefMergeBatch(Workload):
    """configs[0]'s merge (main.go:35-100) batched: P replicas x E entries."""
    name = "refmerge"
    unit = "remote-entries/s"
    dtype = "int64"
    kernel = "refmerge (whole op: k_rm_plan/geo/split/count/scan/write/fold + k_slot_final)"

    def __init__(self, eng, rank, world, replicas, entries, seed=2024):
        from crdt_amd import refmerge, synth
        self.eng = eng
        self.host = synth.refmerge_packed(seed + rank, replicas, entries)
        self.dev = refmerge.to_device(self.host, eng.device)
        out = eng.refmerge_batch(self.dev)
        torch.cuda.synchronize()
        self.n_out = int(out["off"][-1].item())
        h = self.host
        self.n_l, self.n_r, self.n_kv = len(h["l_ts"]), len(h["r_ts"]), len(h["kv_key"])
        self.config = {"workload": f"RefMerge (main.go:35-100) batched: {replicas} replicas x {entries} "
                                   f"Diff entries + ~{entries} RemoteDiff entries each (BASELINE configs[0] "
                                   "shape at scale)", "replicas": replicas, "entries": entries,
                       "n_remote": self.n_r, "n_new_diff": self.n_out, "parallelism": f"replicas x{world}"}

    def units(self):
        return self.n_r

    def bytes_per_launch(self):
        # compulsory: every input once, every output once
        return (self.n_l * 17 + self.n_r * 16 + self.n_kv * 8 + self.n_out * 17
                + self.host["n_slots"] * 13 + int(self.host["str_off"][-1]))

    def step(self):
        self.last = self.eng.refmerge_batch(self.dev)

    def outputs(self):
        return _refmerge_arrays(self.last)

    def io(self):
        o, n, ns = self.last, self.n_out, int(self.host["n_slots"])
        ins = [v for v in self.dev.values() if torch.is_tensor(v)]
        return ins, [o["off"], o["ts"][:n], o["origin"][:n], o["src"][:n], o["st_kind"][:ns], o["st_str"][:ns],
                     o["st_sum"][:ns]]

    def cpu_baseline(self, seconds, threads):
        """oc_refmerge, one replica per call (the reference merges under one
        mutex per Server, main.go:43-44), independent replicas on `threads`
        host threads like the reference's goroutine-per-replica (main.go:321).
        Per-replica compact arrays are prepared before the timed region."""
        from concurrent.futures import ThreadPoolExecutor
        from oracle import oracle
        h = self.host
        kvk, kvv = h["kv_key"].view(np.uint32), h["kv_val"].view(np.uint32)
        jobs = []
        for p in range(min(h["replicas"], 4 * threads)):
            lb, le = int(h["l_off"][p]), int(h["l_off"][p + 1])
            rb, re_ = int(h["r_off"][p]), int(h["r_off"][p + 1])
            lk0, lk1 = int(h["l_kv"][lb]), int(h["l_kv"][le])
            rk0, rk1 = int(h["r_kv"][rb]), int(h["r_kv"][re_])
            kv_key = np.concatenate([kvk[lk0:lk1], kvk[rk0:rk1]]) - np.uint32(p * 62)
            kv_val = np.concatenate([kvv[lk0:lk1], kvv[rk0:rk1]])
            l_kv = (h["l_kv"][lb:le + 1] - lk0).astype(np.uint32)
            r_kv = (h["r_kv"][rb:re_ + 1] - rk0 + (lk1 - lk0)).astype(np.uint32)
            jobs.append((h["l_ts"][lb:le].copy(), h["l_origin"][lb:le].copy(), l_kv, h["r_ts"][rb:re_].copy(),
                         r_kv, kv_key, kv_val, re_ - rb))

        def run(j):
            oracle.refmerge_packed(j[0], j[1], j[2], j[3], j[4], j[5], j[6], h["str_bytes"], h["str_off"], 62)
            return j[7]

        # parity spot-check of the timed batch before timing the CPU: replicas
        # spread over the whole 1000-replica batch == oc_refmerge (new Diff
        # keys, origins, sources and the replica's CurrentState slots)
        out = self.eng.refmerge_batch(self.dev)
        torch.cuda.synchronize()
        off = out["off"].cpu().numpy()
        g = {k: out[k].cpu().numpy() for k in ("ts", "origin", "src", "st_kind", "st_str", "st_sum")}
        P = h["replicas"]
        checked = sorted({0, 1, P // 3, P // 2, (2 * P) // 3, P - 2, P - 1} & set(range(P)))
        for p in checked:
            lb, le = int(h["l_off"][p]), int(h["l_off"][p + 1])
            rb, re_ = int(h["r_off"][p]), int(h["r_off"][p + 1])
            lk0, lk1 = int(h["l_kv"][lb]), int(h["l_kv"][le])
            rk0, rk1 = int(h["r_kv"][rb]), int(h["r_kv"][re_])
            o_ts, o_or, o_src, kind, sstr, ssum = oracle.refmerge_packed(
                h["l_ts"][lb:le], h["l_origin"][lb:le], (h["l_kv"][lb:le + 1] - lk0).astype(np.uint32),
                h["r_ts"][rb:re_], (h["r_kv"][rb:re_ + 1] - rk0 + (lk1 - lk0)).astype(np.uint32),
                np.concatenate([kvk[lk0:lk1], kvk[rk0:rk1]]) - np.uint32(p * 62),
                np.concatenate([kvv[lk0:lk1], kvv[rk0:rk1]]), h["str_bytes"], h["str_off"], 62)
            a, b = int(off[p]), int(off[p + 1])
            src = np.where(o_src >= 0, o_src + lb, o_src - rb)
            assert np.array_equal(g["ts"][a:b], o_ts) and np.array_equal(g["origin"][a:b], o_or), f"replica {p}"
            assert np.array_equal(g["src"][a:b], src), f"replica {p} src"
            sl = slice(p * 62, (p + 1) * 62)
            assert np.array_equal(g["st_kind"][sl], kind), f"replica {p} state"
            assert np.array_equal(g["st_str"][sl].view(np.uint32)[kind == 1], sstr[kind == 1])
            assert np.array_equal(g["st_sum"][sl][kind == 2], ssum[kind == 2])

        done, t0 = 0, time.perf_counter()
        with ThreadPoolExecutor(threads) as ex:
            while time.perf_counter() - t0 < seconds:
                done += sum(ex.map(run, jobs))
        dt = time.perf_counter() - t0
        return {"value": done / dt, "unit": self.unit, "cores": threads, "kind": "port",
                "sample": f"oc_refmerge (C restatement of main.go:35-100), one replica per call, {len(jobs)} "
                          f"replicas of the same batch on {threads} threads, {dt:.1f}s; device output of "
                          f"replicas {checked} checked == oc_refmerge first"}


class RefMergeDelta(RefMergeBatch):
    """The same batch through the incremental replay:
    crdt_refmerge_delta folds only the inserted R entries into a carried
    ts-keyed state.  Each step restores the state of L first (one 1.7 MB
    device copy, inside the timed region) so every step is the same merge."""
    name = "refmerge_delta"
    kernel = "refmerge_delta (whole op: walk passes + k_rp_fold x2 + k_rp_final + state restore)"

    io = None
    e2e_skip = "the step restores its carried replay state first (device-resident by design)"

    def __init__(self, eng, rank, world, replicas, entries, seed=2024):
        super().__init__(eng, rank, world, replicas, entries, seed)
        # the five state arrays as views of one buffer: the restore is ONE copy
        n = max(int(self.dev["n_slots"]), 1)
        self.buf0 = torch.empty(28 * n, dtype=torch.uint8, device=eng.device)
        self.buf = torch.empty_like(self.buf0)
        views = lambda b: {"best_key": b[0:8 * n].view(torch.int64), "sum": b[8 * n:16 * n].view(torch.int64),
                           "best_str": b[16 * n:20 * n].view(torch.int32), "npar": b[20 * n:24 * n].view(torch.int32),
                           "nhold": b[24 * n:28 * n].view(torch.int32)}
        self.st0 = eng.replay_state_init(self.dev, st=views(self.buf0))
        self.st = views(self.buf)
        self.config["workload"] = self.config["workload"].replace("RefMerge", "RefMerge, incremental replay,", 1)
        h = self.host
        self.n_rkv = int(h["r_kv"][-1] - h["r_kv"][0])

    def bytes_per_launch(self):
        # L ts + origin, R ts + kv range + its kvs, the output, the state (read + write), strings
        return (self.n_l * 9 + self.n_r * 16 + self.n_rkv * 8 + self.n_out * 17
                + self.host["n_slots"] * (28 * 2 + 13) + int(self.host["str_off"][-1]))

    def step(self):
        self.buf.copy_(self.buf0)
        self.last = self.eng.refmerge_delta(self.dev, self.st)

    def outputs(self):
        return dict(_refmerge_arrays(self.last), **{"state_" + k: v for k, v in self.st.items()})

    def cpu_baseline(self, seconds, threads):
        return None


class GossipRound(Workload):
    """Anti-entropy round (crdt_amd.gossip): every replica
    of a configs[0]-shaped population pulls a random peer's whole Diff
    (entries + kv pairs re-based to its key slots), all replicas merge in one
    batched call, and the next Diffs are materialised.  Each step restarts
    from the same initial population (the round does not modify its input
    tensors), with a fresh peer draw."""
    name = "gossip_round"
    unit = "remote-entries/s"
    dtype = "int64"
    kernel = ("gossip round through crdt_population_round (refmerge over the peers' Diffs in place + the new Diffs' "
              "kv pairs)")

    def __init__(self, eng, rank, world, replicas, entries, seed=2024):
        from crdt_amd import gossip, synth
        h = synth.refmerge_packed(seed + rank, replicas, entries)
        n_l = len(h["l_ts"])
        host = {"replicas": replicas, "l_off": h["l_off"], "l_ts": h["l_ts"], "l_origin": h["l_origin"],
                "l_kv": h["l_kv"], "kv_key": h["kv_key"].view(np.uint32)[:n_l], "kv_val": h["kv_val"].view(np.uint32)[:n_l],
                "str_bytes": h["str_bytes"], "str_off": h["str_off"]}
        # the round behind the C-ABI (crdt_population_round: what a cgo host of
        # main.go:226-261 calls); CRDT_GOSSIP_IMPL=python: the Python
        # orchestration over the same kernels (gossip.Population) for the A/B
        self.native = os.environ.get("CRDT_GOSSIP_IMPL", "native") != "python"
        if self.native:
            self.pop = gossip.NativePopulation(eng, host, 62)
            self.pop.pull_inplace = True
        else:
            self.pop = gossip.Population(eng, host, 62)
            # (A/B: CRDT_GOSSIP_PULL=assembled builds each RemoteDiff by segmented copies first)
            self.pop.pull_inplace = os.environ.get("CRDT_GOSSIP_PULL", "inplace") != "assembled"
            self.init = self.pop.snapshot()
        self.host = h
        self.rng = np.random.default_rng(seed)
        self.gossip, self.P, self.n_l = gossip, replicas, n_l
        self.peers = gossip.random_peers(self.rng, replicas, 0, replicas)
        if self.native:
            self.pop.round(self.peers)
            self.n_out = self.pop.sizes()[1]
            self.pop.undo()
        else:
            out = self.step()
            torch.cuda.synchronize()
            self.n_out = int(out["off"][-1].item())
        self.config = {"workload": f"gossip round: {replicas} replicas x {entries} Diff entries each pull a random "
                                   "peer's Diff and merge (BASELINE configs[0] shape at scale)",
                       "replicas": replicas, "entries": entries, "n_new_diff": self.n_out,
                       "parallelism": f"replicas x{world}"}

    def units(self):
        return self.n_l                      # every pulled entry (a peer's whole Diff per replica)

    def bytes_per_launch(self):
        # the merge (inputs + outputs once; R read in place from the peers' Diffs),
        # the next Diff's kv pairs (read + write kv pair, write kv range); with
        # assembled pulls (pull_inplace False) also the R assembly (read + write
        # ts, kv range, kv pair)
        n_r, n_out = self.n_l, self.n_out
        asm = 0 if self.pop.pull_inplace else n_r * 24 * 2
        return asm + (self.n_l * 17 + n_r * 16 + n_r * 8 + n_out * 17) + n_out * 24

    def step(self):
        if self.native:                       # every step is the same round from the same Diffs:
            self.pop.round(self.peers)        # the round, then back to the Diffs before it
            self.pop.undo()
            return None
        self.pop.restore(self.init)
        self.last = self.pop.round(self.peers)
        return self.last

    def _round(self):
        self.pop.round(self.peers)

    def outputs(self):
        """Native: every step is the same round, undone after, so the round
        runs once more and the population is read before it is undone."""
        if not self.native:
            return _refmerge_arrays(self.last)
        self._round()
        out = _population_arrays(self.pop.read())
        self.pop.undo()
        return out

    def cpu_baseline(self, seconds, threads):
        """The round's merge on the host: oc_refmerge (C restatement of
        main.go:35-100) of replica p's Diff with its peer's whole Diff as
        remote maps (main.go:245-256), one replica per call, independent
        replicas on `threads` host threads; units = pulled entries.  The
        per-replica arrays (the pull, with key slots made local) are built
        before the timed region."""
        from concurrent.futures import ThreadPoolExecutor
        from oracle import oracle
        h = self.host
        n_l = self.n_l
        kvk, kvv = h["kv_key"].view(np.uint32)[:n_l], h["kv_val"].view(np.uint32)[:n_l]
        jobs = []
        for p in range(min(self.P, 4 * threads)):
            q = int(self.peers[p])
            lb, le = int(h["l_off"][p]), int(h["l_off"][p + 1])
            qb, qe = int(h["l_off"][q]), int(h["l_off"][q + 1])
            lk0, lk1 = int(h["l_kv"][lb]), int(h["l_kv"][le])
            qk0, qk1 = int(h["l_kv"][qb]), int(h["l_kv"][qe])
            kv_key = np.concatenate([kvk[lk0:lk1] - np.uint32(p * 62), kvk[qk0:qk1] - np.uint32(q * 62)])
            kv_val = np.concatenate([kvv[lk0:lk1], kvv[qk0:qk1]])
            l_kv = (h["l_kv"][lb:le + 1] - lk0).astype(np.uint32)
            r_kv = (h["l_kv"][qb:qe + 1] - qk0 + (lk1 - lk0)).astype(np.uint32)
            jobs.append((h["l_ts"][lb:le].copy(), h["l_origin"][lb:le].copy(), l_kv, h["l_ts"][qb:qe].copy(),
                         r_kv, kv_key, kv_val, qe - qb))

        def run(j):
            oracle.refmerge_packed(j[0], j[1], j[2], j[3], j[4], j[5], j[6], h["str_bytes"], h["str_off"], 62)
            return j[7]

        done, t0 = 0, time.perf_counter()
        with ThreadPoolExecutor(threads) as ex:
            while time.perf_counter() - t0 < seconds:
                done += sum(ex.map(run, jobs))
        dt = time.perf_counter() - t0
        return {"value": done / dt, "unit": self.unit, "cores": threads, "kind": "port",
                "sample": f"oc_refmerge (C restatement of main.go:35-100) of a replica's Diff with its peer's "
                          f"pulled Diff, one replica per call, {len(jobs)} replicas of the round on {threads} "
                          f"threads, {dt:.1f}s"}


class GossipRoundWire(GossipRound):
    """The anti-entropy round with its pulls ON THE WIRE (SURVEY §8(f) rows 2
    and 4): every replica's pull arrives as the binary gossip body of a
    random peer's Diff (crdt_server_gossip_binary's format, the wire form of
    Diff.ToJSON, main.go:159), already in HBM; a step decodes all bodies on
    the device (crdt_gossip_decode: keys and values interned into device
    string tables, main.go:245-256), merges every replica in one batched call
    and materialises the next Diffs.  Each step restarts from the same
    population and the same bodies."""
    name = "gossip_round_wire"
    kernel = "gossip round from wire bodies through crdt_population_round_wire (device decode + refmerge + kv output)"

    def __init__(self, eng, rank, world, replicas, entries, seed=2024):
        from crdt_amd import codec, gossip, synth
        h = synth.refmerge_packed(seed + rank, replicas, entries)
        n_l = len(h["l_ts"])
        host = {"replicas": replicas, "l_off": h["l_off"], "l_ts": h["l_ts"], "l_origin": h["l_origin"],
                "l_kv": h["l_kv"], "kv_key": h["kv_key"].view(np.uint32)[:n_l], "kv_val": h["kv_val"].view(np.uint32)[:n_l],
                "str_bytes": h["str_bytes"], "str_off": h["str_off"]}
        # the wire round behind the C-ABI (crdt_population_round_wire: decode +
        # merge in one call, what a cgo host of main.go:226-261 binds);
        # CRDT_GOSSIP_IMPL=python: Population.round_wire over the same kernels
        self.native = os.environ.get("CRDT_GOSSIP_IMPL", "native") != "python"
        self.pop = gossip.NativePopulation(eng, host, 62) if self.native else gossip.Population(eng, host, 62)
        self.host, self.P, self.n_l, self.gossip = h, replicas, n_l, gossip
        names = [c.encode() for c in synth.ALPHABET]
        self.keys, self.vals = codec.StrTab(eng), codec.StrTab(eng)
        self.keys.intern(names)                                   # key id = alphabet index (slot p*62 + k)
        strs = [bytes(h["str_bytes"][h["str_off"][i]:h["str_off"][i + 1]]) for i in range(len(h["str_off"]) - 1)]
        self.vals.intern(strs)                                    # string ids = the packed batch's
        blob, boff = codec.encode_packed_diffs(host, names, 62)
        self.rng = np.random.default_rng(seed)
        self.peers = gossip.random_peers(self.rng, replicas, 0, replicas)
        bodies = [blob[boff[q]:boff[q + 1]] for q in self.peers]       # replica i pulls peers[i]
        self.body_off = np.zeros(replicas + 1, np.int64)
        self.body_off[1:] = np.cumsum([len(b) for b in bodies])
        self.body_bytes = int(self.body_off[-1])
        self.data = torch.frombuffer(bytearray(b"".join(bodies)), dtype=torch.uint8).to(eng.device)
        self.n_e = sum(codec.body_counts(b)[0] for b in bodies)
        self.n_p = sum(codec.body_counts(b)[1] for b in bodies)
        if self.native:
            self.pop.round_wire(self.data, self.body_off, self.keys, self.vals)
            self.n_out = self.pop.sizes()[1]
            self.pop.undo()
        else:
            self.init = self.pop.snapshot()
            self.str0 = (self.pop.str_bytes, self.pop.str_off)
            out = self.step()
            torch.cuda.synchronize()
            self.n_out = int(out["off"][-1].item())
        self.config = {"workload": f"gossip round from the wire: {replicas} replicas x {entries} Diff entries each "
                                   "pull a random peer's Diff as a binary gossip body in HBM, device decode + "
                                   "batched merge (BASELINE configs[0] shape at scale)",
                       "replicas": replicas, "entries": entries, "body_bytes": self.body_bytes,
                       "n_new_diff": self.n_out, "parallelism": f"replicas x{world}"}

    def units(self):
        return self.n_e                      # every pulled entry

    def bytes_per_launch(self):
        # the bodies read once, R written (ts, kv range, kv pair), the merge
        # (inputs + outputs once), the next Diff's kv gather
        n_r, n_out = self.n_e, self.n_out
        return self.body_bytes + n_r * 24 + (self.n_l * 17 + n_r * 16 + n_r * 8 + n_out * 17) + n_out * 24

    def step(self):
        if self.native:                       # the same round from the same Diffs every step
            self.pop.round_wire(self.data, self.body_off, self.keys, self.vals)
            self.pop.undo()
            return None
        self.pop.restore(self.init)
        self.pop.str_bytes, self.pop.str_off = self.str0
        self.last = self.pop.round_wire(self.data, self.body_off.tolist(), self.keys, self.vals, self.n_e, self.n_p)
        return self.last

    def _round(self):
        self.pop.round_wire(self.data, self.body_off, self.keys, self.vals)


class ServerMerge(Workload):
    """The path a Go caller of merge() actually hits (main.go:245-257):
    configs[0]'s 5 replicas x 10k Diff entries (main.go:319-321), each
    pulling a peer's Diff.  A step = for every Server, the ingest of the
    peer's binary gossip body (crdt_server_ingest_binary, main.go:245-256:
    host validation, the body parked in pinned memory) and then ONE
    crdt_servers_merge of all five: H2D of the parked bodies, device decode
    against the context's string tables, the RefMerge kernels over the
    HBM-resident Diffs, the device split back into each server's next Diff,
    and the CurrentState rebuild on the host (server.hip).  Re-merging the
    same pull is a no-op on the state (KAT-5), so every step does the same
    work.  Latency-bound by construction (a few hundred microseconds of
    kernels, host waits between them); the roofline object is reported
    against the device bytes for completeness."""
    name = "server_merge"
    unit = "remote-entries/s"
    dtype = "int64"
    kernel = "crdt_servers_merge end to end (ingest + H2D + device decode + refmerge kernels + split + state)"

    def __init__(self, eng, rank, world, replicas, entries, seed=2024):
        from crdt_amd import refmerge, server, synth
        self.eng, self.server = eng, server
        demo = synth.refmerge_demo(seed + rank, replicas, entries)
        self.demo = demo
        self.srv = []
        for p, (diff, _) in enumerate(demo):
            s = server.Server(eng, 8080 + p)
            for ts, v in diff.items():
                s.Diff.Put(ts, v)
            self.srv.append(s)
        # each replica's pull: the RemoteDiff of the demo, served as a binary
        # gossip body by a host-only peer (its Diff = those remote maps)
        self.bodies = []
        for p, (_, remote) in enumerate(demo):
            peer = server.Server(None, 9000 + p)
            for ts, v in remote.items():
                peer.Diff.Put(ts, dict(v))
            st, body = peer.GossipBinary()
            assert st == 200
            self.bodies.append(body)
            peer.close()
        self.n_r = sum(len(r) for _, r in demo)
        self.step()
        self.n_diff = sum(len(s.DiffSignature) for s in self.srv)
        self.config = {"workload": f"Server.merge() end to end: {replicas} replicas x {entries} Diff entries, "
                                   f"each ingests a peer's pulled Diff (binary gossip body) and all merge in one "
                                   "crdt_servers_merge (BASELINE configs[0], main.go:245-257, :319-321)",
                       "replicas": replicas, "entries": entries, "n_remote": self.n_r, "n_diff": self.n_diff,
                       "parallelism": f"replicas x{world}"}

    def units(self):
        return self.n_r

    def bytes_per_launch(self):
        return self.n_diff * 17 + self.n_r * 16

    def step(self):
        for s, body in zip(self.srv, self.bodies):
            assert s.IngestBinary(body) == 0
        self.server.merge_servers(self.srv)

    def outputs(self):
        """Each server's Diff (ts, local origin) and its CurrentState as the bytes of its sorted "key=value" lines."""
        out = {}
        for p, s in enumerate(self.srv):
            sig = s.DiffSignature
            out[f"s{p}_diff_ts"] = np.array([t for t, _ in sig], np.int64)
            out[f"s{p}_diff_local"] = np.array([o == "local" for _, o in sig], np.uint8)
            state = "".join(f"{k}={v}\n" for k, v in sorted(s.CurrentState.items()))
            out[f"s{p}_state"] = np.frombuffer(state.encode("utf-8", "surrogatepass"), np.uint8)
        return out

    def cpu_baseline(self, seconds, threads):
        """oc_refmerge of each replica's (Diff, pulled RemoteDiff), one replica
        per call on min(replicas, threads) threads -- the reference merges each
        Server under its own mutex in its own goroutine (main.go:43-44, :321).
        Ingest is not timed on this side (the packed arrays are prepared
        first), so the ratio favours the CPU."""
        from concurrent.futures import ThreadPoolExecutor
        from crdt_amd import refmerge
        from oracle import oracle
        jobs = []
        for diff, remote in self.demo:
            pk = refmerge.Packer()
            pk.add_replica(diff, remote)
            h = pk.arrays()
            jobs.append((h["l_ts"], h["l_origin"], h["l_kv"].astype(np.uint32), h["r_ts"], h["r_kv"].astype(np.uint32),
                         h["kv_key"].view(np.uint32), h["kv_val"].view(np.uint32), h["str_bytes"], h["str_off"],
                         int(h["n_slots"]), len(h["r_ts"])))

        def run(j):
            oracle.refmerge_packed(*j[:10])
            return j[10]

        nt = min(len(jobs), threads)
        done, t0 = 0, time.perf_counter()
        with ThreadPoolExecutor(nt) as ex:
            while time.perf_counter() - t0 < seconds:
                done += sum(ex.map(run, jobs))
        dt = time.perf_counter() - t0
        return {"value": done / dt, "unit": self.unit, "cores": nt, "kind": "port",
                "sample": f"oc_refmerge (C restatement of main.go:35-100) of the same {len(jobs)} replicas' Diff + "
                          f"pulled RemoteDiff, one replica per call on {nt} threads, {dt:.1f}s"}


def make_workload(name, eng, rank, world, args):
    if name == "gossip_round":
        return GossipRound(eng, rank, world, args.replicas, args.entries)
    if name == "gossip_round_wire":
        return GossipRoundWire(eng, rank, world, args.replicas, args.entries)
    if name == "server_merge":
        return ServerMerge(eng, rank, world, args.demo_replicas, args.demo_entries)
    if name == "refmerge":
        return RefMergeBatch(eng, rank, world, args.replicas, args.entries)
    if name == "refmerge_delta":
        return RefMergeDelta(eng, rank, world, args.replicas, args.entries)
    if name == "gcounter_join":
        return GCounterJoin(eng, rank, world, args.rows, args.nodes)
    if name == "pncounter_join":
        return PNCounterJoin(eng, rank, world, args.rows, args.nodes)
    if name == "vclock_classify":
        return VClockClassify(eng, rank, world, args.pairs, 128)
    if name in ("lww_merge", "orset_merge"):
        return SetMerge(eng, rank, world, args.set_n, args.key_space, lww=(name == "lww_merge"))
    if name in ("lww_merge_d2", "orset_merge_d2"):
        return SetMergeUnsorted(eng, rank, world, args.set_n, args.key_space, lww=(name == "lww_merge_d2"))
    if name == "shard_fold":
        return ShardFold(eng, rank, world, args.total_rows, args.nodes)
    if name == "shard_join":
        return ShardJoin(eng, rank, world, args.rows, args.nodes)
    if name in ("loopback_set_merge", "loopback_orset_merge"):
        return LoopbackSetMerge(eng, rank, world, args.set_n, args.key_space, args.loopback,
                                lww=(name == "loopback_set_merge"))
    if name == "loopback_gossip_round":
        return LoopbackGossipRound(eng, rank, world, args.replicas, args.entries, args.loopback)
    if name in ("shard_set_merge", "shard_orset_merge"):
        return ShardSetMerge(eng, rank, world, args.set_n, args.key_space, lww=(name == "shard_set_merge"))
    raise SystemExit(f"unknown workload {name}")


def load_traffic(workload: Workload):
    """HBM bytes per launch from the committed rocprofv3 PMC summary, if any."""
    p = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        with open(p) as f:
            d = json.load(f).get(workload.name)
    except (OSError, ValueError):
        return None
    if not d or d.get("bytes_per_launch_algorithmic") != workload.bytes_per_launch():
        return None
    return d.get("hbm_bytes_per_launch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="shard_fold",
                    choices=["gcounter_join", "pncounter_join", "vclock_classify", "lww_merge", "orset_merge",
                             "lww_merge_d2", "orset_merge_d2", "shard_fold", "shard_join", "refmerge",
                             "refmerge_delta", "gossip_round", "gossip_round_wire", "server_merge",
                             "shard_set_merge", "shard_orset_merge", "loopback_set_merge", "loopback_orset_merge",
                             "loopback_gossip_round"])
    ap.add_argument("--loopback", type=int, default=8, help="ranks of the loopback_* workloads (one GPU)")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--nodes", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--set-n", type=int, default=10_000_000)
    ap.add_argument("--key-space", type=int, default=8_000_000)
    ap.add_argument("--total-rows", type=int, default=100_000_000)
    ap.add_argument("--replicas", type=int, default=1000)
    ap.add_argument("--entries", type=int, default=10_000)
    ap.add_argument("--demo-replicas", type=int, default=5)      # main.go:319-321
    ap.add_argument("--demo-entries", type=int, default=10_000)
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write the last step's outputs to DIR/<name>.npy (dump_outputs)")
    ap.add_argument("--full", action="store_true",
                    help="also measure the streaming peaks, the PCIe-inclusive e2e_pcie time and the CPU baseline "
                         "(with its parity spot-check); a plain run only times the steps")
    ap.add_argument("--cpu-seconds", type=float, default=8.0)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-e2e", action="store_true", help="with --full: skip the PCIe-inclusive e2e_pcie measurement")
    ap.add_argument("--no-peaks", action="store_true",
                    help="with --full: skip the self-measured peak sweep")
    ap.add_argument("--option", action="append", default=[],
                    help="name=value kernel knob (crdt_set_option; loads the diagnostic build, A/B runs only)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))          # before any GPU call in this process
    # The result line is the only thing this process writes to stdout: native
    # libraries (RCCL's version banner at communicator init) print to fd 1,
    # so fd 1 is pointed at stderr and the line goes to the saved stdout.
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)
    world, rank, local = dist_init()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE {world}: refusing to report a mismatched n_gpus")
    if args.option:                               # knobs: the diagnostic build (the product has none)
        from crdt_amd import _lib
        _lib.use_diag_build()
        for o in args.option:
            k, v = o.split("=")
            _lib.set_option(k, int(v))

    eng = E.Engine(local)
    wl = make_workload(args.workload, eng, rank, world, args)
    dev = eng.device
    stream = torch.cuda.current_stream(dev)

    for _ in range(args.warmup):
        wl.step()
    torch.cuda.synchronize(dev)
    barrier(world)
    torch.cuda.synchronize(dev)

    evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    mark = None
    if os.environ.get("CRDT_TRACE_MARK"):           # tools/timeline.py: a tiny crdt_stream_copy before each step
        mark = (torch.zeros(64, dtype=torch.int64, device=dev), torch.zeros(64, dtype=torch.int64, device=dev))
    t0 = time.perf_counter()
    evs[0].record(stream)
    for k in range(args.steps):
        if mark is not None:
            eng.stream_copy(mark[0], mark[1], 1, 1)
        wl.step()
        evs[k + 1].record(stream)
    torch.cuda.synchronize(dev)
    barrier(world)
    torch.cuda.synchronize(dev)
    wall = time.perf_counter() - t0

    # kernels cannot return errors: a raised device flag (e.g. a set merge's
    # bounded look-back timing out) means the timed outputs are invalid
    flags = eng.device_status(clear=True)
    if flags:
        raise SystemExit(f"rank {rank}: device-side failure flags 0x{flags:x} during the timed loop: "
                         "outputs invalid, no line reported")
    step_ms = [evs[k].elapsed_time(evs[k + 1]) for k in range(args.steps)]
    gpu_s = sum(step_ms) / 1e3
    elapsed = max_over_ranks(wall, world, dev)
    total_units = sum_over_ranks(wl.units() * args.steps, world, dev)
    value = total_units / elapsed

    if args.dump_outputs:                             # before --full's legs run the step again
        dump_outputs(args.dump_outputs, wl.outputs(), f"rank{rank}_" if world > 1 else "")

    out = None
    if rank == 0:
        avg_ms = float(np.mean(step_ms))
        med_ms = float(np.median(step_ms))
        achieved = wl.bytes_per_launch() / (avg_ms / 1e3) / 1e9
        traffic = load_traffic(wl)
        if not args.full:
            peaks = None
        elif args.no_peaks:
            peaks = {"copy": float("nan"), "read": float("nan"), "skipped": "--no-peaks"}
        else:
            peaks = measure_peaks(eng)
        roof = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                "measured_peak": peaks or {"skipped": "measured with --full"},
                "frac_of_copy_peak": round(achieved / peaks["copy"], 4) if peaks else None,
                "frac_of_read_peak": round(achieved / peaks["read"], 4) if peaks else None,
                "peak_basis": ("read (a read-dominated step: compare frac_of_read_peak)"
                               if getattr(wl, "read_dominated", False) else "copy (reads + writes)"),
                "kernel": wl.kernel, "bytes_per_launch": wl.bytes_per_launch(),
                "avg_launch_us": round(avg_ms * 1e3, 2), "median_launch_us": round(med_ms * 1e3, 2),
                "timing": "HIP events on the launch stream, per step"}
        e2e = measure_e2e(wl) if args.full and world == 1 and not args.no_e2e else None
        cpu = None
        if args.full and world == 1 and not args.no_cpu_baseline and hasattr(wl, "cpu_baseline"):
            threads, aff = cpu_share()
            cpu = wl.cpu_baseline(args.cpu_seconds, threads)
            if cpu is not None:
                cpu["value"] = round(cpu["value"], 1)
                cpu["host_cpu"] = _cpu_model()
                cpu["nproc"] = os.cpu_count()
                cpu["affinity_cpus"] = aff
                cpu["cpu_share"] = ("threads = min(affinity mask, OMP_NUM_THREADS = "
                                    f"{os.environ.get('OMP_NUM_THREADS', 'unset')}): the GPU's host CPU share")
                if aff > threads:                     # the same restatement on the whole host
                    whole = wl.cpu_baseline(args.cpu_seconds, aff)
                    if whole is not None:
                        cpu["whole_host"] = {"value": round(whole["value"], 1), "unit": whole["unit"],
                                             "cores": whole["cores"], "sample": whole["sample"],
                                             "cgroup_cpu_max": _cgroup_cpu_max()}
        from crdt_amd import _lib
        rccl = _lib.rccl_info()                       # the RCCL this process resolved
        config = dict(wl.config)
        if "parallelism" in config:
            config["parallelism"] = f"{config['parallelism']} [RCCL {rccl['version']}]"
        config["rccl"] = rccl
        config["build"] = ("diag: " + ",".join(args.option)) if args.option else "product (libcrdt_amd.so)"
        out = {
            "metric": METRIC, "value": round(value, 1), "unit": wl.unit, "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed * 1e3 / args.steps, 4),
            "higher_is_better": True, "scaling": getattr(wl, "scaling", "weak"),
            "vs_baseline": None, "dtype": wl.dtype,
            "data": "synthetic (SplitMix64-seeded, generated in HBM)",
            "config": config, "roofline": roof, "cpu_baseline": cpu, "e2e_pcie": e2e,
            "gpu_time_s": round(gpu_s, 6),
        }
        if hasattr(wl, "extra"):
            out.update(wl.extra(avg_ms))
        sys.stdout.flush()
        os.write(result_fd, (json.dumps(out) + "\n").encode())
    if getattr(wl, "comm", None) is not None:
        wl.comm.close()                               # before the engine whose context it borrows
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    eng.close()


def _cgroup_cpu_max():
    """This process's cgroup CPU quota ("quota period" or "max"): on a shared
    box the threads of the whole-host baseline may only get this much time."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            return f.read().strip()
    except OSError:
        return None


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


if __name__ == "__main__":
    main()
