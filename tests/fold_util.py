"""Launch geometry, witness schedules and witness populations for the
column-max fold tests (tests/test_gpu_fold_witness.py).

The geometry functions restate how csrc/counters.hip sizes its launches
(crdt_gcounter_fold, join_impl) so a test can pick the rows where a wrong
loop bound would show, and assert that its shape still reaches every loop
when the CU count or a knob default changes.  The schedule is plain numpy,
so it can be run against a deliberately wrong host fold without a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Sequence, Tuple

import numpy as np

U64_MAX = 2**64 - 1


def grid_for(work_items: int, block: int, cap: int) -> int:
    """common.hpp grid_for."""
    return max(1, min((work_items + block - 1) // block, cap))


def shard_cuts(rows: int, world: int = 8) -> List[int]:
    """crdt_shard_range's cuts: shard r = [cuts[r], cuts[r + 1])."""
    from crdt_amd import shard
    cuts = [shard.shard_range(rows, world, r)[0] for r in range(world)] + [rows]
    assert all(shard.shard_range(rows, world, r) == (cuts[r], cuts[r + 1]) for r in range(world))
    return cuts


@dataclass
class FoldGeometry:
    """One crdt_gcounter_fold launch.  pow2 path: a lane reads 16-byte vectors
    i0, i0 + stride, ...; `full_steps` unrolled iterations (unroll * stride
    vectors each) are run by every lane, the `rem` vectors after `full_end`
    are `rem_full` whole strides and one of `rem_part` vectors.  generic path:
    block b reads rows b, b + grid, ...: `stride` = grid rows, unroll 1."""
    path: str
    rows: int
    nodes: int
    grid: int
    unroll: int
    stride: int                     # vectors (pow2) or rows (generic) the whole grid covers per step
    per_row: int                    # vectors per row (pow2), 1 (generic)
    full_steps: int = field(init=False)
    full_end: int = field(init=False)
    rem_full: int = field(init=False)
    rem_part: int = field(init=False)

    def __post_init__(self):
        total = self.rows * self.per_row
        step = self.unroll * self.stride
        self.full_steps = total // step
        self.full_end = self.full_steps * step
        rem = total - self.full_end
        self.rem_full, self.rem_part = rem // self.stride, rem % self.stride

    @property
    def stride_rows(self) -> int:
        return self.stride // self.per_row

    def boundary_rows(self) -> List[int]:
        """Last row of the final full unrolled step, the first row after it,
        and the first and last row of every stride of the remainder."""
        total, out = self.rows * self.per_row, []
        if 0 < self.full_end:
            out.append((self.full_end - 1) // self.per_row)
        a = self.full_end
        while a < total:
            b = min(a + self.stride, total)
            out += [a // self.per_row, (b - 1) // self.per_row]
            a = b
        return out


def fold_geometry(rows: int, nodes: int, cus: int, unroll: int, blocks_per_cu: int, aligned: bool = True) -> FoldGeometry:
    pow2 = 2 <= nodes <= 512 and nodes & (nodes - 1) == 0 and aligned
    if pow2:
        grid = grid_for(rows * nodes // 2, 256 * unroll, cus * blocks_per_cu)
        return FoldGeometry("pow2", rows, nodes, grid, unroll, grid * 256, nodes // 2)
    grid = grid_for(rows, 1, cus * 4)
    return FoldGeometry("generic", rows, nodes, grid, 1, grid, 1)


def pow2_rows(nodes: int, cus: int, blocks_per_cu: int, strides: int = 35, extra_rows: int = 5) -> int:
    """Rows that fill `strides` whole strides of the capped pow2 grid plus
    `extra_rows`.  35 = 2*16 + 3 = 4*8 + 3 = 8*4 + 3 = 17*2 + 1: for unroll 2,
    4, 8 and 16 at least two full unrolled steps, then at least one whole
    stride and a partial one for the remainder loop."""
    stride_rows = cus * blocks_per_cu * 512 // nodes
    return strides * stride_rows + extra_rows


@dataclass
class JoinGeometry:
    n: int
    grid: int
    unroll: int
    stride: int
    full_steps: int
    rem_full: int
    rem_part: int


def join_geometry(n: int, cus: int, unroll: int, blocks_per_cu: int) -> JoinGeometry:
    n2 = n // 2
    grid = grid_for(n2, 256, cus * blocks_per_cu)
    stride = grid * 256
    full = n2 // (unroll * stride)
    rem = n2 - full * unroll * stride
    return JoinGeometry(n, grid, unroll, stride, full, rem // stride, rem % stride)


def join_rows(nodes: int, cus: int, unroll: int, blocks_per_cu: int) -> int:
    """Odd row count (nodes odd: an odd element count) whose vectors are two
    full unrolled steps, one whole remainder stride (unroll > 1) and a partial one."""
    stride = cus * blocks_per_cu * 256
    n2 = (2 * unroll + (1 if unroll > 1 else 0)) * stride + 777
    rows = (2 * n2 + nodes - 1) // nodes
    return rows | 1


# ---------------------------------------------------------------- witness schedule
def witness_values(nodes: int, k: int, base: int = 0) -> np.ndarray:
    """`nodes` distinct values counted down from 2^64-1-base, rotated by k:
    all >= 2^63 (a signed maximum loses), one of them 2^64-1 when base = 0."""
    assert base + nodes < 2**62
    return (np.uint64(U64_MAX - base) - ((np.arange(nodes, dtype=np.uint64) + np.uint64(k)) % np.uint64(nodes)))


def special_rows(rows: int, geom: FoldGeometry, cuts: Sequence[int]) -> List[int]:
    want = [0, rows - 1, 1, rows - 2] + geom.boundary_rows()
    for c in cuts:
        want += [c - 1, c, c + 1]
    out = []
    for r in want:
        if 0 <= r < rows and r not in out:
            out.append(r)
    return out


def witness_schedule(rows: int, nodes: int, special: Sequence[int], seed: int, n_random: int = 8):
    """[(name, row_of_column[nodes], values[nodes])]: every special row with a
    witness in ALL columns in a round of its own, then n_random rounds with
    each column's witness in a seeded random row."""
    rng = np.random.default_rng(seed)
    sched = [(f"row {r}", np.full(nodes, r, np.int64)) for r in special]
    sched += [(f"random {k}", rng.integers(0, rows, nodes, dtype=np.int64)) for k in range(n_random)]
    return [(name, rr, witness_values(nodes, k)) for k, (name, rr) in enumerate(sched)]


def shard_witnesses(cuts: Sequence[int], nodes: int):
    """[(row, cols, values)] for the per-shard check: every shard's LAST row
    carries witnesses in the even columns, its FIRST row in the odd columns,
    so each shard holds exactly one witness per column.  Even-column values
    fall from shard to shard and odd-column values rise, so the row just past
    either end of a shard holds, in its columns, a value above everything
    inside the shard: reading one row too many in either direction, or one
    row too few, changes that shard's fold."""
    world = len(cuts) - 1
    even, odd = np.arange(0, nodes, 2), np.arange(1, nodes, 2)
    out = []
    for r in range(world):
        out.append((cuts[r + 1] - 1, even, np.uint64(U64_MAX) - (np.uint64((r + 1) * nodes) + even.astype(np.uint64))))
        out.append((cuts[r], odd, np.uint64(U64_MAX) - (np.uint64((world - r) * nodes) + odd.astype(np.uint64))))
    return out


def check_schedule(host: np.ndarray, bg_fold: np.ndarray, sched, fold: Callable[[np.ndarray], np.ndarray]) -> List[str]:
    """Run the schedule against a host fold; the names of the rounds it fails
    (the witness round or the restore round).  For checking the tests
    themselves against deliberately wrong folds."""
    cols, failed = np.arange(host.shape[1]), []
    for name, rr, vals in sched:
        saved = host[rr, cols].copy()
        host[rr, cols] = vals
        ok = np.array_equal(fold(host), vals)
        host[rr, cols] = saved
        if not ok or not np.array_equal(fold(host), bg_fold):
            failed.append(name)
    return failed


# ---------------------------------------------------------------- device population
class Population:
    """A synth.counters stream [rows, nodes] with every 2^64-1 cell set to 0,
    on the device (`t`) and on the host (`host`), and its fold (`bg`)."""

    def __init__(self, eng, rows: int, nodes: int, seed: int = 5, stream: int = 4, misaligned: bool = False):
        import torch
        from crdt_amd import synth
        from crdt_amd.engine import as_u64
        from oracle import oracle
        self.eng, self.rows, self.nodes = eng, rows, nodes
        gen = eng.synth_counters(seed, stream, rows, nodes)
        gen.masked_fill_(gen == -1, 0)
        if misaligned:                          # contiguous [rows, nodes] view 8 bytes into a 16-byte-aligned buffer
            self._flat = torch.empty(rows * nodes + 2, dtype=torch.int64, device=eng.device)
            self.t = self._flat[1:1 + rows * nodes].view(rows, nodes)
            self.t.copy_(gen)
        else:
            self.t = gen
        self.host = as_u64(self.t).reshape(rows, nodes)
        head = synth.counters(seed, stream, min(rows * nodes, 8192))
        head[head == np.uint64(U64_MAX)] = 0
        np.testing.assert_array_equal(self.host.reshape(-1)[:len(head)], head)
        self.bg = oracle.gcounter_fold(self.host)
        # the background's column maxima: distinct, each held by exactly one row
        assert len(np.unique(self.bg)) == nodes, "background maxima not distinct"
        assert ((self.host == self.bg[None, :]).sum(axis=0) == 1).all(), "background maximum tied"

    def put(self, rr, cc, vals) -> None:
        import torch
        dev = self.t.device
        v = np.ascontiguousarray(vals, dtype=np.uint64)
        self.t[torch.as_tensor(np.asarray(rr, np.int64), device=dev), torch.as_tensor(np.asarray(cc, np.int64), device=dev)] = \
            torch.from_numpy(v.view(np.int64).copy()).to(dev)
        self.host[rr, cc] = v

    def fold(self) -> np.ndarray:
        from crdt_amd.engine import as_u64
        return as_u64(self.eng.gcounter_fold(self.t))


def run_rounds(pop: Population, sched, fold: Callable[[], Sequence[np.ndarray]], oracle_rounds: Sequence[str] = ()) -> None:
    """Each round: write the witnesses (device and host), every array `fold()`
    returns == the witness vector, restore, every array == the background fold."""
    from oracle import oracle
    cols = np.arange(pop.nodes)
    for name, rr, vals in sched:
        assert (vals > pop.bg).all() and (vals >= np.uint64(2**63)).all() and len(np.unique(vals)) == pop.nodes
        saved = pop.host[rr, cols].copy()
        try:
            pop.put(rr, cols, vals)
            for k, got in enumerate(fold()):
                np.testing.assert_array_equal(got, vals, err_msg=f"witness round '{name}' (output {k})")
            if name in oracle_rounds:
                np.testing.assert_array_equal(oracle.gcounter_fold(pop.host), vals, err_msg=f"oracle, round '{name}'")
        finally:
            pop.put(rr, cols, saved)
        for k, got in enumerate(fold()):
            np.testing.assert_array_equal(got, pop.bg, err_msg=f"after restoring round '{name}' (output {k})")
