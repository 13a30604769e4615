"""Launch geometry and witness populations for the lane-group kernels:
crdt_vclock_classify (csrc/vclock.hip) and the row sums behind
crdt_gcounter_value / crdt_pncounter_value (csrc/counters.hip, k_rowsum*).

Both spread a row over NODES/2 lanes (16 bytes each), pack 64/(NODES/2) rows
into one wave-load, walk the rows in a wave-level grid-stride loop, and fall
back to a one-wave-per-row generic kernel for any other node count or a
pointer that is not 16-byte aligned.  The geometry functions restate how the
two launchers size their grids, so a test can pick the row counts at which a
wrong loop bound would show and assert that its shape still reaches the
second sweep when the CU count or a knob default changes.  The populations
are plain numpy, so tests/test_lanegroup_witness_table.py can run them
against deliberately wrong host classifiers without a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import numpy as np

from fold_util import grid_for

U64_MAX = 2**64 - 1
EQUAL, BEFORE, AFTER, CONCURRENT = 0, 1, 2, 3
SWAP = np.array([EQUAL, AFTER, BEFORE, CONCURRENT], np.uint8)      # classify(b, a) from classify(a, b)
CANARY = 0xFF                                                       # no class: an entry the kernel never wrote
VCLOCK_VECTOR_NODES = (32, 64, 128)
ROWSUM_VECTOR_NODES = (16, 32, 64, 128)
VCLOCK_UNROLLS = (1, 2, 4, 8, 16, 32)
ORDER_MAP_CAP = 4096                                                # crdt_u64_to_ordered_i64's block cap


# ---------------------------------------------------------------- geometry
@dataclass(frozen=True)
class LaneGeometry:
    """One launch of a lane-group kernel.  `rows_per_load` rows share one
    wave-load (64 / lanes per row; 1 for the generic kernel), a wave handles
    `rows_per_iter` rows per loop iteration (rows_per_load x the unroll) and
    one pass of the whole grid, a sweep, covers `sweep` rows."""
    kernel: str                     # "vector" | "generic"
    rows: int
    nodes: int
    grid: int
    cap: int
    waves: int
    rows_per_load: int
    rows_per_iter: int

    @property
    def sweep(self) -> int:
        return self.waves * self.rows_per_iter

    @property
    def full_sweeps(self) -> int:
        return self.rows // self.sweep

    @property
    def partial(self) -> int:
        return self.rows % self.sweep

    def where(self, p: int) -> str:
        """Row p relative to the sweep boundaries, for a failure message."""
        s, off = divmod(p, self.sweep)
        wave, r = divmod(off, self.rows_per_iter)
        return (f"row {p} = sweep {s} + {off} (sweep = {self.sweep} rows; wave {wave}, row {r} of its "
                f"{self.rows_per_iter}; {self.kernel} kernel, grid {self.grid})")


def _lanes(kernel: str, rows: int, nodes: int, cap: int, unroll: int) -> LaneGeometry:
    grid = grid_for(rows * 64, 256, cap)
    rpl = 64 // (nodes // 2) if kernel == "vector" else 1
    return LaneGeometry(kernel, rows, nodes, grid, cap, grid * 4, rpl, rpl * (unroll if kernel == "vector" else 1))


def vclock_unroll(pairs_per_wave: int) -> int:
    """launch_vc's switch: anything it does not name runs U = 4."""
    return pairs_per_wave if pairs_per_wave in (1, 2, 8, 16, 32) else 4


def vclock_geometry(pairs: int, nodes: int, cus: int, pairs_per_wave: int, blocks_per_cu: int,
                    aligned: bool = True) -> LaneGeometry:
    """crdt_vclock_classify: k_vclock<NODES, U> for 16-byte-aligned a and b at
    32 / 64 / 128 nodes, k_vclock_generic (one pair per wave) otherwise."""
    kernel = "vector" if aligned and nodes in VCLOCK_VECTOR_NODES else "generic"
    return _lanes(kernel, pairs, nodes, cus * blocks_per_cu, vclock_unroll(pairs_per_wave))


def rowsum_geometry(rows: int, nodes: int, cus: int, aligned: bool = True) -> LaneGeometry:
    """rowsum<PN>: k_rowsum<NODES> for aligned operands at 16 / 32 / 64 / 128
    nodes, k_rowsum_generic otherwise; at most 8 blocks per CU, no unroll."""
    kernel = "vector" if aligned and nodes in ROWSUM_VECTOR_NODES else "generic"
    return _lanes(kernel, rows, nodes, cus * 8, 1)


def order_map_sweep(n: int) -> int:
    """Elements one pass of k_u64_to_i64 / k_i64_to_u64's grid covers."""
    return grid_for(n, 256, ORDER_MAP_CAP) * 256


def sweep_rows(g: LaneGeometry, sweeps: int = 2, loads: int = 3, extra: int = 1) -> int:
    """Rows that fill `sweeps` sweeps of the CAPPED grid, `loads` more
    wave-loads and `extra` rows; `g` is any geometry of the shape wanted."""
    return sweeps * g.cap * 4 * g.rows_per_iter + loads * g.rows_per_load + extra


def assert_sweeps(g: LaneGeometry, sweeps: int = 2) -> None:
    """The preconditions of a sweep test: the grid is at its cap, every wave
    runs its loop `sweeps` times and some of them once more, and the last
    wave-load is ragged wherever one holds more than one row."""
    assert g.grid == g.cap, f"grid {g.grid} below its cap {g.cap}: {g}"
    assert g.full_sweeps >= sweeps and 0 < g.partial < g.sweep, f"not {sweeps} full sweeps plus a partial one: {g}"
    assert g.rows_per_load == 1 or g.rows % g.rows_per_load != 0, f"no ragged last wave-load: {g}"


# ---------------------------------------------------------------- references
def classify_ref(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The reference: le = all a <= b, ge = all a >= b on uint64."""
    assert a.dtype == np.uint64 and b.dtype == np.uint64 and a.shape == b.shape and a.ndim == 2
    return classes(~(a > b).any(axis=1), ~(a < b).any(axis=1))


def classes(le: np.ndarray, ge: np.ndarray) -> np.ndarray:
    return np.where(le, np.where(ge, EQUAL, BEFORE), np.where(ge, AFTER, CONCURRENT)).astype(np.uint8)


def rowsum_ref(p: np.ndarray, n: Optional[np.ndarray] = None) -> np.ndarray:
    """sum(p) - sum(n) per row in uint64 (wraps), as int64."""
    assert p.dtype == np.uint64 and p.ndim == 2
    s = p.sum(axis=1, dtype=np.uint64)
    if n is not None:
        assert n.dtype == np.uint64 and n.shape == p.shape
        with np.errstate(over="ignore"):
            s = s - n.sum(axis=1, dtype=np.uint64)
    return s.view(np.int64)


def check_population(a: np.ndarray, b: np.ndarray, classify: Callable[[np.ndarray, np.ndarray], np.ndarray]) -> int:
    """Pairs on which `classify(a, b)` differs from the reference."""
    got = np.asarray(classify(a, b))
    assert got.shape == (a.shape[0],)
    return int((got != classify_ref(a, b)).sum())


# ---------------------------------------------------------------- delta kinds
KINDS = 4


def delta(x: np.ndarray, kind: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(lower, higher) for background cells x, 2^32 <= x < 2^62, by kind:
    0  (x, x + 1)
    1  (x|1, (x|1) + 2^32 - 1): the high half rises by one, the low half falls by one
    2  (2^63 - 1, 2^63): the order flips when compared as signed
    3  (0, 2^64 - 1)."""
    x, kind = np.asarray(x, np.uint64), np.asarray(kind)
    odd = x | np.uint64(1)
    lo = np.select([kind == 0, kind == 1, kind == 2], [x, odd, np.uint64(2**63 - 1)], np.uint64(0)).astype(np.uint64)
    hi = np.select([kind == 0, kind == 1, kind == 2], [x + np.uint64(1), odd + np.uint64(2**32 - 1), np.uint64(2**63)],
                   np.uint64(U64_MAX)).astype(np.uint64)
    return lo, hi


def kind_of(lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """The kind a (lower, higher) cell pair was built with, -1 for none: read
    back from the values, so the table test does not trust the generator."""
    lo, hi = np.asarray(lo, np.uint64), np.asarray(hi, np.uint64)
    d = hi - lo
    return np.select([(lo == 0) & (hi == np.uint64(U64_MAX)), (lo == np.uint64(2**63 - 1)) & (hi == np.uint64(2**63)),
                      d == np.uint64(1), (d == np.uint64(2**32 - 1)) & ((lo & np.uint64(1)) == 1)], [3, 2, 0, 1], -1)


def _background(rng, pairs: int, nodes: int) -> np.ndarray:
    return rng.integers(2**32, 2**62, size=(pairs, nodes), dtype=np.uint64)


def _plant(a, b, x, p, col, kind, a_higher) -> None:
    """Cell (p, col): the higher value of `kind` on a's side where a_higher, on b's otherwise."""
    lo, hi = delta(x[p, col], kind)
    a[p, col] = np.where(a_higher, hi, lo)
    b[p, col] = np.where(a_higher, lo, hi)


# ---------------------------------------------------------------- single-witness population
def partners(nodes: int) -> np.ndarray:
    """[3, nodes]: the column that carries b > a when column k carries a > b:
    k ^ 1 (the same 16-byte vector), k + nodes/2 (the other half of the row)
    and k + 1; (k + 1) % nodes wherever one of them is k itself or past the row."""
    k = np.arange(nodes)
    nxt = (k + 1) % nodes
    same_vec = np.where((k ^ 1) < nodes, k ^ 1, nxt)
    half = (k + nodes // 2) % nodes
    return np.stack([same_vec, np.where(half == k, nxt, half), nxt])


def witness_slots(nodes: int) -> int:
    """Pair positions to cover: every sub-row of a wave-load x every u of the
    largest unroll for the vector widths, 64 for generic shapes, 8 for long rows."""
    if nodes in VCLOCK_VECTOR_NODES:
        return 64 // (nodes // 2) * 32
    return 64 if nodes <= 128 else 8


def witness_pairs(nodes: int, slots: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """(a, b) uint64 [pairs, nodes].  The background is a == b, random in
    [2^32, 2^62); every pair's class hangs on one column (two for CONCURRENT).
    Blocks, each `nodes * slots` pairs, pair k * slots + s of a block having
    its witness at column k and index % slots == s, its delta kind (k + s) % 4:
      BEFORE      b > a at k only
      AFTER       a > b at k only
      CONCURRENT  a > b at k, b > a at partners(nodes)[j][k], j = 0, 1, 2   (nodes > 1)
      near miss   a > b at k, b = a + 1 everywhere else: CONCURRENT           (nodes > 1)
      isolated    EQUAL, but every third pair a single-column BEFORE / AFTER,
                  each column once on either side
    The isolated block is padded with EQUAL pairs until pairs % 4 == 3, so the
    last wave-load of a vector kernel is ragged."""
    assert nodes >= 1 and slots >= KINDS
    per = nodes * slots
    k, s = np.divmod(np.arange(per), slots)
    kind = (k + s) % KINDS
    n_conc = 4 if nodes > 1 else 0
    iso = 3 * 2 * nodes
    iso += (3 - ((2 + n_conc) * per + iso)) % 4
    pairs = (2 + n_conc) * per + iso
    rng = np.random.default_rng(seed)
    x = _background(rng, pairs, nodes)
    a, b = x.copy(), x.copy()
    p = np.arange(per)
    _plant(a, b, x, p, k, kind, False)                                    # BEFORE
    _plant(a, b, x, per + p, k, kind, True)                               # AFTER
    for j in range(n_conc - 1):                                           # CONCURRENT
        q = (2 + j) * per + p
        _plant(a, b, x, q, k, kind, True)
        _plant(a, b, x, q, partners(nodes)[j][k], (kind + 1) % KINDS, False)
    if n_conc:                                                            # near miss
        q = 5 * per + p
        b[q] = a[q] + np.uint64(1)
        _plant(a, b, x, q, k, kind, True)
    w = np.arange(2 * nodes)                                              # isolated
    _plant(a, b, x, (2 + n_conc) * per + 3 * w, w % nodes, (w + w // nodes) % KINDS, w >= nodes)
    assert (2 + n_conc) * per % slots == 0 and pairs % 4 == 3
    return a, b


# ---------------------------------------------------------------- dense random-class population
def dense_pairs(nodes: int, pairs: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """Every pair's class drawn uniformly from the four (three at nodes = 1),
    its witness at a seeded random column (CONCURRENT: a second, different
    one), its delta kind random; the background random, so no pair is a copy
    of the pair one sweep, or any other distance, before it."""
    rng = np.random.default_rng(seed)
    x = _background(rng, pairs, nodes)
    a, b = x.copy(), x.copy()
    cls = rng.integers(0, 4 if nodes > 1 else 3, pairs)
    col = rng.integers(0, nodes, pairs)
    col2 = (col + rng.integers(1, max(nodes, 2), pairs)) % nodes
    kind, kind2 = rng.integers(0, KINDS, pairs), rng.integers(0, KINDS, pairs)
    p = np.nonzero(cls != EQUAL)[0]
    _plant(a, b, x, p, col[p], kind[p], cls[p] != BEFORE)                 # AFTER and CONCURRENT: a > b at col
    p = np.nonzero(cls == CONCURRENT)[0]
    _plant(a, b, x, p, col2[p], kind2[p], False)
    return a, b
