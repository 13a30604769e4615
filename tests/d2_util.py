"""Plan shapes, host predicates, offset views and the case table of the
sort / D2 view tests (tests/test_d2_case_table.py, test_gpu_sort_views.py,
test_gpu_d2_views.py).

csrc/sort.hip picks its kernels from the plan (k_sort_plan: which form a
call takes) and from two host predicates on the input pointers (d2_vec: the
vector upsweep and everything behind it; launch_minmax's `aligned`: the
vector minmax).  The functions here restate those rules in plain numpy, so
the case table below can name, for every GPU case, the form and the
predicate class it is meant to reach -- and tests/test_d2_case_table.py
checks that it does, without a GPU.  test_gpu_d2_views.py's drift guard
compares plan_shape with the device's own plan.
"""
from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass
from functools import lru_cache
from typing import Tuple

import numpy as np

U64_MAX = 2**64 - 1
U32_MAX = 2**32 - 1

Shape = namedtuple("Shape", "bk bt br b0 W words s0 P tl tw")


# ---------------------------------------------------------------- k_sort_plan
def _concat(a, b):
    if b is None:
        return a
    return tuple(np.concatenate([x, y]) for x, y in zip(a, b))


def plan_shape(a, b, mode, lww_table=1, or_table=1, key_only=None, widen=False) -> Shape:
    """k_sort_plan for the exact plan of two host sides (key, ts, rep, tomb).

    mode "lww" / "orset": the fused merge (a side bit: b0 = 2; key_only
    defaults to 1 / 2, the product's).  mode "sort": crdt_tuples_sort of `a`
    alone (b None; b0 = 1, the whole composite sorted).  widen: the margin
    of crdt_set_merge_plan(widen=1), 1/256 of each field's span."""
    assert mode in ("lww", "orset", "sort")
    if key_only is None:
        key_only = {"lww": 1, "orset": 2, "sort": 0}[mode]
    if mode == "sort":
        assert b is None or len(b[0]) == 0
        lww_table = or_table = 0
    else:
        lww_table = lww_table if mode == "lww" else 0
        or_table = or_table if mode == "orset" else 0
    key, ts, rep, _ = _concat(a, b)
    n_all = len(key)
    assert n_all > 0, "k_sort_plan is not launched for an empty call"

    def rng(x, cap):
        lo, hi = int(x.min()), int(x.max())
        if widen:
            pad = (hi - lo) >> 8
            lo = lo - pad if lo > pad else 0
            hi = hi + pad if cap - hi > pad else cap
        return hi - lo

    bk = rng(key, U64_MAX).bit_length()
    bt = rng(ts, U64_MAX).bit_length()
    br = rng(rep, U32_MAX).bit_length()
    b0 = 1 if mode == "sort" else 2
    W = bk + bt + br + b0
    words = (W + 63) // 64
    keep = bk
    if key_only == 2:
        keep += (8 - bk % 8) % 8 + 8
    s0 = W - keep if (key_only and words == 1 and W > keep) else 0
    P = (W - s0 + 7) // 8 if W - s0 else 1
    tl = tw = 0
    kb = b0 + br + bt
    if key_only == 1 and lww_table and words == 1 and bk >= 12:
        if bk <= 8 + 15 and kb + 1 <= 32:
            tw = 4
        elif bk <= 8 + 14 and kb + 1 <= 64:
            tw = 8
        if tw:
            tl, s0, P = bk - 8, W - 8, 1
    if or_table and key_only != 1 and words == 1 and 16 <= bk <= 16 + 9 and n_all <= (1280 << (bk - 9)):
        tw, tl, s0, P = 4, 9, W - 16, 2
    return Shape(bk, bt, br, b0, W, words, s0, P, tl, tw)


def form_of(shape: Shape, mode: str) -> str:
    """The kernel chain family d2_body (or crdt_tuples_sort) takes for this plan."""
    if shape.tw and mode == "lww":
        return "lww_table_u32" if shape.tw == 4 else "lww_table_u64"
    if shape.tw and mode == "orset":
        return "or_chunks"
    return f"radix_{shape.words}w"


# byte offsets inside crdt_set_plan (PlanBlob, then its SortPlan h): sort.hip
# static_asserts them next to PlanBlob
_BLOB_H = 24
_PLAN_U32 = {"bk": 24, "bt": 28, "br": 32, "W": 36, "P": 40, "words": 44, "b0": 48, "s0": 52, "tl": 56, "tw": 60}


def blob_shape(plan) -> Tuple[int, int, int, Shape]:
    """(mode, na, nb, Shape) read out of a crdt_set_plan."""
    raw = np.frombuffer(bytes(plan), dtype=np.uint8)
    u32 = lambda off: int(raw[off:off + 4].view(np.uint32)[0])
    u64 = lambda off: int(raw[off:off + 8].view(np.uint64)[0])
    return u32(4), u64(8), u64(16), Shape(**{f: u32(_BLOB_H + o) for f, o in _PLAN_U32.items()})


# ---------------------------------------------------------------- host predicates
def _ptrs(t):
    return t.key.data_ptr(), t.ts.data_ptr(), t.rep.data_ptr(), t.tomb.data_ptr()


def is_vec(A, B, vec_up: int = 1) -> bool:
    """sort.hip d2_vec: key / ts 16-, rep 8-, tomb 2-byte aligned on every
    non-empty side, an even len(A), and sort.vec_up on."""
    def ok(t):
        if len(t) == 0:
            return True
        k, s, r, b = _ptrs(t)
        return not (((k | s) & 15) | (r & 7) | (b & 1))
    return ok(A) and ok(B) and len(A) % 2 == 0 and bool(vec_up)


def minmax_vec(A, B=None) -> bool:
    """launch_minmax's `aligned`: key, ts and rep of every non-empty side 16-byte aligned."""
    def ok(t):
        if t is None or len(t) == 0:
            return True
        k, s, r, _ = _ptrs(t)
        return ((k | s | r) & 15) == 0
    return ok(A) and ok(B)


@dataclass
class _FakeField:
    addr: int

    def data_ptr(self) -> int:
        return self.addr


@dataclass
class FakeSet:
    """A TupleSet's pointers and length without a device: fields of a view
    `offs` elements into 256-byte-aligned buffers (what view_set builds)."""
    key: _FakeField
    ts: _FakeField
    rep: _FakeField
    tomb: _FakeField
    n: int

    def __len__(self) -> int:
        return self.n


def _offs4(off):
    offs = (off,) * 4 if isinstance(off, int) else tuple(off)
    assert len(offs) == 4 and all(o >= 0 for o in offs)
    return offs


def fake_set(n: int, off, base: int = 0x7F0000000000) -> FakeSet:
    assert base % 256 == 0
    o = _offs4(off)
    return FakeSet(*(_FakeField(base + i * 0x100000 + o[i] * w) for i, w in enumerate((8, 8, 4, 1))), n)


# ---------------------------------------------------------------- views in canary buffers
_NP = (np.uint64, np.uint64, np.uint32, np.uint8)
FIELDS = ("key", "ts", "rep", "tomb")


def _canary(f: int, m: int, on: bool) -> np.ndarray:
    """Extreme in every field: a read outside a view moves the plan's ranges
    (and may surface in the output), a store outside a view changes one."""
    if not on:
        return np.zeros(m, _NP[f])
    if f == 3:
        return np.ones(m, np.uint8)
    hi = U64_MAX if f < 2 else U32_MAX
    return np.where(np.arange(m) % 2 == 0, 0, hi).astype(_NP[f])


@dataclass
class Backing:
    bufs: tuple          # the four device buffers
    host: tuple          # what they held when built
    offs: tuple          # the view's first element, per field
    n: int               # the view's length


def view_set(eng, host_tuple, off, pad: int = 8, canary: bool = True):
    """A TupleSet whose fields are views: field f starts off[f] (or `off`)
    elements into its own device buffer and `pad` canary elements follow
    it; everything outside the view is the canary pattern (zeros with
    canary=False).  Returns (set, Backing)."""
    import torch
    from crdt_amd.engine import TupleSet
    offs = _offs4(off)
    n = len(host_tuple[0])
    bufs, host, views = [], [], []
    for f in range(4):
        h = _canary(f, offs[f] + n + pad, canary)
        h[offs[f]:offs[f] + n] = np.ascontiguousarray(host_tuple[f]).astype(_NP[f], copy=False)
        t = torch.from_numpy(h.view(np.int64 if f < 2 else np.int32 if f == 2 else np.uint8).copy()).to(eng.device)
        assert t.data_ptr() % 256 == 0, "test setup: a fresh device buffer is not 256-byte aligned"
        bufs.append(t)
        host.append(h)
        views.append(t[offs[f]:offs[f] + n])
        assert n == 0 or views[-1].data_ptr() == t.data_ptr() + offs[f] * h.itemsize, "test setup: the view's address"
    return TupleSet(*views), Backing(tuple(bufs), tuple(host), offs, n)


def out_set(eng, cap: int, off, pad: int = 8):
    """An output view of `cap` tuples inside canary buffers (zeros inside)."""
    return view_set(eng, tuple(np.zeros(cap, t) for t in _NP), off, pad)


def assert_canaries_intact(b: Backing, whole: bool = False, what: str = "") -> None:
    """Everything outside the view still holds what view_set put there;
    whole=True: the view too (an input must come back unchanged)."""
    for f in range(4):
        got = b.bufs[f].cpu().numpy().view(_NP[f])
        exp = b.host[f]
        lo, hi = b.offs[f], b.offs[f] + b.n
        np.testing.assert_array_equal(got[:lo], exp[:lo], err_msg=f"{what} {FIELDS[f]}: canaries before the view")
        np.testing.assert_array_equal(got[hi:], exp[hi:], err_msg=f"{what} {FIELDS[f]}: canaries after the view")
        if whole:
            np.testing.assert_array_equal(got[lo:hi], exp[lo:hi], err_msg=f"{what} {FIELDS[f]}: the view itself")


def np_sorted(t):
    o = np.lexsort((t[3], t[2], t[1], t[0]))
    return tuple(np.ascontiguousarray(x[o]) for x in t)


def cut(t, n: int):
    return tuple(np.ascontiguousarray(x[:n]) for x in t)


# ---------------------------------------------------------------- D2 inputs, one generator per form
def _fields(rng, m, kbits, tbits, rbits):
    """m tuples whose key / ts / rep offsets span exactly their widths (the
    extremes sit at indices 0 and 1, so every prefix of >= 2 keeps them)."""
    key = rng.integers(0, 2**kbits, m, dtype=np.uint64)
    ts = rng.integers(0, 2**tbits, m, dtype=np.uint64)
    rep = rng.integers(0, 2**rbits, m, dtype=np.uint64)
    for x, b in ((key, kbits), (ts, tbits), (rep, rbits)):
        x[0], x[1] = 0, 2**b - 1
    return key, ts, rep.astype(np.uint32), rng.integers(0, 2, m, dtype=np.uint8)


def _cross(a, b, lo, cnt):
    """b[lo : lo + cnt) repeats a's tags with tombs of its own."""
    for f in range(3):
        b[f][lo:lo + cnt] = a[f][lo:lo + cnt]
    b[3][lo:lo + cnt] = 1 - a[3][lo:lo + cnt]
    b[3][lo:lo + cnt:3] = a[3][lo:lo + cnt:3]


def _shift(t, kbits, tbits):
    """Offsets far from 0 (as test_unsorted_lww_key_tables): the plan works on
    offsets from the minima, the decode adds them back."""
    dk = np.uint64(2**61) if kbits < 60 else np.uint64(0)
    dt = np.uint64(12345) if tbits < 60 else np.uint64(0)
    return t[0] + dk, t[1] + dt, t[2], t[3]


def _gen_bits(seed, na, nb, kbits, tbits, rbits, long_runs=False):
    rng = np.random.default_rng(seed)
    a, b = _fields(rng, na, kbits, tbits, rbits), _fields(rng, nb, kbits, tbits, rbits)
    _cross(a, b, 10, 500)
    b[0][600:700] = b[0][700:800]                            # key ties within a side
    if long_runs:
        # keys whose tuples share every sorted bit of the OR-Set's key-and-digit
        # sort (the key and ts >> 6): runs of 33..100 tuples, over
        # or_run_dedup's 32-tuple limit, duplicate tags and both sides in each
        lo = 1000
        for i, ln in enumerate((33, 40, 64, 70, 100, 35)):
            for s in (a, b):
                s[0][lo:lo + ln] = 3 + 11 * i
                s[1][lo:lo + ln] = (5 + i) * 64 + rng.integers(0, 4, ln, dtype=np.uint64)
                s[2][lo:lo + ln] = rng.integers(0, 3, ln, dtype=np.uint64).astype(np.uint32)
            lo += ln
    pa, pb = rng.permutation(np.arange(2, na)), rng.permutation(np.arange(2, nb))
    a = tuple(np.concatenate([x[:2], x[pa]]) for x in a)
    b = tuple(np.concatenate([x[:2], x[pb]]) for x in b)
    return _shift(a, kbits, tbits), _shift(b, kbits, tbits)


# generator -> (kbits, tbits, rbits, na (even), nb, long_runs); the odd-na
# case drops A's last tuple, the (0, nb - 1) case B's
GENS = {
    "dense17": (17, 20, 6, 12_000, 11_003, False),
    "dense13": (13, 20, 6, 6_000, 5_501, False),
    "dense16_wide_ts": (16, 40, 6, 8_000, 7_003, False),
    "keys10": (10, 20, 6, 6_000, 5_501, True),
    "two_words": (40, 30, 10, 8_000, 7_997, False),
    "three_words": (64, 64, 32, 8_000, 7_997, False),
}
# the form each (generator, mode) is named for
FORMS = {
    ("dense17", "lww"): "lww_table_u32", ("dense17", "orset"): "or_chunks",
    ("dense13", "lww"): "lww_table_u32", ("dense13", "orset"): "radix_1w",
    ("dense16_wide_ts", "lww"): "lww_table_u64", ("dense16_wide_ts", "orset"): "or_chunks",
    ("keys10", "lww"): "radix_1w", ("keys10", "orset"): "radix_1w",
    ("two_words", "lww"): "radix_2w", ("two_words", "orset"): "radix_2w",
    ("three_words", "lww"): "radix_3w", ("three_words", "orset"): "radix_3w",
}
MODE_NAMES = ("lww", "orset")
DENSE = ("dense17", "dense16_wide_ts")                      # both modes on a dense-key form


@lru_cache(maxsize=None)
def gen_sides(gen: str):
    kb, tb, rb, na, nb, long_runs = GENS[gen]
    assert na % 2 == 0
    return _gen_bits(1000 + sorted(GENS).index(gen), na, nb, kb, tb, rb, long_runs)


@dataclass(frozen=True)
class D2Case:
    """One D2 merge: which prefix of the generator's sides, where the views
    start, and the predicate class the case is named for."""
    gen: str
    mode: str
    cls: str
    na: int
    nb: int
    off_a: object          # an element offset, or one per field (key, ts, rep, tomb)
    off_b: object
    off_out: int
    vec: bool
    mm_vec: bool

    @property
    def id(self) -> str:
        return f"{self.gen}-{self.mode}-{self.cls}"

    @property
    def form(self) -> str:
        return FORMS[self.gen, self.mode]

    def sides(self):
        a, b = gen_sides(self.gen)
        return cut(a, self.na), cut(b, self.nb)


def _d2_cases():
    out = []
    for gen, (_, _, _, na, nb, _) in GENS.items():
        for mode in MODE_NAMES:
            def add(cls, na_, nb_, oa, ob, oo, vec, mm):
                out.append(D2Case(gen, mode, cls, na_, nb_, oa, ob, oo, vec, mm))
            # the alignment classes
            add("vec_0_0", na, nb, 0, 0, 1, True, True)
            add("vec_4_4", na, nb, 4, 4, 3, True, True)
            add("vec_mm_scalar_2_2", na, nb, 2, 2, 1, True, False)
            add("odd_na_0_0", na - 1, nb, 0, 0, 3, False, True)
            add("off_1_0", na, nb, 1, 0, 1, False, False)
            add("off_0_1", na, nb, 0, 1, 3, False, False)      # only B misaligned: p.in2
            add("off_3_5", na, nb, 3, 5, 1, False, False)
            # an empty side beside a misaligned one
            add("empty_b_off_1", na, 0, 1, 0, 3, False, False)
            add("empty_a_off_1_nb_odd" if nb % 2 else "empty_a_off_1_nb_even", 0, nb, 0, 1, 1, False, False)
            add("empty_a_off_3_nb_even" if nb % 2 else "empty_a_off_3_nb_odd", 0, nb - 1, 0, 3, 3, False, False)
            if gen in DENSE:
                # exactly one clause of d2_vec fails: even na, every other field aligned.
                # (key, ts, rep, tomb) element offsets; rep off by 1 is 4- but not 8-byte aligned
                add("only_tomb_off", na, nb, (0, 0, 0, 1), 0, 3, False, True)
                add("only_rep_off", na, nb, 0, (0, 0, 1, 0), 1, False, False)
                add("only_ts_off", na, nb, (0, 1, 0, 0), 0, 3, False, False)
    return out


D2_CASES = _d2_cases()
# the sort-knob variants: one aligned even-na and one offset case per mode
D2_KNOB_CASES = [c for m in MODE_NAMES for cls in ("vec_0_0", "off_3_5")
                 for c in D2_CASES if (c.gen, c.mode, c.cls) == ("dense17", m, cls)]


# ---------------------------------------------------------------- planned calls (plan made on aligned inputs)
PLANNED_GENS = ("dense17", "two_words")
PLANNED_OFFS = (1, 3)


@dataclass(frozen=True)
class PlannedCase:
    gen: str
    mode: str
    odd: bool

    @property
    def id(self) -> str:
        return f"{self.gen}-{self.mode}-{'odd' if self.odd else 'even'}_na"

    @property
    def form(self) -> str:
        return FORMS[self.gen, self.mode]

    def sides(self):
        a, b = gen_sides(self.gen)
        return cut(a, GENS[self.gen][3] - (1 if self.odd else 0)), b

    def fresh_sides(self):
        """A permutation of the data with fresh tombs: inside the plan."""
        a, b = self.sides()
        rng = np.random.default_rng(7 + self.odd)
        pa, pb = rng.permutation(len(a[0])), rng.permutation(len(b[0]))
        return ((a[0][pa], a[1][pa], a[2][pa], rng.integers(0, 2, len(pa), dtype=np.uint8)),
                (b[0][pb], b[1][pb], b[2][pb], rng.integers(0, 2, len(pb), dtype=np.uint8)))


PLANNED_CASES = [PlannedCase(g, m, odd) for g in PLANNED_GENS for m in MODE_NAMES for odd in (False, True)]


# ---------------------------------------------------------------- crdt_tuples_sort on views
SORT_OUT_OFF = {1: 2, 2: 3, 3: 4, 4: 1}                     # out's view: another offset than in's
SORT_NS = (1, 2, 4095, 4097, 12_289)


@lru_cache(maxsize=None)
def sort_input(kind: str, n: int):
    """1w: config D's fields (as test_sort_config_d_shape); 2w / 3w: the field
    widths of test_sort_two_words / test_sort_wide_fields_three_words."""
    if kind == "1w":
        from crdt_amd import synth
        return synth.set_tuples(11 + n, 1, n, max(1, n // 2))
    rng = np.random.default_rng(40 + n)
    kb, tb, rb = (40, 30, 10) if kind == "2w" else (64, 64, 32)
    key = rng.integers(0, 2**kb, n, dtype=np.uint64)
    key[:100] = key[100:200]                                 # key ties
    ts = rng.integers(0, 2**tb, n, dtype=np.uint64)
    ts[0], ts[1] = 0, 2**tb - 1
    rep = rng.integers(0, 2**rb, n, dtype=np.uint64).astype(np.uint32)
    return key, ts, rep, rng.integers(0, 2, n, dtype=np.uint8)


@dataclass(frozen=True)
class SortCase:
    kind: str
    n: int
    off: int

    @property
    def id(self) -> str:
        return f"{self.kind}-n{self.n}-off{self.off}"

    @property
    def form(self) -> str:
        return f"radix_{self.kind}"

    @property
    def off_out(self) -> int:
        return SORT_OUT_OFF[self.off]

    @property
    def mm_vec(self) -> bool:
        return self.off == 4          # 1, 3: key / ts off 16 bytes; 2: rep at 8 modulo 16

    def tuples(self):
        return sort_input(self.kind, self.n)


SORT_CASES = ([SortCase("1w", n, off) for off in (1, 2, 3, 4) for n in SORT_NS] +
              [SortCase(k, 12_289, off) for off in (1, 2, 3, 4) for k in ("2w", "3w")])
SORT_KNOB_CASE = SortCase("1w", 12_289, 3)
