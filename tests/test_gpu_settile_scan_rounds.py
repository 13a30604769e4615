"""GPU: the second and third round of the one-workgroup tile scan that the
set-state ops share (k_tile_scan, csrc/settile.hpp).

The scan takes rounds of ``settile.scan_round`` tiles (16384 in the product
build; the diagnostic build also has rounds of 1024) and carries two things
from round to round: the open run's state and the output offset.  Every state
here has 2049 tiles of T items -- two full rounds of 1024 and a third of one
tile -- and puts the run whose decision crosses tiles exactly where a round
ends: in tile 1023, the last of round 0, and tile 1024, the first of round 1.
The spanning cases copy one tag from tile 1023 across all of round 1 into tile
2048, so the state passes through a round that holds no run end.  At 16384 the
same states run in one round on the product build.

Every expectation is the numpy restatement or the oracle merge that the op's
own test file uses; the written output and the count-only call are compared
bit for bit, the outputs being views inside canary buffers."""
import numpy as np
import pytest
import torch

from causal_util import ref_causal
from crdt_amd.engine import TupleSet, as_u64, u64_tensor
from knobs import set_knob
from test_gpu_set_compact import ref_compact
from test_gpu_set_delta import ref_delta
from test_gpu_set_digest import buckets, canon
from test_gpu_set_read import ref_elements

pytestmark = [pytest.mark.gpu, pytest.mark.diag]

T = 2048                       # items per tile
TILES = 2049
N = TILES * T                  # 2 * 1024 * 2048 + 2048
E = 1024 * T                   # the first item of tile 1024 = of round 1 at rounds of 1024
E2 = 2048 * T                  # the first item of tile 2048 = of round 2
G = 64                         # canary elements each side of an output view
CANARY = 0x5a
FIELDS = ("key", "ts", "rep", "tomb")
ROUNDS = [16384, 1024]


@pytest.fixture(params=ROUNDS)
def rounds(request, eng):
    try:
        set_knob("settile.scan_round", request.param)
        yield request.param
    finally:
        set_knob("settile.scan_round", 16384)


def _ordinary(n=N):
    """n single-tuple keys 10 i with distinct tags, every third tombstoned."""
    i = np.arange(n, dtype=np.uint64)
    return 10 * i, 1000 + i, (i % 5).astype(np.uint32), (i % 3 == 0).astype(np.uint8)


def _one_key(t, lo, hi):
    t[0][lo:hi] = 10 * lo
    t[2][lo:hi] = 0


def _one_tag(t, lo, hi):
    _one_key(t, lo, hi)
    t[1][lo:hi] = 1000 + lo


def _sides(t, side):
    """The two operands whose stable merged order is t: items with side 0 / 1."""
    return tuple(np.ascontiguousarray(x[side == 0]) for x in t), tuple(np.ascontiguousarray(x[side == 1]) for x in t)


def _alternate():
    side = (np.arange(N) & 1).astype(np.uint8)
    return side


# ---- outputs inside canary buffers
class Guarded:
    def __init__(self, n, dtype, dev):
        self.n = n
        self.buf = torch.full((n + 2 * G,), CANARY, dtype=dtype, device=dev)
        self.view = self.buf[G:G + n]

    def check(self, k, what):
        """Nothing but the first k entries of the view was written."""
        b = self.buf.cpu().numpy()
        assert (b[:G] == CANARY).all() and (b[G + k:] == CANARY).all(), f"{what}: a write outside the first {k} outputs"
        return b[G:G + k]


class GuardedTuples:
    def __init__(self, n, dev):
        self.f = [Guarded(n, d, dev) for d in (torch.int64, torch.int64, torch.int32, torch.uint8)]
        self.view = TupleSet(*(g.view for g in self.f))

    def check(self, k, what):
        got = [g.check(k, f"{what} {name}") for g, name in zip(self.f, FIELDS)]
        return got[0].view(np.uint64), got[1].view(np.uint64), got[2].view(np.uint32), got[3]


def _same(got, exp, what):
    for g, e, f in zip(got, exp, FIELDS):
        np.testing.assert_array_equal(g, e, err_msg=f"{what} {f}")


def _count(c):
    return int(as_u64(c)[0])


# ---- the four ops, each: count-only == written count == the reference, outputs bit for bit
def _elements(eng, t, lww, what):
    exp = ref_elements(*t, lww)
    Td = TupleSet.from_numpy(*t, eng.device)
    out = Guarded(N, torch.int64, eng.device)
    _, cnt = eng.set_elements(Td, lww, out=out.view)
    only = eng.set_cardinality(Td, lww)
    assert _count(only) == len(exp) == _count(cnt), (what, _count(only), _count(cnt), len(exp))
    np.testing.assert_array_equal(out.check(len(exp), what).view(np.uint64), exp, err_msg=what)
    assert eng.device_status(clear=True) == 0
    return exp


def _compact(eng, t, lww, cut, what):
    exp = ref_compact(t, lww, cut)
    Td, Cd = TupleSet.from_numpy(*t, eng.device), u64_tensor(cut, eng.device)
    out, src = GuardedTuples(N, eng.device), Guarded(N, torch.int64, eng.device)
    _, _, cnt = eng.set_compact(Td, lww, Cd, out=out.view, src=src.view)
    only = eng.set_compact_count(Td, lww, Cd)
    k = len(exp[0])
    assert _count(only) == k == _count(cnt), (what, _count(only), _count(cnt), k)
    _same(out.check(k, what), exp, what)
    s = src.check(k, what + " src")
    for f in range(3):                                   # the source carries the output's tag, and is its first copy
        np.testing.assert_array_equal(t[f][s], exp[f], err_msg=f"{what} src -> {FIELDS[f]}")
    first = np.ones(N, bool)
    first[1:] = (t[0][1:] != t[0][:-1]) | (t[1][1:] != t[1][:-1]) | (t[2][1:] != t[2][:-1])
    assert first[s].all(), what + ": a source index that is not its tag's first copy"
    assert eng.device_status(clear=True) == 0
    return exp


def _delta(eng, src, dst, lww, what):
    exp = ref_delta(src, dst, lww)
    S, D = TupleSet.from_numpy(*src, eng.device), TupleSet.from_numpy(*dst, eng.device)
    out = GuardedTuples(len(src[0]), eng.device)
    _, cnt = eng.set_delta(S, D, lww, out=out.view)
    only = eng.set_delta_count(S, D, lww)
    k = len(exp[0])
    assert _count(only) == k == _count(cnt), (what, _count(only), _count(cnt), k)
    _same(out.check(k, what), exp, what)
    assert eng.device_status(clear=True) == 0
    return exp


def _causal(eng, a, ca, b, cb, what):
    exp, esrc, _, _ = ref_causal(a, ca, b, cb)
    A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
    Ca = None if ca is None else u64_tensor(ca, eng.device)
    Cb = None if cb is None else u64_tensor(cb, eng.device)
    out, src = GuardedTuples(N, eng.device), Guarded(N, torch.int64, eng.device)
    _, _, _, cnt = eng.causal_merge(A, Ca, B, Cb, out=out.view, src=src.view)
    only = eng.causal_merge_count(A, Ca, B, Cb)
    k = len(exp[0])
    assert _count(only) == k == _count(cnt), (what, _count(only), _count(cnt), k)
    _same(out.check(k, what), exp, what)
    np.testing.assert_array_equal(src.check(k, what + " src"), esrc, err_msg=what + " src")
    assert eng.device_status(clear=True) == 0
    return exp, esrc


def _has_tag(exp, key, ts):
    i = np.searchsorted(exp[0], np.uint64(key))
    return i < len(exp[0]) and exp[0][i] == key and exp[1][i] == ts


COVER = np.full(5, 1000 + E + 10, np.uint64)   # a context that covers the tags of items 0 .. E + 10, the special ones among them


# ---- 1. a run that ends in tile 1024, decided by a copy in tile 1023
@pytest.mark.parametrize("live_before", [True, False])
def test_elements_key_run_ends_in_round_1(eng, rounds, live_before):
    """Key 10 (E - 2) holds four tags, two each side of the round edge.  Its
    tags in tile 1024 are dead, so the tile alone says "not a member": with a
    live tag in tile 1023 the carry turns the key on.  Otherwise its second tag
    has a dead copy in tile 1023 and a live one in tile 1024: the tile alone
    says "member", the carry turns it off."""
    t = _ordinary()
    _one_key(t, E - 2, E + 2)
    if live_before:
        t[3][E - 2:E + 2] = [0, 1, 1, 1]
    else:
        t[1][E] = t[1][E - 1]
        t[3][E - 2:E + 2] = [1, 1, 0, 1]
    exp = _elements(eng, t, False, f"elements, live_before={live_before}")
    assert (np.uint64(10 * (E - 2)) in exp) == live_before


@pytest.mark.parametrize("tombs,stable", [((1, 0), True), ((1, 0), False), ((0, 0), True)])
def test_compact_tag_run_ends_in_round_1(eng, rounds, tombs, stable):
    """One tag with a copy in tile 1023 and one in tile 1024, under a cut: the
    copy in tile 1023 makes it dead, so it is dropped when stable and kept with
    tomb 1 when not; with both copies live it is kept with tomb 0."""
    t = _ordinary()
    _one_tag(t, E - 1, E + 1)
    t[3][E - 1:E + 1] = tombs
    cut = np.full(5, 1000 + E + (10 if stable else -10), np.uint64)
    exp = _compact(eng, t, False, cut, f"compact, tombs={tombs}, stable={stable}")
    i = np.searchsorted(exp[0], np.uint64(10 * (E - 1)))
    kept = i < len(exp[0]) and exp[0][i] == 10 * (E - 1)
    assert kept == (not (tombs[0] and stable))
    if kept:
        assert exp[3][i] == tombs[0]


@pytest.mark.parametrize("tomb_d,tomb_s", [(0, 0), (1, 1), (0, 1)])
def test_delta_tag_run_ends_in_round_1(eng, rounds, tomb_d, tomb_s):
    """Merged item E - 1 is dst's copy of a tag, item E src's: tile 1024 alone
    sees no dst copy and ships the tag; under the carry it ships only with
    tomb_s = 1 and tomb_d = 0."""
    t = _ordinary()
    side = _alternate()
    _one_tag(t, E - 1, E + 1)
    side[E - 1], side[E] = 0, 1
    t[3][E - 1], t[3][E] = tomb_d, tomb_s
    dst, src = _sides(t, side)
    assert len(src[0]) + len(dst[0]) == N
    exp = _delta(eng, src, dst, False, f"delta, tomb_d={tomb_d}, tomb_s={tomb_s}")
    assert _has_tag(exp, 10 * (E - 1), 1000 + E - 1) == (tomb_s == 1 and tomb_d == 0)


@pytest.mark.parametrize("tomb_a,tomb_b,cover", [(0, 0, True), (0, 1, False), (1, 0, True)])
def test_causal_tag_run_ends_in_round_1(eng, rounds, tomb_a, tomb_b, cover):
    """Merged item E - 1 is a's copy of a tag, item E b's.  (0, 0) under
    covering contexts: tile 1024 alone sees a tag present in b alone and
    covered by a, dropped; with a's copy it is present in both and kept, from
    a.  (0, 1) under empty contexts: alone it is absent; a's live copy keeps
    it.  (1, 0) under covering contexts: dropped either way."""
    t = _ordinary()
    t[3][:] = 0                                          # (plain tags: present, kept or dropped by the contexts alone)
    side = _alternate()
    _one_tag(t, E - 1, E + 1)
    side[E - 1], side[E] = 0, 1
    t[3][E - 1], t[3][E] = tomb_a, tomb_b
    a, b = _sides(t, side)
    ctx = COVER if cover else None
    exp, esrc = _causal(eng, a, ctx, b, ctx, f"causal, tombs=({tomb_a}, {tomb_b}), cover={cover}")
    kept = _has_tag(exp, 10 * (E - 1), 1000 + E - 1)
    assert kept == (tomb_a == 0 and (tomb_b == 0 or not cover))
    if kept:
        i = np.searchsorted(exp[0], np.uint64(10 * (E - 1)))
        assert esrc[i] == int(np.count_nonzero(side[:E - 1] == 0))      # a's copy


# ---- 2. one tag from tile 1023 across all of round 1 into tile 2048
LO, HI = E - 5, E2 + 7


def _spanning():
    t = _ordinary()
    _one_tag(t, LO, HI)
    t[3][LO:HI] = 0
    t[3][LO] = 1                                         # the only tombstone: the first copy, in round 0
    return t


def test_one_tag_spans_round_1_elements_and_compact(eng, rounds):
    t = _spanning()
    exp = _elements(eng, t, False, "elements, spanning tag")
    assert np.uint64(10 * LO) not in exp                 # tile 2048 alone says "member"
    for stable in (True, False):
        cut = np.full(5, 1000 + LO + (1 if stable else -1), np.uint64)
        exp = _compact(eng, t, False, cut, f"compact, spanning tag, stable={stable}")
        assert _has_tag(exp, 10 * LO, 1000 + LO) == (not stable)


def test_one_tag_spans_round_1_delta_and_causal(eng, rounds):
    t = _spanning()
    side = _alternate()
    side[LO:HI - 1], side[HI - 1] = 0, 1                 # every copy dst's / a's but the last
    a, b = _sides(t, side)
    # delta: src's copy is dead; tile 2048 alone sees live dst copies and ships it, dst's first copy is dead too
    t[3][HI - 1] = 1
    dst, src = _sides(t, side)
    exp = _delta(eng, src, dst, False, "delta, spanning tag")
    assert not _has_tag(exp, 10 * LO, 1000 + LO)
    # causal: tile 2048 alone sees the tag present in both; a's first copy is dead, and a's context covers it
    exp, _ = _causal(eng, a, COVER, b, COVER, "causal, spanning tag")
    assert not _has_tag(exp, 10 * LO, 1000 + LO)
    exp, esrc = _causal(eng, a, None, b, None, "causal, spanning tag, empty contexts")
    i = np.searchsorted(exp[0], np.uint64(10 * LO))
    assert _has_tag(exp, 10 * LO, 1000 + LO) and esrc[i] == -1 - (len(b[0]) - 1 - int(np.count_nonzero(side[HI:] == 1)))


# ---- 3. the offset base alone: no records, outputs in every round
def test_base_carry_lww_compact(eng, rounds):
    t = _ordinary()
    _one_key(t, E - 3, E + 3)                            # a key over the round edge: its last tuple wins
    cut = np.full(5, 1000 + N // 3, np.uint64)
    exp = _compact(eng, t, True, cut, "compact, LWW")
    assert 0 < len(exp[0]) < N - 5


def test_base_carry_select(eng, rounds):
    t = _ordinary()
    sp = (10 * np.arange(1, 64, dtype=np.uint64)) * np.uint64(N // 64)
    flags = (np.arange(64) % 3 != 1).astype(np.uint8)
    Td = TupleSet.from_numpy(*t, eng.device)
    Sd, Fd = u64_tensor(sp, eng.device), torch.from_numpy(flags).to(eng.device)
    for lww in (True, False):
        m = canon(t, lww)
        keep = flags[buckets(sp, m[0])] != 0
        exp = tuple(np.ascontiguousarray(x[keep]) for x in m)
        what = f"select, lww={lww}"
        out, src = GuardedTuples(N, eng.device), Guarded(N, torch.int64, eng.device)
        _, _, cnt = eng.set_select(Td, lww, Sd, Fd, out=out.view, src=src.view)
        only = eng.set_select_count(Td, lww, Sd, Fd)
        k = len(exp[0])
        assert 0 < k < N and _count(only) == k == _count(cnt), (what, _count(only), _count(cnt), k)
        _same(out.check(k, what), exp, what)
        np.testing.assert_array_equal(src.check(k, what + " src"), np.flatnonzero(np.isin(t[0], exp[0])), err_msg=what)
    assert eng.device_status(clear=True) == 0
