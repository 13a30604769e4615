"""GPU: range digests of a sorted LWW / OR-Set state, their diff and the
selection of the differing key ranges (crdt_set_digest, crdt_set_digest_diff,
crdt_set_select; csrc/setdigest.hip), and crdt_amd.reconcile on top of them.

The expectation is independent of the kernels: the oracle's merge with an
empty side (the canonical tuples), numpy's searchsorted(side="right") for the
bucket, synth.splitmix64 for the tuple hash and np.add.at for the wrapping
sums.  The selection's source indices are checked against the engine's own
merge_src(t, {}) under the same numpy bucket filter.  A tile of the kernels is
T tuples, a wave takes 512 of them, a mask word 64: the hand-built cases put
tag and key runs, and splitters, on those edges."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from crdt_amd import _lib, reconcile, synth
from crdt_amd.engine import TupleSet, as_u64, u64_tensor
from oracle import oracle

pytestmark = pytest.mark.gpu

T = 2048                       # tuples per tile
WAVE = 512                     # tuples per wave
WORD = 64                      # tuples per mask word
DEV_RANGE = 2                  # CRDT_DEV_RANGE
E_INVAL, E_RANGE = -1, -6
M64 = 2**64 - 1
U64 = np.uint64
FIELDS = ("key", "ts", "rep", "tomb")
DT = (np.uint64, np.uint64, np.uint32, np.uint8)


# ---- the semantics, in numpy over the oracle's merge with an empty side
def _empty():
    return tuple(np.zeros(0, d) for d in DT)


def _tup(key, ts, rep, tomb):
    return tuple(np.ascontiguousarray(np.asarray(x, dtype=d)) for x, d in zip((key, ts, rep, tomb), DT))


def _merge(lww):
    return oracle.lww_merge if lww else oracle.orset_merge


def canon(t, lww):
    return tuple(np.ascontiguousarray(x) for x in _merge(lww)(t, _empty()))


def tuple_hash(key, ts, rep, tomb):
    sm = synth.splitmix64
    return sm(sm(sm(key) ^ ts.astype(U64)) ^ ((rep.astype(U64) << U64(1)) | tomb.astype(U64)))


def buckets(sp, key):
    return np.searchsorted(np.asarray(sp, U64), key, side="right")


def ref_digest(t, lww, sp):
    key, ts, rep, tomb = canon(t, lww)
    b = buckets(sp, key)
    h, c = np.zeros(len(sp) + 1, U64), np.zeros(len(sp) + 1, U64)
    with np.errstate(over="ignore"):
        np.add.at(h, b, tuple_hash(key, ts, rep, tomb))
        np.add.at(c, b, U64(1))
    return h, c


def _sort(t):
    return synth.sort_tuples_np(*t)


@functools.lru_cache(maxsize=16)
def _side(side, n, ks):
    return tuple(np.ascontiguousarray(x) for x in _sort(synth.set_tuples(2024, side, n, ks)))


@functools.lru_cache(maxsize=16)
def _both(n, ks):
    """Both sides concatenated: a sorted state that holds duplicate tags."""
    a, b = _side(0, n, ks), _side(1, n, ks)
    return tuple(np.ascontiguousarray(x) for x in _sort(tuple(np.concatenate([x, y]) for x, y in zip(a, b))))


def _splitters(t, m):
    """reconcile.key_splitters in numpy: every ceil(n / (m + 1))-th key."""
    n = len(t[0])
    if n == 0 or m == 0:
        return np.zeros(m, U64)
    step = -(-n // (m + 1))
    return np.ascontiguousarray(t[0][np.minimum(np.arange(1, m + 1) * step, n - 1)])


def _fill(n, key0, seed):
    """n distinct single-copy tags, keys key0 .., about a third dead, reps 0 .. 3."""
    rng = np.random.default_rng(seed)
    return _tup(key0 + np.arange(n, dtype=np.uint64), rng.integers(1, 100, n), rng.integers(0, 4, n),
                rng.integers(0, 3, n) == 0)


def _cat(*ts):
    return tuple(np.ascontiguousarray(np.concatenate([t[f] for t in ts])) for f in range(4))


def _cut(t, n):
    return tuple(np.ascontiguousarray(x[:n]) for x in t)


def _assert_tuples(got, exp, msg):
    for g, e, f in zip(got, exp, FIELDS):
        np.testing.assert_array_equal(g, e, err_msg=f"{msg} {f}")


def _dev(eng, v):
    return u64_tensor(np.array([v], np.uint64), eng.device)


def _sp_dev(eng, sp):
    return None if len(sp) == 0 else u64_tensor(np.asarray(sp, U64), eng.device)


def _digest(eng, t, lww, sp, Td=None, n_dev=None, Sd=None):
    Td = TupleSet.from_numpy(*t, eng.device) if Td is None else Td
    Sd = _sp_dev(eng, sp) if Sd is None else Sd
    h, c = eng.set_digest(Td, lww, Sd, n_dev=n_dev)
    return as_u64(h).copy(), as_u64(c).copy()


def _check(eng, t, sp, Td=None, n_dev=None, Sd=None):
    """Both modes: the GPU digest of t over sp == the expectation, bit for bit,
    no device flag.  `t` is what the call must read.  Returns {lww: (hash, count)}."""
    res = {}
    for lww in (True, False):
        eh, ec = ref_digest(t, lww, sp)
        gh, gc = _digest(eng, t, lww, sp, Td=Td, n_dev=n_dev, Sd=Sd)
        np.testing.assert_array_equal(gc, ec, err_msg=f"lww={lww} count")
        np.testing.assert_array_equal(gh, eh, err_msg=f"lww={lww} hash")
        res[lww] = (gh, gc)
    assert eng.device_status(clear=True) == 0
    return res


# ---- 0. the reference itself, as run on the CPU
def test_reference_properties():
    t = _side(0, 5000, 700)
    doubled = tuple(np.repeat(x, 2) for x in t)
    for lww, total in ((True, 700), (False, 5000)):
        h, c = ref_digest(t, lww, _splitters(t, 63))
        assert int(c.sum()) == total
        h2, c2 = ref_digest(doubled, lww, _splitters(t, 63))
        np.testing.assert_array_equal(h, h2)
        np.testing.assert_array_equal(c, c2)


# ---- 1. randomised states
@pytest.mark.parametrize("n,ks", [(5000, 700), (20000, 3000)])
def test_random_states(eng, n, ks):
    for t in (_side(0, n, ks), _both(n, ks)):
        Td = TupleSet.from_numpy(*t, eng.device)
        for m in (0, 1, 63, 699):
            _check(eng, t, _splitters(t, m), Td=Td)
        many = np.arange(ks + 300, dtype=U64)                # more splitters than distinct keys
        res = _check(eng, t, many, Td=Td)
        assert (res[False][1] == 0).sum() >= 300


@pytest.mark.parametrize("lww", [True, False])
def test_invariances(eng, lww):
    t = _both(5000, 700)
    sp = _splitters(t, 63)
    h, c = _digest(eng, t, lww, sp)
    assert c.sum() == len(canon(t, lww)[0]) < len(t[0])
    hm, cm = _digest(eng, canon(t, lww), lww, sp)            # digest(t) == digest(merge(t, {}))
    np.testing.assert_array_equal(h, hm)
    np.testing.assert_array_equal(c, cm)
    hd, cd = _digest(eng, tuple(np.repeat(x, 2) for x in t), lww, sp)   # ... == digest(t, every tuple doubled)
    np.testing.assert_array_equal(h, hd)
    np.testing.assert_array_equal(c, cd)
    h0, c0 = _digest(eng, t, lww, np.zeros(0, U64))          # the buckets sum to the m = 0 digest
    with np.errstate(over="ignore"):
        assert h0[0] == np.add.reduce(h) and c0[0] == c.sum()
    assert eng.device_status(clear=True) == 0


# ---- 2. sizes around the word, wave and tile edges
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097])
def test_sizes(eng, n):
    t = _cut(_both(5000, 700), n)
    _check(eng, t, _splitters(t, 63))
    _check(eng, t, np.zeros(0, U64))


@pytest.mark.parametrize("edge", [WORD, WAVE, T, 2 * T])
@pytest.mark.parametrize("where", ["first", "last"])
def test_tag_across_an_edge(eng, edge, where):
    """7 copies of one tag from edge - 3 on, its only tombstoned copy the first
    (before the edge) or the last (after it)."""
    start, copies = edge - 3, 7
    tomb = np.zeros(copies, np.uint8)
    tomb[0 if where == "first" else -1] = 1
    K = 10**6
    run = _tup(np.full(copies, K), np.full(copies, 50), np.full(copies, 2), tomb)
    t = _cat(_fill(start, 0, 1), run, _fill(100, K + 1, 2))
    sp = np.array([start // 2, K, K + 1, K + 50], U64)       # the tag alone in bucket 2
    res = _check(eng, t, sp)
    one = lambda dead: tuple_hash(np.array([K], U64), np.array([50], U64), np.array([2], np.uint32),
                                  np.array([dead], np.uint8))[0]
    assert res[False][1][2] == 1 and res[False][0][2] == one(1)              # OR-Set: the OR
    assert res[True][1][2] == 1 and res[True][0][2] == one(where == "first")  # LWW: the first copy's


@pytest.mark.parametrize("where", [0, 4999, None])
def test_tag_copied_5000_times(eng, where):
    """One tag over more than two tiles; the tombstone in copy 0, in the last copy, in none."""
    n = 5000
    tomb = np.zeros(n, np.uint8)
    if where is not None:
        tomb[where] = 1
    K = 10**6
    run = _tup(np.full(n, K), np.full(n, 9), np.full(n, 1), tomb)
    sp = np.array([5, K, K + 1], U64)
    for pre in (0, 777):                                     # the run from a tile's start, and from inside one
        t = _cat(_fill(pre, 0, 1), run, _fill(37, K + 1, 3))
        res = _check(eng, t, sp)
        assert res[False][1][2] == 1 and res[True][1][2] == 1
        h = lambda dead: tuple_hash(np.array([K], U64), np.array([9], U64), np.array([1], np.uint32),
                                    np.array([dead], np.uint8))[0]
        assert res[False][0][2] == h(where is not None)
        assert res[True][0][2] == h(where == 0)


@pytest.mark.parametrize("first_dead", [True, False])
def test_lww_winner_copies_across_a_tile_edge(eng, first_dead):
    """One key whose run spans a tile edge; its winner tag has 3 copies before
    the edge and 3 after, and the first copy's tomb differs from the others'."""
    K, n, c = 10**6, 300, 6
    ts = np.arange(1, n + 1, dtype=np.uint64)
    run = _tup(np.full(n, K), ts, np.full(n, 1), np.arange(n) % 3 == 0)
    ct = np.array([1 if first_dead else 0] + [0 if first_dead else 1] * (c - 1), np.uint8)
    win = _tup(np.full(c, K), np.full(c, n + 1), np.full(c, 1), ct)
    pre = _fill(T - n - 3, 0, 5)
    t = _cat(pre, run, win, _fill(50, K + 1, 6))
    assert len(pre[0]) + n == T - 3
    sp = np.array([K, K + 1], U64)
    res = _check(eng, t, sp)
    h = tuple_hash(np.array([K], U64), np.array([n + 1], U64), np.array([1], np.uint32),
                   np.array([first_dead], np.uint8))[0]
    assert res[True][1][1] == 1 and res[True][0][1] == h


# ---- 3. extreme keys and splitters
def test_extreme_keys_and_splitters(eng):
    t = _cat(_tup([0, 0, 1], [1, 2, 1], [0, 0, 0], [0, 1, 0]), _fill(3000, 10, 4),
             _tup([M64 - 1, M64, M64], [5, 5, 6], [1, 1, 1], [1, 0, 0]))
    for sp in ([0], [M64], [0, 0], [M64, M64], [0, 0, 1, 1, 2**63, 2**63, M64 - 1, M64, M64], [1, M64 - 1],
               [2**63 - 1, 2**63]):
        _check(eng, t, np.array(sp, U64))
    res = _check(eng, t, np.array([0, M64], U64))            # key 0 is in bucket 1, key 2^64 - 1 in bucket 2
    assert res[False][1].tolist() == [0, len(t[0]) - 2, 2] and res[True][1].tolist() == [0, len(t[0]) - 3, 1]


def test_splitter_equal_to_a_tiles_first_key(eng):
    """splitters[j] <= key: the key equal to a splitter belongs to the bucket above."""
    t = _fill(3 * T + 100, 0, 9)                             # key i at index i
    for sp in ([T], [T, 2 * T], [T - 1, T, T + 1], [WAVE, T, T + WAVE], [WORD, 3 * T]):
        res = _check(eng, t, np.array(sp, U64))
        c = res[False][1]
        bounds = [0] + sp + [3 * T + 100]
        assert c.tolist() == [bounds[i + 1] - bounds[i] for i in range(len(sp) + 1)]


# ---- 4. offset views
@pytest.mark.parametrize("off", [1, 3])
def test_offset_views(eng, off):
    t = _both(5000, 700)
    F = TupleSet.from_numpy(*t, eng.device)
    sub = tuple(np.ascontiguousarray(x[off:]) for x in t)
    sp = _splitters(sub, 63)
    Sfull = u64_tensor(np.concatenate([np.full(off, M64, U64), sp]), eng.device)
    Td = TupleSet(F.key[off:], F.ts[off:], F.rep[off:], F.tomb[off:])
    _check(eng, sub, sp, Td=Td, Sd=Sfull[off:])
    hh = torch.zeros(len(sp) + 1 + off, dtype=torch.int64, device=eng.device)   # ... and of the outputs
    cc = torch.zeros(len(sp) + 1 + off, dtype=torch.int64, device=eng.device)
    flags = torch.ones(len(sp) + 1 + off, dtype=torch.uint8, device=eng.device)
    for lww in (True, False):
        eng.set_digest(Td, lww, Sfull[off:], hash_out=hh[off:], count_out=cc[off:])
        eh, ec = ref_digest(sub, lww, sp)
        np.testing.assert_array_equal(as_u64(hh)[off:], eh)
        np.testing.assert_array_equal(as_u64(cc)[off:], ec)
        assert not as_u64(hh)[:off].any() and not as_u64(cc)[:off].any()
        _check_select(eng, sub, lww, sp, np.ones(len(sp) + 1, np.uint8), Td=Td, Sd=Sfull[off:], Fd=flags[off:])
    assert eng.device_status(clear=True) == 0


# ---- 5. the tuple count on the device
def test_device_count(eng):
    t = _side(0, 5000, 700)
    Td = TupleSet.from_numpy(*t, eng.device)
    for n in (5000, 3000, 2049, 2048, 2047, 1, 0):           # a count at or below the capacity reads that prefix
        sub = _cut(t, n)
        _check(eng, sub, _splitters(t, 63), Td=Td, n_dev=_dev(eng, n))


@pytest.mark.parametrize("lww", [True, False])
def test_chained_off_a_merge(eng, lww):
    a, b = _side(0, 5000, 700), _side(1, 5000, 700)
    A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
    cap = len(a[0]) + len(b[0])
    mo = TupleSet.empty(cap, eng.device)
    mo.key.fill_(0)                                          # sentinels past the merge's count: they must not count
    mo.ts.fill_(0)
    mo.rep.fill_(0)
    mo.tomb.fill_(1)
    mo, cnt = (eng.lww_merge if lww else eng.orset_merge)(A, B, out=mo, trim=False)
    m = _merge(lww)(a, b)
    sp = _splitters(m, 63)
    h, c = eng.set_digest(mo, lww, _sp_dev(eng, sp), n_dev=cnt)
    assert 0 < int(as_u64(cnt)[0]) < cap
    eh, ec = ref_digest(m, lww, sp)
    np.testing.assert_array_equal(as_u64(h), eh)
    np.testing.assert_array_equal(as_u64(c), ec)
    flags = np.arange(64) % 2 == 0
    _check_select(eng, m, lww, sp, flags.astype(np.uint8), Td=mo, n_dev=cnt)
    assert eng.device_status(clear=True) == 0


@pytest.mark.parametrize("bad", [5001, M64])
def test_device_count_out_of_range(eng, bad):
    t = _side(0, 5000, 700)
    Td = TupleSet.from_numpy(*t, eng.device)
    sp = _splitters(t, 63)
    Sd = _sp_dev(eng, sp)
    flags = torch.ones(64, dtype=torch.uint8, device=eng.device)
    assert eng.device_status(clear=True) == 0
    for lww in (True, False):
        h, c = eng.set_digest(Td, lww, Sd, n_dev=_dev(eng, bad))
        assert (as_u64(h) == M64).all() and (as_u64(c) == M64).all() and len(as_u64(h)) == 64
        assert eng.device_status(clear=True) & DEV_RANGE
        assert eng.device_status(clear=True) == 0            # cleared
        good = eng.set_digest(Td, lww, Sd)                   # a poisoned digest flags everything
        f, nd = eng.digest_diff((h, c), good)
        assert f.cpu().numpy().all() and int(nd.item()) == 64
        f, nd = eng.digest_diff((h, c), (h, c))              # ... even against another poisoned one
        assert f.cpu().numpy().all() and int(nd.item()) == 64
        out = TupleSet.empty(5000, eng.device)
        src = torch.full((5000,), 0x5a5a, dtype=torch.int64, device=eng.device)
        for x in (out.key, out.ts, out.rep, out.tomb):
            x.fill_(0x5a)
        _, _, cnt = eng.set_select(Td, lww, Sd, flags, n_dev=_dev(eng, bad), out=out, src=src)
        assert as_u64(cnt)[0] == M64
        assert eng.device_status(clear=True) & DEV_RANGE
        assert all(bool((x == 0x5a).all()) for x in (out.key, out.ts, out.rep, out.tomb))
        assert bool((src == 0x5a5a).all())
        only = eng.set_select_count(Td, lww, Sd, flags, n_dev=_dev(eng, bad))
        assert as_u64(only)[0] == M64
        assert eng.device_status(clear=True) & DEV_RANGE
    _check(eng, t, sp, Td=Td)                                # the next calls are exact


# ---- 6. witness: one field of one tuple changes exactly its bucket's hash
def test_witness(eng):
    t = _fill(3 * T + 100, 0, 11)                            # single-copy tags, key i at index i
    sp = np.arange(100, 3 * T + 100, 100, dtype=U64)         # bucket b = keys [100 b, 100 b + 100)
    for at in (T, 2 * T - 1, 777):                           # a tile's first tuple, a tile's last, an ordinary one
        b = at // 100
        base = {lww: ref_digest(t, lww, sp) for lww in (True, False)}
        got0 = _check(eng, t, sp)
        for field in ("tomb", "ts", "rep"):
            f = FIELDS.index(field)
            mod = [x.copy() for x in t]
            mod[f][at] = (1 - mod[f][at]) if field == "tomb" else mod[f][at] + 1
            mod = tuple(mod)
            got = _check(eng, mod, sp)
            for lww in (True, False):
                eh, ec = ref_digest(mod, lww, sp)
                for h0, c0, h1, c1 in ((base[lww][0], base[lww][1], eh, ec), got0[lww] + got[lww]):
                    diff = np.flatnonzero(h0 != h1)
                    assert diff.tolist() == [b], (field, at, lww)
                    np.testing.assert_array_equal(c0, c1)
        gone = tuple(np.delete(x, at) for x in t)            # the tuple removed: that bucket's count, too
        got = _check(eng, gone, sp)
        for lww in (True, False):
            assert np.flatnonzero(got0[lww][0] != got[lww][0]).tolist() == [b]
            assert np.flatnonzero(got0[lww][1] != got[lww][1]).tolist() == [b]
            assert got[lww][1][b] == got0[lww][1][b] - 1


# ---- 7. select
def _ref_select(eng, t, lww, sp, flags):
    """canon(t) and the engine's merge_src(t, {}) indices under the numpy bucket filter."""
    m = canon(t, lww)
    keep = np.asarray(flags)[buckets(sp, m[0])] != 0
    Td = TupleSet.from_numpy(*t, eng.device)
    out, cnt, src = (eng.lww_merge_src if lww else eng.orset_merge_src)(Td, TupleSet.empty(0, eng.device))
    k = int(cnt.item())
    assert k == len(m[0])
    _assert_tuples(tuple(x[:k] for x in out.to_numpy()), m, "merge_src(t, {}) against the oracle")
    return tuple(np.ascontiguousarray(x[keep]) for x in m), src.cpu().numpy()[:k][keep]


def _check_select(eng, t, lww, sp, flags, Td=None, n_dev=None, Sd=None, Fd=None):
    Td = TupleSet.from_numpy(*t, eng.device) if Td is None else Td
    Sd = _sp_dev(eng, sp) if Sd is None else Sd
    Fd = torch.from_numpy(np.ascontiguousarray(flags, dtype=np.uint8)).to(eng.device) if Fd is None else Fd
    exp, esrc = _ref_select(eng, t, lww, sp, flags)
    out, src, cnt = eng.set_select(Td, lww, Sd, Fd, n_dev=n_dev, with_src=True)
    k = int(as_u64(cnt)[0])
    assert k == len(exp[0]), f"lww={lww}: count {k}, expected {len(exp[0])}"
    got = tuple(x[:k] for x in out.to_numpy())
    _assert_tuples(got, exp, f"lww={lww}")
    np.testing.assert_array_equal(src.cpu().numpy()[:k], esrc, err_msg=f"lww={lww} src")
    out2, cnt2 = eng.set_select(Td, lww, Sd, Fd, n_dev=n_dev)              # without the source indices
    assert int(as_u64(cnt2)[0]) == k
    _assert_tuples(tuple(x[:k] for x in out2.to_numpy()), exp, f"lww={lww} (no src)")
    only = eng.set_select_count(Td, lww, Sd, Fd, n_dev=n_dev)
    assert int(as_u64(only)[0]) == k, f"lww={lww}: count-only"
    assert eng.device_status(clear=True) == 0
    return got


def _patterns(m):
    z = np.zeros(m + 1, np.uint8)
    first, last = z.copy(), z.copy()
    first[0], last[m] = 1, 7                                 # (any nonzero byte is a set flag)
    return {"none": z, "all": np.ones(m + 1, np.uint8), "alternating": (np.arange(m + 1) % 2).astype(np.uint8),
            "first": first, "last": last}


@pytest.mark.parametrize("pattern", ["none", "all", "alternating", "first", "last"])
@pytest.mark.parametrize("m", [0, 63, 699])
def test_select(eng, pattern, m):
    for t in (_both(5000, 700), _cut(_both(5000, 700), T + 1)):
        sp = _splitters(t, m)
        flags = _patterns(m)[pattern]
        for lww in (True, False):
            got = _check_select(eng, t, lww, sp, flags)
            if pattern == "none":
                assert len(got[0]) == 0
            if pattern == "all":                             # merge(t, {}) bit for bit
                _assert_tuples(got, canon(t, lww), "all flags")


@pytest.mark.parametrize("n", [0, 1, 64, 65, 513, 2047, 2049, 4097])
def test_select_sizes(eng, n):
    t = _cut(_both(5000, 700), n)
    sp = _splitters(t, 15)
    for lww in (True, False):
        _check_select(eng, t, lww, sp, (np.arange(16) % 3 != 1).astype(np.uint8))


def test_select_long_runs(eng):
    """A tag over more than two tiles and a key run over a tile edge, selected and not."""
    K = 10**6
    n = 5000
    tomb = np.zeros(n, np.uint8)
    tomb[0] = 1
    run = _tup(np.full(n, K), np.full(n, 9), np.full(n, 1), tomb)
    keyrun = _tup(np.full(300, K + 5), np.arange(1, 301), np.full(300, 1), np.arange(300) % 3 == 0)
    t = _cat(_fill(777, 0, 1), run, keyrun, _fill(37, K + 6, 3))
    sp = np.array([5, K, K + 1, K + 5], U64)
    for flags in ([1, 1, 1, 1, 1], [0, 0, 1, 0, 0], [1, 1, 0, 1, 0], [0, 0, 0, 0, 1]):
        for lww in (True, False):
            _check_select(eng, t, lww, sp, np.array(flags, np.uint8))


def test_map_select(eng):
    t = _both(5000, 700)
    n = len(t[0])
    val = torch.arange(n, dtype=torch.int64, device=eng.device) * 3 + 1
    Td = TupleSet.from_numpy(*t, eng.device)
    sp = _splitters(t, 63)
    flags = (np.arange(64) % 2).astype(np.uint8)
    Fd = torch.from_numpy(flags).to(eng.device)
    for lww in (True, False):
        exp, esrc = _ref_select(eng, t, lww, sp, flags)
        out, oval, cnt = eng.map_select(Td, val, lww, _sp_dev(eng, sp), Fd)
        k = int(as_u64(cnt)[0])
        _assert_tuples(tuple(x[:k] for x in out.to_numpy()), exp, f"lww={lww}")
        np.testing.assert_array_equal(oval.cpu().numpy()[:k], esrc.astype(np.int64) * 3 + 1)
    assert eng.device_status(clear=True) == 0


# ---- 8. diff on hand-made arrays
def test_digest_diff(eng):
    ha = np.array([1, 2, 3, 4, 5, 6, M64, 0], U64)
    ca = np.array([1, 1, 2, 0, M64, M64, 3, 0], U64)
    hb = np.array([1, 9, 3, 4, 5, 6, M64, 0], U64)
    cb = np.array([1, 1, 3, 0, 7, M64, 3, 0], U64)
    exp = np.array([0, 1, 1, 0, 1, 1, 0, 0], np.uint8)       # hash; count; equal; ~0 on one side; on both; hash ~0 is
    d = lambda h, c: (u64_tensor(h, eng.device), u64_tensor(c, eng.device))    # an ordinary value
    f, nd = eng.digest_diff(d(ha, ca), d(hb, cb))
    np.testing.assert_array_equal(f.cpu().numpy(), exp)
    assert int(nd.item()) == 4
    f, nd = eng.digest_diff(d(hb, cb), d(ha, ca))
    np.testing.assert_array_equal(f.cpu().numpy(), exp)
    n = 1000                                                 # more than one workgroup
    rng = np.random.default_rng(3)
    h, c = rng.integers(0, 2**63, n).astype(U64), rng.integers(0, 100, n).astype(U64)
    h2, c2 = h.copy(), c.copy()
    at = rng.choice(n, 37, replace=False)
    h2[at[:20]] += U64(1)
    c2[at[20:]] += U64(1)
    f, nd = eng.digest_diff(d(h, c), d(h2, c2))
    assert np.flatnonzero(f.cpu().numpy()).tolist() == sorted(at.tolist()) and int(nd.item()) == 37
    f, nd = eng.digest_diff(d(h, c), d(h, c))
    assert not f.cpu().numpy().any() and int(nd.item()) == 0
    nd.fill_(77)                                             # no buckets: the count store alone
    eng._bind()
    _lib.call("crdt_set_digest_diff", eng.ctx, None, None, None, None, 0, None, nd.data_ptr(), ctx=eng.ctx)
    assert int(nd.item()) == 0
    assert eng.device_status(clear=True) == 0


# ---- 9. host-side errors: refused before any launch
def test_host_errors(eng):
    t = _side(0, 5000, 700)
    n = 1000
    Td = TupleSet.from_numpy(*(x[:n] for x in t), eng.device)
    O = TupleSet.empty(n, eng.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=eng.device)
    src = torch.zeros(n, dtype=torch.int64, device=eng.device)
    Sd = u64_tensor(_splitters(t, 63), eng.device)
    hh = torch.zeros(64, dtype=torch.int64, device=eng.device)
    cc = torch.zeros(64, dtype=torch.int64, device=eng.device)
    Fd = torch.ones(64, dtype=torch.uint8, device=eng.device)
    ct, co, cp, sp_, spl = Td.c(), O.c(), cnt.data_ptr(), src.data_ptr(), Sd.data_ptr()
    ref = lambda x: C.byref(x) if x is not None else None

    def status(fn, *args):
        eng._bind()
        with pytest.raises(_lib.CrdtError) as ei:
            _lib.call(fn, eng.ctx, *args, ctx=eng.ctx)
        return ei.value.status

    def dig(mode, tt, h=hh.data_ptr(), c=cc.data_ptr(), s=spl, m=63, n_max=n):
        return status("crdt_set_digest", mode, ref(tt), n_max, None, s, m, h, c)

    def sel(mode, tt, o, s_out, count, s=spl, m=63, f=Fd.data_ptr(), n_max=n):
        return status("crdt_set_select", mode, ref(tt), n_max, None, s, m, f, ref(o), s_out, count)

    def tup(x, **kw):
        f = {"key": x.key.data_ptr(), "ts": x.ts.data_ptr(), "rep": x.rep.data_ptr(), "tomb": x.tomb.data_ptr()}
        f.update(kw)
        return _lib.crdt_tuples(f["key"], f["ts"], f["rep"], f["tomb"])

    assert dig(0, None) == E_INVAL and dig(1, ct, h=None) == E_INVAL and dig(1, ct, c=None) == E_INVAL
    assert dig(2, ct) == E_INVAL and dig(-1, ct) == E_INVAL
    assert dig(0, ct, s=None) == E_INVAL                     # splitters NULL with m > 0
    assert dig(0, ct, s=spl + 4) == E_INVAL and dig(0, ct, h=hh.data_ptr() + 4) == E_INVAL
    assert dig(0, ct, h=cc.data_ptr()) == E_INVAL            # the outputs overlap each other, t, the splitters
    assert dig(0, ct, h=Td.key.data_ptr()) == E_INVAL and dig(1, ct, c=spl) == E_INVAL
    assert dig(0, ct, n_max=2**62) == E_RANGE and dig(1, ct, m=2**24) == E_RANGE
    assert sel(0, None, None, None, cp) == E_INVAL and sel(1, ct, co, None, None) == E_INVAL
    assert sel(2, ct, None, None, cp) == E_INVAL
    assert sel(0, ct, None, None, cp, f=None) == E_INVAL and sel(0, ct, None, None, cp, s=None) == E_INVAL
    assert sel(0, ct, None, sp_, cp) == E_INVAL              # source indices without out
    assert sel(1, ct, co, sp_ + 4, cp) == E_INVAL
    assert sel(0, ct, ct, None, cp) == E_INVAL               # out overlapping t, the splitters, the flags, src
    assert sel(1, ct, tup(O, key=spl), None, cp) == E_INVAL
    assert sel(1, ct, tup(O, tomb=Fd.data_ptr() + 63), None, cp) == E_INVAL
    assert sel(1, ct, tup(O, key=sp_), sp_, cp) == E_INVAL
    assert sel(0, ct, co, Td.ts.data_ptr(), cp) == E_INVAL
    assert sel(0, ct, None, None, cp, n_max=2**62) == E_RANGE and sel(1, ct, None, None, cp, m=2**24) == E_RANGE
    for f, by in (("key", 4), ("ts", 4), ("rep", 2)):        # natural alignment of every operand
        for mode in (0, 1):
            assert dig(mode, tup(Td, **{f: getattr(Td, f).data_ptr() + by})) == E_INVAL
            assert sel(mode, tup(Td, **{f: getattr(Td, f).data_ptr() + by}), None, None, cp) == E_INVAL
            assert sel(mode, ct, tup(O, **{f: getattr(O, f).data_ptr() + by}), None, cp) == E_INVAL
    for f in FIELDS:                                         # NULL field pointers with n_max > 0
        assert dig(0, tup(Td, **{f: None})) == E_INVAL
        assert sel(1, ct, tup(O, **{f: None}), None, cp) == E_INVAL
    h8 = hh.data_ptr()
    assert status("crdt_set_digest_diff", h8, h8, h8, h8, 64, Fd.data_ptr(), None) == E_INVAL
    assert status("crdt_set_digest_diff", None, h8, h8, h8, 64, Fd.data_ptr(), cp) == E_INVAL
    assert status("crdt_set_digest_diff", h8, h8, h8, h8, 64, None, cp) == E_INVAL
    assert status("crdt_set_digest_diff", h8, h8, h8, h8 + 4, 64, Fd.data_ptr(), cp) == E_INVAL
    assert status("crdt_set_digest_diff", h8, h8, h8, h8, 64, Fd.data_ptr(), h8 + 8) == E_INVAL
    assert status("crdt_set_digest_diff", h8, h8, h8, h8, 2**24 + 1, Fd.data_ptr(), cp) == E_RANGE
    assert int(cnt.item()) == 0 and eng.device_status(clear=True) == 0
    eng._bind()                                              # n_max == 0: zeroed outputs / the count store, nothing read
    hh.fill_(5)
    cc.fill_(5)
    cnt.fill_(77)
    none = _lib.crdt_tuples(None, None, None, None)
    _lib.call("crdt_set_digest", eng.ctx, 0, C.byref(none), 0, None, spl, 63, hh.data_ptr(), cc.data_ptr(), ctx=eng.ctx)
    _lib.call("crdt_set_select", eng.ctx, 1, C.byref(none), 0, None, spl, 63, Fd.data_ptr(), None, None, cp, ctx=eng.ctx)
    assert not hh.any() and not cc.any() and int(cnt.item()) == 0
    _check(eng, _cut(t, n), _splitters(t, 63), Td=Td)


# ---- 10. end to end: one reconciliation round
def _edited(lww):
    """A = a 40000-tuple state with duplicate tags, keys doubled (odd keys are
    free); B = A with one edit in each of four chosen buckets of a 64-bucket
    split, each of which changes the canonical tuples in both modes."""
    a = _both(20000, 3000)
    A = _tup(a[0] * U64(2), a[1], a[2], a[3])
    sp = _splitters(A, 63)
    bk = buckets(sp, A[0])
    assert len(np.unique(bk)) == 64
    where = {"insert": 3, "tombstone": 17, "higher": 40, "remove": 63}
    B = [x.copy() for x in A]
    add = []
    first = lambda b: int(np.flatnonzero(bk == b)[0])
    k = A[0][first(where["insert"])]                         # a key no state holds
    add.append((k + U64(1), 12345, 7, 0))
    # a key whose LWW winner tag has one live copy: that copy is both the tag's first and its only one
    for b in (where["tombstone"], where["remove"]):
        lone = None
        idx = np.flatnonzero(bk == b)
        for i in idx[::-1]:
            last_of_key = i + 1 == len(A[0]) or A[0][i + 1] != A[0][i]
            single = i == 0 or (A[0][i - 1], A[1][i - 1], A[2][i - 1]) != (A[0][i], A[1][i], A[2][i])
            if last_of_key and single and A[3][i] == 0:
                lone = i
                break
        assert lone is not None
        if b == where["tombstone"]:
            B[3][lone] = 1
        else:
            gone = lone
    k = A[0][first(where["higher"])]
    add.append((k, 2**21, 1, 0))
    B = tuple(np.delete(x, gone) for x in B)
    B = _cat(B, _tup(*zip(*add)))
    B = tuple(np.ascontiguousarray(x) for x in _sort(B))
    return A, B, sp, sorted(where.values())


@pytest.mark.parametrize("lww", [True, False])
def test_reconcile_round(eng, lww):
    A, B, sp, edited = _edited(lww)
    Ad, Bd = TupleSet.from_numpy(*A, eng.device), TupleSet.from_numpy(*B, eng.device)
    Sd = reconcile.key_splitters(Ad, 63)
    np.testing.assert_array_equal(as_u64(Sd), sp)
    (ma, ca), (mb, cb), flags, (ship_a, ship_b) = reconcile.reconcile_round(eng, Ad, Bd, lww, Sd)
    f = flags.cpu().numpy()
    assert np.flatnonzero(f).tolist() == edited              # exactly the edited buckets
    for (m, c), (x, y) in (((ma, ca), (A, B)), ((mb, cb), (B, A))):
        exp = _merge(lww)(x, y)
        k = int(as_u64(c)[0])
        assert k == len(exp[0])
        _assert_tuples(tuple(v[:k] for v in m.to_numpy()), exp, "merged")
    for ship, t in ((ship_a, A), (ship_b, B)):               # the reference's tuples in the flagged buckets
        m = canon(t, lww)
        assert int(as_u64(ship)[0]) == int((f[buckets(sp, m[0])] != 0).sum()) > 0
    assert int(as_u64(ship_b)[0]) < len(canon(B, lww)[0]) // 8
    selb, _ = eng.set_select(Bd, lww, Sd, flags, trim=True)
    have = set(zip(*(x.tolist() for x in selb.to_numpy())))
    delta = eng.set_delta(Bd, Ad, lww, trim=True)
    assert len(delta) > 0
    assert all(d in have for d in zip(*(x.tolist() for x in delta.to_numpy())))
    assert eng.device_status(clear=True) == 0
    (ma, ca), (mb, cb), flags, (ship_a, ship_b) = reconcile.reconcile_round(eng, Ad, Ad, lww, Sd)   # in sync
    assert not flags.cpu().numpy().any() and int(ship_a.item()) == 0 and int(ship_b.item()) == 0
    exp = canon(A, lww)
    assert int(ca.item()) == int(cb.item()) == len(exp[0])
    _assert_tuples(tuple(v[:len(exp[0])] for v in ma.to_numpy()), exp, "in sync")
    assert eng.device_status(clear=True) == 0


def test_key_splitters(eng):
    t = _both(5000, 700)
    Td = TupleSet.from_numpy(*t, eng.device)
    for m in (0, 1, 63, 699, 20000):
        np.testing.assert_array_equal(as_u64(reconcile.key_splitters(Td, m)), _splitters(t, m))
    assert reconcile.key_splitters(TupleSet.empty(0, eng.device), 5).tolist() == [0] * 5


# ---- 11. captured in a graph: digest -> diff -> select -> merge after reserve
@pytest.mark.parametrize("lww", [True, False])
def test_graph_capture(eng, lww):
    A, B, sp, edited = _edited(lww)
    Ad, Bd = TupleSet.from_numpy(*A, eng.device), TupleSet.from_numpy(*B, eng.device)
    Sd = u64_tensor(sp, eng.device)
    eng.reserve(64 << 20)
    (ma, ca), _, _, _ = reconcile.reconcile_round(eng, Ad, Bd, lww, Sd)              # eager
    torch.cuda.synchronize()
    exp = _merge(lww)(A, B)
    k = int(as_u64(ca)[0])
    _assert_tuples(tuple(v[:k] for v in ma.to_numpy()), exp, "eager")
    ha, hb = (tuple(torch.zeros(64, dtype=torch.int64, device=eng.device) for _ in range(2)) for _ in range(2))
    flags = torch.zeros(64, dtype=torch.uint8, device=eng.device)
    n_diff, shipped, count = (torch.zeros(1, dtype=torch.int64, device=eng.device) for _ in range(3))
    sel = TupleSet.empty(len(Bd), eng.device)
    out = TupleSet.empty(len(Ad) + len(Bd), eng.device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        eng.set_digest(Ad, lww, Sd, hash_out=ha[0], count_out=ha[1])
        eng.set_digest(Bd, lww, Sd, hash_out=hb[0], count_out=hb[1])
        eng.digest_diff(ha, hb, flags=flags, n_diff=n_diff)
        for x, s in ((sel.key, Bd.key), (sel.ts, Bd.ts), (sel.rep, Bd.rep), (sel.tomb, Bd.tomb)):
            x.copy_(s[-1:].expand(x.shape[0]))               # (reconcile._ship_and_merge's padding)
        eng.set_select(Bd, lww, Sd, flags, out=sel, count=shipped)
        (eng.lww_merge if lww else eng.orset_merge)(Ad, sel, out=out, count=count, trim=False)
    for rep in range(2):
        for x in (out.key, out.ts, out.rep, out.tomb, count, shipped, n_diff, flags, sel.key) + ha + hb:
            x.fill_(0)
        g.replay()
        torch.cuda.synchronize()
        assert np.flatnonzero(flags.cpu().numpy()).tolist() == edited and int(n_diff.item()) == len(edited)
        assert int(as_u64(count)[0]) == k
        _assert_tuples(tuple(v[:k] for v in out.to_numpy()), exp, f"replay {rep}")
    assert eng.device_status(clear=True) == 0
