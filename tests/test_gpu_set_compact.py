"""GPU: tombstone compaction of a sorted LWW / OR-Set state under a
causal-stability cut (crdt_set_compact; csrc/setcompact.hip).

compact(t, cut) = merge(t, {}) without its stable dead tuples; a tag (key, ts,
rep) is stable iff rep < n_cut and ts <= cut[rep], unsigned.  The expectation
has three independent parts: the oracle's merge with an empty side, a numpy
filter over it, and (source indices) the engine's own merge_src(t, {}) under
the same filter.  A tile of the kernels is T tuples, a wave takes 512 of them,
a mask word 64: the hand-built cases put tag and key runs across those edges."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from crdt_amd import _lib, synth
from crdt_amd.engine import TupleSet, as_u64, u64_tensor
from oracle import oracle

pytestmark = pytest.mark.gpu

T = 2048                       # tuples per tile of the compaction kernels
WAVE = 512                     # tuples per wave of the count pass
WORD = 64                      # tuples per mask word
DEV_RANGE = 2                  # CRDT_DEV_RANGE
E_INVAL, E_RANGE = -1, -6
M64 = 2**64 - 1
M32 = 2**32 - 1
FIELDS = ("key", "ts", "rep", "tomb")
DT = (np.uint64, np.uint64, np.uint32, np.uint8)
CUT = np.random.default_rng(7).integers(0, 2**20, 64, dtype=np.uint64)
NOCUT = np.zeros(0, np.uint64)


# ---- the semantics: the oracle's merge with an empty side, then a numpy filter
def _empty():
    return tuple(np.zeros(0, d) for d in DT)


def _tup(key, ts, rep, tomb):
    return tuple(np.ascontiguousarray(np.asarray(x, dtype=d)) for x, d in zip((key, ts, rep, tomb), DT))


def _merge(lww):
    return oracle.lww_merge if lww else oracle.orset_merge


def _keep(m, cut):
    """The filter over a merged state: ~(tomb == 1 & rep < n_cut & ts <= cut[min(rep, n_cut - 1)])."""
    key, ts, rep, tomb = m
    n_cut = len(cut)
    if n_cut == 0:
        return np.ones(len(key), bool)
    c = cut[np.minimum(rep.astype(np.int64), n_cut - 1)]
    return ~((tomb == 1) & (rep.astype(np.int64) < n_cut) & (ts <= c))


def ref_compact(t, lww, cut):
    m = _merge(lww)(t, _empty())
    k = _keep(m, cut)
    return tuple(np.ascontiguousarray(x[k]) for x in m)


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


def _assert_tuples(got, exp, msg):
    for g, e, f in zip(got, exp, FIELDS):
        np.testing.assert_array_equal(g, e, err_msg=f"{msg} {f}")


def _dev(eng, v):
    return u64_tensor(np.array([v], np.uint64), eng.device)


def _cut_dev(eng, cut):
    return None if len(cut) == 0 else u64_tensor(cut, eng.device)


def _ref_src(eng, t, lww, cut):
    """The engine's merge_src(t, {}) indices under the same filter."""
    Td = TupleSet.from_numpy(*t, eng.device)
    out, cnt, src = (eng.lww_merge_src if lww else eng.orset_merge_src)(Td, TupleSet.empty(0, eng.device))
    k = int(cnt.item())
    m = tuple(x[:k] for x in out.to_numpy())
    return src.cpu().numpy()[:k][_keep(m, cut)]


def _check(eng, t, cut, Td=None, n_dev=None, Cd=None, src_ref=True):
    """Both modes: tuples, count (and source indices) == the expectation, the
    count-only call == the full call, no device flag.  `t` is what the call
    must read: all of Td, or its first *n_dev tuples.  Returns {lww: (tuples, src)}."""
    Td = TupleSet.from_numpy(*t, eng.device) if Td is None else Td
    Cd = _cut_dev(eng, cut) if Cd is None else Cd
    res = {}
    for lww in (True, False):
        name = "lww" if lww else "orset"
        exp = ref_compact(t, lww, cut)
        out, src, cnt = eng.set_compact(Td, lww, Cd, n_dev=n_dev, with_src=True)
        k = int(as_u64(cnt)[0])
        assert k == len(exp[0]), f"{name}: count {k}, expected {len(exp[0])}"
        got = tuple(x[:k] for x in out.to_numpy())
        _assert_tuples(got, exp, name)
        s = src.cpu().numpy()[:k]
        # whatever the copy, the source carries the output's tag
        for f in range(3):
            np.testing.assert_array_equal(t[f][s], exp[f], err_msg=f"{name} src -> {FIELDS[f]}")
        if src_ref:
            np.testing.assert_array_equal(s, _ref_src(eng, t, lww, cut), err_msg=f"{name} src")
        out2, cnt2 = eng.set_compact(Td, lww, Cd, n_dev=n_dev)            # without the source indices
        assert int(as_u64(cnt2)[0]) == k
        _assert_tuples(tuple(x[:k] for x in out2.to_numpy()), exp, f"{name} (no src)")
        only = eng.set_compact_count(Td, lww, Cd, n_dev=n_dev)
        assert int(as_u64(only)[0]) == k, f"{name}: count-only"
        assert eng.device_status(clear=True) == 0
        res[lww] = (got, s)
    return res


# ---- 1. randomised states
@pytest.mark.parametrize("n,ks", [(5000, 700), (20000, 3000)])
def test_random_states(eng, n, ks):
    for t in (_side(0, n, ks), _both(n, ks)):
        for lww in (True, False):                            # the case discriminates: a kernel that ignores the
            m = _merge(lww)(t, _empty())                     # cut, or the tomb, cannot pass
            keep = _keep(m, CUT)
            assert (~keep).sum() >= 1 and (keep & (m[3] == 1)).sum() >= 1
        _check(eng, t, CUT)
        _check(eng, t, NOCUT)
    # side 0 as counted on the CPU: (OR-Set dropped, dead kept, LWW dropped, dead kept)
    counted = {(5000, 700): (260, 239, 16, 65), (20000, 3000): (1042, 885, 48, 222)}[(n, ks)]
    got = ()
    for lww in (False, True):
        m = _merge(lww)(_side(0, n, ks), _empty())
        keep = _keep(m, CUT)
        got += (int((~keep).sum()), int((keep & (m[3] == 1)).sum()))
    assert got == counted


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17])
def test_sizes(eng, n):
    t = tuple(np.ascontiguousarray(x[:n]) for x in _both(5000, 700))
    _check(eng, t, CUT)


# ---- 2. one tag copied across a word, a wave and a tile edge
def _fill(n, key0, seed):
    """n distinct single-copy tags, keys key0 .., about a third dead, reps 0 .. 3."""
    rng = np.random.default_rng(seed)
    return _tup(key0 + np.arange(n, dtype=np.uint64), rng.integers(1, 100, n), rng.integers(0, 4, n),
                rng.integers(0, 3, n) == 0)


def _cat(*ts):
    return tuple(np.ascontiguousarray(np.concatenate([t[f] for t in ts])) for f in range(4))


@pytest.mark.parametrize("edge", [WORD, WAVE, T])
@pytest.mark.parametrize("where", ["first", "last", "none"])
@pytest.mark.parametrize("stable", [True, False])
def test_tag_across_an_edge(eng, edge, where, stable):
    """7 copies of one tag from edge - 3 on; its only tombstoned copy before
    the edge, after it, or nowhere."""
    start, copies = edge - 3, 7
    tomb = np.zeros(copies, np.uint8)
    if where != "none":
        tomb[0 if where == "first" else -1] = 1
    K = 10**6
    run = _tup(np.full(copies, K), np.full(copies, 50), np.full(copies, 2), tomb)
    t = _cat(_fill(start, 0, 1), run, _fill(100, K + 1, 2))
    cut = np.array([40, 60, 50 if stable else 49, 10], np.uint64)
    res = _check(eng, t, cut)
    got, src = res[False]
    at = np.flatnonzero(got[0] == K)
    if where != "none" and stable:
        assert len(at) == 0
    else:
        assert len(at) == 1 and got[3][at[0]] == (where != "none")
        assert src[at[0]] == start                           # the first copy, before the edge
    got, src = res[True]
    at = np.flatnonzero(got[0] == K)
    if where == "first" and stable:                          # LWW: the first copy's tomb decides
        assert len(at) == 0
    else:
        assert len(at) == 1 and got[3][at[0]] == (where == "first") and src[at[0]] == start


@pytest.mark.parametrize("where", [0, 2 * T + 5, 5 * T - 1, None])
@pytest.mark.parametrize("stable", [True, False])
def test_tag_spanning_five_tiles(eng, where, stable):
    """One tag in every slot of 5 tiles: the carry crosses whole tiles."""
    n = 5 * T
    tomb = np.zeros(n, np.uint8)
    if where is not None:
        tomb[where] = 1
    K = 10**6
    t = _cat(_fill(0, 0, 1), _tup(np.full(n, K), np.full(n, 9), np.full(n, 1), tomb), _fill(37, K + 1, 3))
    cut = np.array([50, 9 if stable else 8], np.uint64)
    res = _check(eng, t, cut)
    got, src = res[False]
    at = np.flatnonzero(got[0] == K)
    if where is not None and stable:
        assert len(at) == 0
    else:
        assert len(at) == 1 and got[3][at[0]] == (where is not None) and src[at[0]] == 0
    # ... and with tuples before it, so the run starts and ends inside tiles
    _check(eng, _cat(_fill(777, 0, 4), tuple(x[:n] for x in t), _fill(37, K + 1, 3)), cut)


# ---- 3. one key spanning 5 tiles whose LWW winner is its last tuple
@pytest.mark.parametrize("case", ["dead-stable", "dead-unstable", "live", "copies-first-dead", "copies-first-live"])
def test_key_spanning_five_tiles(eng, case):
    n = 5 * T - 5 if case.startswith("copies") else 5 * T
    K = 10**6
    ts = np.arange(1, n + 1, dtype=np.uint64)
    tomb = (np.arange(n) % 3 == 0).astype(np.uint8)
    tomb[-1] = 0 if case == "live" else 1
    run = _tup(np.full(n, K), ts, np.full(n, 1), tomb)
    wts = n                                                  # the winner's ts
    if case.startswith("copies"):                            # the winner tag copied across the last tile edge:
        c = 6                                                # 3 copies before it, 3 after
        first_dead = case == "copies-first-dead"
        ct = np.array([1 if first_dead else 0] + [0 if first_dead else 1] * (c - 1), np.uint8)
        run = _cat(tuple(x[:-1] for x in run), _tup(np.full(c, K), np.full(c, wts), np.full(c, 1), ct))
        pre = _fill(3, 0, 5)
        first = len(pre[0]) + n - 1
        assert first == 5 * T - 3 and first + c - 1 == 5 * T + 2
    else:
        pre = _fill(0, 0, 5)
        first = n - 1
    t = _cat(pre, run, _fill(50, K + 1, 6))
    cut = np.array([10, wts - 1 if case == "dead-unstable" else wts], np.uint64)
    got, src = _check(eng, t, cut)[True]
    at = np.flatnonzero(got[0] == K)
    gone = case in ("dead-stable", "copies-first-dead")
    if gone:
        assert len(at) == 0
    else:
        dead = case == "dead-unstable"
        assert len(at) == 1 and got[1][at[0]] == wts and got[3][at[0]] == dead and src[at[0]] == first


# ---- 4. the boundaries of the stability test
def test_stability_boundaries(eng):
    H = 2**63
    cut = np.array([100, H, M64, 5], np.uint64)              # n_cut = 4
    rows = [  # key, ts, rep, dropped (every tuple dead, one tag per key)
        (1, 100, 0, True), (2, 101, 0, False), (3, 0, 0, True),                 # ts == cut, cut + 1
        (4, 5, 3, True), (5, 6, 3, False), (6, 5, 4, False), (7, 0, 4, False),  # rep == n_cut - 1 / n_cut
        (8, 0, M32, False), (9, M64, M32, False),                               # rep = 2^32 - 1
        (10, H - 1, 1, True), (11, H, 1, True), (12, H + 1, 1, False), (13, M64, 1, False),
        (14, M64, 2, True), (15, M64 - 1, 2, True), (16, 0, 2, True),           # cut = 2^64 - 1
        (17, H + 5, 3, False), (18, M64, 3, False), (19, H, 0, False),          # a signed compare drops these
    ]
    t = _tup([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], np.ones(len(rows)))
    live = _tup(t[0], t[1], t[2], np.zeros(len(rows)))
    exp = tuple(x[[not r[3] for r in rows]] for x in t)
    for lww, (got, _) in _check(eng, t, cut).items():
        _assert_tuples(got, exp, f"lww={lww}")
    for lww, (got, _) in _check(eng, live, cut).items():     # nothing dead: nothing goes
        _assert_tuples(got, live, f"live lww={lww}")
    wide = np.concatenate([cut, np.array([5], np.uint64)])   # n_cut = 5: rep 4 is now inside
    for lww, (got, _) in _check(eng, t, wide).items():
        assert (6 not in got[0]) and (7 not in got[0]) and (8 in got[0])
    one = np.array([M64], np.uint64)                         # n_cut = 1: only rep 0
    for lww, (got, _) in _check(eng, t, one).items():
        _assert_tuples(got, tuple(x[t[2] != 0] for x in t), f"n_cut=1 lww={lww}")


def test_no_cut_is_the_merge_bit_for_bit(eng):
    """n_cut == 0 with cut_dev NULL: the engine's own merge(t, {})."""
    t = _both(5000, 700)
    Td = TupleSet.from_numpy(*t, eng.device)
    E = TupleSet.empty(0, eng.device)
    for lww in (True, False):
        m = (eng.lww_merge if lww else eng.orset_merge)(Td, E).to_numpy()
        out, cnt = eng.set_compact(Td, lww, None)
        k = int(as_u64(cnt)[0])
        assert k == len(m[0]) < len(t[0])
        _assert_tuples(tuple(x[:k] for x in out.to_numpy()), m, f"lww={lww}")
        out, cnt = eng.set_compact(Td, lww, torch.empty(0, dtype=torch.int64, device=eng.device))
        assert int(as_u64(cnt)[0]) == k
    assert eng.device_status(clear=True) == 0


# ---- 5. extremes
def test_everything_and_nothing_dropped(eng):
    t = _both(5000, 700)
    dead = _tup(t[0], t[1], t[2], np.ones(len(t[0])))
    live = _tup(t[0], t[1], t[2], np.zeros(len(t[0])))
    top = np.full(64, M64, np.uint64)
    Dd = TupleSet.from_numpy(*dead, eng.device)
    for lww in (True, False):
        out = TupleSet.empty(len(Dd), eng.device)
        src = torch.full((len(Dd),), 0x5a5a, dtype=torch.int64, device=eng.device)
        for x in (out.key, out.ts, out.rep, out.tomb):
            x.fill_(0x5a)
        _, _, cnt = eng.set_compact(Dd, lww, u64_tensor(top, eng.device), out=out, src=src)
        assert int(as_u64(cnt)[0]) == 0
        assert all(bool((x == 0x5a).all()) for x in (out.key, out.ts, out.rep, out.tomb))   # out untouched
        assert bool((src == 0x5a5a).all())
    assert eng.device_status(clear=True) == 0
    _check(eng, dead, top)
    for s in (live, dead):                                   # nothing goes: live under any cut, dead under a zero cut
        res = _check(eng, s, top if s is live else np.zeros(64, np.uint64))
        for lww in (True, False):
            exp = _merge(lww)(s, _empty())
            if s is dead:                                    # (ts == 0 tags are stable even under a zero cut)
                exp = tuple(x[exp[1] != 0] for x in exp)
            _assert_tuples(res[lww][0], exp, f"lww={lww}")


# ---- 6. properties on the randomised inputs
def _compact_np(eng, t, lww, cut):
    Td = TupleSet.from_numpy(*t, eng.device)
    out, cnt = eng.set_compact(Td, lww, _cut_dev(eng, cut))
    k = int(as_u64(cnt)[0])
    return tuple(np.ascontiguousarray(x[:k]) for x in out.to_numpy())


def _elements(eng, t, lww):
    keys, cnt = eng.set_elements(TupleSet.from_numpy(*t, eng.device), lww)
    return as_u64(keys)[:int(as_u64(cnt)[0])]


@pytest.mark.parametrize("lww", [True, False])
def test_properties(eng, lww):
    t = _both(5000, 700)
    c1 = _compact_np(eng, t, lww, CUT)
    assert 0 < len(c1[0]) < len(_merge(lww)(t, _empty())[0])
    for cut in (CUT, np.full(64, M64, np.uint64), CUT[:17]):  # the members never change
        np.testing.assert_array_equal(_elements(eng, _compact_np(eng, t, lww, cut), lww), _elements(eng, t, lww))
    _assert_tuples(_compact_np(eng, c1, lww, CUT), c1, "idempotent")
    hi = CUT + np.random.default_rng(8).integers(0, 2**18, 64, dtype=np.uint64)
    c2 = _compact_np(eng, t, lww, hi)                        # a cut >= another: a subsequence of its result
    assert len(c2[0]) < len(c1[0])
    s1 = list(zip(*(x.tolist() for x in c1)))
    pos = {v: i for i, v in enumerate(s1)}
    at = [pos[v] for v in zip(*(x.tolist() for x in c2))]    # (KeyError: a tuple the lower cut had dropped)
    assert at == sorted(at)
    assert eng.device_status(clear=True) == 0


def test_compaction_commutes_with_the_merge(eng):
    """OR-Set: merge(compact(a), compact(b)) == compact(merge(a, b)) for a, b
    that agree on the tombs of stable tags (the caller's obligation)."""
    a, b = _side(0, 5000, 700), _side(1, 5000, 700)
    m = oracle.orset_merge(a, b)
    dead = {(k, s, r) for k, s, r, d in zip(*(x.tolist() for x in m)) if d}
    fixed = []
    for t in (a, b):
        st = ~_keep(_tup(t[0], t[1], t[2], np.ones(len(t[0]))), CUT)        # stable tags
        isdead = np.array([g in dead for g in zip(*(x.tolist() for x in t[:3]))])
        fixed.append(_tup(t[0], t[1], t[2], np.where(st & isdead, 1, t[3])))
    a, b = fixed
    assert (a[3] != _side(0, 5000, 700)[3]).any() or (b[3] != _side(1, 5000, 700)[3]).any()
    ca, cb = _compact_np(eng, a, False, CUT), _compact_np(eng, b, False, CUT)
    lhs = eng.orset_merge(TupleSet.from_numpy(*ca, eng.device), TupleSet.from_numpy(*cb, eng.device)).to_numpy()
    mm = eng.orset_merge(TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)).to_numpy()
    rhs = _compact_np(eng, mm, False, CUT)
    assert len(rhs[0]) < len(mm[0])
    _assert_tuples(lhs, rhs, "commutes")
    _assert_tuples(rhs, ref_compact(oracle.orset_merge(a, b), False, CUT), "oracle")
    assert eng.device_status(clear=True) == 0


# ---- 7. a value column compacted with the tuples
@pytest.mark.parametrize("es", [1, 8, 16])
def test_map_compact(eng, es):
    t = _both(5000, 700)
    n = len(t[0])
    i = np.arange(n, dtype=np.int64)
    if es == 1:
        f = lambda x: ((x * 7 + 3) & 0x7f).astype(np.int8)
    elif es == 8:
        f = lambda x: x * 3 + 1
    else:
        f = lambda x: np.stack([x, ~x], axis=1)
    val = torch.from_numpy(np.ascontiguousarray(f(i))).to(eng.device)
    Td = TupleSet.from_numpy(*t, eng.device)
    for lww in (True, False):
        exp = ref_compact(t, lww, CUT)
        out, oval, cnt = eng.map_compact(Td, val, lww, u64_tensor(CUT, eng.device))
        k = int(as_u64(cnt)[0])
        _assert_tuples(tuple(x[:k] for x in out.to_numpy()), exp, f"lww={lww}")
        src = _ref_src(eng, t, lww, CUT)
        np.testing.assert_array_equal(oval.cpu().numpy()[:k], f(src.astype(np.int64)))
    assert eng.device_status(clear=True) == 0


# ---- 8. chained off a merge's device count
@pytest.mark.parametrize("lww", [True, False])
def test_chained_off_a_merge(eng, lww):
    a, b = _side(0, 5000, 700), _side(1, 5000, 700)
    A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
    cap = len(a[0]) + len(b[0])
    mo = TupleSet.empty(cap, eng.device)
    mo.key.fill_(0)                                          # sentinels past the merge's count: key 0 (before every
    mo.ts.fill_(0)                                           # tuple), dead and stable / live -- they must not count
    mo.rep.fill_(0)
    mo.tomb.copy_(torch.arange(cap, device=eng.device) % 2)
    mo, cnt = (eng.lww_merge if lww else eng.orset_merge)(A, B, out=mo, trim=False)
    k = int(as_u64(cnt)[0])
    assert 0 < k < cap
    m = _merge(lww)(a, b)
    exp = ref_compact(m, lww, CUT)
    out, src, c2 = eng.set_compact(mo, lww, u64_tensor(CUT, eng.device), n_dev=cnt, with_src=True)
    k2 = int(as_u64(c2)[0])
    assert k2 == len(exp[0]) < k
    _assert_tuples(tuple(x[:k2] for x in out.to_numpy()), exp, "chained")
    assert int(src[:k2].max().item()) < k
    assert int(as_u64(eng.set_compact_count(mo, lww, u64_tensor(CUT, eng.device), n_dev=cnt))[0]) == k2
    assert eng.device_status(clear=True) == 0


# ---- 9. a device count past the capacity
@pytest.mark.parametrize("bad", [5001, M64])
def test_device_count_out_of_range(eng, bad):
    t = _side(0, 5000, 700)
    Td = TupleSet.from_numpy(*t, eng.device)
    Cd = u64_tensor(CUT, eng.device)
    assert eng.device_status(clear=True) == 0
    for lww in (True, False):
        out = TupleSet.empty(5000, eng.device)
        src = torch.full((5000,), 0x5a5a, dtype=torch.int64, device=eng.device)
        for x in (out.key, out.ts, out.rep, out.tomb):
            x.fill_(0x5a)
        _, _, cnt = eng.set_compact(Td, lww, Cd, n_dev=_dev(eng, bad), out=out, src=src)
        assert as_u64(cnt)[0] == M64
        assert eng.device_status(clear=True) & DEV_RANGE
        assert all(bool((x == 0x5a).all()) for x in (out.key, out.ts, out.rep, out.tomb))
        assert bool((src == 0x5a5a).all())
        only = eng.set_compact_count(Td, lww, Cd, n_dev=_dev(eng, bad))
        assert as_u64(only)[0] == M64
        assert eng.device_status(clear=True) & DEV_RANGE
    _check(eng, t, CUT, Td=Td)                               # the next calls are exact
    _check(eng, t, CUT, Td=Td, n_dev=_dev(eng, 5000))        # a count AT the capacity is in range
    for n in (3000, 2049, 2048, 2047, 1, 0):                 # a shorter count reads that prefix
        _check(eng, tuple(np.ascontiguousarray(x[:n]) for x in t), CUT, Td=Td, n_dev=_dev(eng, n))


# ---- 10. unaligned views
@pytest.mark.parametrize("off", [1, 3])
def test_unaligned_views(eng, off):
    t = _both(5000, 700)
    F = TupleSet.from_numpy(*t, eng.device)
    pad = np.concatenate([np.full(off, M64, np.uint64), CUT])
    Cfull = u64_tensor(pad, eng.device)
    for fo in (1, 3):                                        # element offsets of the fields and of the cut
        _check(eng, tuple(np.ascontiguousarray(x[fo:]) for x in t), CUT,
               Td=TupleSet(F.key[fo:], F.ts[fo:], F.rep[fo:], F.tomb[fo:]), Cd=Cfull[off:])
    n = len(t[0]) - off
    out = TupleSet.empty(n + 8, eng.device)                  # ... and of the outputs
    src = torch.empty(n + 8, dtype=torch.int64, device=eng.device)
    o = TupleSet(out.key[off:off + n], out.ts[off:off + n], out.rep[off:off + n], out.tomb[off:off + n])
    sub = tuple(np.ascontiguousarray(x[off:]) for x in t)
    for lww in (True, False):
        _, s, cnt = eng.set_compact(TupleSet(F.key[off:], F.ts[off:], F.rep[off:], F.tomb[off:]), lww, Cfull[off:],
                                    out=o, src=src[off:off + n])
        exp = ref_compact(sub, lww, CUT)
        k = int(as_u64(cnt)[0])
        _assert_tuples(tuple(x[:k] for x in o.to_numpy()), exp, f"lww={lww}")
        np.testing.assert_array_equal(s.cpu().numpy()[:k], _ref_src(eng, sub, lww, CUT))
    assert eng.device_status(clear=True) == 0


# ---- 11. host-side errors: refused before any launch
def test_host_errors(eng):
    t = _side(0, 5000, 700)
    n = 1000
    Td = TupleSet.from_numpy(*(x[:n] for x in t), eng.device)
    O = TupleSet.empty(n, eng.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=eng.device)
    src = torch.zeros(n, dtype=torch.int64, device=eng.device)
    Cd = u64_tensor(CUT, eng.device)
    ct, co, cp, sp, cutp = Td.c(), O.c(), cnt.data_ptr(), src.data_ptr(), Cd.data_ptr()

    def raw(mode, tt, o, s, count, cut=cutp, n_cut=64, n_max=n):
        eng._bind()
        ref = lambda x: C.byref(x) if x is not None else None
        with pytest.raises(_lib.CrdtError) as ei:
            _lib.call("crdt_set_compact", eng.ctx, mode, ref(tt), n_max, None, cut, n_cut, ref(o), s, count,
                      ctx=eng.ctx)
        return ei.value.status

    def tup(x, **kw):
        f = {"key": x.key.data_ptr(), "ts": x.ts.data_ptr(), "rep": x.rep.data_ptr(), "tomb": x.tomb.data_ptr()}
        f.update(kw)
        return _lib.crdt_tuples(f["key"], f["ts"], f["rep"], f["tomb"])

    with pytest.raises(_lib.CrdtError) as ei:                # NULL ctx
        _lib.call("crdt_set_compact", None, 0, C.byref(ct), n, None, cutp, 64, None, None, cp)
    assert ei.value.status == E_INVAL
    assert raw(0, None, None, None, cp) == E_INVAL           # NULL t / count
    assert raw(1, ct, co, None, None) == E_INVAL
    assert raw(2, ct, None, None, cp) == E_INVAL             # bad mode
    assert raw(-1, ct, co, None, cp) == E_INVAL
    for f in FIELDS:                                         # NULL field pointers with n_max > 0
        assert raw(0, tup(Td, **{f: None}), None, None, cp) == E_INVAL
        assert raw(1, ct, tup(O, **{f: None}), None, cp) == E_INVAL
    for f, by in (("key", 4), ("ts", 4), ("rep", 2)):        # natural alignment of every operand
        for mode in (0, 1):
            assert raw(mode, tup(Td, **{f: getattr(Td, f).data_ptr() + by}), None, None, cp) == E_INVAL
            assert raw(mode, ct, tup(O, **{f: getattr(O, f).data_ptr() + by}), None, cp) == E_INVAL
    assert raw(0, ct, None, None, cp, cut=None) == E_INVAL   # cut NULL with n_cut > 0
    assert raw(1, ct, co, None, cp, cut=cutp + 4) == E_INVAL # cut / src misaligned
    assert raw(1, ct, co, sp + 4, cp) == E_INVAL
    assert raw(0, ct, None, sp, cp) == E_INVAL               # source indices without out
    assert raw(0, ct, ct, None, cp) == E_INVAL               # out overlapping t, the cut, src
    assert raw(1, ct, tup(O, ts=Td.ts.data_ptr() + 8 * (n - 1)), None, cp) == E_INVAL
    assert raw(0, ct, tup(O, tomb=Td.key.data_ptr() + 8 * (n - 1) + 7), None, cp) == E_INVAL
    assert raw(1, ct, tup(O, key=cutp + 8 * 63), None, cp) == E_INVAL
    assert raw(1, ct, tup(O, key=sp), sp, cp) == E_INVAL
    assert raw(0, ct, co, Td.ts.data_ptr(), cp) == E_INVAL   # src overlapping t, the cut
    assert raw(0, ct, co, cutp, cp) == E_INVAL
    assert raw(0, ct, None, None, cp, n_max=2**62) == E_RANGE
    assert raw(1, ct, None, None, cp, n_max=2**61) == E_RANGE   # more tiles than a launch holds
    assert raw(1, ct, None, None, cp, n_cut=2**32) == E_RANGE
    assert int(cnt.item()) == 0 and eng.device_status(clear=True) == 0
    cnt.fill_(77)                                            # n_max == 0: the count store alone, nothing read
    eng._bind()
    _lib.call("crdt_set_compact", eng.ctx, 0, C.byref(_lib.crdt_tuples(None, None, None, None)), 0, None, None, 0,
              None, None, cp, ctx=eng.ctx)
    assert int(cnt.item()) == 0
    _check(eng, tuple(np.ascontiguousarray(x[:n]) for x in t), CUT, Td=Td)


# ---- 12. captured in a graph: compact + gather after reserve
@pytest.mark.parametrize("lww", [True, False])
def test_graph_capture(eng, lww):
    t = _both(5000, 700)
    n = len(t[0])
    Td = TupleSet.from_numpy(*t, eng.device)
    Cd = u64_tensor(CUT, eng.device)
    val = torch.arange(n, dtype=torch.int64, device=eng.device) * 5 + 2
    none = val[:0]
    eng.reserve(1 << 20)
    out, src, cnt = eng.set_compact(Td, lww, Cd, with_src=True)          # eager
    oval = eng.gather_src(src, val, none, n_dev=cnt)
    torch.cuda.synchronize()
    k = int(as_u64(cnt)[0])
    eager = tuple(x[:k].copy() for x in out.to_numpy()) + (oval.cpu().numpy()[:k].copy(),)
    _assert_tuples(eager[:4], ref_compact(t, lww, CUT), "eager")
    g_out, g_src = TupleSet.empty(n, eng.device), torch.empty(n, dtype=torch.int64, device=eng.device)
    g_cnt, g_val = torch.zeros(1, dtype=torch.int64, device=eng.device), torch.empty(n, dtype=torch.int64, device=eng.device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        eng.set_compact(Td, lww, Cd, out=g_out, src=g_src, count=g_cnt)
        eng.gather_src(g_src, val, none, n_dev=g_cnt, out=g_val)
    for rep in range(2):
        for x in (g_out.key, g_out.ts, g_out.rep, g_out.tomb, g_val, g_cnt):
            x.fill_(0)
        g.replay()
        torch.cuda.synchronize()
        assert int(as_u64(g_cnt)[0]) == k
        _assert_tuples(tuple(x[:k] for x in g_out.to_numpy()), eager[:4], f"replay {rep}")
        np.testing.assert_array_equal(g_val.cpu().numpy()[:k], eager[4], err_msg=f"replay {rep} values")
    assert eng.device_status(clear=True) == 0
