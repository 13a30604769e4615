"""GPU: set deltas -- the tuples of one sorted LWW / OR-Set state another lacks
(crdt_set_delta; csrc/setdelta.hip) against a numpy restatement of the
semantics, the oracle's merges and the engine's own merges.  Reference analog:
the gossip pull ships the entire Diff (main.go:153-170, :245-256).

delta(src, dst) = the smallest D with merge(dst, D) == merge(dst, src), dst the
left (tie-winning) operand.  A tile of the kernels is T merge items of the
stable merged order of (dst, src); a count thread takes 4 of them, a wave 256,
a bitmap word 64: the hand-built cases put tag and key runs across those edges."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from crdt_amd import _lib, synth
from crdt_amd.engine import TupleSet, as_u64, u64_tensor
from oracle import oracle

pytestmark = pytest.mark.gpu

T = 2048                       # merge items per tile of the delta kernels
WAVE = 256                     # merge items per wave of the count pass
DEV_RANGE = 2                  # CRDT_DEV_RANGE
E_INVAL, E_RANGE = -1, -6
M64 = 2**64 - 1
FIELDS = ("key", "ts", "rep", "tomb")
DT = (np.uint64, np.uint64, np.uint32, np.uint8)


# ---- the semantics, restated in numpy
def _tags(t):
    """Distinct tags of sorted tuples: (first index of each tag run, tomb-OR of each run)."""
    key, ts, rep, tomb = t
    n = len(key)
    new = np.ones(n, bool)
    new[1:] = (key[1:] != key[:-1]) | (ts[1:] != ts[:-1]) | (rep[1:] != rep[:-1])
    first = np.flatnonzero(new)
    tor = np.zeros(len(first), np.uint8)
    if n:
        np.maximum.at(tor, np.cumsum(new) - 1, (tomb != 0).astype(np.uint8))
    return first, tor


def ref_delta(src, dst, lww):
    key, ts, rep, tomb = src
    if len(key) == 0:
        return tuple(x[:0] for x in src)
    fs, tor_s = _tags(src)
    fd, tor_d = _tags(dst)
    if lww:
        # src's winner per key: the last tag run of the key, the tomb of its first copy
        last = np.ones(len(fs), bool)
        last[:-1] = key[fs][1:] != key[fs][:-1]
        w = fs[last]
        dk = dst[0][fd]
        dlast = np.ones(len(fd), bool)
        dlast[:-1] = dk[1:] != dk[:-1]
        dw = fd[dlast]                                   # dst's maximal tag per key
        dkeys = dst[0][dw]
        pos = np.searchsorted(dkeys, key[w])
        has = np.zeros(len(w), bool)
        inb = pos < len(dkeys)
        has[inb] = dkeys[pos[inb]] == key[w][inb]
        p = np.where(has, pos, 0)
        if len(dw):
            dts, drep = dst[1][dw][p], dst[2][dw][p]
            greater = (ts[w] > dts) | ((ts[w] == dts) & (rep[w] > drep))
        else:
            greater = np.zeros(len(w), bool)
        ship = ~has | greater
        i = w[ship]
        return key[i], ts[i], rep[i], tomb[i]
    # OR-Set: the distinct tags of both sides in one stable order, dst's copy first
    ns, nd = len(fs), len(fd)
    k = np.concatenate([dst[0][fd], key[fs]])
    t = np.concatenate([dst[1][fd], ts[fs]])
    r = np.concatenate([dst[2][fd], rep[fs]])
    side = np.concatenate([np.zeros(nd, np.uint8), np.ones(ns, np.uint8)])
    tor = np.concatenate([tor_d, tor_s])
    o = np.lexsort((side, r, t, k))
    k, t, r, side, tor = k[o], t[o], r[o], side[o], tor[o]
    has = np.zeros(len(o), bool)
    has[1:] = (side[1:] == 1) & (side[:-1] == 0) & (k[1:] == k[:-1]) & (t[1:] == t[:-1]) & (r[1:] == r[:-1])
    tor_prev = np.zeros(len(o), np.uint8)
    tor_prev[1:] = tor[:-1]
    ship = (side == 1) & (~has | ((tor == 1) & (tor_prev == 0)))
    return k[ship], t[ship], r[ship], tor[ship]


def _merge(lww):
    return oracle.lww_merge if lww else oracle.orset_merge


def _empty():
    return tuple(np.zeros(0, d) for d in DT)


def _tup(key, ts, rep, tomb):
    return tuple(np.ascontiguousarray(np.asarray(x, dtype=d)) for x, d in zip((key, ts, rep, tomb), DT))


def _sort(t):
    return synth.sort_tuples_np(*t)


def _cat(*ts):
    return _sort(tuple(np.concatenate([t[f] for t in ts]) for f in range(4)))


@functools.lru_cache(maxsize=64)
def _sets(seed, side, n, ks):
    return synth.sort_tuples_np(*synth.set_tuples(seed, side, n, ks))


def _assert_tuples(got, exp, msg):
    for g, e, f in zip(got, exp, FIELDS):
        np.testing.assert_array_equal(g, e, err_msg=f"{msg} {f}")


def _check(eng, src, dst, S=None, Dd=None, ns_dev=None, nd_dev=None, exp=None):
    """Both modes: tuples and count == the restatement, the count-only call ==
    the full call, no device flag.  Returns {lww: D}."""
    S = TupleSet.from_numpy(*src, eng.device) if S is None else S
    Dd = TupleSet.from_numpy(*dst, eng.device) if Dd is None else Dd
    res = {}
    for lww in (True, False):
        name = "lww" if lww else "orset"
        e = ref_delta(src, dst, lww) if exp is None else exp[lww]
        out, cnt = eng.set_delta(S, Dd, lww, n_src_dev=ns_dev, n_dst_dev=nd_dev)
        only = eng.set_delta_count(S, Dd, lww, n_src_dev=ns_dev, n_dst_dev=nd_dev)
        c = int(cnt.item())
        assert c == len(e[0]), (name, c, len(e[0]))
        assert int(only.item()) == c, (name, int(only.item()), c)
        got = out.slice(c).to_numpy()
        _assert_tuples(got, e, name)
        res[lww] = got
    assert eng.device_status(clear=True) == 0
    return res


# ---- 1. sizes x key spaces, both skews
SIZES = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 100_000]


@pytest.mark.parametrize("ns", SIZES)
def test_sizes_and_key_spaces(eng, ns):
    for nd in SIZES:
        if ns == nd == 100_000:
            continue                                     # (the oracle test's and the known answers' pair)
        for ks in sorted({1, 7, max(1, max(ns, nd) // 3), 10**9}):
            src, dst = _sets(11, 1, ns, ks), _sets(11, 0, nd, ks)
            _check(eng, src, dst)


@pytest.mark.parametrize("ns,nd", [(2049, 100_000), (100_000, 2049)])
def test_skewed_pairs(eng, ns, nd):
    for ks in (1, 7, 100_000 // 3, 10**9):
        _check(eng, _sets(13, 1, ns, ks), _sets(13, 0, nd, ks))


# ---- 2. the restatement against the oracle (CPU only, but it pins the reference the GPU is held to)
def _multiset(t):
    return sorted(zip(*(x.tolist() for x in t)))


@pytest.mark.parametrize("ns,nd", [(2049, 100_000), (100_000, 100_000)])
def test_restatement_against_the_oracle(ns, nd):
    for ks in (7, 50_000):
        src, dst = _sets(3, 1, ns, ks), _sets(3, 0, nd, ks)
        for lww in (True, False):
            m = _merge(lww)
            D = ref_delta(src, dst, lww)
            full = m(dst, src)
            _assert_tuples(m(dst, D), full, "merge(dst, D)")
            assert len(ref_delta(src, full, lww)[0]) == 0
            assert len(ref_delta(full, full, lww)[0]) == 0
            own = set(_multiset(m(src, _empty())))
            d = _multiset(D)
            assert len(set(d)) == len(d) and set(d) <= own
            _assert_tuples(ref_delta(src, _empty(), lww), m(src, _empty()), "delta(src, {})")
            assert len(ref_delta(_empty(), dst, lww)[0]) == 0


# ---- 3. known answers: |D| of |merge(src, {})|, (LWW, OR-Set)
KNOWN = {
    (71, 50_000, 30_000, 20_000): ((12_203, 18_355), (48_692, 50_000)),
    (5, 4_097, 4_097, 1_000): ((476, 984), (3_905, 4_097)),
    (9, 100_000, 100_000, 7): ((1, 7), (95_388, 99_983)),
    (3, 2_049, 100_000, 50_000): ((864, 2_007), (1_930, 2_049)),
    (3, 100_000, 2_049, 50_000): ((42_638, 43_247), (99_881, 100_000)),
}


@pytest.mark.diag
@pytest.mark.parametrize("case", sorted(KNOWN))
def test_known_answers(eng, case):
    seed, ns, nd, ks = case
    src, dst = _sets(seed, 1, ns, ks), _sets(seed, 0, nd, ks)
    for lww, (d, own) in zip((True, False), KNOWN[case]):
        assert len(ref_delta(src, dst, lww)[0]) == d, "the restatement disagrees with the table"
        assert len(_merge(lww)(src, _empty())[0]) == own
    got = _check(eng, src, dst)
    assert (len(got[True][0]), len(got[False][0])) == (KNOWN[case][0][0], KNOWN[case][1][0])
    full = _check(eng, src, _empty())                    # delta(src, {}) == merge(src, {})
    for lww in (True, False):
        _assert_tuples(full[lww], _merge(lww)(src, _empty()), "delta(src, {})")


# ---- 4. GPU round trip
def test_round_trip_through_the_merges(eng):
    src, dst = _sets(71, 1, 50_000, 20_000), _sets(71, 0, 30_000, 20_000)
    S, Dd = TupleSet.from_numpy(*src, eng.device), TupleSet.from_numpy(*dst, eng.device)
    for lww in (True, False):
        merge = eng.lww_merge if lww else eng.orset_merge
        D = eng.set_delta(S, Dd, lww, trim=True)
        assert 0 < len(D) < len(S)
        via, full = merge(Dd, D), merge(Dd, S)
        assert len(via) == len(full)
        _assert_tuples(via.to_numpy(), full.to_numpy(), "merge(dst, delta)")
        assert int(eng.set_delta_count(S, full, lww).item()) == 0
    assert eng.device_status(clear=True) == 0


# ---- 5. chained off device counts, nothing read back
def test_chained_off_device_counts(eng):
    src, dst = _sets(71, 1, 50_000, 20_000), _sets(71, 0, 30_000, 20_000)
    S, Dd = TupleSet.from_numpy(*src, eng.device), TupleSet.from_numpy(*dst, eng.device)
    for lww in (True, False):
        merge = eng.lww_merge if lww else eng.orset_merge
        cap = len(S) + len(Dd)
        out = TupleSet.empty(cap, eng.device)
        # the capacity past the count: unsorted tuples that would ship (descending keys below every real one)
        out.key.copy_(torch.arange(cap, 0, -1, dtype=torch.int64, device=eng.device))
        out.ts.fill_(-1)
        out.rep.fill_(-1)
        out.tomb.fill_(1)
        _, mc = merge(Dd, S, out=out, trim=False)
        zero = eng.set_delta_count(S, out, lww, n_dst_dev=mc)
        back, bc = eng.set_delta(out, Dd, lww, n_src_dev=mc)
        bonly = eng.set_delta_count(out, Dd, lww, n_src_dev=mc)
        merged = _merge(lww)(dst, src)                   # (everything above was enqueued with no read-back)
        assert int(mc.item()) == len(merged[0]) < cap
        assert int(zero.item()) == 0
        exp = ref_delta(merged, dst, lww)
        assert int(bc.item()) == len(exp[0]) == int(bonly.item()) > 0
        _assert_tuples(back.slice(len(exp[0])).to_numpy(), exp, "delta(merged, dst)")
    assert eng.device_status(clear=True) == 0


# ---- 6. run-end decisions at edges, built by hand
def _ordinary(n):
    """n single-tuple keys 10 i (distinct tags), every third tombstoned."""
    i = np.arange(n)
    return _tup(10 * i, 1000 + i, i % 5, i % 3 == 0)


def _pick(t, idx):
    return tuple(x[idx] for x in t)


def _long_run(n, lo, hi):
    """_ordinary(n) with tuples [lo, hi) ONE key 10 lo, ascending distinct tags (ts 1000 + i, rep 0)."""
    key, ts, rep, tomb = _ordinary(n)
    key[lo:hi] = 10 * lo
    rep[lo:hi] = 0
    return key, ts, rep, tomb


@pytest.mark.parametrize("long_in_dst", [True, False])
def test_lww_key_run_across_many_tiles(eng, long_in_dst):
    """6a / 6b: one key holds 20_000 tuples on one side; the other side's one
    tuple of it is below, at (opposite tomb) and above the run's last tag."""
    n, lo, hi = 24_000, 100, 20_100
    big = _long_run(n, lo, hi)
    last_ts, k = 1000 + hi - 1, 10 * lo
    last_tomb = int(big[3][hi - 1])
    others = _pick(_ordinary(n), np.r_[0:lo:7, hi:n:7])  # ordinary tuples the long side also holds
    for ts, rep, rel in ((last_ts - 1, 4, "less"), (last_ts, 0, "equal"), (last_ts, 1, "greater"),
                         (last_ts + 1, 0, "greater")):
        one = _tup([k], [ts], [rep], [1 - last_tomb])
        small = _cat(others, one)
        src, dst = (small, big) if long_in_dst else (big, small)
        got = _check(eng, src, dst)
        ships = bool((got[True][0] == k).any())
        # the long side's run end against the single tuple; an equal tag never ships
        want = (rel == "greater") if long_in_dst else (rel == "less")
        assert ships == want, (rel, long_in_dst)
        if ships:
            i = int(np.flatnonzero(got[True][0] == k)[0])
            win = (ts, rep, 1 - last_tomb) if long_in_dst else (last_ts, 0, last_tomb)
            assert (int(got[True][1][i]), int(got[True][2][i]), int(got[True][3][i])) == win


EDGES = [64, WAVE, T, 2 * T, 3 * T]


def _twin(n, a):
    """_ordinary(n) with tuple a + 1 a second copy of tuple a's tag."""
    key, ts, rep, tomb = _ordinary(n)
    key[a + 1], ts[a + 1], rep[a + 1] = key[a], ts[a], rep[a]
    return key, ts, rep, tomb


@pytest.mark.parametrize("edge", EDGES)
def test_orset_src_copies_straddle_an_edge(eng, edge):
    """6c: one tag with a src copy each side of merged position `edge`; its
    tomb pairs x the tag absent / live / dead in dst."""
    n = 3 * T + 40
    for in_dst in (None, 0, 1):
        h = 0 if in_dst is None else 1                   # dst's copy is merged before src's two
        a = edge - 1 - h
        for tombs in ((0, 0), (0, 1), (1, 0), (1, 1)):
            src = _twin(n, a)
            src[3][a:a + 2] = tombs
            tag = (int(src[0][a]), int(src[1][a]), int(src[2][a]))
            rest = _pick(_ordinary(n), np.arange(edge + 5, n, 3))   # (merged after the edge: positions before it are src's)
            dst = rest if in_dst is None else _cat(rest, _tup([tag[0]], [tag[1]], [tag[2]], [in_dst]))
            got = _check(eng, src, dst)[False]
            hit = np.flatnonzero((got[0] == tag[0]) & (got[1] == tag[1]) & (got[2] == tag[2]))
            tor = tombs[0] | tombs[1]
            want = in_dst is None or (tor == 1 and in_dst == 0)
            assert len(hit) == (1 if want else 0), (edge, in_dst, tombs)
            if want:
                assert int(got[3][hit[0]]) == tor


@pytest.mark.parametrize("edge", EDGES)
def test_orset_dst_copies_straddle_an_edge(eng, edge):
    """6d: the same with dst's two copies each side of the edge, src's copy
    (absent / live / dead) merged right after them."""
    n = 3 * T + 40
    a = edge - 1
    for in_src in (None, 0, 1):
        for tombs in ((0, 0), (0, 1), (1, 0), (1, 1)):
            dst = _twin(n, a)
            dst[3][a:a + 2] = tombs
            tag = (int(dst[0][a]), int(dst[1][a]), int(dst[2][a]))
            rest = _pick(_ordinary(n), np.arange(edge + 5, n, 3))
            src = rest if in_src is None else _cat(rest, _tup([tag[0]], [tag[1]], [tag[2]], [in_src]))
            got = _check(eng, src, dst)[False]
            hit = np.flatnonzero((got[0] == tag[0]) & (got[1] == tag[1]) & (got[2] == tag[2]))
            want = in_src == 1 and (tombs[0] | tombs[1]) == 0
            assert len(hit) == (1 if want else 0), (edge, in_src, tombs)
            if want:
                assert int(got[3][hit[0]]) == 1


def test_one_key_three_tiles_on_both_sides(eng):
    """6e: one key spanning three tiles on each side, tags interleaved and shared."""
    m = 3 * T
    rng = np.random.default_rng(17)
    i = np.arange(m)
    pre, post = _pick(_ordinary(40), np.arange(0, 10)), _pick(_ordinary(40), np.arange(30, 40))
    for tie in ("src_above", "dst_above", "equal"):
        s_ts, d_ts = 2 * i, 3 * i                        # shared at the multiples of 6
        if tie == "src_above":
            s_ts = np.r_[s_ts[:-1], 10**6]
        elif tie == "equal":
            s_ts = np.r_[s_ts[:-1], d_ts[-1]]
        src = _cat(pre, _tup(np.full(m, 200), s_ts, np.zeros(m), rng.integers(0, 2, m)), post)
        dst = _cat(_pick(pre, np.arange(0, 10, 2)), _tup(np.full(m, 200), d_ts, np.zeros(m), rng.integers(0, 2, m)))
        got = _check(eng, src, dst)
        assert bool((got[True][0] == 200).any()) == (tie == "src_above")
        assert 0 < int((got[False][0] == 200).sum()) < m


# ---- 7. identical and flipped states, concatenated duplicates
def test_identical_flipped_and_duplicated_states(eng):
    a = _sets(5, 0, 50_000, 20_000)
    none = {True: _empty(), False: _empty()}
    _check(eng, a, a, exp=none)
    flipped = (a[0], a[1], a[2], (1 - a[3]).astype(np.uint8))
    got = _check(eng, a, flipped)                        # dst = src with every tomb flipped
    assert len(got[True][0]) == 0                        # LWW: ties keep dst
    dead = a[3] == 1                                     # (the generator's tags are distinct: one copy each)
    assert len(_tags(a)[0]) == len(a[0])
    _assert_tuples(got[False], _pick(a, dead), "orset flipped")
    cat = tuple(np.concatenate([x, y]) for x, y in zip(a, flipped))
    order = np.lexsort((cat[2], cat[1], cat[0]))         # stable: a's copy of a tag first
    dup = tuple(np.ascontiguousarray(x[order]) for x in cat)
    for half in (a, flipped):
        got = _check(eng, dup, half)
        assert len(got[True][0]) == 0
        assert len(got[False][0]) == int((half[3] == 0).sum())
        _check(eng, half, dup, exp=none)


# ---- 8. uint64 extremes
def test_uint64_extremes(eng):
    src = _tup([0, 0, 5, M64, M64], [7, M64, 1, M64 - 1, M64], [M64 >> 32, 0, 3, M64 >> 32, M64 >> 32], [0, 1, 0, 1, 0])
    absent = _tup([1, M64 - 1], [M64, M64], [M64 >> 32, 0], [0, 0])
    got = _check(eng, src, absent)
    _assert_tuples(got[False], src, "orset, none in dst")
    _assert_tuples(got[True], _pick(src, [1, 2, 4]), "lww, none in dst")
    none = {True: _empty(), False: _empty()}
    _check(eng, src, src, exp=none)
    below = _tup([0, M64], [M64, M64], [0, (M64 >> 32) - 1], [0, 1])    # key 0 tied, key 2^64-1 one rep below
    got = _check(eng, src, below)
    _assert_tuples(got[True], _pick(src, [2, 4]), "lww")
    _assert_tuples(got[False], _pick(src, [0, 1, 2, 3, 4]), "orset")    # (0, M64, 0): src dead, dst live


# ---- 9. unaligned views
@pytest.mark.parametrize("so", [1, 3, 7, 13])
def test_unaligned_views(eng, so):
    fs, fd = _sets(41, 1, 20_000, 9_000), _sets(41, 0, 20_000, 9_000)
    FS, FD = TupleSet.from_numpy(*fs, eng.device), TupleSet.from_numpy(*fd, eng.device)
    for do in (1, 3, 7, 13):
        _check(eng, tuple(x[so:] for x in fs), tuple(x[do:] for x in fd),
               S=TupleSet(FS.key[so:], FS.ts[so:], FS.rep[so:], FS.tomb[so:]),
               Dd=TupleSet(FD.key[do:], FD.ts[do:], FD.rep[do:], FD.tomb[do:]))


# ---- 10. a device count past the capacity
@pytest.mark.parametrize("bad", [5001, M64])
@pytest.mark.parametrize("on_src", [True, False])
def test_device_count_out_of_range(eng, bad, on_src):
    src, dst = _sets(9, 1, 5000, 700), _sets(9, 0, 5000, 700)
    S, Dd = TupleSet.from_numpy(*src, eng.device), TupleSet.from_numpy(*dst, eng.device)

    def dev(v):
        return u64_tensor(np.array([v], np.uint64), eng.device)

    kw = {"n_src_dev" if on_src else "n_dst_dev": dev(bad)}
    assert eng.device_status(clear=True) == 0
    for lww in (True, False):
        out = TupleSet.empty(5000, eng.device)
        for x in (out.key, out.ts, out.rep, out.tomb):
            x.fill_(0x5a)
        _, cnt = eng.set_delta(S, Dd, lww, out=out, **kw)
        assert as_u64(cnt)[0] == M64
        assert eng.device_status(clear=True) & DEV_RANGE
        assert all(bool((x == 0x5a).all()) for x in (out.key, out.ts, out.rep, out.tomb))
        only = eng.set_delta_count(S, Dd, lww, **kw)
        assert as_u64(only)[0] == M64
        assert eng.device_status(clear=True) & DEV_RANGE
    _check(eng, src, dst, S=S, Dd=Dd)                    # the next calls are exact
    _check(eng, src, dst, S=S, Dd=Dd, ns_dev=dev(5000), nd_dev=dev(5000))   # a count AT the capacity is in range
    for ns, nd in ((3000, 5000), (5000, 1234), (2047, 1), (0, 5000), (5000, 0)):  # a shorter count reads that prefix
        _check(eng, tuple(x[:ns] for x in src), tuple(x[:nd] for x in dst), S=S, Dd=Dd, ns_dev=dev(ns), nd_dev=dev(nd))


# ---- 11. host-side errors: refused before any launch
def test_host_errors(eng):
    src, dst = _sets(3, 1, 1000, 100), _sets(3, 0, 1000, 100)
    S, Dd = TupleSet.from_numpy(*src, eng.device), TupleSet.from_numpy(*dst, eng.device)
    O = TupleSet.empty(1000, eng.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=eng.device)
    cs, cd, co, cp = S.c(), Dd.c(), O.c(), cnt.data_ptr()

    def raw(mode, s, d, o, count, ns=1000, nd=1000):
        eng._bind()
        ref = lambda x: C.byref(x) if x is not None else None
        with pytest.raises(_lib.CrdtError) as ei:
            _lib.call("crdt_set_delta", eng.ctx, mode, ref(s), ns, None, ref(d), nd, None, ref(o), count, ctx=eng.ctx)
        return ei.value.status

    def tup(t, **kw):
        f = {"key": t.key.data_ptr(), "ts": t.ts.data_ptr(), "rep": t.rep.data_ptr(), "tomb": t.tomb.data_ptr()}
        f.update(kw)
        return _lib.crdt_tuples(f["key"], f["ts"], f["rep"], f["tomb"])

    with pytest.raises(_lib.CrdtError) as ei:               # NULL ctx
        _lib.call("crdt_set_delta", None, 0, C.byref(cs), 1000, None, C.byref(cd), 1000, None, None, cp)
    assert ei.value.status == E_INVAL
    assert raw(0, None, cd, None, cp) == E_INVAL            # NULL src / dst / count
    assert raw(0, cs, None, None, cp) == E_INVAL
    assert raw(1, cs, cd, co, None) == E_INVAL
    assert raw(2, cs, cd, None, cp) == E_INVAL              # bad mode
    assert raw(-1, cs, cd, co, cp) == E_INVAL
    for f in FIELDS:                                        # NULL field pointers on a side with n_max > 0
        assert raw(0, tup(S, **{f: None}), cd, None, cp) == E_INVAL
        assert raw(1, cs, tup(Dd, **{f: None}), None, cp) == E_INVAL
    for f, by in (("key", 4), ("ts", 4), ("rep", 2)):       # natural alignment of every operand
        for lww in (0, 1):
            assert raw(lww, tup(S, **{f: getattr(S, f).data_ptr() + by}), cd, None, cp) == E_INVAL
            assert raw(lww, cs, tup(Dd, **{f: getattr(Dd, f).data_ptr() + by}), None, cp) == E_INVAL
            assert raw(lww, cs, cd, tup(O, **{f: getattr(O, f).data_ptr() + by}), cp) == E_INVAL
    assert raw(0, cs, cd, cs, cp) == E_INVAL                # out overlapping an input
    assert raw(1, cs, cd, cd, cp) == E_INVAL
    assert raw(1, cs, cd, tup(O, ts=Dd.ts.data_ptr() + 8 * 999), cp) == E_INVAL   # ... its last element
    assert raw(0, cs, cd, tup(O, tomb=S.key.data_ptr() + 8 * 999 + 7), cp) == E_INVAL
    with pytest.raises(_lib.CrdtError) as ei:
        eng.set_delta(S, Dd, True, out=S)
    assert ei.value.status == E_INVAL
    assert raw(0, cs, cd, None, cp, ns=2**62) == E_RANGE
    assert raw(1, cs, cd, None, cp, nd=2**62) == E_RANGE
    assert raw(1, cs, cd, None, cp, ns=2**61, nd=2**61) == E_RANGE   # more tiles than a launch holds
    assert int(cnt.item()) == 0 and eng.device_status(clear=True) == 0
    cnt.fill_(77)                                           # ns_max == 0: the count store alone, no side read
    eng._bind()
    _lib.call("crdt_set_delta", eng.ctx, 0, C.byref(_lib.crdt_tuples(None, None, None, None)), 0, None, C.byref(cd),
              1000, None, None, cp, ctx=eng.ctx)
    assert int(cnt.item()) == 0
    _check(eng, src, dst, S=S, Dd=Dd)
