"""GPU: the read side of the keyed sets -- live elements, cardinality and
membership of a sorted LWW / OR-Set state (crdt_set_elements,
crdt_u64_contains; csrc/setread.hip) against a numpy restatement of the
merges' own semantics and against the oracle's merge with an empty side.
Reference analog: CurrentState served on GET /data (main.go:129-139).

Tile = 2048 tuples (four waves of eight 64-tuple mask words): the hand-built
cases put key and tag runs across word, wave and tile edges."""
import ctypes as C

import numpy as np
import pytest
import torch

from crdt_amd import _lib, shard, synth
from crdt_amd.engine import TupleSet, as_u64, u64_tensor
from oracle import oracle
from test_shard_gloo import rank_sets, stable_rank_merge

pytestmark = pytest.mark.gpu

T = 2048                       # tuples per tile of the read kernels
DEV_RANGE = 2                  # CRDT_DEV_RANGE
E_INVAL = -1                   # CRDT_E_INVAL
M64 = 2**64 - 1


def ref_elements(key, ts, rep, tomb, lww):
    n = len(key)
    if n == 0:
        return key[:0]
    tag_new = np.ones(n, bool)
    tag_new[1:] = (key[1:] != key[:-1]) | (ts[1:] != ts[:-1]) | (rep[1:] != rep[:-1])
    first = np.flatnonzero(tag_new)
    tkey = key[first]
    if lww:
        last = np.ones(len(first), bool)
        last[:-1] = tkey[1:] != tkey[:-1]
        w = first[last]
        return key[w][tomb[w] == 0]
    tor = np.zeros(len(first), np.uint8)
    np.maximum.at(tor, np.cumsum(tag_new) - 1, tomb)
    return np.unique(tkey[tor == 0])


def _empty_side(t):
    return tuple(x[:0] for x in t)


def oracle_elements(t, lww):
    """The keys of merge(t, {}) whose (OR-Set: any) output tuple has tomb == 0."""
    k, _, _, tomb = (oracle.lww_merge if lww else oracle.orset_merge)(t, _empty_side(t))
    return np.unique(k[tomb == 0])


def _sets(seed, n, ks):
    return synth.sort_tuples_np(*synth.set_tuples(seed, 0, n, ks))


def _read(eng, dev, lww, n_dev=None):
    """(keys, count, cardinality) of one mode, read back."""
    keys, cnt = eng.set_elements(dev, lww, n_dev=n_dev)
    card = eng.set_cardinality(dev, lww, n_dev=n_dev)
    c = int(cnt.item())
    return as_u64(keys)[:c], c, int(card.item())


def _check(eng, t, exp=None, dev=None):
    """Both modes: the keys, the count and the key-less cardinality == the reference."""
    dev = TupleSet.from_numpy(*t, eng.device) if dev is None else dev
    res = {}
    for lww in (True, False):
        e = ref_elements(*t, lww) if exp is None else exp[lww]
        keys, c, card = _read(eng, dev, lww)
        name = "lww" if lww else "orset"
        np.testing.assert_array_equal(keys, e, err_msg=name)
        assert c == len(e), (name, c, len(e))
        assert card == c, (name, card, c)
        res[lww] = keys
    assert eng.device_status(clear=True) == 0
    return res


# ---- 1. sizes x key spaces
KNOWN = {(2047, 10): (9, 10), (4097, 1000): (887, 971), (100_000, 7): (6, 7), (100_000, 50_000): (38850, 41723)}


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 8193, 100_000])
def test_sizes_and_key_spaces(eng, n):
    for ks in (1, 7, max(1, n // 3), 10**9):
        t = _sets(31 + n, n, ks)
        _check(eng, t)
        if n in (2049, 100_000):                          # the restatement itself == the oracle's merge with {}
            for lww in (True, False):
                np.testing.assert_array_equal(ref_elements(*t, lww), oracle_elements(t, lww))


@pytest.mark.parametrize("n,ks", sorted(KNOWN))
def test_known_answers(eng, n, ks):
    got = _check(eng, _sets(31 + n, n, ks))
    assert (len(got[True]), len(got[False])) == KNOWN[(n, ks)]


# ---- 2. one key across many tiles
def test_one_key_across_many_tiles(eng):
    n = 20_000
    key = np.zeros(n, np.uint64)
    ts = np.repeat(np.arange(n // 4, dtype=np.uint64), 4)
    rep = np.tile(np.array([0, 0, 1, 1], np.uint32), n // 4)
    zero, none = np.zeros(1, np.uint64), np.zeros(0, np.uint64)
    got = _check(eng, (key, ts, rep, (np.arange(n) % 3 == 0).astype(np.uint8)))
    np.testing.assert_array_equal(got[True], none)
    np.testing.assert_array_equal(got[False], zero)
    got = _check(eng, (key, ts, rep, (np.arange(n) % 5 == 0).astype(np.uint8)))
    np.testing.assert_array_equal(got[True], zero)
    np.testing.assert_array_equal(got[False], zero)


# ---- 3. carry cases, built by hand
NC = 3 * T + 10


def _ordinary():
    """NC single-tuple keys 10 i (distinct tags), every third tombstoned."""
    i = np.arange(NC)
    return ((10 * i).astype(np.uint64), (1000 + i).astype(np.uint64), (i % 5).astype(np.uint32),
            (i % 3 == 0).astype(np.uint8))


def _with_key(lo, hi, tomb, same_tag=()):
    """Tuples [lo, hi) become ONE key (10 lo, between its ordinary neighbours)
    with distinct ascending tags and the given tombs; each index pair in
    same_tag carries one tag."""
    key, ts, rep, tb = _ordinary()
    key[lo:hi] = 10 * lo
    rep[lo:hi] = 0
    for a, b in same_tag:
        ts[b] = ts[a]
    tb[lo:hi] = tomb
    return key, ts, rep, tb


@pytest.mark.parametrize("live_at", [100, T + 500, 3 * T + 2, None])
def test_carry_key_spanning_all_tiles(eng, live_at):
    lo, hi = 3, NC - 3
    tomb = np.ones(hi - lo, np.uint8)
    if live_at is not None:
        tomb[live_at - lo] = 0
    t = _with_key(lo, hi, tomb)
    got = _check(eng, t)
    assert (np.uint64(10 * lo) in got[False]) == (live_at is not None)
    assert np.uint64(10 * lo) not in got[True]           # the key's last tag is tombstoned
    assert 0 < len(got[False]) < NC


@pytest.mark.parametrize("edge", [64, 512, T, 2 * T, 3 * T])
@pytest.mark.parametrize("tombs", [(1, 0), (0, 1), (0, 0), (1, 1)])
def test_carry_tag_straddles_an_edge(eng, edge, tombs):
    """One tag with a copy each side of a word / wave / tile edge, the key's
    other tags dead: the OR-Set member test is the OR over both copies; for
    LWW (the tag is the key's maximal one) the FIRST copy decides."""
    lo, hi = edge - 3, edge + 1
    tomb = np.ones(hi - lo, np.uint8)
    tomb[-2:] = tombs
    t = _with_key(lo, hi, tomb, same_tag=[(edge - 1, edge)])
    got = _check(eng, t)
    k = np.uint64(10 * lo)
    assert (k in got[False]) == (tombs == (0, 0))
    assert (k in got[True]) == (tombs[0] == 0)
    # ... and the same tag followed by more of the key (not its maximal tag): LWW reads the later tag
    tomb = np.ones(hi + 2 - lo, np.uint8)
    tomb[2:4] = tombs
    got = _check(eng, _with_key(lo, hi + 2, tomb, same_tag=[(edge - 1, edge)]))
    assert (k in got[False]) == (tombs == (0, 0)) and k not in got[True]


# ---- 4. duplicate-heavy
def test_duplicate_heavy(eng):
    a = _sets(5, 50_000, 20_000)
    flipped = (a[0], a[1], a[2], (1 - a[3]).astype(np.uint8))
    cat = tuple(np.concatenate([x, y]) for x, y in zip(a, flipped))
    order = np.lexsort((cat[2], cat[1], cat[0]))         # stable: a's copy of a tag first
    got = _check(eng, tuple(x[order] for x in cat))
    assert len(got[False]) == 0 and len(got[True]) == 16535
    odd = a[3].copy()
    odd[1::2] = 1 - odd[1::2]
    cat = tuple(np.concatenate([x, y]) for x, y in zip(a, (a[0], a[1], a[2], odd)))
    _check(eng, tuple(x[order] for x in cat))


# ---- 5. uint64 extremes
def test_uint64_extremes(eng):
    key = np.array([0, 5, 2**63, 2**64 - 1], np.uint64)
    ts = np.array([2**64 - 1, 0, 2**63, 1], np.uint64)
    rep = np.array([0, 2**32 - 1, 7, 7], np.uint32)
    tomb = np.array([0, 1, 0, 1], np.uint8)
    for tb in (tomb, 1 - tomb):
        got = _check(eng, (key, ts, rep, tb.astype(np.uint8)))
        np.testing.assert_array_equal(got[True], key[tb == 0])
        np.testing.assert_array_equal(got[False], key[tb == 0])


# ---- 6. unaligned views
@pytest.mark.parametrize("off", [1, 3, 7, 13])
def test_unaligned_views(eng, off):
    full = _sets(41 + off, 20_000, 9_000)
    F = TupleSet.from_numpy(*full, eng.device)
    _check(eng, tuple(x[off:] for x in full), dev=TupleSet(F.key[off:], F.ts[off:], F.rep[off:], F.tomb[off:]))


# ---- 7. chaining off a merge's device count
def test_chained_off_a_merge_count(eng):
    sa = synth.sort_tuples_np(*synth.set_tuples(71, 0, 50_000, 20_000))
    sb = synth.sort_tuples_np(*synth.set_tuples(71, 1, 30_000, 20_000))
    A, B = TupleSet.from_numpy(*sa, eng.device), TupleSet.from_numpy(*sb, eng.device)
    for lww in (True, False):
        merge = eng.lww_merge if lww else eng.orset_merge
        out = TupleSet.empty(len(A) + len(B), eng.device)
        out.key.fill_(-1)                                 # the capacity past the count is never read
        _, mc = merge(A, B, out=out, trim=False)
        keys, cnt = eng.set_elements(out, lww, n_dev=mc)  # (nothing read back in between)
        card = eng.set_cardinality(out, lww, n_dev=mc)
        exp = ref_elements(*(oracle.lww_merge if lww else oracle.orset_merge)(sa, sb), lww)
        assert int(cnt.item()) == len(exp) == int(card.item())
        np.testing.assert_array_equal(as_u64(keys)[:len(exp)], exp)
    ab = eng.orset_merge(A, B)
    ba = eng.orset_merge(B, A)
    ka, ca = eng.set_elements(ab, False)
    kb, cb = eng.set_elements(ba, False)
    assert int(ca.item()) == int(cb.item())
    np.testing.assert_array_equal(as_u64(ka)[:int(ca.item())], as_u64(kb)[:int(cb.item())])
    assert eng.device_status(clear=True) == 0


# ---- 8. a device count past the capacity
@pytest.mark.parametrize("bad", [5001, M64])
def test_n_dev_out_of_range(eng, bad):
    t = _sets(9, 5000, 700)
    dev = TupleSet.from_numpy(*t, eng.device)
    nd = u64_tensor(np.array([bad], np.uint64), eng.device)
    assert eng.device_status(clear=True) == 0
    for lww in (True, False):
        out = torch.full((5000,), 0x5a5a5a5a, dtype=torch.int64, device=eng.device)
        _, cnt = eng.set_elements(dev, lww, n_dev=nd, out=out)
        assert as_u64(cnt)[0] == M64
        assert eng.device_status(clear=True) & DEV_RANGE
        assert bool((out == 0x5a5a5a5a).all())
        card = eng.set_cardinality(dev, lww, n_dev=nd)
        assert as_u64(card)[0] == M64
        assert eng.device_status(clear=True) & DEV_RANGE
        res = eng.keys_contain(dev.key, dev.key[:100].clone(), n_dev=nd)
        assert not bool(res.any()) and eng.device_status(clear=True) & DEV_RANGE
    _check(eng, t, dev=dev)                               # the next calls are exact
    nd = u64_tensor(np.array([5000], np.uint64), eng.device)
    for lww in (True, False):
        keys, c, card = _read(eng, dev, lww, n_dev=nd)    # a count AT the capacity is in range
        np.testing.assert_array_equal(keys, ref_elements(*t, lww))
        assert card == c
    assert eng.device_status(clear=True) == 0


# ---- 9. membership
def test_keys_contain(eng):
    t = _sets(13, 60_000, 30_000)
    dev = TupleSet.from_numpy(*t, eng.device)
    keys, cnt = eng.set_elements(dev, False)
    live = ref_elements(*t, False)
    dead = np.setdiff1d(np.unique(t[0]), live)
    assert len(live) > 1000 and len(dead) > 500
    rng = np.random.default_rng(3)
    absent = rng.integers(0, 2**64 - 1, 40_000, dtype=np.uint64, endpoint=True)
    probes = np.concatenate([rng.choice(live, 30_000), rng.choice(dead, 29_998), absent,
                             np.array([0, M64], np.uint64)])
    assert len(probes) == 100_000
    rng.shuffle(probes)
    P = u64_tensor(probes, eng.device)
    got = eng.keys_contain(keys, P, n_dev=cnt).cpu().numpy()
    np.testing.assert_array_equal(got, np.isin(probes, live).astype(np.uint8))
    exact = keys[:len(live)].clone()                      # the host-side length, no device count
    np.testing.assert_array_equal(eng.keys_contain(exact, P).cpu().numpy(), got)
    half = len(live) // 2                                 # keys past a shorter device count are not found
    nd = u64_tensor(np.array([half], np.uint64), eng.device)
    got = eng.keys_contain(keys, P, n_dev=nd).cpu().numpy()
    np.testing.assert_array_equal(got, np.isin(probes, live[:half]).astype(np.uint8))
    for m in (0, 1):
        got = eng.keys_contain(exact, u64_tensor(live[7:7 + m], eng.device)).cpu().numpy()
        np.testing.assert_array_equal(got, np.ones(m, np.uint8))
    for n in (1, 15, 16, 17, 255, 256, 257, 4099):       # the search's step shapes, extremes as keys
        ks = np.unique(np.concatenate([rng.integers(0, 1000, n, dtype=np.uint64), np.array([0, M64], np.uint64)]))
        pr = np.concatenate([np.arange(0, 1002, dtype=np.uint64), np.array([M64 - 1, M64], np.uint64)])
        got = eng.keys_contain(u64_tensor(ks, eng.device), u64_tensor(pr, eng.device)).cpu().numpy()
        np.testing.assert_array_equal(got, np.isin(pr, ks).astype(np.uint8))
    none = torch.empty(0, dtype=torch.int64, device=eng.device)
    assert not bool(eng.keys_contain(none, P).any())
    assert eng.device_status(clear=True) == 0


# ---- 10. host-side errors: refused before any launch
def test_host_errors(eng):
    t = _sets(3, 1000, 100)
    dev = TupleSet.from_numpy(*t, eng.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=eng.device)
    ct = dev.c()

    def raw(mode, tuples, keys_out, count, n_max=1000):
        eng._bind()
        with pytest.raises(_lib.CrdtError) as ei:
            _lib.call("crdt_set_elements", eng.ctx, mode, C.byref(tuples) if tuples is not None else None, n_max,
                      None, keys_out, count, ctx=eng.ctx)
        return ei.value.status

    assert raw(2, ct, None, cnt.data_ptr()) == E_INVAL            # bad mode
    assert raw(-1, ct, None, cnt.data_ptr()) == E_INVAL
    assert raw(0, ct, None, None) == E_INVAL                      # NULL count
    assert raw(1, ct, dev.key.data_ptr(), cnt.data_ptr()) == E_INVAL          # keys_out aliasing t.key
    assert raw(1, ct, dev.ts.data_ptr() + 8 * 999, cnt.data_ptr()) == E_INVAL  # ... overlapping t.ts's last element
    mis = _lib.crdt_tuples(dev.key.data_ptr(), dev.ts.data_ptr() + 4, dev.rep.data_ptr(), dev.tomb.data_ptr())
    assert raw(0, mis, None, cnt.data_ptr()) == E_INVAL           # misaligned ts
    with pytest.raises(_lib.CrdtError) as ei:
        eng.set_elements(dev, True, out=dev.key)
    assert ei.value.status == E_INVAL
    assert raw(0, None, None, cnt.data_ptr(), n_max=0) == E_INVAL   # NULL tuples
    assert raw(0, ct, None, cnt.data_ptr(), n_max=2**62) == -6      # CRDT_E_RANGE
    assert int(cnt.item()) == 0 and eng.device_status(clear=True) == 0
    _check(eng, t, dev=dev)


# ---- 11. a distributed population's cardinality
@pytest.mark.parametrize("lww", [True, False])
def test_shard_set_cardinality(lww):
    R = 4
    comm = shard.Comm.loopback(0, R)
    try:
        sets = [rank_sets(17, r, 6000 - 500 * r, 4000 + 500 * r, 9000) for r in range(R)]
        assert sum(len(s[0][0]) + len(s[1][0]) for s in sets) == 40_000
        A = [TupleSet.from_numpy(*s[0], "cuda:0") for s in sets]
        B = [TupleSet.from_numpy(*s[1], "cuda:0") for s in sets]
        whole = (oracle.lww_merge if lww else oracle.orset_merge)(stable_rank_merge([s[0] for s in sets]),
                                                                  stable_rank_merge([s[1] for s in sets]))
        torch.cuda.synchronize()
        outs, counts = comm.set_merge_local_dev(A, B, lww=lww)
        cards = shard.set_cardinality(comm, outs, counts, lww)
        comm.sync()
        exp = len(ref_elements(*whole, lww))
        assert 0 < exp < len(whole[0])
        assert [int(c.item()) for c in cards] == [exp] * R
    finally:
        comm.close()
