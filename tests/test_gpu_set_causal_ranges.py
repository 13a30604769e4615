"""GPU: the range-restricted causal OR-Set merge -- a whole (tuples, context)
state merged with what a peer shipped for the buckets whose digests differ
(crdt_orset_merge_causal_ranges; csrc/setcausal.hip) -- and
the digest round built on it (crdt_amd.reconcile.causal_round).  Every result
is bit-exact against the numpy restatement in tests/causal_ranges_util.py
(itself held to ref_causal over replica histories by
tests/test_set_causal_ranges_ref.py): tuples, source indices, merged context
and count.  Outputs are views inside canary buffers.

A tile of the count pass is T merge items of the stable merged order of (a, b);
a thread takes 4 of them, a bitmap word 64, a wave 256: the hand-built cases put
bucket edges on those edges."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from causal_ranges_util import bucket, ideal_flags, np_select, pick, ref_causal_ranges
from causal_util import FIELDS, History, cat, ctx_max, empty, live_keys, present, ref_causal, tup
from crdt_amd import _lib, reconcile, synth
from crdt_amd.engine import TupleSet, as_u64, u64_tensor
from oracle import oracle

pytestmark = pytest.mark.gpu

T = 2048                       # merge items per tile of the causal kernels
DEV_RANGE = 2                  # CRDT_DEV_RANGE
E_INVAL, E_RANGE = -1, -6
M64 = 2**64 - 1
PAD = 8                        # canary elements either side of an output view
NAME = "crdt_orset_merge_causal_ranges"


@functools.lru_cache(maxsize=64)
def _side(seed, side, n, ks):
    return synth.sort_tuples_np(*synth.set_tuples(seed, side, n, ks))


@functools.lru_cache(maxsize=8)
def _ctx(seed, n=64):
    return np.random.default_rng(seed).integers(0, 2**20, n).astype(np.uint64)


def _dev(eng, v):
    return u64_tensor(np.array([v], np.uint64), eng.device)


def _cdev(eng, c):
    return None if c is None else u64_tensor(np.asarray(c, np.uint64), eng.device)


def _fdev(eng, flags):
    return torch.from_numpy(np.ascontiguousarray(flags, dtype=np.uint8)).to(eng.device)


def _assert_tuples(got, exp, msg):
    for g, e, f in zip(got, exp, FIELDS):
        np.testing.assert_array_equal(g, e, err_msg=f"{msg} {f}")


def _canary(eng, n, nc):
    """(tuple buffer, its view of n; src buffer, view; ctx buffer, view of nc), every byte 0x5a."""
    tb = TupleSet.empty(n + 2 * PAD, eng.device)
    sb = torch.empty(n + 2 * PAD, dtype=torch.int64, device=eng.device)
    cb = torch.empty(nc + 2 * PAD, dtype=torch.int64, device=eng.device)
    for x in (tb.key, tb.ts, tb.rep, tb.tomb, sb, cb):
        x.view(torch.uint8).fill_(0x5a)
    tv = TupleSet(tb.key[PAD:PAD + n], tb.ts[PAD:PAD + n], tb.rep[PAD:PAD + n], tb.tomb[PAD:PAD + n])
    return tb, tv, sb, sb[PAD:PAD + n], cb, cb[PAD:PAD + nc]


def _untouched(x, lo, hi):
    """Every byte of x outside elements [lo, hi) is still 0x5a."""
    h = x.cpu().numpy()
    b = h.view(np.uint8).reshape(len(h), -1)
    return bool((b[:lo] == 0x5a).all() and (b[hi:] == 0x5a).all())


def _check(eng, a, ca, b, cb, sp, flags, A=None, B=None, Ca=None, Cb=None, SP=None, FL=None, na_dev=None, nb_dev=None):
    """Tuples, source indices, merged context and count == the restatement;
    the call without source indices and the count-only call agree; nothing is
    written outside the outputs' first `count` (context: n_ctx) elements; no
    device flag.  b: the tuples the call sees (the prefix under nb_dev).
    Returns (tuples, src)."""
    A = TupleSet.from_numpy(*a, eng.device) if A is None else A
    B = TupleSet.from_numpy(*b, eng.device) if B is None else B
    Ca = _cdev(eng, ca) if Ca is None else Ca
    Cb = _cdev(eng, cb) if Cb is None else Cb
    sp = np.zeros(0, np.uint64) if sp is None else np.asarray(sp, np.uint64)
    if SP is None and len(sp):
        SP = u64_tensor(sp, eng.device)
    FL = _fdev(eng, flags) if FL is None else FL
    exp, esrc, ectx = ref_causal_ranges(a, ca, b, cb, sp, flags)
    n, nc = len(A) + len(B), len(ectx)
    tb, tv, sb, sv, xb, xv = _canary(eng, n, nc)
    kw = dict(n_a_dev=na_dev, n_b_dev=nb_dev)
    _, _, _, cnt = eng.causal_merge_ranges(A, Ca, B, Cb, SP, FL, out=tv, src=sv, ctx_out=xv, **kw)
    plain, co2, cnt2 = eng.causal_merge_ranges(A, Ca, B, Cb, SP, FL, **kw)
    only = eng.causal_merge_ranges_count(A, Ca, B, Cb, SP, FL, **kw)
    k = int(cnt.item())
    assert k == len(exp[0]), (k, len(exp[0]))
    assert int(only.item()) == k and int(cnt2.item()) == k
    got = tv.slice(k).to_numpy()
    _assert_tuples(got, exp, "ranged")
    _assert_tuples(plain.slice(k).to_numpy(), exp, "ranged without src")
    gsrc = sv[:k].cpu().numpy()
    np.testing.assert_array_equal(gsrc, esrc, err_msg="src")
    np.testing.assert_array_equal(as_u64(xv), ectx, err_msg="ctx_out")
    np.testing.assert_array_equal(as_u64(co2), ectx, err_msg="ctx_out without src")
    for x in (tb.key, tb.ts, tb.rep, tb.tomb, sb):
        assert _untouched(x, PAD, PAD + k)
    assert _untouched(xb, PAD, PAD + nc)
    assert eng.device_status(clear=True) == 0
    return got, gsrc


def _quantiles(keys, m):
    """m ascending splitters at the quantiles of the sorted keys (reconcile.key_splitters' rule)."""
    n = len(keys)
    if m == 0 or n == 0:
        return np.zeros(m, np.uint64)
    step = -(-n // (m + 1))
    return np.ascontiguousarray(keys[np.minimum(np.arange(1, m + 1) * step, n - 1)]).astype(np.uint64)


# ---- 1. random states, b a real selection, flags from real digests
SIZES = [3, T - 1, T, T + 1, 3 * T + 5, 50_000]


@functools.lru_cache(maxsize=64)
def _pair(seed, na, nb, ks, m):
    """Two sides that hold the same tuples (a with more copies) in every other
    bucket of m quantile splitters, cut to na and nb tuples."""
    a0, b0 = _side(seed, 0, na, ks), _side(seed, 1, nb, ks)
    sp = _quantiles(np.sort(np.concatenate([a0[0], b0[0]])), m)
    ea, eb = bucket(a0[0], sp) % 2 == 0, bucket(b0[0], sp) % 2 == 0
    a, b = cat(a0, pick(b0, eb), pick(a0, ea)), cat(b0, pick(a0, ea))
    return tuple(x[:na] for x in a), tuple(x[:nb] for x in b), sp


def _digest_flags(eng, A, B, SP):
    flags, _ = eng.digest_diff(eng.set_digest(A, False, SP), eng.set_digest(B, False, SP))
    return flags


@pytest.mark.parametrize("m", [0, 1, 7, 255])
@pytest.mark.parametrize("na", SIZES)
def test_random_states(eng, na, m):
    ca, cb = _ctx(1), _ctx(2)
    partial = 0
    for i, nb in enumerate(SIZES):
        ks = (8, 2**40)[(i + SIZES.index(na)) % 2] if max(na, nb) < 50_000 else 2**40
        a, b, sp = _pair(11, na, nb, ks, m)
        A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
        SP = u64_tensor(sp, eng.device) if m else None
        FL = _digest_flags(eng, A, B, SP)
        flags = FL.cpu().numpy()
        np.testing.assert_array_equal(flags, ideal_flags(a, b, sp))
        partial += 0 < int(flags.sum()) < m + 1
        sel, ship = eng.set_select(B, False, SP, FL)
        exp_sel, _ = np_select(b, sp, flags)
        assert int(ship.item()) == len(exp_sel[0])
        _check(eng, a, ca, exp_sel, cb, sp, flags, A=A, B=sel.slice(len(B)), SP=SP, FL=FL, nb_dev=ship)
    if m >= 7:
        assert partial > 0                               # some but not all buckets flagged


# ---- 2. the two identities
@pytest.mark.parametrize("n", [T + 1, 50_000])
def test_all_flags_set_is_the_plain_merge(eng, n):
    """Byte-equal to causal_merge on the same operands, with and without src."""
    a, b = _side(13, 0, n, 900), _side(13, 1, n - 5, 900)
    A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
    Ca, Cb = _cdev(eng, _ctx(1)), _cdev(eng, _ctx(2))
    for m in (0, 7, 255):
        sp = _quantiles(a[0], m)
        SP, FL = (u64_tensor(sp, eng.device) if m else None), _fdev(eng, np.ones(m + 1, np.uint8))
        for with_src in (True, False):
            outs = []
            for call in (lambda **kw: eng.causal_merge(A, Ca, B, Cb, **kw),
                         lambda **kw: eng.causal_merge_ranges(A, Ca, B, Cb, SP, FL, **kw)):
                out = TupleSet.empty(len(A) + len(B), eng.device)
                src = torch.empty(len(A) + len(B), dtype=torch.int64, device=eng.device) if with_src else None
                for x in (out.key, out.ts, out.rep, out.tomb) + ((src,) if with_src else ()):
                    x.view(torch.uint8).fill_(0x5a)
                r = call(out=out, src=src)
                outs.append((out, src, r[-2], r[-1]))
            (o1, s1, c1, k1), (o2, s2, c2, k2) = outs
            assert int(k1.item()) == int(k2.item()) > 0
            for x, y in zip((o1.key, o1.ts, o1.rep, o1.tomb, c1), (o2.key, o2.ts, o2.rep, o2.tomb, c2)):
                assert torch.equal(x, y)
            if with_src:
                assert torch.equal(s1, s2)
    assert eng.device_status(clear=True) == 0


@pytest.mark.parametrize("n", [T + 1, 50_000])
def test_no_flag_set_is_a_alone(eng, n):
    a, b = _side(17, 0, n, 900), _side(17, 1, n + 9, 900)
    for m in (0, 7):
        sp = _quantiles(b[0], m)
        got, src = _check(eng, a, _ctx(1), b, _ctx(2), sp, np.zeros(m + 1, np.uint8))
        _assert_tuples(got, present(a), "present(a)")
        assert len(got[0]) > 0 and bool((src >= 0).all())


def test_empty_sides(eng):
    a, b = _side(19, 0, 3000, 50), _side(19, 1, 2500, 50)
    sp = _quantiles(a[0], 7)
    for flags in (np.zeros(8, np.uint8), np.ones(8, np.uint8), (np.arange(8) % 2).astype(np.uint8)):
        got, _ = _check(eng, a, _ctx(4), empty(), _ctx(5), sp, flags)
        assert 0 < len(got[0]) <= len(present(a)[0])
        got, _ = _check(eng, empty(), _ctx(4), b, _ctx(5), sp, flags)    # b's tags come out of flagged buckets alone
        assert (len(got[0]) > 0) == bool(flags.any())
        got, _ = _check(eng, empty(), None, empty(), None, sp, flags)
        assert len(got[0]) == 0


# ---- 3. bucket edges
LOW, HIGH = np.zeros(5, np.uint64), np.full(5, M64, np.uint64)


def _line(n, base=0, edge=None, twins=False):
    """A merged line of n items, item i at merged position i: single-tuple tags
    (every third one b's, some tombstoned) and, every 13 positions, a's copy
    and then b's of one tag (both live / a's dead / b's dead in turn).  Under
    ca = LOW and cb = HIGH a single of a survives iff its bucket is unflagged
    and a single of b iff it is flagged, so one item in the wrong bucket shows.
    edge: no such pair lies on items edge - 3 .. edge + 2, so that item edge
    opens a tag and item edge - 1 closes another; with twins the items (edge -
    2, edge - 1) and (edge, edge + 1) are pairs instead: a run ends on a b copy
    just below the edge and one opens on an a copy at it.
    Returns (a, b, key_at): key_at[i] the key of merged item i."""
    ka, kb, key_at = [], [], np.zeros(n, np.uint64)
    forced = {edge - 2, edge} if edge is not None and twins else set()
    clear = set() if edge is None else set(range(edge - 3, edge + 3))
    i = 0
    while i < n:
        key, e = base + 10 * i, i
        pair = i in forced or (i % 13 == 5 and i not in clear and i + 1 not in clear)
        if pair and i + 1 < n:
            v = (i // 13) % 3
            ka.append((key, 1000 + e, e % 5, int(v == 1)))
            kb.append((key, 1000 + e, e % 5, int(v == 2)))
            key_at[i] = key_at[i + 1] = key
            i += 2
            continue
        (kb if i % 3 == 2 else ka).append((key, 1000 + e, e % 5, int(i % 11 == 0)))
        key_at[i] = key
        i += 1
    mk = lambda rows: tup(*[[r[f] for r in rows] for f in range(4)])
    return mk(ka), mk(kb), key_at


def _first_of_tag(key_at, p):
    """p, or p + 1 when item p is the second copy of a pair."""
    return p + 1 if p > 0 and key_at[p] == key_at[p - 1] else p


EDGES = [4 * 37 + 3, 64 * 5, 256 * 3, T - 1, T, T + 1]   # a thread's items 3 | 4, a word, a wave, around the tile


@pytest.mark.parametrize("twins", [False, True])
@pytest.mark.parametrize("p", EDGES)
def test_bucket_edge_at_a_merged_position(eng, p, twins):
    """The first key of the upper bucket is merged item p exactly and equals
    the splitter (a splitter equal to a key puts the key into the upper
    bucket), or the splitter lies strictly between items p - 1 and p.  Both
    sides hold tags on both sides of the edge."""
    a, b, key_at = _line(T + 300, edge=p, twins=twins)
    assert _first_of_tag(key_at, p) == p and key_at[p - 1] != key_at[p]      # the edge is where the id says
    assert (key_at[p - 2] == key_at[p - 1]) == twins and (key_at[p] == key_at[p + 1]) == twins
    side = np.concatenate([np.zeros(len(a[0])), np.ones(len(b[0]))])
    keys = np.concatenate([a[0], b[0]])
    np.testing.assert_array_equal(keys[np.lexsort((side, keys))], key_at)    # item i is merged item i
    for spl in (int(key_at[p]), int(key_at[p]) - 5):
        for flags in ((0, 1), (1, 0)):
            got, _ = _check(eng, a, LOW, b, HIGH, [spl], np.array(flags, np.uint8))
            up = got[0] >= spl
            # singles: a's live ones of the unflagged bucket and b's of the flagged one, no others
            single_a, single_b = ~np.isin(a[0], b[0]) & (a[3] == 0), ~np.isin(b[0], a[0]) & (b[3] == 0)
            for t, single, kept_if_flagged in ((a, single_a, False), (b, single_b, True)):
                for upper in (False, True):
                    mine = t[0][single & ((t[0] >= spl) == upper)]
                    assert len(mine) > 0                 # the side holds tags on this side of the edge
                    there = np.isin(mine, got[0][up == upper])
                    assert there.all() if bool(flags[int(upper)]) == kept_if_flagged else not there.any()


def test_one_key_buckets_alternating_across_a_tile(eng):
    """Every key its own bucket, flagged and unflagged in turn: every item
    searches.  Without pairs every merged item is a bucket of its own, the
    tile's last and the next tile's first included."""
    for a, b, key_at in (_line(T + 100), _line(T + 100, edge=T)):
        sp = np.unique(key_at)
        for first in (0, 1):
            flags = ((np.arange(len(sp) + 1) + first) % 2).astype(np.uint8)
            got, _ = _check(eng, a, LOW, b, HIGH, sp, flags)
            assert 0 < len(got[0]) < len(sp)


def test_many_splitters(eng):
    """More splitters than keys (64 < m, 64^2 < m and 64^3 < m: every depth of
    the wave's 64-ary search), most buckets empty, a key on a splitter or not."""
    a, b, key_at = _line(T + 100)
    top = int(key_at[-1]) + 40
    for m in (65, 4097, 300_000):
        sp = (np.arange(1, m + 1, dtype=np.uint64) * np.uint64(top)) // np.uint64(m)
        flags = (np.arange(m + 1) % 3 == 1).astype(np.uint8)
        got, _ = _check(eng, a, LOW, b, HIGH, sp, flags)
        assert 0 < len(got[0])


def test_empty_buckets_from_equal_splitters(eng):
    a, b, key_at = _line(T + 100)
    k1, k2 = int(key_at[_first_of_tag(key_at, 700)]), int(key_at[_first_of_tag(key_at, T)])
    sp = [k1, k1, k1, k2, k2]                            # buckets 1, 2 and 4 are empty
    for flags in ((0, 1, 1, 1, 1, 0), (1, 0, 0, 0, 0, 1), (0, 1, 0, 0, 1, 1), (1, 0, 1, 1, 0, 0)):
        _check(eng, a, LOW, b, HIGH, sp, np.array(flags, np.uint8))
    sp = np.full(300, k1, np.uint64)                     # one value 300 times: buckets 0 and 300 hold everything
    for f0, f1 in ((0, 1), (1, 0)):
        flags = np.full(301, 1 - f0, np.uint8)
        flags[0], flags[300] = f0, f1
        _check(eng, a, LOW, b, HIGH, sp, flags)


def test_keys_and_splitters_above_2_63(eng):
    """The line crosses 2^63: a signed compare puts its upper half first."""
    n = T + 100
    a, b, key_at = _line(n, base=2**63 - 10 * (n // 2))
    assert int(key_at[0]) < 2**63 <= int(key_at[-1])
    mid = int(key_at[_first_of_tag(key_at, n // 2)])
    for sp in ([mid], [2**63], [int(key_at[3]), 2**63 - 1, 2**63 + 11, int(key_at[-3])], [M64], [M64 - 1, M64]):
        for first in (0, 1):
            flags = ((np.arange(len(sp) + 1) + first) % 2).astype(np.uint8)
            _check(eng, a, LOW, b, HIGH, sp, flags)


def test_one_bucket(eng):
    a, b, _ = _line(T + 100)
    for SP in (None, torch.empty(0, dtype=torch.int64, device=eng.device)):
        got0, _ = _check(eng, a, LOW, b, HIGH, None, np.array([0], np.uint8), SP=SP)
        _assert_tuples(got0, present(a), "flag 0")
        got1, _ = _check(eng, a, LOW, b, HIGH, None, np.array([1], np.uint8), SP=SP)
        _assert_tuples(got1, ref_causal(a, LOW, b, HIGH)[0], "flag 1")
        assert len(got0[0]) != len(got1[0])


# ---- 4. carries
def _long(na_c, nb_c, dead_a, dead_b):
    """One tag (300, 77, 2) with na_c copies on a and then nb_c on b, between
    single-tuple keys on both sides; the copies at dead_a / dead_b tombstoned."""
    i = np.arange(60)
    plain = tup(10 * i, 1000 + i, i % 5, i % 3 == 0)
    pre, post = pick(plain, np.arange(0, 20)), pick(plain, np.arange(40, 60))
    ta, tb = np.zeros(na_c, np.uint8), np.zeros(nb_c, np.uint8)
    ta[list(dead_a)] = 1
    tb[list(dead_b)] = 1
    a = cat(pre, tup(np.full(na_c, 300), np.full(na_c, 77), np.full(na_c, 2), ta), post)
    b = cat(pick(pre, np.arange(0, 20, 2)), tup(np.full(nb_c, 300), np.full(nb_c, 77), np.full(nb_c, 2), tb),
            pick(post, np.arange(1, 20, 2)))
    return a, b


@pytest.mark.parametrize("flagged", [False, True])
def test_one_tag_across_three_tiles(eng, flagged):
    """T + 50 copies on a, then T + 50 on b: the run ends on a b copy two tiles
    after a's first.  Unflagged: a alone decides, whatever b and the contexts
    hold.  Flagged: the plain rule, b's live copy deciding under ctx_a."""
    low, high = np.zeros(3, np.uint64), np.full(3, 77, np.uint64)
    sp = [295, 305]                                      # the tag's key alone in bucket 1
    flags = np.array([0, 1, 0] if flagged else [1, 0, 1], np.uint8)
    for dead_a in ((), (0,), (T + 49,)):
        for dead_b in ((), (T + 49,)):
            a, b = _long(T + 50, T + 50, dead_a, dead_b)
            for ca, cb in ((low, low), (high, high), (low, high), (high, low)):
                got, src = _check(eng, a, ca, b, cb, sp, flags)
                hit = np.flatnonzero(got[0] == 300)
                pa, pb = not dead_a, not dead_b
                want = ((pa and pb) or (pa and cb is low) or (pb and ca is low)) if flagged else pa
                assert len(hit) == (1 if want else 0), (flagged, dead_a, dead_b)
                if want:                                 # a's first copy; b's only where a does not hold it present
                    assert int(src[hit[0]]) == (20 if pa else -(10 + 1))


def test_redecided_run_end_in_an_unflagged_bucket(eng):
    """Two a copies of one tag at merged items T - 1 and T (and, in turn, a b
    copy at T + 1): the run end is a tile's first or second item and the scan
    re-decides it under the carry.  Unflagged with ctx_b covering the tag: it
    survives iff a holds it present."""
    n = T + 40
    i = np.arange(n)
    for in_b in (None, 0, 1):
        for tombs in ((0, 0), (1, 0), (0, 1)):
            key, ts, rep, tomb = (x.copy() for x in tup(10 * i, 1000 + i, i % 5, i % 3 == 0))
            p = T - 1
            key[p + 1], ts[p + 1], rep[p + 1] = key[p], ts[p], rep[p]
            tomb[p:p + 2] = tombs
            a = (key, ts, rep, tomb)
            tag = (int(key[p]), int(ts[p]), int(rep[p]))
            rest = pick(tup(10 * i + 1, 1000 + i, i % 5, i % 3 == 0), np.arange(T + 5, n, 3))   # (merged after the tag)
            b = rest if in_b is None else cat(rest, tup([tag[0]], [tag[1]], [tag[2]], [in_b]))
            for flagged in (False, True):
                sp, flags = [tag[0], tag[0] + 1], np.array([1, int(flagged), 1], np.uint8)
                got, src = _check(eng, a, LOW, b, HIGH, sp, flags)
                hit = np.flatnonzero(got[0] == tag[0])
                pa, pb = tombs == (0, 0), in_b == 0
                want = (pa and pb) or pb if flagged else pa      # flagged: ctx_b covers it, ctx_a does not
                assert len(hit) == (1 if want else 0), (in_b, tombs, flagged)
                if want:
                    assert int(src[hit[0]]) == (p if pa else -(int(np.flatnonzero(b[0] == tag[0])[0]) + 1))


# ---- 5. b's copies in unflagged buckets are ignored
def test_unselected_b_with_sparse_flags(eng):
    a, b = _side(19, 0, 30_000, 2**40), _side(19, 1, 30_000, 2**40)
    sp = _quantiles(a[0], 255)
    flags = np.zeros(256, np.uint8)
    flags[[3, 77, 130, 200, 255]] = 1
    ca, cb = _ctx(1), _ctx(2)
    got, _ = _check(eng, a, ca, b, cb, sp, flags)
    plain = ref_causal(a, ca, b, cb)[0]
    assert len(got[0]) != len(plain[0]) or not np.array_equal(got[0], plain[0])
    in_b = np.isin(got[0], b[0]) & ~np.isin(got[0], a[0])    # b's keys come out of the flagged buckets alone
    assert in_b.any() and bool((flags[bucket(got[0][in_b], sp)] == 1).all())


# ---- 6. the round
@functools.lru_cache(maxsize=2)
def _replicas(n=40_000, m=255):
    """Two states that differ in five of 256 buckets: there A lacks tuples B
    holds, B lacks tuples A holds and each has tuples the other never saw."""
    base, extra = _side(23, 0, n, 2**40), _side(23, 1, n // 4, 2**40)
    sp = _quantiles(base[0], m)
    hot = np.isin(bucket(base[0], sp), [3, 77, 130, 200, 255])
    idx = np.arange(n)
    a = pick(base, ~(hot & (idx % 3 == 0)))
    xh = np.isin(bucket(extra[0], sp), [3, 77, 130, 200, 255])
    b = cat(pick(base, ~(hot & (idx % 3 == 1))), pick(extra, xh))
    return a, b, sp


def test_round_gives_both_replicas_the_merge(eng):
    a, b, sp = _replicas()
    ca, cb = _ctx(1), _ctx(2)
    A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
    Ca, Cb, SP = _cdev(eng, ca), _cdev(eng, cb), u64_tensor(sp, eng.device)
    (ma, ka, xa), (mb, kb, xb), FL, (ship_a, ship_b) = reconcile.causal_round(eng, A, Ca, B, Cb, SP)
    full, xf, kf = eng.causal_merge(A, Ca, B, Cb)
    k = int(kf.item())
    exp, _, ectx, _ = ref_causal(a, ca, b, cb)
    assert int(ka.item()) == k == int(kb.item()) == len(exp[0])
    for mrg, name in ((ma, "MA"), (mb, "MB"), (full, "causal_merge")):
        _assert_tuples(mrg.slice(k).to_numpy(), exp, name)
    for x in (xa, xb, xf):
        np.testing.assert_array_equal(as_u64(x), ectx)
    flags = FL.cpu().numpy()
    np.testing.assert_array_equal(np.flatnonzero(flags), [3, 77, 130, 200, 255])
    sel_a, sel_b = np_select(a, sp, flags)[0], np_select(b, sp, flags)[0]
    assert int(ship_a.item()) == len(sel_a[0]) and int(ship_b.item()) == len(sel_b[0])
    assert 0 < len(sel_b[0]) < len(b[0]) // 20
    # the input discriminates: the plain merge with the selection is wrong
    nv, _, nk = eng.causal_merge(A, Ca, TupleSet.from_numpy(*sel_b, eng.device), Cb)
    naive = nv.slice(int(nk.item())).to_numpy()
    assert len(naive[0]) != k or not np.array_equal(naive[0], exp[0])
    assert eng.device_status(clear=True) == 0


def test_history_with_every_merge_a_round(eng):
    """test_gpu_set_causal.py's history in causal form, every merge done by
    causal_round: the dots equal the oracle's live tags after every step."""
    h = History(37)
    merges = partial = 0
    for _ in range(300):
        op, x, y = h.step()
        if op != "merge":
            continue
        merges += 1
        sp = np.sort(h.rng.integers(0, 13, int(h.rng.integers(0, 6)))).astype(np.uint64)
        SP = u64_tensor(sp, eng.device) if len(sp) else None
        A, B = TupleSet.from_numpy(*h.dots[x], eng.device), TupleSet.from_numpy(*h.dots[y], eng.device)
        (ma, ka, xa), (mb, kb, xb), FL, _ = reconcile.causal_round(eng, A, _cdev(eng, h.clock[x]), B,
                                                                  _cdev(eng, h.clock[y]), SP)
        flags = FL.cpu().numpy()
        partial += 0 < int(flags.sum()) < len(flags)
        keys, kc = eng.set_elements(ma, False, n_dev=ka)
        h.tomb[x] = oracle.orset_merge(h.tomb[x], h.tomb[y])
        h.dots[x] = ma.slice(int(ka.item())).to_numpy()
        h.clock[x] = as_u64(xa).copy()
        np.testing.assert_array_equal(as_u64(keys)[:int(kc.item())], live_keys(h.tomb[x]))
        _assert_tuples(h.dots[x], present(h.tomb[x]), "dots == live tags")
        _assert_tuples(mb.slice(int(kb.item())).to_numpy(), h.dots[x], "MB == MA")
        np.testing.assert_array_equal(as_u64(xb), h.clock[x])
    assert merges > 50 and partial > 10 and any(len(d[0]) for d in h.dots)
    assert eng.device_status(clear=True) == 0


# ---- 7. contracts
def _sparse(eng, a, m=31, every=4):
    sp = _quantiles(a[0], m)
    flags = (np.arange(m + 1) % every == 1).astype(np.uint8)
    return sp, flags, u64_tensor(sp, eng.device), _fdev(eng, flags)


def test_count_only_writes_nothing_else(eng):
    a, b = _side(41, 0, 5000, 700), _side(41, 1, 5000, 700)
    A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
    sp, flags, SP, FL = _sparse(eng, a)
    Ca, Cb = _cdev(eng, _ctx(1)), _cdev(eng, _ctx(2))
    cnt = torch.full((3,), 0x5a5a, dtype=torch.int64, device=eng.device)
    eng.causal_merge_ranges_count(A, Ca, B, Cb, SP, FL, count=cnt[1:2])
    exp = ref_causal_ranges(a, _ctx(1), b, _ctx(2), sp, flags)[0]
    assert cnt.cpu().tolist() == [0x5a5a, len(exp[0]), 0x5a5a]
    for t, ref in ((A, a), (B, b)):
        _assert_tuples(t.to_numpy(), ref, "inputs untouched")
    np.testing.assert_array_equal(as_u64(SP), sp)
    np.testing.assert_array_equal(FL.cpu().numpy(), flags)
    assert eng.device_status(clear=True) == 0


def test_map_merge_moves_the_named_values(eng):
    """b and b_val are map_select's tuples and column, its count the merge's n_b_dev."""
    a, b = _side(43, 0, 5000, 700), _side(43, 1, 6000, 700)
    A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
    sp, flags, SP, FL = _sparse(eng, a)
    ca, cb = _ctx(1), _ctx(2)
    sel, ssrc = np_select(b, sp, flags)
    exp, esrc, _ = ref_causal_ranges(a, ca, sel, cb, sp, flags)
    k = len(exp[0])
    assert (esrc < 0).any() and (esrc >= 0).any()
    for width in (None, 4):                              # 4-byte and 16-byte values
        shape = lambda n: (n,) if width is None else (n, width)
        va = torch.arange(int(np.prod(shape(len(a[0])))), dtype=torch.int32, device=eng.device).reshape(shape(len(a[0]))) * 3 + 1
        vb = -torch.arange(int(np.prod(shape(len(b[0])))), dtype=torch.int32, device=eng.device).reshape(shape(len(b[0]))) - 7
        sb, sval, ship = eng.map_select(B, vb, False, SP, FL)
        out, val, _, cnt = eng.causal_map_merge_ranges(A, va, _cdev(eng, ca), sb, sval, _cdev(eng, cb), SP, FL, n_b_dev=ship)
        assert int(cnt.item()) == k and int(ship.item()) == len(sel[0])
        _assert_tuples(out.slice(k).to_numpy(), exp, "map merge")
        ha, hb = va.cpu().numpy(), vb.cpu().numpy()[ssrc]    # the shipped column: b's values at the selection's sources
        want = np.where((esrc >= 0).reshape((-1,) + (1,) * (ha.ndim - 1)), ha[np.maximum(esrc, 0)],
                        hb[np.maximum(-(esrc + 1), 0)])
        np.testing.assert_array_equal(val.cpu().numpy()[:k], want)
    assert eng.device_status(clear=True) == 0


def test_chained_off_device_counts(eng):
    """A merge's output under its device count as a, a selection under its
    device count as b: nothing is read back in between, and the capacities
    past the counts hold tuples that would survive."""
    a0, b0, c = _side(47, 0, 5000, 700), _side(47, 1, 5000, 700), _side(48, 1, 3000, 700)
    A0, B0, Cc = (TupleSet.from_numpy(*x, eng.device) for x in (a0, b0, c))
    ca, cb, cc = _ctx(1), _ctx(2), _ctx(3)
    m1, _, e1, _ = ref_causal(a0, ca, b0, cb)
    sp, flags, SP, _ = _sparse(eng, m1)
    flags[-1] = 1                                        # (the sentinels' bucket: a b copy there would count)
    FL = _fdev(eng, flags)
    cap = len(a0[0]) + len(b0[0])
    out = TupleSet.empty(cap, eng.device)
    sel = TupleSet.empty(len(c[0]), eng.device)
    for t in (out, sel):                                 # live, uncovered sentinels past the counts
        t.key.fill_(-1)
        t.ts.fill_(-1)
        t.rep.fill_(-1)
        t.tomb.fill_(0)
    _, ctx1, cnt1 = eng.causal_merge(A0, _cdev(eng, ca), B0, _cdev(eng, cb), out=out)
    _, ship = eng.set_select(Cc, False, SP, FL, out=sel)
    exp_sel = np_select(c, sp, flags)[0]
    assert int(cnt1.item()) == len(m1[0]) < cap and int(ship.item()) == len(exp_sel[0]) < len(c[0])
    _check(eng, m1, e1, exp_sel, cc, sp, flags, A=out, B=sel, Ca=ctx1, SP=SP, FL=FL, na_dev=cnt1, nb_dev=ship)
    # mirrored: the selection as a, the merge's output as b
    _check(eng, exp_sel, cc, m1, e1, sp, flags, A=sel, B=out, Cb=ctx1, SP=SP, FL=FL, na_dev=ship, nb_dev=cnt1)


@pytest.mark.parametrize("bad", [5001, M64])
@pytest.mark.parametrize("on_a", [True, False])
def test_device_count_out_of_range(eng, bad, on_a):
    a, b = _side(9, 0, 5000, 700), _side(9, 1, 5000, 700)
    A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
    sp, flags, SP, FL = _sparse(eng, a)
    ca, cb = _ctx(1), _ctx(2)
    Ca, Cb = _cdev(eng, ca), _cdev(eng, cb)
    kw = {"n_a_dev" if on_a else "n_b_dev": _dev(eng, bad)}
    assert eng.device_status(clear=True) == 0
    tb, tv, sb, sv, xb, xv = _canary(eng, 10_000, 64)
    _, _, _, cnt = eng.causal_merge_ranges(A, Ca, B, Cb, SP, FL, out=tv, src=sv, ctx_out=xv, **kw)
    assert as_u64(cnt)[0] == M64
    assert eng.device_status(clear=True) & DEV_RANGE
    assert all(_untouched(x, 0, 0) for x in (tb.key, tb.ts, tb.rep, tb.tomb, sb))
    np.testing.assert_array_equal(as_u64(xv), ctx_max(ca, cb))           # the contexts alone decide it
    assert _untouched(xb, PAD, PAD + 64)
    only = eng.causal_merge_ranges_count(A, Ca, B, Cb, SP, FL, **kw)
    assert as_u64(only)[0] == M64
    assert eng.device_status(clear=True) & DEV_RANGE
    _check(eng, a, ca, b, cb, sp, flags, A=A, B=B, Ca=Ca, Cb=Cb, SP=SP, FL=FL)          # the next calls are exact
    _check(eng, a, ca, b, cb, sp, flags, A=A, B=B, SP=SP, FL=FL, na_dev=_dev(eng, 5000), nb_dev=_dev(eng, 5000))
    for na, nb in ((3000, 5000), (5000, 1234), (2047, 1), (0, 5000), (5000, 0), (0, 0)):   # a shorter count reads that prefix
        _check(eng, tuple(x[:na] for x in a), ca, tuple(x[:nb] for x in b), cb, sp, flags, A=A, B=B, SP=SP, FL=FL,
               na_dev=_dev(eng, na), nb_dev=_dev(eng, nb))


@pytest.mark.parametrize("off", [1, 3])
def test_offset_views(eng, off):
    """Every field of both operands, both contexts, the splitters and the flags
    at an odd element offset (the outputs are offset views in every test)."""
    fa, fb = _side(51, 0, 20_000, 9_000), _side(51, 1, 20_000, 9_000)
    FA, FB = TupleSet.from_numpy(*fa, eng.device), TupleSet.from_numpy(*fb, eng.device)
    ca, cb = _ctx(1), _ctx(2)
    a, b = tuple(x[off:] for x in fa), tuple(x[off + 2:] for x in fb)
    sp = _quantiles(a[0], 63)
    flags = (np.arange(64) % 3 == 1).astype(np.uint8)
    Pa = u64_tensor(np.concatenate([np.full(off, M64, np.uint64), ca]), eng.device)
    Pb = u64_tensor(np.concatenate([np.full(off + 2, M64, np.uint64), cb]), eng.device)
    Ps = u64_tensor(np.concatenate([np.zeros(off, np.uint64), sp, np.zeros(2, np.uint64)]), eng.device)
    Pf = _fdev(eng, np.concatenate([np.ones(off, np.uint8), flags, np.ones(2, np.uint8)]))
    view = lambda t, o: TupleSet(t.key[o:], t.ts[o:], t.rep[o:], t.tomb[o:])
    _check(eng, a, ca, b, cb, sp, flags, A=view(FA, off), B=view(FB, off + 2), Ca=Pa[off:], Cb=Pb[off + 2:],
           SP=Ps[off:off + 63], FL=Pf[off:off + 64])


def test_host_errors(eng):
    a, b = _side(3, 0, 1000, 100), _side(3, 1, 1000, 100)
    A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
    O = TupleSet.empty(2000, eng.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=eng.device)
    src = torch.zeros(2000, dtype=torch.int64, device=eng.device)
    Ca, Cb = _cdev(eng, _ctx(1)), _cdev(eng, _ctx(2))
    Co = torch.zeros(64, dtype=torch.int64, device=eng.device)
    sp, flags, SP, FL = _sparse(eng, a)
    ca, cb, co, cp, sq = A.c(), B.c(), O.c(), cnt.data_ptr(), src.data_ptr()
    xa, xb, xo, xs, xf = Ca.data_ptr(), Cb.data_ptr(), Co.data_ptr(), SP.data_ptr(), FL.data_ptr()
    ref = lambda x: C.byref(x) if x is not None else None

    def raw(ta, tb, o, s, count, na=1000, nb=1000, pa=xa, pb=xb, la=64, lb=64, po=xo, nad=None, nbd=None, ps=xs, m=31,
            pf=xf):
        eng._bind()
        with pytest.raises(_lib.CrdtError) as ei:
            _lib.call(NAME, eng.ctx, ref(ta), na, nad, pa, la, ref(tb), nb, nbd, pb, lb, ps, m, pf, ref(o), s, po, count,
                      ctx=eng.ctx)
        return ei.value.status

    def fld(t, **kw):
        f = {"key": t.key.data_ptr(), "ts": t.ts.data_ptr(), "rep": t.rep.data_ptr(), "tomb": t.tomb.data_ptr()}
        f.update(kw)
        return _lib.crdt_tuples(f["key"], f["ts"], f["rep"], f["tomb"])

    with pytest.raises(_lib.CrdtError) as ei:               # NULL ctx
        _lib.call(NAME, None, C.byref(ca), 1000, None, xa, 64, C.byref(cb), 1000, None, xb, 64, xs, 31, xf, None, None,
                  None, cp)
    assert ei.value.status == E_INVAL
    # the ranged arguments
    assert raw(ca, cb, None, None, cp, ps=None) == E_INVAL  # NULL splitters with m > 0
    assert raw(ca, cb, None, None, cp, pf=None) == E_INVAL  # NULL flags
    assert raw(ca, cb, None, None, cp, pf=None, ps=None, m=0) == E_INVAL
    assert raw(ca, cb, None, None, cp, ps=xs + 4) == E_INVAL   # misaligned splitters
    assert raw(ca, cb, None, None, cp, m=2**24) == E_RANGE
    assert raw(ca, cb, None, None, cp, m=2**40) == E_RANGE
    assert raw(ca, cb, fld(O, key=xs), None, cp) == E_INVAL          # out / src / ctx_out overlapping the splitters ...
    assert raw(ca, cb, fld(O, tomb=xs + 8 * 30 + 7), None, cp) == E_INVAL   # ... their last byte
    assert raw(ca, cb, co, xs, cp) == E_INVAL
    assert raw(ca, cb, None, None, cp, po=xs) == E_INVAL
    assert raw(ca, cb, fld(O, tomb=xf), None, cp) == E_INVAL         # ... the flags
    assert raw(ca, cb, fld(O, tomb=xf + 31), None, cp) == E_INVAL    # ... the last of the m + 1
    assert raw(ca, cb, fld(O, ts=xf & ~7), None, cp) == E_INVAL
    # crdt_orset_merge_causal's
    assert raw(None, cb, None, None, cp) == E_INVAL         # NULL a / b / count
    assert raw(ca, None, None, None, cp) == E_INVAL
    assert raw(ca, cb, co, None, None) == E_INVAL
    for f in FIELDS:                                        # NULL field pointers on a side with n_max > 0, and of out
        assert raw(fld(A, **{f: None}), cb, None, None, cp) == E_INVAL
        assert raw(ca, fld(B, **{f: None}), None, None, cp) == E_INVAL
        assert raw(ca, cb, fld(O, **{f: None}), None, cp) == E_INVAL
    for f, by in (("key", 4), ("ts", 4), ("rep", 2)):       # natural alignment of every operand
        assert raw(fld(A, **{f: getattr(A, f).data_ptr() + by}), cb, None, None, cp) == E_INVAL
        assert raw(ca, fld(B, **{f: getattr(B, f).data_ptr() + by}), None, None, cp) == E_INVAL
        assert raw(ca, cb, fld(O, **{f: getattr(O, f).data_ptr() + by}), None, cp) == E_INVAL
    assert raw(ca, cb, None, None, cp, pa=None) == E_INVAL  # a context NULL with n_ctx > 0
    assert raw(ca, cb, None, None, cp, pb=xb + 4) == E_INVAL
    assert raw(ca, cb, None, None, cp, po=xo + 4) == E_INVAL
    assert raw(ca, cb, None, None, cp, nad=cp + 4) == E_INVAL
    assert raw(ca, cb, None, None, cp, nbd=cp + 4) == E_INVAL
    assert raw(ca, cb, co, sq + 4, cp) == E_INVAL
    assert raw(ca, cb, None, sq, cp) == E_INVAL             # source indices without out
    assert raw(ca, cb, ca, None, cp) == E_INVAL             # out overlapping a, b, a context, src, ctx_out
    assert raw(ca, cb, fld(O, ts=B.ts.data_ptr() + 8 * 999), None, cp) == E_INVAL
    assert raw(ca, cb, fld(O, key=xb + 8 * 63), None, cp) == E_INVAL
    assert raw(ca, cb, fld(O, key=sq), sq, cp) == E_INVAL
    assert raw(ca, cb, co, xo, cp) == E_INVAL
    assert raw(ca, cb, None, None, cp, po=xa) == E_INVAL
    assert raw(ca, cb, None, None, cp, na=2**62) == E_RANGE
    assert raw(ca, cb, None, None, cp, na=2**61, nb=2**61, po=None) == E_RANGE   # more tiles than a launch holds
    assert raw(ca, cb, None, None, cp, la=2**32) == E_RANGE
    assert int(cnt.item()) == 0 and eng.device_status(clear=True) == 0
    cnt.fill_(77)                                           # no tuples: the count store and the ctx_out write alone
    Co.fill_(-1)
    eng._bind()
    none = _lib.crdt_tuples(None, None, None, None)
    _lib.call(NAME, eng.ctx, C.byref(none), 0, None, xa, 64, C.byref(none), 0, None, None, 0, None, 0, xf, None, None, xo,
              cp, ctx=eng.ctx)
    assert int(cnt.item()) == 0
    np.testing.assert_array_equal(as_u64(Co), _ctx(1))
    with pytest.raises(ValueError):
        eng.causal_merge_ranges(A, Ca, B, Cb, SP, FL, out=TupleSet.empty(1999, eng.device))
    with pytest.raises(ValueError):
        eng.causal_merge_ranges(A, Ca, B, Cb, SP, FL[:31])
    _check(eng, a, _ctx(1), b, _ctx(2), sp, flags, A=A, B=B, Ca=Ca, Cb=Cb, SP=SP, FL=FL)


def test_graph_capture(eng):
    """One linear capture of a selection, the ranged merge chained off its
    count and a gather, after a reserve; replayed over changed inputs."""
    a, b = _side(53, 0, 5000, 700), _side(53, 1, 4000, 700)
    A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
    n = len(a[0]) + len(b[0])
    sp, flags, SP, FL = _sparse(eng, a)
    Ca, Cb = _cdev(eng, _ctx(1)), _cdev(eng, _ctx(2))
    va = torch.arange(len(a[0]), dtype=torch.int64, device=eng.device) * 5 + 2
    vb = -torch.arange(len(b[0]), dtype=torch.int64, device=eng.device) - 9
    eng.reserve(1 << 20)
    g_sel, g_ship = TupleSet.empty(len(b[0]), eng.device), torch.zeros(1, dtype=torch.int64, device=eng.device)
    g_out, g_src = TupleSet.empty(n, eng.device), torch.empty(n, dtype=torch.int64, device=eng.device)
    g_cnt, g_val = torch.zeros(1, dtype=torch.int64, device=eng.device), torch.empty(n, dtype=torch.int64, device=eng.device)
    g_ctx = torch.empty(64, dtype=torch.int64, device=eng.device)

    def work():
        eng.set_select(B, False, SP, FL, out=g_sel, count=g_ship)
        eng.causal_merge_ranges(A, Ca, g_sel, Cb, SP, FL, n_b_dev=g_ship, out=g_out, src=g_src, ctx_out=g_ctx, count=g_cnt)
        eng.gather_src(g_src, va, vb, n_dev=g_cnt, out=g_val)

    work()                                               # eager: warm
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        work()
    ha = va.cpu().numpy()
    for rep, (sa, sb) in enumerate(((1, 2), (7, 8), (2, 1))):
        ca, cb = _ctx(sa), _ctx(sb)
        Ca.copy_(u64_tensor(ca, eng.device))             # the contexts change between replays ...
        Cb.copy_(u64_tensor(cb, eng.device))
        a2 = (a[0], a[1], a[2], np.roll(a[3], rep))      # ... which of a's tuples are tombstoned ...
        A.tomb.copy_(torch.from_numpy(a2[3].copy()).to(eng.device))
        f2 = np.roll(flags, rep)                         # ... and which buckets are flagged
        FL.copy_(_fdev(eng, f2))
        for x in (g_out.key, g_out.ts, g_out.rep, g_out.tomb, g_val, g_cnt, g_ctx, g_ship):
            x.fill_(0)
        g.replay()
        torch.cuda.synchronize()
        sel, _ = np_select(b, sp, f2)
        exp, esrc, ectx = ref_causal_ranges(a2, ca, sel, cb, sp, f2)
        k = len(exp[0])
        assert int(as_u64(g_cnt)[0]) == k and int(as_u64(g_ship)[0]) == len(sel[0])
        _assert_tuples(tuple(x[:k] for x in g_out.to_numpy()), exp, f"replay {rep}")
        np.testing.assert_array_equal(as_u64(g_ctx), ectx)
        # the gather reads b's column at the selection's positions: src names the selection's tuples
        hb = vb.cpu().numpy()
        want = np.where(esrc >= 0, ha[np.maximum(esrc, 0)], hb[np.maximum(-(esrc + 1), 0)])
        np.testing.assert_array_equal(g_val.cpu().numpy()[:k], want, err_msg=f"replay {rep} values")
    assert eng.device_status(clear=True) == 0
