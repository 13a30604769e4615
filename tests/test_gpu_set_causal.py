"""GPU: the tombstone-free OR-Set -- the causal merge of two (tuples, context)
states (crdt_orset_merge_causal; csrc/setcausal.hip), bit-exact against the
numpy restatement of the rule in tests/causal_util.py (itself held to the
oracle's tombstone-form merge by tests/test_set_causal_ref.py), the engine's
compaction and the oracle's OR-Set merge.  No reference analog: the reference's
Diff only grows.

A tile of the kernels is T merge items of the stable merged order of (a, b); a
count thread takes 4 of them, a wave 256, a bitmap word 64: the hand-built
cases put tag runs across those edges."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from causal_util import FIELDS, History, cat, ctx_max, empty, live_keys, present, ref_causal, tup
from crdt_amd import _lib, synth
from crdt_amd.engine import TupleSet, as_u64, u64_tensor
from oracle import oracle

pytestmark = pytest.mark.gpu

T = 2048                       # merge items per tile of the causal kernels
WAVE = 256                     # merge items per wave of the count pass
DEV_RANGE = 2                  # CRDT_DEV_RANGE
E_INVAL, E_RANGE = -1, -6
M64 = 2**64 - 1
KINDS = ("both", "a_kept", "a_dropped", "b_kept", "b_dropped", "absent")


@functools.lru_cache(maxsize=64)
def _side(seed, side, n, ks):
    return synth.sort_tuples_np(*synth.set_tuples(seed, side, n, ks))


@functools.lru_cache(maxsize=8)
def _ctx(seed, n=64):
    """n uniform values below 2^20: about half of the generator's tags are covered."""
    return np.random.default_rng(seed).integers(0, 2**20, n).astype(np.uint64)


def _dev(eng, v):
    return u64_tensor(np.array([v], np.uint64), eng.device)


def _cdev(eng, c):
    return None if c is None else u64_tensor(np.asarray(c, np.uint64), eng.device)


def _assert_tuples(got, exp, msg):
    for g, e, f in zip(got, exp, FIELDS):
        np.testing.assert_array_equal(g, e, err_msg=f"{msg} {f}")


def _check(eng, a, ca, b, cb, A=None, B=None, Ca=None, Cb=None, na_dev=None, nb_dev=None, swap=True):
    """Tuples, source indices, merged context and count == the restatement, the
    count-only call == the full call, either operand order gives equal tuples
    and contexts, no device flag.  Returns (tuples, src, kinds)."""
    A = TupleSet.from_numpy(*a, eng.device) if A is None else A
    B = TupleSet.from_numpy(*b, eng.device) if B is None else B
    Ca = _cdev(eng, ca) if Ca is None else Ca
    Cb = _cdev(eng, cb) if Cb is None else Cb
    exp, esrc, ectx, kinds = ref_causal(a, ca, b, cb)
    out, src, co, cnt = eng.causal_merge(A, Ca, B, Cb, n_a_dev=na_dev, n_b_dev=nb_dev, with_src=True)
    plain, co2, cnt2 = eng.causal_merge(A, Ca, B, Cb, n_a_dev=na_dev, n_b_dev=nb_dev)
    only = eng.causal_merge_count(A, Ca, B, Cb, n_a_dev=na_dev, n_b_dev=nb_dev)
    k = int(cnt.item())
    assert k == len(exp[0]), (k, len(exp[0]))
    assert int(only.item()) == k and int(cnt2.item()) == k
    got = out.slice(k).to_numpy()
    _assert_tuples(got, exp, "a, b")
    _assert_tuples(plain.slice(k).to_numpy(), exp, "a, b without src")
    gsrc = src[:k].cpu().numpy()
    np.testing.assert_array_equal(gsrc, esrc, err_msg="src")
    np.testing.assert_array_equal(as_u64(co), ectx, err_msg="ctx_out")
    np.testing.assert_array_equal(as_u64(co2), ectx, err_msg="ctx_out without src")
    if swap:
        rout, rco, rcnt = eng.causal_merge(B, Cb, A, Ca, n_a_dev=nb_dev, n_b_dev=na_dev)
        assert int(rcnt.item()) == k
        _assert_tuples(rout.slice(k).to_numpy(), exp, "b, a")
        np.testing.assert_array_equal(as_u64(rco), ectx, err_msg="ctx_out of b, a")
    assert eng.device_status(clear=True) == 0
    return got, gsrc, kinds


# ---- 1. random states: sizes x key spaces, both operand orders
SIZES = [1, 63, T - 1, T + 1, 3 * T + 5, 50_000]


@pytest.mark.parametrize("na", SIZES)
def test_random_states(eng, na):
    ca, cb = _ctx(1), _ctx(2)
    for ks in (8, 2**40):
        for nb in SIZES:
            a, b = _side(11, 0, na, ks), _side(11, 1, nb, ks)
            _, _, kinds = _check(eng, a, ca, b, cb)
            if min(na, nb) >= T - 1:                     # every case of the rule occurs, kept and dropped
                assert all(kinds[x] > 0 for x in KINDS), (na, nb, ks, kinds)


@pytest.mark.parametrize("n", SIZES)
def test_merge_with_itself(eng, n):
    for ks in (8, 2**40):
        a = _side(13, 1, n, ks)
        # (the obligation: a state's own context covers its present tags)
        own = np.full(64, 2**20, np.uint64)
        got, src, _ = _check(eng, a, own, a, own)
        _assert_tuples(got, present(a), "merge(A, A)")
        assert bool((src >= 0).all())


# ---- 2. hand-built edges
def _ordinary(n):
    """n single-tuple keys 10 i (distinct tags), every third tombstoned."""
    i = np.arange(n)
    return tup(10 * i, 1000 + i, i % 5, i % 3 == 0)


def _pick(t, idx):
    return tuple(np.ascontiguousarray(x[idx]) for x in t)


def _twin(n, p):
    """_ordinary(n) with tuple p + 1 a second copy of tuple p's tag."""
    key, ts, rep, tomb = _ordinary(n)
    key[p + 1], ts[p + 1], rep[p + 1] = key[p], ts[p], rep[p]
    return key, ts, rep, tomb


@pytest.mark.parametrize("edge", [64, WAVE, T])
def test_run_end_at_an_edge(eng, edge):
    """One tag of two a copies (and none / a live / a dead b copy) whose run ends
    one before, at and one after merged position `edge`; the other side's
    context covers the tag or not."""
    n = T + 40
    low, high = np.zeros(5, np.uint64), np.full(5, M64, np.uint64)
    for d in (-1, 0, 1):
        for in_b in (None, 0, 1):
            h = 0 if in_b is None else 1                 # b's copy is merged after a's two
            p = edge + d - 2 - h                         # the run's last item is merged item edge + d - 1
            for tombs in ((0, 0), (0, 1), (1, 0)):
                a = _twin(n, p)
                a[3][p:p + 2] = tombs
                tag = (int(a[0][p]), int(a[1][p]), int(a[2][p]))
                rest = _pick(_ordinary(n), np.arange(edge + 5, n, 3))   # (merged after the edge)
                b = rest if in_b is None else cat(rest, tup([tag[0]], [tag[1]], [tag[2]], [in_b]))
                for ca, cb in ((low, low), (high, high), (low, high), (high, low)):
                    got, src, _ = _check(eng, a, ca, b, cb, swap=False)
                    hit = np.flatnonzero((got[0] == tag[0]) & (got[1] == tag[1]) & (got[2] == tag[2]))
                    pa, pb = tombs == (0, 0), in_b == 0
                    want = (pa and pb) or (pa and cb is low) or (pb and ca is low)
                    assert len(hit) == (1 if want else 0), (edge, d, in_b, tombs)
                    if want:
                        assert int(src[hit[0]]) == (p if pa else -(int(np.flatnonzero(b[0] == tag[0])[0]) + 1))


def _long(na_c, nb_c, dead_a, dead_b):
    """One tag with na_c copies on a and nb_c on b between ordinary tuples; the
    copies at dead_a / dead_b (indices among the side's copies) tombstoned."""
    pre, post = _pick(_ordinary(60), np.arange(0, 20)), _pick(_ordinary(60), np.arange(40, 60))
    ta, tb = np.zeros(na_c, np.uint8), np.zeros(nb_c, np.uint8)
    ta[list(dead_a)] = 1
    tb[list(dead_b)] = 1
    a = cat(pre, tup(np.full(na_c, 300), np.full(na_c, 77), np.full(na_c, 2), ta), post)
    b = cat(_pick(pre, np.arange(0, 20, 2)), tup(np.full(nb_c, 300), np.full(nb_c, 77), np.full(nb_c, 2), tb))
    return a, b


def test_one_tag_across_many_tiles(eng):
    """2T + 100 copies on a, T + 7 on b: presence is decided by a copy three
    tiles before the run end; each side present only, both and neither."""
    low, high = np.zeros(3, np.uint64), np.full(3, 77, np.uint64)
    for dead_a, dead_b in (((), ()), ((5,), ()), ((), (3,)), ((0,), (T,)), ((2 * T + 99,), ()), ((), (T + 6,))):
        a, b = _long(2 * T + 100, T + 7, dead_a, dead_b)
        for ca, cb in ((low, low), (high, high), (low, high), (high, low)):
            got, src, _ = _check(eng, a, ca, b, cb)
            hit = np.flatnonzero(got[0] == 300)
            pa, pb = not dead_a, not dead_b
            want = (pa and pb) or (pa and cb is low) or (pb and ca is low)
            assert len(hit) == (1 if want else 0), (dead_a, dead_b)
            if want:                                     # the first copy on the present side, a before b
                assert int(src[hit[0]]) == (20 if pa else -(10 + 1))


def test_covered_boundaries(eng):
    """ts == ctx[rep] is covered, ctx[rep] + 1 is not; the compare is unsigned;
    a rep at or past n_ctx is never covered."""
    ctx = np.array([100, M64, 5, 2**63], np.uint64)
    one = tup([1, 2, 3, 4, 5, 6, 7, 8, 9, 10],
              [100, 101, M64, M64 - 1, 2**63, 2**63 + 1, 2**63, 0, 0, M64],
              [0, 0, 1, 1, 2, 3, 3, 4, 2**32 - 1, 0],
              np.zeros(10))
    keep = [2, 5, 6, 8, 9, 10]                           # keys of the uncovered tags
    for a, ca, b, cb in ((one, None, empty(), ctx), (empty(), ctx, one, None)):
        got, _, _ = _check(eng, a, ca, b, cb)
        np.testing.assert_array_equal(got[0], keep)
    got, _, _ = _check(eng, one, None, empty(), ctx[:0])  # an empty context covers nothing
    assert len(got[0]) == 10
    got, _, _ = _check(eng, one, None, empty(), ctx[:1])  # n_ctx == 1: rep 1 .. are past it
    np.testing.assert_array_equal(got[0], [2, 3, 4, 5, 6, 7, 8, 9, 10])


def test_context_lengths_differ(eng):
    a, b = _side(17, 0, 5000, 900), _side(17, 1, 4000, 900)
    full = _ctx(3)
    for la, lb in ((64, 0), (0, 64), (64, 17), (1, 64), (0, 0), (80, 64)):
        ca = None if la == 0 else np.resize(full, la)
        cb = None if lb == 0 else np.resize(full[::-1], lb)
        _check(eng, a, ca, b, cb)


def test_source_of_a_tag_dead_on_a(eng):
    """A tombstoned copy on a and the live one on b: b's copy is named, though
    a's is first in merged order."""
    a = tup([5, 7, 7, 9], [1, 4, 4, 1], [0, 3, 3, 0], [0, 0, 1, 0])
    b = tup([6, 7, 7], [1, 4, 4], [0, 3, 3], [1, 0, 0])
    got, src, _ = _check(eng, a, np.array([9], np.uint64), b, np.array([0, 0, 0, 9], np.uint64))
    # a's context stops before rep 3: b's live (7, 4, 3) stays; b's context covers none of a's rep-0 tags
    _assert_tuples(got, tup([5, 7, 9], [1, 4, 1], [0, 3, 0], [0, 0, 0]), "dead on a")
    np.testing.assert_array_equal(src, [0, -2, 3])
    got, src, _ = _check(eng, b, np.array([0, 0, 0, 9], np.uint64), a, np.array([9], np.uint64))
    np.testing.assert_array_equal(src, [-1, 1, -4])      # now a side: b's first live copy, index 1


def test_empty_sides(eng):
    a, ca, cb = _side(19, 0, 3000, 50), _ctx(4), _ctx(5)
    got, _, _ = _check(eng, a, ca, empty(), cb)
    assert 0 < len(got[0]) < len(present(a)[0])
    _check(eng, a, ca, empty(), None)
    got, _, _ = _check(eng, empty(), ca, empty(), cb)
    assert len(got[0]) == 0
    _check(eng, empty(), None, empty(), None)


# ---- 3. against code that already exists
@pytest.mark.parametrize("n", [T + 1, 50_000])
def test_against_compaction_under_a_full_cut(eng, n):
    """No other side and no context: a's present tags, which is what compaction
    keeps alive under a cut that makes every tombstone stable."""
    t = _side(23, 1, n, 700)
    Td = TupleSet.from_numpy(*t, eng.device)
    cut = u64_tensor(np.full(64, M64, np.uint64), eng.device)
    exp, ecnt = eng.set_compact(Td, False, cut)
    out, _, cnt = eng.causal_merge(Td, _cdev(eng, _ctx(6)), TupleSet.empty(0, eng.device), None)
    k = int(cnt.item())
    assert k == int(ecnt.item()) and 0 < k < n
    _assert_tuples(out.slice(k).to_numpy(), exp.slice(k).to_numpy(), "compact under a full cut")
    assert eng.device_status(clear=True) == 0


def _run_history(seed, steps, on_merge):
    h = History(seed)
    merges = 0
    for _ in range(steps):
        op, x, y = h.step()
        if op == "merge":
            merges += 1
            on_merge(h, x, y)
    return h, merges


def test_tombstone_form_replicas(eng):
    """Tombstone-form replicas with their clocks: the causal merge is the live
    tuples of the oracle's OR-Set merge."""
    seen = []

    def on_merge(h, x, y):
        merged = oracle.orset_merge(h.tomb[x], h.tomb[y])
        got, _, _ = _check(eng, h.tomb[x], h.clock[x], h.tomb[y], h.clock[y], swap=False)
        _assert_tuples(got, present(merged), "live tuples of the tombstone merge")
        seen.append(int(merged[3].sum()))
        h.tomb[x], h.clock[x] = merged, ctx_max(h.clock[x], h.clock[y])

    _, merges = _run_history(31, 300, on_merge)
    assert merges > 50 and max(seen) > 0


def test_history_in_causal_form(eng):
    """The same history kept in causal form by the GPU and in tombstone form by
    the oracle: equal set_elements at the merged replica after every merge."""
    def on_merge(h, x, y):
        A, B = TupleSet.from_numpy(*h.dots[x], eng.device), TupleSet.from_numpy(*h.dots[y], eng.device)
        out, ctx, cnt = eng.causal_merge(A, _cdev(eng, h.clock[x]), B, _cdev(eng, h.clock[y]))
        keys, kc = eng.set_elements(out, False, n_dev=cnt)
        h.tomb[x] = oracle.orset_merge(h.tomb[x], h.tomb[y])
        h.dots[x] = out.slice(int(cnt.item())).to_numpy()
        h.clock[x] = as_u64(ctx).copy()
        np.testing.assert_array_equal(as_u64(keys)[:int(kc.item())], live_keys(h.tomb[x]))
        _assert_tuples(h.dots[x], present(h.tomb[x]), "dots == live tags")

    h, merges = _run_history(37, 300, on_merge)
    assert merges > 50 and any(len(d[0]) for d in h.dots)
    assert eng.device_status(clear=True) == 0


# ---- 4. contracts
def test_count_only_writes_nothing_else(eng):
    a, b = _side(41, 0, 5000, 700), _side(41, 1, 5000, 700)
    A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
    Ca, Cb = _cdev(eng, _ctx(1)), _cdev(eng, _ctx(2))
    cnt = torch.full((3,), 0x5a5a, dtype=torch.int64, device=eng.device)
    eng.causal_merge_count(A, Ca, B, Cb, count=cnt[1:2])
    exp = ref_causal(a, _ctx(1), b, _ctx(2))[0]
    assert cnt.cpu().tolist() == [0x5a5a, len(exp[0]), 0x5a5a]
    for t, ref in ((A, a), (B, b)):
        _assert_tuples(t.to_numpy(), ref, "inputs untouched")
    assert eng.device_status(clear=True) == 0


def test_map_merge_moves_the_named_values(eng):
    a, b = _side(43, 0, 5000, 700), _side(43, 1, 6000, 700)
    A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
    ca, cb = _ctx(1), _ctx(2)
    exp, esrc, _, _ = ref_causal(a, ca, b, cb)
    k = len(exp[0])
    for dtype, width in ((torch.int32, None), (torch.int32, 4)):    # 4-byte and 16-byte values
        shape = lambda n: (n,) if width is None else (n, width)
        va = torch.arange(int(np.prod(shape(len(a[0])))), dtype=dtype, device=eng.device).reshape(shape(len(a[0]))) * 3 + 1
        vb = -torch.arange(int(np.prod(shape(len(b[0])))), dtype=dtype, device=eng.device).reshape(shape(len(b[0]))) - 7
        out, val, _, cnt = eng.causal_map_merge(A, va, _cdev(eng, ca), B, vb, _cdev(eng, cb))
        assert int(cnt.item()) == k
        _assert_tuples(out.slice(k).to_numpy(), exp, "map merge")
        ha, hb = va.cpu().numpy(), vb.cpu().numpy()
        want = np.where((esrc >= 0).reshape((-1,) + (1,) * (ha.ndim - 1)), ha[np.maximum(esrc, 0)],
                        hb[np.maximum(-(esrc + 1), 0)])
        np.testing.assert_array_equal(val.cpu().numpy()[:k], want)
    assert eng.device_status(clear=True) == 0


def test_chained_off_device_counts(eng):
    """The merge's output, its capacity filled with tuples that would survive,
    merged again under its device count: nothing is read back in between."""
    a, b, c = _side(47, 0, 5000, 700), _side(47, 1, 5000, 700), _side(48, 1, 3000, 700)
    A, B, Cc = (TupleSet.from_numpy(*x, eng.device) for x in (a, b, c))
    ca, cb, cc = _ctx(1), _ctx(2), _ctx(3)
    cap = len(a[0]) + len(b[0])
    out = TupleSet.empty(cap, eng.device)
    out.key.fill_(-1)                                    # live, uncovered sentinels past the count
    out.ts.fill_(-1)
    out.rep.fill_(-1)
    out.tomb.fill_(0)
    _, ctx1, cnt1 = eng.causal_merge(A, _cdev(eng, ca), B, _cdev(eng, cb), out=out)
    out2, ctx2, cnt2 = eng.causal_merge(out, ctx1, Cc, _cdev(eng, cc), n_a_dev=cnt1)
    only = eng.causal_merge_count(Cc, _cdev(eng, cc), out, ctx1, n_b_dev=cnt1)
    m1, _, e1, _ = ref_causal(a, ca, b, cb)
    m2, _, e2, _ = ref_causal(m1, e1, c, cc)
    assert int(cnt1.item()) == len(m1[0]) < cap
    k = int(cnt2.item())
    assert k == len(m2[0]) == int(only.item())
    _assert_tuples(out2.slice(k).to_numpy(), m2, "chained")
    np.testing.assert_array_equal(as_u64(ctx2), e2)
    assert eng.device_status(clear=True) == 0


@pytest.mark.parametrize("bad", [5001, M64])
@pytest.mark.parametrize("on_a", [True, False])
def test_device_count_out_of_range(eng, bad, on_a):
    a, b = _side(9, 0, 5000, 700), _side(9, 1, 5000, 700)
    A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
    ca, cb = _ctx(1), _ctx(2)
    Ca, Cb = _cdev(eng, ca), _cdev(eng, cb)
    kw = {"n_a_dev" if on_a else "n_b_dev": _dev(eng, bad)}
    assert eng.device_status(clear=True) == 0
    out = TupleSet.empty(10_000, eng.device)
    src = torch.full((10_000,), 0x5a5a, dtype=torch.int64, device=eng.device)
    ctx_out = torch.full((64,), -1, dtype=torch.int64, device=eng.device)
    for x in (out.key, out.ts, out.rep, out.tomb):
        x.fill_(0x5a)
    _, _, _, cnt = eng.causal_merge(A, Ca, B, Cb, out=out, src=src, ctx_out=ctx_out, **kw)
    assert as_u64(cnt)[0] == M64
    assert eng.device_status(clear=True) & DEV_RANGE
    assert all(bool((x == 0x5a).all()) for x in (out.key, out.ts, out.rep, out.tomb))
    assert bool((src == 0x5a5a).all())
    np.testing.assert_array_equal(as_u64(ctx_out), ctx_max(ca, cb))      # the contexts alone decide it
    only = eng.causal_merge_count(A, Ca, B, Cb, **kw)
    assert as_u64(only)[0] == M64
    assert eng.device_status(clear=True) & DEV_RANGE
    _check(eng, a, ca, b, cb, A=A, B=B, Ca=Ca, Cb=Cb)    # the next calls are exact
    _check(eng, a, ca, b, cb, A=A, B=B, na_dev=_dev(eng, 5000), nb_dev=_dev(eng, 5000))   # a count AT the capacity
    for na, nb in ((3000, 5000), (5000, 1234), (2047, 1), (0, 5000), (5000, 0), (0, 0)):  # a shorter count reads that prefix
        _check(eng, tuple(x[:na] for x in a), ca, tuple(x[:nb] for x in b), cb, A=A, B=B, na_dev=_dev(eng, na),
               nb_dev=_dev(eng, nb))


@pytest.mark.parametrize("off", [1, 3])
def test_offset_views(eng, off):
    """Every field of every operand, and both contexts, at an odd element offset."""
    fa, fb = _side(51, 0, 20_000, 9_000), _side(51, 1, 20_000, 9_000)
    FA, FB = TupleSet.from_numpy(*fa, eng.device), TupleSet.from_numpy(*fb, eng.device)
    ca, cb = _ctx(1), _ctx(2)
    Pa = u64_tensor(np.concatenate([np.full(off, M64, np.uint64), ca]), eng.device)
    Pb = u64_tensor(np.concatenate([np.full(off + 2, M64, np.uint64), cb]), eng.device)
    view = lambda t, o: TupleSet(t.key[o:], t.ts[o:], t.rep[o:], t.tomb[o:])
    a, b = tuple(x[off:] for x in fa), tuple(x[off + 2:] for x in fb)
    _check(eng, a, ca, b, cb, A=view(FA, off), B=view(FB, off + 2), Ca=Pa[off:], Cb=Pb[off + 2:])
    n = len(a[0]) + len(b[0])
    out, src = TupleSet.empty(n + 8, eng.device), torch.empty(n + 8, dtype=torch.int64, device=eng.device)
    ctx_out = torch.empty(64 + 8, dtype=torch.int64, device=eng.device)
    o = TupleSet(out.key[off:off + n], out.ts[off:off + n], out.rep[off:off + n], out.tomb[off:off + n])
    _, s, co, cnt = eng.causal_merge(view(FA, off), Pa[off:], view(FB, off + 2), Pb[off + 2:], out=o,
                                     src=src[off:off + n], ctx_out=ctx_out[off:off + 64])
    exp, esrc, ectx, _ = ref_causal(a, ca, b, cb)
    k = int(cnt.item())
    _assert_tuples(tuple(x[:k] for x in o.to_numpy()), exp, "offset outputs")
    np.testing.assert_array_equal(s.cpu().numpy()[:k], esrc)
    np.testing.assert_array_equal(as_u64(co), ectx)
    assert eng.device_status(clear=True) == 0


def test_host_errors(eng):
    a, b = _side(3, 0, 1000, 100), _side(3, 1, 1000, 100)
    A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
    O = TupleSet.empty(2000, eng.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=eng.device)
    src = torch.zeros(2000, dtype=torch.int64, device=eng.device)
    Ca, Cb = _cdev(eng, _ctx(1)), _cdev(eng, _ctx(2))
    Co = torch.zeros(64, dtype=torch.int64, device=eng.device)
    ca, cb, co, cp, sp = A.c(), B.c(), O.c(), cnt.data_ptr(), src.data_ptr()
    xa, xb, xo = Ca.data_ptr(), Cb.data_ptr(), Co.data_ptr()
    ref = lambda x: C.byref(x) if x is not None else None

    def raw(ta, tb, o, s, count, na=1000, nb=1000, pa=xa, pb=xb, la=64, lb=64, po=xo, nad=None, nbd=None):
        eng._bind()
        with pytest.raises(_lib.CrdtError) as ei:
            _lib.call("crdt_orset_merge_causal", eng.ctx, ref(ta), na, nad, pa, la, ref(tb), nb, nbd, pb, lb, ref(o), s,
                      po, count, ctx=eng.ctx)
        return ei.value.status

    def fld(t, **kw):
        f = {"key": t.key.data_ptr(), "ts": t.ts.data_ptr(), "rep": t.rep.data_ptr(), "tomb": t.tomb.data_ptr()}
        f.update(kw)
        return _lib.crdt_tuples(f["key"], f["ts"], f["rep"], f["tomb"])

    with pytest.raises(_lib.CrdtError) as ei:               # NULL ctx
        _lib.call("crdt_orset_merge_causal", None, C.byref(ca), 1000, None, xa, 64, C.byref(cb), 1000, None, xb, 64,
                  None, None, None, cp)
    assert ei.value.status == E_INVAL
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
    assert raw(ca, cb, None, None, cp, pb=None) == E_INVAL
    assert raw(ca, cb, None, None, cp, pa=xa + 4) == E_INVAL   # contexts, lengths, src, ctx_out misaligned
    assert raw(ca, cb, None, None, cp, pb=xb + 4) == E_INVAL
    assert raw(ca, cb, None, None, cp, po=xo + 4) == E_INVAL
    assert raw(ca, cb, None, None, cp, nad=cp + 4) == E_INVAL
    assert raw(ca, cb, None, None, cp, nbd=cp + 4) == E_INVAL
    assert raw(ca, cb, co, sp + 4, cp) == E_INVAL
    assert raw(ca, cb, None, sp, cp) == E_INVAL             # source indices without out
    assert raw(ca, cb, ca, None, cp) == E_INVAL             # out overlapping a, b, a context, src, ctx_out
    assert raw(ca, cb, cb, None, cp) == E_INVAL
    assert raw(ca, cb, fld(O, ts=B.ts.data_ptr() + 8 * 999), None, cp) == E_INVAL    # ... its last element
    assert raw(ca, cb, fld(O, tomb=A.key.data_ptr() + 8 * 999 + 7), None, cp) == E_INVAL
    assert raw(ca, cb, fld(O, key=xa + 8 * 63), None, cp) == E_INVAL
    assert raw(ca, cb, fld(O, key=xb + 8 * 63), None, cp) == E_INVAL
    assert raw(ca, cb, fld(O, key=sp), sp, cp) == E_INVAL
    assert raw(ca, cb, fld(O, ts=xo), None, cp) == E_INVAL
    assert raw(ca, cb, co, A.ts.data_ptr(), cp) == E_INVAL  # src overlapping a, b, a context, ctx_out
    assert raw(ca, cb, co, B.key.data_ptr(), cp) == E_INVAL
    assert raw(ca, cb, co, xb, cp) == E_INVAL
    assert raw(ca, cb, co, xo, cp) == E_INVAL
    assert raw(ca, cb, None, None, cp, po=xa) == E_INVAL    # ctx_out overlapping a context, a side
    assert raw(ca, cb, None, None, cp, po=xb + 8 * 63) == E_INVAL
    assert raw(ca, cb, None, None, cp, po=A.key.data_ptr()) == E_INVAL
    assert raw(ca, cb, None, None, cp, na=2**62) == E_RANGE
    assert raw(ca, cb, None, None, cp, nb=2**62) == E_RANGE
    assert raw(ca, cb, None, None, cp, na=2**61, nb=2**61, po=None) == E_RANGE   # more tiles than a launch holds
    assert raw(ca, cb, None, None, cp, la=2**32) == E_RANGE
    assert raw(ca, cb, None, None, cp, lb=2**32) == E_RANGE
    assert int(cnt.item()) == 0 and eng.device_status(clear=True) == 0
    cnt.fill_(77)                                           # no tuples: the count store and the ctx_out write alone
    Co.fill_(-1)
    eng._bind()
    none = _lib.crdt_tuples(None, None, None, None)
    _lib.call("crdt_orset_merge_causal", eng.ctx, C.byref(none), 0, None, xa, 64, C.byref(none), 0, None, None, 0, None,
              None, xo, cp, ctx=eng.ctx)
    assert int(cnt.item()) == 0
    np.testing.assert_array_equal(as_u64(Co), _ctx(1))
    with pytest.raises(ValueError):
        eng.causal_merge(A, Ca, B, Cb, out=TupleSet.empty(1999, eng.device))
    _check(eng, a, _ctx(1), b, _ctx(2), A=A, B=B, Ca=Ca, Cb=Cb)


def test_graph_capture(eng):
    """One linear capture of the merge and a gather after a reserve, replayed
    over changed inputs."""
    a, b = _side(53, 0, 5000, 700), _side(53, 1, 4000, 700)
    A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
    n = len(a[0]) + len(b[0])
    Ca, Cb = _cdev(eng, _ctx(1)), _cdev(eng, _ctx(2))
    va = torch.arange(len(a[0]), dtype=torch.int64, device=eng.device) * 5 + 2
    vb = -torch.arange(len(b[0]), dtype=torch.int64, device=eng.device) - 9
    eng.reserve(1 << 20)
    g_out, g_src = TupleSet.empty(n, eng.device), torch.empty(n, dtype=torch.int64, device=eng.device)
    g_cnt, g_val = torch.zeros(1, dtype=torch.int64, device=eng.device), torch.empty(n, dtype=torch.int64, device=eng.device)
    g_ctx = torch.empty(64, dtype=torch.int64, device=eng.device)
    eng.causal_merge(A, Ca, B, Cb, out=g_out, src=g_src, ctx_out=g_ctx, count=g_cnt)   # eager: warm
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        eng.causal_merge(A, Ca, B, Cb, out=g_out, src=g_src, ctx_out=g_ctx, count=g_cnt)
        eng.gather_src(g_src, va, vb, n_dev=g_cnt, out=g_val)
    ha, hb = va.cpu().numpy(), vb.cpu().numpy()
    for rep, (sa, sb) in enumerate(((1, 2), (7, 8), (2, 1))):
        ca, cb = _ctx(sa), _ctx(sb)
        Ca.copy_(u64_tensor(ca, eng.device))             # the contexts change between replays ...
        Cb.copy_(u64_tensor(cb, eng.device))
        a2 = (a[0], a[1], a[2], np.roll(a[3], rep))      # ... and which of a's tuples are tombstoned
        A.tomb.copy_(torch.from_numpy(a2[3].copy()).to(eng.device))
        for x in (g_out.key, g_out.ts, g_out.rep, g_out.tomb, g_val, g_cnt, g_ctx):
            x.fill_(0)
        g.replay()
        torch.cuda.synchronize()
        exp, esrc, ectx, _ = ref_causal(a2, ca, b, cb)
        k = len(exp[0])
        assert int(as_u64(g_cnt)[0]) == k
        _assert_tuples(tuple(x[:k] for x in g_out.to_numpy()), exp, f"replay {rep}")
        np.testing.assert_array_equal(as_u64(g_ctx), ectx)
        want = np.where(esrc >= 0, ha[np.maximum(esrc, 0)], hb[np.maximum(-(esrc + 1), 0)])
        np.testing.assert_array_equal(g_val.cpu().numpy()[:k], want, err_msg=f"replay {rep} values")
    assert eng.device_status(clear=True) == 0
