"""GPU: counter-map state from increment logs (crdt_cmap_combine / _add /
_from_ops and Engine.cmap_ingest; csrc/countermap.hpp, entry points in
csrc/counters.hip) against the two CPU restatements of
tests/cmap_ingest_util.py, bit for bit, with the device status 0 after every
exact call.

A tile of the combine is T = 2048 cells, a word 64 and a wave 512; a tile of
the add is T items of the stable merged order.  The hand-built cases put runs
of equal (key, rep) on and across those edges and assert on the CPU that they
lie where they are meant to before the GPU runs."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmap_ingest_util as iu
import cmap_util as cu
import test_gpu_cmap as t_cmap
from crdt_amd import _lib
from crdt_amd.engine import CounterMap, as_u64, u64_tensor

pytestmark = pytest.mark.gpu

T = t_cmap.T
DEV_RANGE, E_INVAL, E_RANGE, M64 = t_cmap.DEV_RANGE, t_cmap.E_INVAL, t_cmap.E_RANGE, t_cmap.M64
U64, U32 = np.uint64, np.uint32
_dev, _up, _cut, _n, _take, _eq = t_cmap._dev, t_cmap._up, t_cmap._cut, t_cmap._n, t_cmap._take, t_cmap._eq


# ---------------------------------------------------------------- helpers
def _u32(eng, x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=U32).view(np.int32).copy()).to(eng.device)


def _ops(eng, ops):
    return u64_tensor(ops[0], eng.device), _u32(eng, ops[1]), u64_tensor(ops[2], eng.device), u64_tensor(ops[3], eng.device)


def check_combine(eng, t, n=None, idx=None, src=None, what="combine", bad_idx=False):
    """t: sorted cells with repeats; idx / src: the indexed form (src = the p and n columns)."""
    assert iu.is_sorted(_cut(t, len(t[0]) if n is None else n))
    if idx is None:
        Tt = _up(eng, t)
    else:
        Tt = CounterMap(u64_tensor(t[0], eng.device), _u32(eng, t[1]), u64_tensor(src[0], eng.device),
                        u64_tensor(src[1], eng.device))
    kw = dict(n_dev=None if n is None else _dev(eng, n), idx=None if idx is None else _u32(eng, idx))
    et = t if n is None else _cut(t, n)
    exp = iu.combine_np(et, None if idx is None else idx[:len(et[0])], src)
    if len(et[0]) <= 64:
        _eq(iu.combine_d(et, None if idx is None else idx[:len(et[0])], src), exp, what + ": the restatements")
    assert cu.is_state(exp)
    cap, k = len(t[0]), len(exp[0])
    given = CounterMap.empty(max(cap, 1), eng.device)
    for x in (given.key, given.rep, given.p, given.n):
        x.fill_(0x5a)
    gc = torch.full((1,), -5, dtype=torch.int64, device=eng.device)
    out, cnt = eng.cmap_combine(Tt, out=given, count=gc, **kw)
    assert out is given and cnt is gc
    _eq(_take(given, gc), exp, what + " (given outputs)")
    assert all(bool((x[k:] == 0x5a).all()) for x in (given.key, given.rep, given.p, given.n)), what + ": cells past the count"
    status = eng.device_status(clear=True)
    assert (status & DEV_RANGE) if bad_idx else status == 0, what
    out, cnt = eng.cmap_combine(Tt, **kw)
    _eq(_take(out, cnt), exp, what)
    if not bad_idx:
        out, cnt = eng.cmap_combine(Tt, trim=True, **kw)
        assert len(out) == k and _n(cnt) == k
        _eq(out.to_numpy(), exp, what + " (trim)")
    assert _n(eng.cmap_combine_count(Tt, n_dev=kw["n_dev"])) == k, what + " (count alone)"
    eng.device_status(clear=True)
    return exp


def check_add(eng, t, d, nt=None, nd=None, what="add"):
    Tt, D = _up(eng, t), _up(eng, d)
    kw = dict(n_t_dev=None if nt is None else _dev(eng, nt), n_d_dev=None if nd is None else _dev(eng, nd))
    et, ed = (t if nt is None else _cut(t, nt)), (d if nd is None else _cut(d, nd))
    exp = iu.add_np(et, ed)
    if len(exp[0]) <= 64:
        _eq(iu.add_d(et, ed), exp, what + ": the restatements")
    t_cmap._two_sided(eng, lambda **k: eng.cmap_add(Tt, D, **kw, **k), lambda: eng.cmap_add_count(Tt, D, **kw), exp,
                      len(Tt) + len(D), what)
    return exp


def check_from_ops(eng, ops, what="from_ops"):
    exp = iu.from_ops_np(ops)
    if len(ops[0]) <= 64:
        _eq(iu.from_ops_d(ops), exp, what + ": the restatements")
    assert cu.is_state(exp)
    m, k = len(ops[0]), len(exp[0])
    dev = _ops(eng, ops)
    out, cnt = eng.cmap_from_ops(*dev)
    _eq(_take(out, cnt), exp, what)
    given = CounterMap.empty(max(m, 1), eng.device)
    for x in (given.key, given.rep, given.p, given.n):
        x.fill_(0x5a)
    out, cnt = eng.cmap_from_ops(*dev, out=given)
    assert out is given
    _eq(_take(given, cnt), exp, what + " (given out)")
    assert all(bool((x[k:] == 0x5a).all()) for x in (given.key, given.rep, given.p, given.n)), what + ": cells past the count"
    out, cnt = eng.cmap_from_ops(*dev, trim=True)
    assert len(out) == k
    _eq(out.to_numpy(), exp, what + " (trim)")
    for got, was in zip(dev, ops):                        # the log itself is not written
        assert np.array_equal(got.cpu().numpy().view(was.dtype), was), what
    assert eng.device_status(clear=True) == 0, what
    return exp


def _cells(n, seed=0):
    """n distinct ascending cells, 1 to 3 replicas a key, amounts below 2^40."""
    rng = np.random.default_rng(seed + n)
    i = np.arange(n, dtype=np.int64)
    key = (i // 3 * 5 + 2).astype(U64)
    rep = (i % 3 * 2 + 1).astype(U32)
    t = key, rep, rng.integers(0, 1 << 40, size=n, dtype=U64), rng.integers(0, 1 << 40, size=n, dtype=U64)
    assert cu.is_state(t)
    return t


def _run_log(lengths, wrap=False):
    """One run of equal (key, rep) per entry of lengths, three replicas a key."""
    lengths = np.asarray(lengths)
    r = np.repeat(np.arange(len(lengths)), lengths)
    i = np.arange(len(r), dtype=U64)
    p = i * U64(2654435761) % U64(1 << 40) + U64(1)
    if wrap:
        p = U64(M64) - i * U64(977)
    t = (r // 3).astype(U64) * U64(3) + U64(1), (r % 3).astype(U32), p, (i * U64(40503) + U64(7)) % U64(1 << 41)
    assert iu.is_sorted(t)
    return t


# ---------------------------------------------------------------- 1. known answers and witnesses
def test_known_answers(eng):
    ops = iu.log([5, 3, 5, 3, 5, 9], [1, 0, 1, 2, 0, 1], [1, 2, 10, 4, 7, 0], [0, 1, 2, 0, 0, 0])
    exp = cu.state([3, 3, 5, 5, 9], [0, 2, 0, 1, 1], [2, 4, 7, 11, 0], [1, 0, 0, 2, 0])
    _eq(check_from_ops(eng, ops), exp, "from_ops, typed out")            # (9, 1): zero sums keep the cell
    _eq(check_combine(eng, iu.sorted_log(ops)), exp, "combine, typed out")
    t = cu.state([3, 5, 7], [0, 1, 0], [1, 1, 1], [5, 5, 5])
    d = cu.state([3, 5, 8], [0, 0, 2], [2, 3, 0], [1, 0, 0])
    _eq(check_add(eng, t, d), cu.state([3, 5, 5, 7, 8], [0, 0, 1, 0, 2], [3, 3, 1, 1, 0], [6, 0, 5, 5, 0]), "add, typed out")


def test_unsigned_witnesses(eng):
    big = 2**63
    # a signed order would put key 2^63 + 1 before key 1 and rep 2^31 + 5 before rep 3; (2^64 - 1) + 2 = 1
    ops = iu.log([big + 1, 1, 1, big + 1, 1, 1], [0, 2**31 + 5, 3, 0, 3, 2**31 + 5], [M64, 2, 3, 2, 4, big],
                 [big, 0, 0, big, 0, big])
    exp = cu.state([1, 1, big + 1], [3, 2**31 + 5, 0], [7, big + 2, 1], [0, big, 0])
    _eq(check_from_ops(eng, ops), exp, "from_ops")
    srt = iu.sorted_log(ops)
    assert srt[0].tolist() == [1, 1, 1, 1, big + 1, big + 1] and srt[1].tolist() == [3, 3, 2**31 + 5, 2**31 + 5, 0, 0]
    _eq(check_combine(eng, srt), exp, "combine")
    t = cu.state([1, big + 1], [2**31 + 5, 0], [big - 2, M64], [big, 5])
    _eq(check_add(eng, t, exp), cu.state([1, 1, big + 1], [3, 2**31 + 5, 0], [7, 0, 0], [0, 0, 5]), "add")


# ---------------------------------------------------------------- 2. edge lengths
EDGE_LENGTHS = [0, 1, 2, 63, 64, 65, 511, 512, 513, T - 1, T, T + 1, 2 * T + 17]


@pytest.mark.parametrize("n", EDGE_LENGTHS)
def test_edge_lengths(eng, n):
    t = _cells(n)
    _eq(check_combine(eng, t, what=f"distinct n={n}"), t, "combine of a state is the identity")
    r = _cut(iu.expand(_cells((n + 2) // 3, seed=1), 3), n)
    exp = check_combine(eng, r, what=f"runs of 3 n={n}")
    assert len(exp[0]) == (n + 2) // 3


# ---------------------------------------------------------------- 3. runs across boundaries
def _one_long(start, length, tail=40):
    return [1] * start + [length] + [1] * tail, (start, start + length)


RUN_SHAPES = {
    "across 63/64": _one_long(62, 4),
    "across 511/512": _one_long(510, 4),
    "across T-1/T": _one_long(T - 2, 4),
    "ending at T-1": _one_long(T - 5, 5),
    "beginning at T": _one_long(T, 5),
    "3T+5 cells from mid-tile": _one_long(1000, 3 * T + 5),
    "the whole input": ([2 * T + 100], (0, 2 * T + 100)),
    "runs of T on the tile grid": ([T, T, 1, T - 1, 17], (0, T)),
}


@pytest.mark.parametrize("name", sorted(RUN_SHAPES))
def test_runs_across_boundaries(eng, name):
    lengths, (lo, hi) = RUN_SHAPES[name]
    t = _run_log(lengths, wrap=name == "the whole input")
    cell = lambda i: (int(t[0][i]), int(t[1][i]))         # noqa: E731
    # the CPU side: the run lies where it is meant to
    assert cell(lo) == cell(hi - 1) and (lo == 0 or cell(lo - 1) != cell(lo)) and (hi == len(t[0]) or cell(hi) != cell(hi - 1))
    exp = check_combine(eng, t, what=name)
    assert len(exp[0]) == len(lengths)
    if name == "the whole input":                          # the partial sums wrapped
        assert sum(int(x) for x in t[2]) > 2**64 and int(exp[2][0]) == sum(int(x) for x in t[2]) % 2**64
    idx = np.random.default_rng(3).permutation(len(t[0])).astype(U32)    # the same runs through the gather
    src = (np.empty_like(t[2]), np.empty_like(t[3]))
    src[0][idx], src[1][idx] = t[2], t[3]
    _eq(check_combine(eng, t, idx=idx, src=src, what=name + " (idx)"), exp, "idx form")


def test_tile_edge_decided_by_one_column(eng):
    i = np.arange(2 * T + 9)
    # same key, another rep at T - 1 | T: a head by rep alone
    by_rep = (((i + 2) // 4).astype(U64), ((i + 2) % 4).astype(U32), (i * 3 + 1).astype(U64), (i % 7).astype(U64))
    assert by_rep[0][T - 1] == by_rep[0][T] and by_rep[1][T - 1] != by_rep[1][T] and cu.is_state(by_rep)
    _eq(check_combine(eng, by_rep, what="a head by rep alone"), by_rep, "identity")
    # same rep, another key at T - 1 | T, runs of two elsewhere
    by_key = ((i // 2).astype(U64), np.full(len(i), 7, U32), (i * 5 + 2).astype(U64), (i % 3).astype(U64))
    assert by_key[0][T - 1] != by_key[0][T] and by_key[0][T - 2] == by_key[0][T - 1] and by_key[0][T] == by_key[0][T + 1]
    exp = check_combine(eng, by_key, what="a head by key alone")
    assert len(exp[0]) == T + 5
    # ... and a run of two across the edge in each form: no head at T
    shifted = tuple(c[1:] for c in by_key)
    assert shifted[0][T - 1] == shifted[0][T]
    check_combine(eng, shifted, what="no head at T")
    same_rep_run = (((i + 1) // 4).astype(U64), ((i + 1) % 4 // 2).astype(U32), by_rep[2], by_rep[3])
    assert (same_rep_run[0][T - 1], same_rep_run[1][T - 1]) == (same_rep_run[0][T], same_rep_run[1][T])
    check_combine(eng, same_rep_run, what="no head at T (runs of two by rep)")


# ---------------------------------------------------------------- 4. the idx form
def test_idx_forms(eng):
    ops = iu.random_log(np.random.default_rng(4), 3 * T + 17, 500, big=True)
    order = np.lexsort((ops[1], ops[0]))
    srt = iu.perm(ops, order)
    exp = iu.from_ops_np(ops)
    n = len(order)
    ident = np.arange(n, dtype=U32)
    _eq(check_combine(eng, srt, idx=ident, src=(srt[2], srt[3]), what="identity"), exp, "identity")
    rev = ident[::-1].copy()
    _eq(check_combine(eng, srt, idx=rev, src=(srt[2][::-1].copy(), srt[3][::-1].copy()), what="reversed"), exp, "reversed")
    _eq(check_combine(eng, srt, idx=order.astype(U32), src=(ops[2], ops[3]), what="the sort's permutation"), exp, "perm")
    # a source longer than the cells: only the indexed elements count
    long_src = (np.concatenate([ops[2], ops[2]]), np.concatenate([ops[3], ops[3]]))
    _eq(check_combine(eng, srt, idx=(order + n).astype(U32), src=long_src, what="a longer source"), exp, "longer source")
    # with a device length below the buffer
    check_combine(eng, t_cmap._poisoned(srt, 2 * T + 5), n=2 * T + 5, idx=order.astype(U32), src=(ops[2], ops[3]),
                  what="idx with a device length")


@pytest.mark.parametrize("bad", [3 * T + 17, 2**32 - 1])
def test_idx_out_of_range_contributes_zero(eng, bad):
    ops = iu.random_log(np.random.default_rng(5), 3 * T + 17, 500)
    order = np.lexsort((ops[1], ops[0]))
    srt = iu.perm(ops, order)
    idx = order.astype(U32)
    for at in (0, T - 1, T, 3 * T + 16):
        idx[at] = bad
    assert eng.device_status(clear=True) == 0
    got = check_combine(eng, srt, idx=idx, src=(ops[2], ops[3]), what=f"idx {bad}", bad_idx=True)
    exact = iu.from_ops_np(ops)
    assert np.array_equal(got[0], exact[0]) and np.array_equal(got[1], exact[1])
    assert 0 < int((got[2] != exact[2]).sum()) <= 4       # every other cell is still exact
    check_combine(eng, srt, idx=order.astype(U32), src=(ops[2], ops[3]), what="the next call is exact")


# ---------------------------------------------------------------- 5. device lengths and refusals
def test_device_lengths_below_the_buffer(eng):
    t = _cut(iu.expand(_cells(2100, seed=2), 3), 6161)
    for n in (0, 1, 2047, 2048, 2049, 4101, 6161):
        check_combine(eng, t_cmap._poisoned(t, n), n=n, what=f"n_dev={n}")
    a, b = t_cmap._pair(6161, 6161, seed=3)
    for na, nb in ((4101, 4001), (0, 4001), (4101, 0), (6161, 6161), (1, 1)):
        check_add(eng, t_cmap._poisoned(a, na), t_cmap._poisoned(b, nb), nt=na, nd=nb, what=f"add {na}, {nb}")


@pytest.mark.parametrize("bad", [6162, M64])
def test_device_length_out_of_range(eng, bad):
    a, b = t_cmap._pair(6161, 6161, seed=3)
    A, B = _up(eng, a), _up(eng, b)
    assert eng.device_status(clear=True) == 0

    def fresh(n):
        out = CounterMap.empty(n, eng.device)
        for x in (out.key, out.rep, out.p, out.n):
            x.fill_(0x5a)
        return out

    def untouched(out):
        return all(bool((x == 0x5a).all()) for x in (out.key, out.rep, out.p, out.n))

    out = fresh(6161)
    _, cnt = eng.cmap_combine(A, n_dev=_dev(eng, bad), out=out)
    assert _n(cnt) == M64 and eng.device_status(clear=True) & DEV_RANGE and untouched(out)
    _, cnt = eng.cmap_combine(A, n_dev=_dev(eng, bad), idx=_u32(eng, np.arange(6161)), out=out)
    assert _n(cnt) == M64 and eng.device_status(clear=True) & DEV_RANGE and untouched(out)
    assert _n(eng.cmap_combine_count(A, n_dev=_dev(eng, bad))) == M64 and eng.device_status(clear=True) & DEV_RANGE
    for side in ("n_t_dev", "n_d_dev"):
        out = fresh(12322)
        _, cnt = eng.cmap_add(A, B, out=out, **{side: _dev(eng, bad)})
        assert _n(cnt) == M64 and eng.device_status(clear=True) & DEV_RANGE and untouched(out)
        assert _n(eng.cmap_add_count(A, B, **{side: _dev(eng, bad)})) == M64 and eng.device_status(clear=True) & DEV_RANGE
    check_combine(eng, a, what="the next calls are exact")
    check_add(eng, a, b)


def test_device_counts_chain_with_no_read_back(eng):
    ops = iu.random_log(np.random.default_rng(6), 3 * T + 17, 700)
    srt = iu.sorted_log(ops)
    st = iu.from_ops_np(ops)
    comb, cnt = eng.cmap_combine(_up(eng, srt))            # the combine's count is the read's length
    keys, P, N, value, kc = eng.cmap_values(comb, n_dev=cnt)
    exp = cu.values_np(st)
    k = _n(kc)
    _eq((as_u64(keys)[:k], as_u64(P)[:k], as_u64(N)[:k], value.cpu().numpy()[:k]), exp, "combine -> values")
    t = cu.random_state(np.random.default_rng(7), 2000, 700, reps=4)
    t = (t[0] * U64(7) + U64(3), t[1], t[2], t[3])
    out, oc = eng.cmap_add(_up(eng, t), comb, n_d_dev=cnt)  # ... and the add's batch length
    _eq(_take(out, oc), iu.add_np(t, st), "combine -> add")
    again, ac = eng.cmap_combine(out, n_dev=oc)            # a state combines to itself
    _eq(_take(again, ac), iu.add_np(t, st), "add -> combine")
    assert eng.device_status(clear=True) == 0


def test_host_errors(eng):
    a = _cells(1000)
    A, O = _up(eng, a), CounterMap.empty(2000, eng.device)
    B = _up(eng, _cells(1000, seed=5))
    cnt = torch.zeros(1, dtype=torch.int64, device=eng.device)
    idx = _u32(eng, np.arange(1000))
    ops = _ops(eng, a)
    ca, cb, co, cp = A.c(), B.c(), O.c(), cnt.data_ptr()
    ref = lambda x: C.byref(x) if x is not None else None   # noqa: E731

    def cm(t, **kw):
        f = {"key": t.key.data_ptr(), "rep": t.rep.data_ptr(), "p": t.p.data_ptr(), "n": t.n.data_ptr()}
        f.update(kw)
        return _lib.crdt_cmap(f["key"], f["rep"], f["p"], f["n"])

    def status(fn, *args):
        eng._bind()
        with pytest.raises(_lib.CrdtError) as ei:
            _lib.call(fn, eng.ctx, *args, ctx=eng.ctx)
        return ei.value.status

    def combine(t, o, count, n=1000, ix=None, n_src=0):
        return status("crdt_cmap_combine", ref(t), n, None, ix, n_src, ref(o), count)

    def add(x, y, o, count, nt=1000, nd=1000):
        return status("crdt_cmap_add", ref(x), nt, None, ref(y), nd, None, ref(o), count)

    def from_ops(o, count, m=1000, k=ops[0].data_ptr(), r=ops[1].data_ptr(), dp=ops[2].data_ptr(), dn=ops[3].data_ptr()):
        return status("crdt_cmap_from_ops", k, r, dp, dn, m, ref(o), count)

    assert combine(None, None, cp) == E_INVAL               # NULL state / count
    assert combine(ca, co, None) == E_INVAL
    for f, by in (("key", 4), ("rep", 2), ("p", 4), ("n", 4)):
        assert combine(cm(A, **{f: None}), None, cp) == E_INVAL
        assert combine(ca, cm(O, **{f: None}), cp) == E_INVAL
        assert combine(cm(A, **{f: getattr(A, f).data_ptr() + by}), None, cp) == E_INVAL
        assert combine(ca, cm(O, **{f: getattr(O, f).data_ptr() + by}), cp) == E_INVAL
    assert combine(ca, ca, cp) == E_INVAL                   # out overlapping the input
    assert combine(ca, cm(O, p=A.n.data_ptr() + 8 * 999), cp) == E_INVAL
    assert combine(ca, cm(O, rep=idx.data_ptr() + 4 * 999), cp, ix=idx.data_ptr(), n_src=1000) == E_INVAL   # ... idx
    assert combine(ca, cm(O, key=A.p.data_ptr() + 8 * 1500), cp, ix=idx.data_ptr(), n_src=2000) == E_INVAL  # ... the source
    assert combine(ca, None, cp, ix=idx.data_ptr() + 2, n_src=1000) == E_INVAL
    assert combine(ca, None, cp, ix=idx.data_ptr(), n_src=0) == E_INVAL
    assert combine(ca, None, cp, n=2**62) == E_RANGE
    assert add(None, cb, None, cp) == E_INVAL
    assert add(ca, None, None, cp) == E_INVAL
    assert add(ca, cb, co, None) == E_INVAL
    assert add(cm(A, p=None), cb, None, cp) == E_INVAL
    assert add(ca, cm(B, rep=B.rep.data_ptr() + 2), None, cp) == E_INVAL
    assert add(ca, cb, ca, cp) == E_INVAL
    assert add(ca, cb, cb, cp) == E_INVAL
    assert add(ca, cb, None, cp, 2**62) == E_RANGE
    assert add(ca, cb, None, cp, 2**61, 2**61) == E_RANGE
    assert from_ops(None, cp) == E_INVAL
    assert from_ops(co, None) == E_INVAL
    assert from_ops(co, cp, k=None) == E_INVAL
    assert from_ops(co, cp, r=None) == E_INVAL
    assert from_ops(co, cp, dp=None) == E_INVAL
    assert from_ops(co, cp, dn=None) == E_INVAL
    assert from_ops(cm(O, n=None), cp) == E_INVAL
    assert from_ops(co, cp, k=ops[0].data_ptr() + 4) == E_INVAL
    assert from_ops(co, cp, r=ops[1].data_ptr() + 2) == E_INVAL
    assert from_ops(cm(O, key=ops[2].data_ptr()), cp) == E_INVAL     # out overlapping the log
    assert from_ops(co, cp, m=2**32) == E_RANGE
    assert from_ops(co, cp, m=2**40) == E_RANGE
    with pytest.raises(_lib.CrdtError) as ei:               # NULL ctx
        _lib.call("crdt_cmap_combine", None, C.byref(ca), 1000, None, None, 0, None, cp)
    assert ei.value.status == E_INVAL
    with pytest.raises(ValueError):
        eng.cmap_add(A, B, out=CounterMap.empty(1999, eng.device))
    assert int(cnt.item()) == 0 and eng.device_status(clear=True) == 0
    # lengths of 0: the count store alone, no column read (the fields may be NULL)
    none = _lib.crdt_cmap(None, None, None, None)
    eng._bind()
    for fn, args in (("crdt_cmap_combine", (C.byref(none), 0, None, None, 0, None, cp)),
                     ("crdt_cmap_add", (C.byref(none), 0, None, C.byref(none), 0, None, None, cp)),
                     ("crdt_cmap_from_ops", (None, None, None, None, 0, C.byref(none), cp))):
        cnt.fill_(77)
        _lib.call(fn, eng.ctx, *args, ctx=eng.ctx)
        assert int(cnt.item()) == 0, fn
    check_combine(eng, a)


# ---------------------------------------------------------------- 6. the additive join
def test_add_parity_and_empty_sides(eng):
    a, b = t_cmap._pair(7000, 5305)
    t_cmap._assert_not_vacuous(a, b)
    exp = check_add(eng, a, b)
    _eq(check_add(eng, b, a), exp, "add commutes")
    e, one = cu.state(), cu.state([5], [1], [3], [4])
    for x, y in ((e, e), (e, one), (one, e), (one, one), (a, e), (e, a), (one, cu.state([5], [0], [0], [0]))):
        check_add(eng, x, y)
    big = _cut(a, 1)
    wrapped = check_add(eng, (big[0], big[1], np.array([M64], U64), np.array([2**63], U64)),
                        (big[0], big[1], np.array([2], U64), np.array([2**63], U64)))
    assert wrapped[2].tolist() == [1] and wrapped[3].tolist() == [0]


@pytest.mark.parametrize("q", [2047, 4095])
def test_add_shared_cell_on_a_tile_boundary(eng, q):
    a, b = t_cmap._straddle(q, True)                         # (asserts the pair at merged items q, q + 1)
    exp = check_add(eng, a, b, what=f"add q={q}")
    at = int(np.searchsorted(exp[0], q))
    assert exp[2][at] == U64(2 * (3 * q + 10) + 1)


def test_add_equals_apply_for_one_replicas_batch(eng):
    rng = np.random.default_rng(5)
    t = cu.random_state(rng, 5461, 2000)
    keys = np.sort(rng.choice(2600, size=700, replace=False)).astype(U64)
    dp = rng.integers(0, 1 << 40, size=700, dtype=U64)
    dn = rng.integers(0, 1 << 40, size=700, dtype=U64)
    dp[::9] = M64
    dp[5], dn[5] = 0, 0                                      # a zero op still creates its cell
    Tt = _up(eng, t)
    for rep in (3, 2**31 + 1):
        batch = (keys, np.full(700, rep, U32), dp, dn)
        applied, ac = eng.cmap_apply(Tt, rep, *(u64_tensor(x, eng.device) for x in (keys, dp, dn)))
        added, dc = eng.cmap_add(Tt, _up(eng, batch))
        _eq(_take(added, dc), _take(applied, ac), f"add == apply, rep {rep}")
        _eq(_take(added, dc), cu.apply_np(t, rep, keys, dp, dn), "... == the CPU apply")
    assert eng.device_status(clear=True) == 0


# ---------------------------------------------------------------- 7. from_ops and ingest
@pytest.mark.parametrize("m", [0, 1, 65, T + 1, 3 * T + 17])
def test_from_ops_random_logs(eng, m):
    ops = iu.random_log(np.random.default_rng(m), m, max(1, m // 40), reps=4, big=True)
    exp = check_from_ops(eng, ops, what=f"m={m}")
    assert m < 65 or len(exp[0]) < m // 4                  # heavy repeats


def test_from_ops_orders(eng):
    ops = iu.random_log(np.random.default_rng(8), 3 * T + 17, 300, big=True)
    exp = iu.from_ops_np(ops)
    srt = iu.sorted_log(ops)
    _eq(check_from_ops(eng, srt, what="sorted"), exp, "a log already sorted")
    _eq(check_from_ops(eng, iu.perm(srt, np.arange(len(srt[0]) - 1, -1, -1)), what="reversed"), exp, "a log reversed")
    one = (np.full(T + 9, 2**63 + 5, U64), np.full(T + 9, 2**31 + 1, U32), np.full(T + 9, M64, U64),
           np.arange(T + 9, dtype=U64))
    got = check_from_ops(eng, one, what="one cell")
    assert len(got[0]) == 1 and int(got[2][0]) == (M64 * (T + 9)) % 2**64
    rng = np.random.default_rng(9)
    first = second = None
    for _ in range(2):                                     # two shuffles: identical bytes
        out, cnt = eng.cmap_from_ops(*_ops(eng, iu.perm(ops, rng.permutation(len(ops[0])))))
        first, second = second, [x.tobytes() for x in _take(out, cnt)]
    assert first == second and eng.device_status(clear=True) == 0


def test_ingest(eng):
    rng = np.random.default_rng(10)
    t = cu.random_state(rng, 1000, 300, reps=4)
    t = (t[0] * U64(7) + U64(3), t[1], t[2], t[3])
    for m in (0, 1, 3 * T + 17):
        ops = iu.random_log(rng, m, 300, big=True)
        exp = iu.add_np(t, iu.from_ops_np(ops))
        out, cnt = eng.cmap_ingest(_up(eng, t), *_ops(eng, ops))
        _eq(_take(out, cnt), exp, f"ingest m={m}")
        out, cnt = eng.cmap_ingest(_up(eng, t_cmap._poisoned(t, 700)), *_ops(eng, ops), n_t_dev=_dev(eng, 700))
        _eq(_take(out, cnt), iu.add_np(_cut(t, 700), iu.from_ops_np(ops)), f"ingest m={m}, a device length")
    assert len(exp[0]) < 1000 + len(iu.from_ops_np(ops)[0])   # the log hits cells of t
    assert eng.device_status(clear=True) == 0


def test_three_replicas_ingest_and_converge(eng):
    rng = np.random.default_rng(11)
    total = {}
    states = []
    for node in range(3):
        S, n = CounterMap.empty(1, eng.device), _dev(eng, 0)
        for _ in range(2):                                   # a node ingests its own replica's events, unsorted, keys repeated
            ops = (rng.integers(0, 900, size=1500, dtype=U64), np.full(1500, node, U32),
                   rng.integers(0, 1000, size=1500, dtype=U64), rng.integers(0, 1000, size=1500, dtype=U64))
            for k, p, q in zip(ops[0].tolist(), ops[2].tolist(), ops[3].tolist()):
                total[k] = total.get(k, 0) + p - q
            S, n = eng.cmap_ingest(S, *_ops(eng, ops), n_t_dev=n)
        states.append((S, n))
    M, n = states[0]
    for S, k in states[1:]:
        M, n = eng.cmap_merge(M, S, n_a_dev=n, n_b_dev=k)
    keys, _, _, value, kc = eng.cmap_values(M, n_dev=n, trim=True)
    assert as_u64(keys).tolist() == sorted(total)
    assert value.cpu().numpy().tolist() == [total[k] for k in sorted(total)]
    assert eng.device_status(clear=True) == 0
