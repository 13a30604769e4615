"""CPU: the set section of crdt_amd/engine.py, from a Python call to "which C
function, with which pointers and lengths, and what comes back" -- on a stub
Engine (tests/engine_stub.py) whose C calls are recorded, so no kernel runs.
For every public method: the C call and its whole argument list, the results'
arity, order, dtype, capacity and storage, the synchronisation ``trim`` costs
(one device-status read, or none), and every refusal with its message."""
from itertools import product

import pytest
import torch

from crdt_amd import _lib
from engine_stub import P, T, Tb, base, cap, i32, i64, is_tuples, same, stub, tuples, tuples_cap, u8

NS = (0, 1, 5)                                   # tuples per side
MS = (0, 3)                                      # operations, probes, splitters
I64, I32, U8 = torch.int64, torch.int32, torch.uint8


def one_call(rec, fn):
    (name, args), = rec.c_calls()
    assert name == fn
    return args


def fresh(t, n, dtype=I64):
    """t is a buffer the wrapper allocated: dtype and capacity max(n, 1)."""
    return t.dtype == dtype and cap(t) == max(n, 1)


def fresh_tuples(s, n):
    return tuples_cap(s) == (max(n, 1),) * 4


# ---------------------------------------------------------------- the tail shared by out / src / count methods
def check_tail(call, n, fn, out_i, src_i, extras=0, trim_default=False, bare=False, has_src_arg=True):
    """``call(e, **kw)`` runs a method that returns (out[, src], *extras,
    count) -- or, where ``bare``, the sliced out alone under trim -- with
    out / src of capacity n: every combination of with_src, a given src, given
    out / count, and trim (None: the default)."""
    srcs = product((False, True), (False, True)) if has_src_arg else [(False, False)]
    for (with_src, give_src), give, trim in product(srcs, (False, True), (None, False, True)):
        k = 1 if n < 2 else 2
        e, rec = stub(k)
        out, count = (tuples(n + 2), i64(1)) if give else (None, None)
        src = i64(n + 1) if give_src else None
        kw = dict(out=out, count=count)
        if has_src_arg:
            kw.update(src=src, with_src=with_src)
        if trim is not None:
            kw["trim"] = trim
        res = call(e, **kw)
        has_src = with_src or give_src
        trimmed = trim_default if trim is None else trim
        args = one_call(rec, fn)
        if bare and trimmed:
            r_out, r_src, r_count = res, None, None
        else:
            assert isinstance(res, tuple) and len(res) == 2 + extras + has_src
            r_out, r_count, r_src = res[0], res[-1], res[1] if has_src else None
        # the buffers: given ones come back as the same storage, others are allocated at capacity max(n, 1)
        if give:
            assert same(r_out, out) and (r_count is None or r_count is count)
        else:
            assert fresh_tuples(r_out, n) and (r_count is None or (r_count.dtype == I64 and r_count.shape == (1,)))
        if give_src:
            assert same(r_src, src)
        elif has_src:
            assert fresh(r_src, n)
        assert args[out_i] == T(r_out)
        if r_count is not None:
            assert args[-1] == P(r_count)
        elif give:
            assert args[-1] == P(count)
        else:                                     # allocated inside and not returned: k, written through it, was read
            assert args[-1]
        if has_src_arg:
            assert args[src_i] == P(r_src)
        # trim: one status read and slices of length k; else no synchronisation and the whole buffers
        if trimmed:
            assert [c[1][1] for c in rec.status_reads()] == [1] and rec.calls[-1][0] == "crdt_ctx_device_status"
            assert is_tuples(r_out, k) and (r_src is None or r_src.shape == (k,))
        else:
            assert rec.status_reads() == []
            assert is_tuples(r_out, n + 2 if give else max(n, 1))
            assert r_src is None or r_src.shape == (n + 1 if give_src else max(n, 1),)
    e, rec = stub(1, status=4)                    # a device-side failure flag: trim raises
    with pytest.raises(_lib.CrdtLibraryError, match="device-side failure flags 0x4"):
        call(e, trim=True)
    if trim_default:
        e, rec = stub(1, status=4)
        with pytest.raises(_lib.CrdtLibraryError):
            call(e)


def refuses(call, msg, empty=True):
    """``call(e)`` raises ValueError(msg); with ``empty`` no C call was made before."""
    e, rec = stub(1)
    with pytest.raises(ValueError) as ei:
        call(e)
    assert str(ei.value) == msg
    if empty:
        assert rec.calls == []


def bad_tensors(good: torch.Tensor):
    """(tensor, _check's message) for each way _check refuses a stand-in of ``good``."""
    es, n = good.element_size(), max(good.numel(), 2)
    other = {8: I32, 4: I64, 1: I64}[es]
    return [(torch.zeros(2 * n, dtype=good.dtype)[::2], "tensors must be contiguous"),
            (torch.zeros(n, dtype=other), f"expected {es}-byte elements, got {other}"),
            (torch.zeros(n, dtype=good.dtype, device="meta"), "tensor on meta, engine on cpu")]


def check_refuses_tensor(call, good):
    """``call(e, t)`` passes t where ``good`` would go: each of _check's refusals, before any C call."""
    for t, msg in bad_tensors(good):
        refuses(lambda e: call(e, t), msg)


def check_refuses_tuples(call, n=5):
    """``call(e, s)`` passes the TupleSet s: each field's refusals."""
    for f in ("key", "ts", "rep", "tomb"):
        for t, msg in bad_tensors(getattr(tuples(n), f)):
            s = tuples(n)
            setattr(s, f, t)
            refuses(lambda e: call(e, s), msg)


# ---------------------------------------------------------------- the LWW / OR-Set merges
MERGES = [("lww_merge", "crdt_lww_merge"), ("orset_merge", "crdt_orset_merge"),
          ("lww_merge_unsorted", "crdt_lww_merge_unsorted"), ("orset_merge_unsorted", "crdt_orset_merge_unsorted")]


@pytest.mark.parametrize("meth,fn", MERGES)
@pytest.mark.parametrize("na,nb", [(0, 0), (1, 0), (0, 5), (5, 1), (5, 5)])
def test_merges(meth, fn, na, nb):
    a, b = tuples(na), tuples(nb, 100)
    check_tail(lambda e, **kw: getattr(e, meth)(a, b, **kw), na + nb, fn, 4, None, trim_default=True, bare=True,
               has_src_arg=False)
    e, rec = stub(1)
    out, count = getattr(e, meth)(a, b, trim=False)
    assert one_call(rec, fn) == (T(a), na, T(b), nb, T(out), P(count))
    assert is_tuples(getattr(e, meth)(a, b), 1)                  # trim defaults to True


@pytest.mark.parametrize("meth,fn", MERGES)
def test_merges_refuse(meth, fn):
    a, b = tuples(5), tuples(5, 100)
    check_refuses_tuples(lambda e, s: getattr(e, meth)(s, b))
    check_refuses_tuples(lambda e, s: getattr(e, meth)(a, s))
    check_refuses_tuples(lambda e, s: getattr(e, meth)(a, b, out=s), 10)


SRC_MERGES = [("lww_merge_src", "crdt_lww_merge_src"), ("orset_merge_src", "crdt_orset_merge_src")]


@pytest.mark.parametrize("meth,fn", SRC_MERGES)
@pytest.mark.parametrize("na,nb", [(0, 0), (1, 0), (5, 1), (5, 5)])
def test_src_merges(meth, fn, na, nb):
    a, b, n = tuples(na), tuples(nb, 100), na + nb
    e, rec = stub(1)
    out, count, src = getattr(e, meth)(a, b)
    assert one_call(rec, fn) == (T(a), na, T(b), nb, T(out), P(src), P(count))
    assert fresh_tuples(out, n) and is_tuples(out, max(n, 1)) and fresh(src, n) and src.shape == (max(n, 1),)
    assert count.dtype == I64 and count.shape == (1,)
    e, rec = stub(1)
    o, s = tuples(n + 2), i64(n + 1)
    out, count, src = getattr(e, meth)(a, b, out=o, src=s)
    assert out is o and src is s and count.shape == (1,)
    assert one_call(rec, fn) == (T(a), na, T(b), nb, T(o), P(s), P(count))
    assert rec.status_reads() == []


@pytest.mark.parametrize("meth,fn", SRC_MERGES)
def test_src_merges_refuse(meth, fn):
    a, b = tuples(5), tuples(1, 100)
    msg = "merge_src: out and src (int64) must hold len(a) + len(b) entries"
    refuses(lambda e: getattr(e, meth)(a, b, src=i64(5)), msg)
    refuses(lambda e: getattr(e, meth)(a, b, src=torch.zeros(6, dtype=torch.float64)), msg)
    refuses(lambda e: getattr(e, meth)(a, b, out=tuples(5)), msg)
    check_refuses_tensor(lambda e, t: getattr(e, meth)(a, b, src=t), i64(6))
    check_refuses_tuples(lambda e, s: getattr(e, meth)(s, b))
    check_refuses_tuples(lambda e, s: getattr(e, meth)(a, s))
    check_refuses_tuples(lambda e, s: getattr(e, meth)(a, b, out=s), 6)


@pytest.mark.parametrize("lww", [True, False])
@pytest.mark.parametrize("na,nb", [(0, 0), (5, 1)])
def test_merge_unsorted_planned(lww, na, nb):
    a, b, out, count, plan = tuples(na), tuples(nb, 100), tuples(na + nb), i64(1), _lib.crdt_set_plan()
    e, rec = stub()
    assert e.merge_unsorted_planned(lww, plan, a, b, out, count) is None
    fn = "crdt_lww_merge_unsorted_planned" if lww else "crdt_orset_merge_unsorted_planned"
    args = one_call(rec, fn)
    assert args[0] is plan and args[1:] == (T(a), na, T(b), nb, T(out), P(count))
    assert rec.status_reads() == []


@pytest.mark.parametrize("lww,widen", product([True, False], [False, True]))
def test_set_merge_plan_and_count_unsorted(lww, widen):
    a, b = tuples(5), tuples(1, 100)
    e, rec = stub()
    plan = e.set_merge_plan(lww, a, b, widen=widen)
    args = one_call(rec, "crdt_set_merge_plan")
    assert isinstance(plan, _lib.crdt_set_plan) and args[-1] is plan
    assert args[:-1] == (0 if lww else 1, T(a), 5, T(b), 1, 1 if widen else 0)
    e, rec = stub(3)
    assert e.count_unsorted(a) == 3
    args = one_call(rec, "crdt_tuples_count_unsorted")
    assert args[:2] == (T(a), 5) and len(args) == 3 and args[2]


def test_merge_unsorted_planned_refuses():
    a, b, out, count, plan = tuples(5), tuples(5, 100), tuples(10), i64(1), _lib.crdt_set_plan()
    check_refuses_tuples(lambda e, s: e.merge_unsorted_planned(True, plan, s, b, out, count))
    check_refuses_tuples(lambda e, s: e.merge_unsorted_planned(True, plan, a, s, out, count))
    check_refuses_tuples(lambda e, s: e.merge_unsorted_planned(False, plan, a, b, s, count))


@pytest.mark.parametrize("n", NS)
def test_sort_tuples(n):
    t = tuples(n)
    e, rec = stub()
    out = e.sort_tuples(t)
    assert one_call(rec, "crdt_tuples_sort") == (T(t), n, T(out))
    assert is_tuples(out, n) and tuples_cap(out) == (n,) * 4      # exactly n, not max(n, 1)
    e, rec = stub()
    o = tuples(n + 2)
    assert e.sort_tuples(t, out=o) is o
    assert one_call(rec, "crdt_tuples_sort") == (T(t), n, T(o))
    check_refuses_tuples(lambda e, s: e.sort_tuples(s))
    check_refuses_tuples(lambda e, s: e.sort_tuples(tuples(5), out=s))


@pytest.mark.parametrize("na,nb", [(0, 0), (1, 0), (5, 1), (5, 5)])
def test_tuples_merge(na, nb):
    a, b, n = tuples(na), tuples(nb, 100), na + nb
    e, rec = stub()
    out = e.tuples_merge(a, b)
    assert is_tuples(out, n) and fresh_tuples(out, n)
    args = one_call(rec, "crdt_tuples_merge")
    assert args[:4] == (T(a), na, T(b), nb) and args[4] == Tb(out)
    e, rec = stub()
    o = tuples(n + 2)
    out = e.tuples_merge(a, b, out=o)
    assert is_tuples(out, n) and same(out, o)
    assert one_call(rec, "crdt_tuples_merge") == (T(a), na, T(b), nb, T(o))
    assert rec.status_reads() == []


def test_tuples_merge_refuses():
    a, b = tuples(5), tuples(5, 100)
    check_refuses_tuples(lambda e, s: e.tuples_merge(s, b))
    check_refuses_tuples(lambda e, s: e.tuples_merge(a, s))
    check_refuses_tuples(lambda e, s: e.tuples_merge(a, b, out=s), 10)


@pytest.mark.parametrize("n,m", product(NS, MS))
def test_lower_bound_u64(n, m):
    keys, probes = i64(n), i64(m)
    e, rec = stub()
    out = e.lower_bound_u64(keys, probes)
    assert one_call(rec, "crdt_u64_lower_bound") == (P(keys), n, P(probes), m, P(out))
    assert out.dtype == I64 and out.shape == (m,)
    check_refuses_tensor(lambda e, t: e.lower_bound_u64(t, probes), i64(5))
    check_refuses_tensor(lambda e, t: e.lower_bound_u64(keys, t), i64(3))


# ---------------------------------------------------------------- the gather and the map merges
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("col", [(I64, ()), (U8, ()), (I32, (4,)), (torch.int16, (1,))])
@pytest.mark.parametrize("with_n_dev", [False, True])
def test_gather_src(n, col, with_n_dev):
    dtype, row = col
    src, a_col, b_col = i64(n), torch.zeros((5,) + row, dtype=dtype), torch.zeros((3,) + row, dtype=dtype)
    n_dev = i64(1) if with_n_dev else None
    es = a_col.element_size() * (row[0] if row else 1)
    e, rec = stub()
    out = e.gather_src(src, a_col, b_col, n_dev=n_dev)
    assert one_call(rec, "crdt_src_gather") == (P(src), n, P(n_dev), P(a_col), 5, P(b_col), 3, P(out), es)
    assert out.dtype == dtype and out.shape == (max(n, 1),) + row
    e, rec = stub()
    o = torch.zeros((n + 2,) + row, dtype=dtype)
    assert e.gather_src(src, a_col, b_col, n_dev=n_dev, out=o) is o
    assert one_call(rec, "crdt_src_gather") == (P(src), n, P(n_dev), P(a_col), 5, P(b_col), 3, P(o), es)
    assert rec.status_reads() == []


def test_gather_src_refuses():
    src, a, b = i64(5), i64(5), i64(3)
    shape = "gather_src: a_col and b_col must share one dtype and be 1-D (or [n, w] rows)"
    refuses(lambda e: e.gather_src(src, a, i32(3)), shape)
    refuses(lambda e: e.gather_src(src, a, torch.zeros(3, 1, dtype=I64)), shape)
    refuses(lambda e: e.gather_src(src, torch.zeros(5, 1, 1, dtype=I64), torch.zeros(3, 1, 1, dtype=I64)), shape)
    refuses(lambda e: e.gather_src(src, torch.zeros((), dtype=I64), torch.zeros((), dtype=I64)), shape)
    refuses(lambda e: e.gather_src(src, torch.zeros(5, 2, dtype=I32), torch.zeros(3, 4, dtype=I32)),
            "gather_src: a_col and b_col rows differ in width")
    refuses(lambda e: e.gather_src(src, torch.zeros(5, 3, dtype=U8), torch.zeros(3, 3, dtype=U8)),
            "gather_src: 3-byte elements (1, 2, 4, 8 or 16)")
    refuses(lambda e: e.gather_src(src, torch.zeros(5, 4, dtype=I64), torch.zeros(3, 4, dtype=I64)),
            "gather_src: 32-byte elements (1, 2, 4, 8 or 16)")
    one_d = "gather_src: src must be a 1-D int64 tensor"
    refuses(lambda e: e.gather_src(torch.zeros(5, dtype=torch.float64), a, b), one_d)
    refuses(lambda e: e.gather_src(torch.zeros(5, 1, dtype=I64), a, b), one_d)
    holds = "gather_src: out must hold len(src) elements of the columns' dtype"
    refuses(lambda e: e.gather_src(src, a, b, out=i64(4)), holds)
    refuses(lambda e: e.gather_src(src, a, b, out=torch.zeros(5, dtype=torch.float64)), holds)
    refuses(lambda e: e.gather_src(src, a, b, out=torch.zeros(5, 1, dtype=I64)), holds)
    check_refuses_tensor(lambda e, t: e.gather_src(t, a, b), src)
    check_refuses_tensor(lambda e, t: e.gather_src(src, a, b, n_dev=t), i64(1))
    for bad, msg in bad_tensors(a)[::2]:                         # the columns' element size is free
        refuses(lambda e: e.gather_src(src, bad, b), msg)
        refuses(lambda e: e.gather_src(src, a, b, out=bad), msg)


def check_composite(rec, first_fn, src_i, a_val, b_val, out_val, count, n_b=None):
    """A composite's two calls: ``first_fn`` with source indices, then one
    gather of all of them chained off the first call's count tensor."""
    (fn1, args1), (fn2, args2) = rec.c_calls()
    assert fn1 == first_fn and fn2 == "crdt_src_gather"
    src_ptr = args1[src_i]
    assert src_ptr is not None and args1[-1] == P(count)
    n_b = b_val.shape[0] if n_b is None else n_b
    assert args2[0] == src_ptr and args2[2] == P(count) and args2[3:] == (
        P(a_val), a_val.shape[0], P(b_val), n_b, P(out_val), a_val.element_size())
    assert rec.status_reads() == []
    return args1, args2[1]


@pytest.mark.parametrize("meth,fn", [("lww_map_merge", "crdt_lww_merge_src"),
                                     ("orset_map_merge", "crdt_orset_merge_src")])
@pytest.mark.parametrize("na,nb", [(0, 0), (1, 0), (5, 1), (5, 5)])
def test_map_merges(meth, fn, na, nb):
    a, b, av, bv, n = tuples(na), tuples(nb, 100), i32(na), i32(nb), na + nb
    e, rec = stub(1)
    out, out_val, count = getattr(e, meth)(a, av, b, bv)
    args1, n_src = check_composite(rec, fn, 5, av, bv, out_val, count)
    assert args1[:5] == (T(a), na, T(b), nb, T(out)) and n_src == max(n, 1)
    assert fresh_tuples(out, n) and fresh(out_val, n, I32) and count.shape == (1,)
    msg = "map_merge: one value per tuple on each side"
    refuses(lambda e: getattr(e, meth)(a, i32(na + 1), b, bv), msg)
    refuses(lambda e: getattr(e, meth)(a, av, b, i32(nb + 1)), msg)


# ---------------------------------------------------------------- set reads
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("lww", [True, False])
@pytest.mark.parametrize("with_n_dev", [False, True])
def test_set_elements_cardinality(n, lww, with_n_dev):
    t, n_dev, mode = tuples(n), i64(1) if with_n_dev else None, 0 if lww else 1
    e, rec = stub(1)
    keys, count = e.set_elements(t, lww, n_dev=n_dev)
    assert one_call(rec, "crdt_set_elements") == (mode, T(t), n, P(n_dev), P(keys), P(count))
    assert fresh(keys, n) and keys.shape == (max(n, 1),) and count.dtype == I64 and count.shape == (1,)
    e, rec = stub(1)
    o, c = i64(n + 2), i64(1)
    keys, count = e.set_elements(t, lww, n_dev, o, c)
    assert keys is o and count is c
    assert one_call(rec, "crdt_set_elements") == (mode, T(t), n, P(n_dev), P(o), P(c))
    e, rec = stub(1)
    count = e.set_cardinality(t, lww, n_dev=n_dev)
    assert one_call(rec, "crdt_set_elements") == (mode, T(t), n, P(n_dev), None, P(count))
    assert count.dtype == I64 and count.shape == (1,)
    e, rec = stub(1)
    assert e.set_cardinality(t, lww, n_dev, c) is c
    assert one_call(rec, "crdt_set_elements") == (mode, T(t), n, P(n_dev), None, P(c))
    assert rec.status_reads() == []


def test_set_elements_cardinality_refuse():
    t = tuples(5)
    refuses(lambda e: e.set_elements(t, True, out=i64(4)), "set_elements: out holds fewer keys than t has tuples")
    check_refuses_tensor(lambda e, x: e.set_elements(t, True, out=x), i64(5))
    for meth in ("set_elements", "set_cardinality"):
        check_refuses_tuples(lambda e, s: getattr(e, meth)(s, False))
        check_refuses_tensor(lambda e, x: getattr(e, meth)(t, False, n_dev=x), i64(1))
        check_refuses_tensor(lambda e, x: getattr(e, meth)(t, False, count=x), i64(1))


@pytest.mark.parametrize("n,m", product(NS, MS))
@pytest.mark.parametrize("with_n_dev", [False, True])
def test_keys_contain(n, m, with_n_dev):
    keys, probes, n_dev = i64(n), i64(m), i64(1) if with_n_dev else None
    e, rec = stub()
    res = e.keys_contain(keys, probes, n_dev=n_dev)
    assert one_call(rec, "crdt_u64_contains") == (P(keys), n, P(n_dev), P(probes), m, P(res))
    assert res.dtype == U8 and res.shape == (m,)
    check_refuses_tensor(lambda e, t: e.keys_contain(t, probes), i64(5))
    check_refuses_tensor(lambda e, t: e.keys_contain(keys, t), i64(3))
    check_refuses_tensor(lambda e, t: e.keys_contain(keys, probes, n_dev=t), i64(1))


# ---------------------------------------------------------------- set deltas
@pytest.mark.parametrize("ns,nd", [(0, 0), (1, 5), (5, 0), (5, 5)])
@pytest.mark.parametrize("lww", [True, False])
def test_set_delta(ns, nd, lww):
    src, dst, mode = tuples(ns), tuples(nd, 100), 0 if lww else 1
    check_tail(lambda e, **kw: e.set_delta(src, dst, lww, **kw), ns, "crdt_set_delta", 7, None, bare=True,
               has_src_arg=False)
    for n_s, n_d in product((None, i64(1)), (None, i64(1))):
        e, rec = stub(1)
        out, count = e.set_delta(src, dst, lww, n_src_dev=n_s, n_dst_dev=n_d)
        assert one_call(rec, "crdt_set_delta") == (mode, T(src), ns, P(n_s), T(dst), nd, P(n_d), T(out), P(count))
        e, rec = stub(1)
        count = e.set_delta_count(src, dst, lww, n_src_dev=n_s, n_dst_dev=n_d)
        assert one_call(rec, "crdt_set_delta") == (mode, T(src), ns, P(n_s), T(dst), nd, P(n_d), None, P(count))
        assert count.dtype == I64 and count.shape == (1,) and rec.status_reads() == []
    e, rec = stub(1)
    c = i64(1)
    assert e.set_delta_count(src, dst, lww, count=c) is c
    assert one_call(rec, "crdt_set_delta")[-1] == P(c)


def test_set_delta_refuses():
    src, dst = tuples(5), tuples(5, 100)
    refuses(lambda e: e.set_delta(src, dst, True, out=tuples(4)), "set_delta: out holds fewer tuples than src")
    check_refuses_tuples(lambda e, s: e.set_delta(src, dst, True, out=s))
    for meth in ("set_delta", "set_delta_count"):
        check_refuses_tuples(lambda e, s: getattr(e, meth)(s, dst, True))
        check_refuses_tuples(lambda e, s: getattr(e, meth)(src, s, True))
        check_refuses_tensor(lambda e, t: getattr(e, meth)(src, dst, False, n_src_dev=t), i64(1))
        check_refuses_tensor(lambda e, t: getattr(e, meth)(src, dst, False, n_dst_dev=t), i64(1))
        check_refuses_tensor(lambda e, t: getattr(e, meth)(src, dst, False, count=t), i64(1))


# ---------------------------------------------------------------- compaction
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("lww", [True, False])
def test_set_compact(n, lww):
    t, mode = tuples(n), 0 if lww else 1
    check_tail(lambda e, **kw: e.set_compact(t, lww, None, **kw), n, "crdt_set_compact", 6, 7)
    for cut, n_dev in product((None, i64(0), i64(4)), (None, i64(1))):
        n_cut = 0 if cut is None else cut.numel()
        e, rec = stub(1)
        out, count = e.set_compact(t, lww, cut, n_dev=n_dev)
        assert one_call(rec, "crdt_set_compact") == (mode, T(t), n, P(n_dev), P(cut), n_cut, T(out), None, P(count))
        e, rec = stub(1)
        count = e.set_compact_count(t, lww, cut, n_dev=n_dev)
        assert one_call(rec, "crdt_set_compact") == (mode, T(t), n, P(n_dev), P(cut), n_cut, None, None, P(count))
        assert count.dtype == I64 and count.shape == (1,) and rec.status_reads() == []
    e, rec = stub(1)
    c = i64(1)
    assert e.set_compact_count(t, lww, None, count=c) is c
    assert one_call(rec, "crdt_set_compact")[-1] == P(c)


def test_set_compact_refuses():
    t = tuples(5)
    refuses(lambda e: e.set_compact(t, True, None, out=tuples(4)), "set_compact: out holds fewer tuples than t")
    msg = "set_compact: src must be int64 and hold len(t) entries"
    refuses(lambda e: e.set_compact(t, True, None, src=i64(4)), msg)
    refuses(lambda e: e.set_compact(t, True, None, src=torch.zeros(5, dtype=torch.float64)), msg)
    check_refuses_tensor(lambda e, x: e.set_compact(t, True, None, src=x), i64(5))
    check_refuses_tuples(lambda e, s: e.set_compact(t, True, None, out=s))
    for meth in ("set_compact", "set_compact_count"):
        check_refuses_tuples(lambda e, s: getattr(e, meth)(s, False, None))
        check_refuses_tensor(lambda e, x: getattr(e, meth)(t, False, x), i64(4))
        check_refuses_tensor(lambda e, x: getattr(e, meth)(t, False, None, n_dev=x), i64(1))
        check_refuses_tensor(lambda e, x: getattr(e, meth)(t, False, None, count=x), i64(1))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("lww", [True, False])
def test_map_compact(n, lww):
    t, val, cut = tuples(n), i32(n), i64(4)
    e, rec = stub(1)
    out, out_val, count = e.map_compact(t, val, lww, cut)
    args1, n_src = check_composite(rec, "crdt_set_compact", 7, val, val[:0], out_val, count)
    assert args1[:7] == (0 if lww else 1, T(t), n, None, P(cut), 4, T(out)) and n_src == max(n, 1)
    assert fresh_tuples(out, n) and is_tuples(out, max(n, 1)) and fresh(out_val, n, I32) and count.shape == (1,)
    refuses(lambda e: e.map_compact(t, i32(n + 1), lww, cut), "map_compact: one value per tuple")


# ---------------------------------------------------------------- map reads
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("lww", [True, False])
def test_map_read(n, lww):
    t, mode = tuples(n), 0 if lww else 1
    for with_keys, with_nsib, n_dev in product((True, False), (False, True), (None, i64(1))):
        e, rec = stub(1)
        keys, win, nsib, count = e.map_read(t, lww, n_dev=n_dev, with_keys=with_keys, with_nsib=with_nsib)
        assert one_call(rec, "crdt_map_read") == (mode, T(t), n, P(n_dev), P(keys), P(win), P(nsib), P(count))
        assert (keys is not None) == with_keys and (nsib is not None) == with_nsib
        assert fresh(win, n) and win.shape == (max(n, 1),) and count.dtype == I64 and count.shape == (1,)
        assert keys is None or (fresh(keys, n) and keys.shape == (max(n, 1),))
        assert nsib is None or (fresh(nsib, n, I32) and nsib.shape == (max(n, 1),))
        assert rec.status_reads() == []
    e, rec = stub(1)                                             # the defaults: keys, no nsib
    keys, win, nsib, count = e.map_read(t, lww)
    assert keys is not None and nsib is None
    e, rec = stub(1)                                             # given buffers win over the with_ flags
    k, w, s, c = i64(n + 2), i64(n + 1), i32(n + 3), i64(1)
    res = e.map_read(t, lww, with_keys=False, with_nsib=False, keys=k, win=w, nsib=s, count=c)
    assert all(x is y for x, y in zip(res, (k, w, s, c))) and len(res) == 4
    assert one_call(rec, "crdt_map_read") == (mode, T(t), n, None, P(k), P(w), P(s), P(c))


def test_map_read_refuses():
    t = tuples(5)
    msg = "map_read: win must be int64 and hold len(t) rows"
    refuses(lambda e: e.map_read(t, True, win=i64(4)), msg)
    refuses(lambda e: e.map_read(t, True, win=torch.zeros(5, dtype=torch.float64)), msg)
    msg = "map_read: keys / nsib hold fewer rows than t has tuples"
    refuses(lambda e: e.map_read(t, True, keys=i64(4)), msg)
    refuses(lambda e: e.map_read(t, True, nsib=i32(4)), msg)
    check_refuses_tuples(lambda e, s: e.map_read(s, False))
    check_refuses_tensor(lambda e, x: e.map_read(t, False, win=x), i64(5))
    check_refuses_tensor(lambda e, x: e.map_read(t, False, keys=x), i64(5))
    check_refuses_tensor(lambda e, x: e.map_read(t, False, nsib=x), i32(5))
    check_refuses_tensor(lambda e, x: e.map_read(t, False, n_dev=x), i64(1))
    check_refuses_tensor(lambda e, x: e.map_read(t, False, count=x), i64(1))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("lww", [True, False])
@pytest.mark.parametrize("with_n_dev", [False, True])
def test_map_values(n, lww, with_n_dev):
    t, val, n_dev = tuples(n), i32(n), i64(1) if with_n_dev else None
    e, rec = stub(1)
    keys, values, count = e.map_values(t, val, lww, n_dev=n_dev)
    args1, n_src = check_composite(rec, "crdt_map_read", 5, val, val[:0], values, count)
    assert args1[:5] == (0 if lww else 1, T(t), n, P(n_dev), P(keys)) and args1[6] is None and n_src == max(n, 1)
    assert fresh(keys, n) and fresh(values, n, I32) and count.shape == (1,)
    refuses(lambda e: e.map_values(t, i32(n + 1), lww), "map_values: one value per tuple")


@pytest.mark.parametrize("n,m", product(NS, MS))
@pytest.mark.parametrize("lww", [True, False])
def test_map_lookup(n, m, lww):
    t, probes, mode = tuples(n), i64(m), 0 if lww else 1
    for with_nsib, n_dev in product((False, True), (None, i64(1))):
        e, rec = stub()
        win, nsib = e.map_lookup(t, probes, lww, n_dev=n_dev, with_nsib=with_nsib)
        args = one_call(rec, "crdt_map_lookup")
        assert args[:6] == (mode, T(t), n, P(n_dev), P(probes), m) and len(args) == 8
        assert win.shape == (m,) and fresh(win, m) and (nsib is not None) == with_nsib     # [:m] views
        assert nsib is None or (nsib.shape == (m,) and fresh(nsib, m, I32))
        assert args[6:] == (P(win), P(nsib)) and rec.status_reads() == []
    e, rec = stub()
    w, s = i64(m + 2), i32(m + 1)
    res = e.map_lookup(t, probes, lww, win=w, nsib=s)
    assert res[0] is w and res[1] is s and len(res) == 2
    assert one_call(rec, "crdt_map_lookup") == (mode, T(t), n, None, P(probes), m, P(w), P(s))


def test_map_lookup_refuses():
    t, probes = tuples(5), i64(3)
    msg = "map_lookup: win must be int64 and hold one entry per probe"
    refuses(lambda e: e.map_lookup(t, probes, True, win=i64(2)), msg)
    refuses(lambda e: e.map_lookup(t, probes, True, win=torch.zeros(3, dtype=torch.float64)), msg)
    refuses(lambda e: e.map_lookup(t, probes, True, nsib=i32(2)),
            "map_lookup: nsib holds fewer entries than there are probes")
    check_refuses_tuples(lambda e, s: e.map_lookup(s, probes, False))
    check_refuses_tensor(lambda e, x: e.map_lookup(t, x, False), probes)
    check_refuses_tensor(lambda e, x: e.map_lookup(t, probes, False, win=x), i64(3))
    check_refuses_tensor(lambda e, x: e.map_lookup(t, probes, False, nsib=x), i32(3))
    check_refuses_tensor(lambda e, x: e.map_lookup(t, probes, False, n_dev=x), i64(1))


@pytest.mark.parametrize("n,m", product(NS, MS))
@pytest.mark.parametrize("default", [7, "tensor"])
@pytest.mark.parametrize("row", [(), (2,)])
def test_map_get(n, m, default, row):
    t, probes, val, n_dev = tuples(n), i64(m), torch.zeros((n,) + row, dtype=I32), i64(1)
    default = torch.full(row or (1,), 7, dtype=I64) if default == "tensor" else default
    e, rec = stub()
    out = e.map_get(t, val, probes, default, True, n_dev=n_dev)
    (fn1, args1), (fn2, args2) = rec.c_calls()
    assert fn1 == "crdt_map_lookup" and args1[:6] == (0, T(t), n, P(n_dev), P(probes), m) and args1[7] is None
    win_ptr = args1[6]                                           # the gather reads the lookup's win, all m of it
    assert fn2 == "crdt_src_gather" and args2[:5] == (win_ptr, m, None, P(val), n)
    assert args2[6] == 1 and args2[7] == base(out) and args2[8] == 4 * (row[0] if row else 1)
    assert (win_ptr == 0) == (m == 0) and args2[5] not in (None, 0)      # b side: the one-element default column
    assert out.dtype == I32 and out.shape == (m,) + row and cap(out) == max(m, 1) * (row[0] if row else 1)
    assert rec.status_reads() == []
    refuses(lambda e: e.map_get(t, i32(n + 1), probes, 0, True), "map_get: one value per tuple")


# ---------------------------------------------------------------- the causal merges
def causal_args(a, ctx_a, b, ctx_b, n_a, n_b, mid, out, src, ctx_out, count):
    return (T(a), len(a), P(n_a), P(ctx_a), 0 if ctx_a is None else ctx_a.numel(),
            T(b), len(b), P(n_b), P(ctx_b), 0 if ctx_b is None else ctx_b.numel(), *mid,
            None if out is None else T(out), P(src), P(ctx_out), P(count))


def causal_forms(m):
    """(method, count-only method, C function, extra positional arguments,
    their C arguments) for the plain form and, given m splitters, the ranges form."""
    spl, flags = i64(m), u8(m + 1)
    yield "causal_merge", "causal_merge_count", "crdt_orset_merge_causal", (), ()
    for s in (spl, None) if m == 0 else (spl,):
        yield ("causal_merge_ranges", "causal_merge_ranges_count", "crdt_orset_merge_causal_ranges", (s, flags),
               (P(s) if m else None, m, P(flags)))


@pytest.mark.parametrize("na,nb", [(0, 0), (1, 0), (5, 1), (5, 5)])
@pytest.mark.parametrize("m", MS)
def test_causal_merges(na, nb, m):
    a, b, n = tuples(na), tuples(nb, 100), na + nb
    for meth, count_meth, fn, extra, mid in causal_forms(m):
        k = len(mid)
        check_tail(lambda e, **kw: getattr(e, meth)(a, i64(2), b, i64(3), *extra, **kw), n, fn, 10 + k, 11 + k,
                   extras=1)
        for ctx_a, ctx_b, n_a, n_b in [(None, None, None, None), (i64(4), None, i64(1), None),
                                       (i64(2), i64(3), None, i64(1)), (None, i64(0), i64(1), i64(1))]:
            nc = max(0 if ctx_a is None else ctx_a.numel(), 0 if ctx_b is None else ctx_b.numel())
            e, rec = stub(1)
            out, ctx_out, count = getattr(e, meth)(a, ctx_a, b, ctx_b, *extra, n_a_dev=n_a, n_b_dev=n_b)
            assert one_call(rec, fn) == causal_args(a, ctx_a, b, ctx_b, n_a, n_b, mid, out, None, ctx_out, count)
            assert ctx_out.dtype == I64 and ctx_out.shape == (nc,)            # the longer context's length
            e, rec = stub(1)
            co = i64(nc + 2)
            res = getattr(e, meth)(a, ctx_a, b, ctx_b, *extra, n_a_dev=n_a, n_b_dev=n_b, ctx_out=co, with_src=True)
            assert len(res) == 4 and res[2] is co
            assert one_call(rec, fn) == causal_args(a, ctx_a, b, ctx_b, n_a, n_b, mid, res[0], res[1], co, res[3])
            e, rec = stub(1)
            count = getattr(e, count_meth)(a, ctx_a, b, ctx_b, *extra, n_a_dev=n_a, n_b_dev=n_b)
            assert one_call(rec, fn) == causal_args(a, ctx_a, b, ctx_b, n_a, n_b, mid, None, None, None, count)
            assert count.dtype == I64 and count.shape == (1,) and rec.status_reads() == []
        e, rec = stub(1)
        c = i64(1)
        assert getattr(e, count_meth)(a, None, b, None, *extra, count=c) is c
        assert one_call(rec, fn)[-1] == P(c)


@pytest.mark.parametrize("ranges", [False, True])
def test_causal_merges_refuse(ranges):
    a, b, ca, cb = tuples(5), tuples(1, 100), i64(2), i64(3)
    who = "causal_merge_ranges" if ranges else "causal_merge"
    extra = (i64(3), u8(4)) if ranges else ()
    full = lambda e, **kw: getattr(e, who)(a, ca, b, cb, *extra, **kw)
    refuses(lambda e: full(e, out=tuples(5)), f"{who}: out holds fewer tuples than len(a) + len(b)")
    msg = f"{who}: src must be int64 and hold len(a) + len(b) entries"
    refuses(lambda e: full(e, src=i64(5)), msg)
    refuses(lambda e: full(e, src=torch.zeros(6, dtype=torch.float64)), msg)
    refuses(lambda e: full(e, ctx_out=i64(2)), f"{who}: ctx_out holds fewer entries than the longer context")
    check_refuses_tensor(lambda e, x: full(e, src=x), i64(6))
    check_refuses_tensor(lambda e, x: full(e, ctx_out=x), i64(3))
    check_refuses_tuples(lambda e, s: full(e, out=s), 6)
    for meth in (who, who + "_count"):
        f = lambda e, a_=a, ca_=ca, b_=b, cb_=cb, **kw: getattr(e, meth)(a_, ca_, b_, cb_, *extra, **kw)
        check_refuses_tuples(lambda e, s: f(e, a_=s))
        check_refuses_tuples(lambda e, s: f(e, b_=s))
        check_refuses_tensor(lambda e, x: f(e, ca_=x), ca)
        check_refuses_tensor(lambda e, x: f(e, cb_=x), cb)
        check_refuses_tensor(lambda e, x: f(e, n_a_dev=x), i64(1))
        check_refuses_tensor(lambda e, x: f(e, n_b_dev=x), i64(1))
        check_refuses_tensor(lambda e, x: f(e, count=x), i64(1))
        if ranges:
            g = lambda e, spl, flags: getattr(e, meth)(a, ca, b, cb, spl, flags)
            msg = "causal_merge_ranges: flags must hold len(splitters) + 1 entries"
            refuses(lambda e: g(e, i64(3), u8(3)), msg)
            refuses(lambda e: g(e, None, u8(0)), msg)
            check_refuses_tensor(lambda e, x: g(e, x, u8(4)), i64(3))
            check_refuses_tensor(lambda e, x: g(e, i64(3), x), u8(4))


@pytest.mark.parametrize("na,nb", [(0, 0), (5, 1), (5, 5)])
def test_causal_map_merges(na, nb):
    a, b, av, bv, ca, cb, n = tuples(na), tuples(nb, 100), i32(na), i32(nb), i64(2), i64(3), na + nb
    e, rec = stub(1)
    out, out_val, ctx_out, count = e.causal_map_merge(a, av, ca, b, bv, cb)
    args1, n_src = check_composite(rec, "crdt_orset_merge_causal", 11, av, bv, out_val, count)
    assert args1 == causal_args(a, ca, b, cb, None, None, (), out, torch.empty(0), ctx_out, count)[:11] + args1[11:]
    assert args1[12:] == (P(ctx_out), P(count)) and n_src == max(n, 1)
    assert fresh_tuples(out, n) and fresh(out_val, n, I32) and ctx_out.shape == (3,) and count.shape == (1,)
    for m, n_b in product(MS, (None, i64(1))):
        spl, flags = i64(m), u8(m + 1)
        e, rec = stub(1)
        out, out_val, ctx_out, count = e.causal_map_merge_ranges(a, av, ca, b, bv, cb, spl, flags, n_b_dev=n_b)
        args1, n_src = check_composite(rec, "crdt_orset_merge_causal_ranges", 14, av, bv, out_val, count)
        mid = (P(spl) if m else None, m, P(flags))
        assert args1[:14] == causal_args(a, ca, b, cb, None, n_b, mid, out, None, None, None)[:14]
        assert args1[15:] == (P(ctx_out), P(count)) and n_src == max(n, 1)
        assert fresh_tuples(out, n) and fresh(out_val, n, I32) and ctx_out.shape == (3,)
    for who, extra in (("causal_map_merge", ()), ("causal_map_merge_ranges", (i64(0), u8(1)))):
        msg = f"{who}: one value per tuple on each side"
        refuses(lambda e: getattr(e, who)(a, i32(na + 1), ca, b, bv, cb, *extra), msg)
        refuses(lambda e: getattr(e, who)(a, av, ca, b, i32(nb + 1), cb, *extra), msg)


# ---------------------------------------------------------------- the mutators
def apply_args(causal, t, n_dev, clock, rep, keys, kinds, out, src, clock_out, count):
    m = keys.numel()
    return (1 if causal else 0, T(t), len(t), P(n_dev), P(clock), clock.numel(), rep, P(keys) if m else None,
            P(kinds) if m else None, m, None if out is None else T(out), P(src), P(clock_out), P(count))


@pytest.mark.parametrize("n,m", product(NS, MS))
@pytest.mark.parametrize("causal", [False, True])
def test_set_apply(n, m, causal):
    t, clock, keys, kinds = tuples(n), i64(4), i64(m), u8(m)
    check_tail(lambda e, **kw: e.set_apply(t, clock, 2, keys, kinds, causal, **kw), n + m, "crdt_set_apply", 10, 11,
               extras=1, trim_default=True)
    for n_dev, rep in ((None, 0), (i64(1), 2 ** 32 - 1)):
        e, rec = stub(1)
        out, clock_out, count = e.set_apply(t, clock, rep, keys, kinds, causal, n_dev=n_dev, trim=False)
        assert one_call(rec, "crdt_set_apply") == apply_args(causal, t, n_dev, clock, rep, keys, kinds, out, None,
                                                             clock_out, count)
        assert clock_out.dtype == I64 and clock_out.shape == (4,)
        e, rec = stub(1)
        co = i64(6)
        res = e.set_apply(t, clock, rep, keys, kinds, causal, n_dev=n_dev, clock_out=co, with_src=True, trim=False)
        assert len(res) == 4 and res[2] is co
        assert one_call(rec, "crdt_set_apply") == apply_args(causal, t, n_dev, clock, rep, keys, kinds, res[0], res[1],
                                                             co, res[3])
        for co in (None, i64(4)):
            e, rec = stub(1)
            count = e.set_apply_count(t, clock, rep, keys, kinds, causal, n_dev=n_dev, clock_out=co)
            assert one_call(rec, "crdt_set_apply") == apply_args(causal, t, n_dev, clock, rep, keys, kinds, None, None,
                                                                 co, count)
            assert count.dtype == I64 and count.shape == (1,) and rec.status_reads() == []
    e, rec = stub(1)
    c = i64(1)
    assert e.set_apply_count(t, clock, 0, keys, kinds, causal, count=c) is c
    assert one_call(rec, "crdt_set_apply")[-1] == P(c)


def test_set_apply_refuses():
    t, clock, keys, kinds = tuples(5), i64(4), i64(3), u8(3)
    full = lambda e, **kw: e.set_apply(t, clock, 2, keys, kinds, False, **kw)
    refuses(lambda e: full(e, out=tuples(7)), "set_apply: out holds fewer tuples than len(t) + len(op_keys)")
    msg = "set_apply: src must be int64 and hold len(t) + len(op_keys) entries"
    refuses(lambda e: full(e, src=i64(7)), msg)
    refuses(lambda e: full(e, src=torch.zeros(8, dtype=torch.float64)), msg)
    check_refuses_tensor(lambda e, x: full(e, src=x), i64(8))
    check_refuses_tuples(lambda e, s: full(e, out=s), 8)
    for meth in ("set_apply", "set_apply_count"):
        f = lambda e, t_=t, clock_=clock, rep=2, keys_=keys, kinds_=kinds, **kw: getattr(e, meth)(
            t_, clock_, rep, keys_, kinds_, True, **kw)
        refuses(lambda e: f(e, kinds_=u8(2)), "set_apply: one kind per operation key")
        refuses(lambda e: f(e, kinds_=u8(4)), "set_apply: one kind per operation key")
        refuses(lambda e: f(e, rep=-1), "set_apply: rep is a uint32")
        refuses(lambda e: f(e, rep=2 ** 32), "set_apply: rep is a uint32")
        refuses(lambda e: f(e, clock_out=i64(3)), "set_apply: clock_out holds fewer entries than clock")
        check_refuses_tuples(lambda e, s: f(e, t_=s))
        check_refuses_tensor(lambda e, x: f(e, clock_=x), clock)
        check_refuses_tensor(lambda e, x: f(e, keys_=x, kinds_=u8(x.numel())), keys)
        check_refuses_tensor(lambda e, x: f(e, kinds_=x), kinds)
        check_refuses_tensor(lambda e, x: f(e, n_dev=x), i64(1))
        check_refuses_tensor(lambda e, x: f(e, clock_out=x), i64(4))
        check_refuses_tensor(lambda e, x: f(e, count=x), i64(1))


@pytest.mark.parametrize("n,m", product(NS, MS))
@pytest.mark.parametrize("causal", [False, True])
def test_map_apply(n, m, causal):
    t, val, clock, keys, kinds, vals = tuples(n), i32(n), i64(4), i64(m), u8(m), i32(m)
    e, rec = stub(1)
    out, out_val, clock_out, count = e.map_apply(t, val, clock, 2, keys, kinds, vals, causal)
    args1, n_src = check_composite(rec, "crdt_set_apply", 11, val, vals, out_val, count)   # no status read: no trim
    assert args1[:11] == apply_args(causal, t, None, clock, 2, keys, kinds, out, None, None, None)[:11]
    assert args1[12:] == (P(clock_out), P(count)) and n_src == max(n + m, 1)
    assert fresh_tuples(out, n + m) and is_tuples(out, max(n + m, 1)) and fresh(out_val, n + m, I32)
    assert clock_out.shape == (4,) and count.shape == (1,)
    msg = "map_apply: one value per tuple and per operation"
    refuses(lambda e: e.map_apply(t, i32(n + 1), clock, 2, keys, kinds, vals, causal), msg)
    refuses(lambda e: e.map_apply(t, val, clock, 2, keys, kinds, i32(m + 1), causal), msg)


# ---------------------------------------------------------------- digests and select
@pytest.mark.parametrize("n,m", product(NS, MS))
@pytest.mark.parametrize("lww", [True, False])
def test_set_digest(n, m, lww):
    t, mode = tuples(n), 0 if lww else 1
    for spl, n_dev in product((i64(m), None) if m == 0 else (i64(m),), (None, i64(1))):
        e, rec = stub()
        h, c = e.set_digest(t, lww, spl, n_dev=n_dev)
        assert one_call(rec, "crdt_set_digest") == (mode, T(t), n, P(n_dev), P(spl) if m else None, m, P(h), P(c))
        assert h.dtype == c.dtype == I64 and h.shape == c.shape == (m + 1,) and rec.status_reads() == []
        e, rec = stub()
        ho, co = i64(m + 2), i64(m + 1)
        res = e.set_digest(t, lww, spl, n_dev, ho, co)
        assert res[0] is ho and res[1] is co and len(res) == 2
        assert one_call(rec, "crdt_set_digest") == (mode, T(t), n, P(n_dev), P(spl) if m else None, m, P(ho), P(co))


def test_set_digest_refuses():
    t, spl = tuples(5), i64(3)
    msg = "set_digest: the outputs must hold len(splitters) + 1 entries"
    refuses(lambda e: e.set_digest(t, True, spl, hash_out=i64(3)), msg)
    refuses(lambda e: e.set_digest(t, True, spl, count_out=i64(3)), msg)
    refuses(lambda e: e.set_digest(t, True, None, hash_out=i64(0)), msg)
    check_refuses_tuples(lambda e, s: e.set_digest(s, False, spl))
    check_refuses_tensor(lambda e, x: e.set_digest(t, False, x), spl)
    check_refuses_tensor(lambda e, x: e.set_digest(t, False, spl, n_dev=x), i64(1))
    check_refuses_tensor(lambda e, x: e.set_digest(t, False, spl, hash_out=x), i64(4))
    check_refuses_tensor(lambda e, x: e.set_digest(t, False, spl, count_out=x), i64(4))


@pytest.mark.parametrize("nb", [0, 1, 4])
def test_digest_diff(nb):
    da, db = (i64(nb), i64(nb)), (i64(nb), i64(nb))
    e, rec = stub(1)
    flags, n_diff = e.digest_diff(da, db)
    args = one_call(rec, "crdt_set_digest_diff")
    assert args[:5] == (P(da[0]), P(da[1]), P(db[0]), P(db[1]), nb) and args[6] == P(n_diff)
    assert flags.dtype == U8 and flags.shape == (nb,) and cap(flags) == max(nb, 1)        # flags[:nb]
    assert args[5] == base(flags)
    assert n_diff.dtype == I64 and n_diff.shape == (1,) and rec.status_reads() == []
    e, rec = stub(1)
    f, c = u8(nb + 2), i64(1)
    flags, n_diff = e.digest_diff(da, db, f, c)
    assert flags.shape == (nb,) and same(flags, f) and n_diff is c
    assert one_call(rec, "crdt_set_digest_diff") == (P(da[0]), P(da[1]), P(db[0]), P(db[1]), nb, P(f), P(c))


def test_digest_diff_refuses():
    good = lambda: [i64(4), i64(4), i64(4), i64(4)]
    for i in range(1, 4):
        x = good()
        x[i] = i64(3)
        refuses(lambda e: e.digest_diff((x[0], x[1]), (x[2], x[3])), "digest_diff: the four arrays differ in length")
    refuses(lambda e: e.digest_diff(tuple(good()[:2]), tuple(good()[2:]), flags=u8(3)),
            "digest_diff: flags holds fewer entries than the digests have buckets")
    for i in range(4):
        def call(e, t):
            x = good()
            x[i] = t
            return e.digest_diff((x[0], x[1]), (x[2], x[3]))
        check_refuses_tensor(call, i64(4))
    check_refuses_tensor(lambda e, t: e.digest_diff(tuple(good()[:2]), tuple(good()[2:]), flags=t), u8(4))
    check_refuses_tensor(lambda e, t: e.digest_diff(tuple(good()[:2]), tuple(good()[2:]), n_diff=t), i64(1))


@pytest.mark.parametrize("n,m", product(NS, MS))
@pytest.mark.parametrize("lww", [True, False])
def test_set_select(n, m, lww):
    t, flags, mode = tuples(n), u8(m + 1), 0 if lww else 1
    for spl in (i64(m), None) if m == 0 else (i64(m),):
        check_tail(lambda e, **kw: e.set_select(t, lww, spl, flags, **kw), n, "crdt_set_select", 7, 8)
        for n_dev in (None, i64(1)):
            head = (mode, T(t), n, P(n_dev), P(spl) if m else None, m, P(flags))
            e, rec = stub(1)
            out, count = e.set_select(t, lww, spl, flags, n_dev=n_dev)
            assert one_call(rec, "crdt_set_select") == head + (T(out), None, P(count))
            e, rec = stub(1)
            count = e.set_select_count(t, lww, spl, flags, n_dev=n_dev)
            assert one_call(rec, "crdt_set_select") == head + (None, None, P(count))
            assert count.dtype == I64 and count.shape == (1,) and rec.status_reads() == []
    e, rec = stub(1)
    c = i64(1)
    assert e.set_select_count(t, lww, None, u8(1), count=c) is c
    assert one_call(rec, "crdt_set_select")[-1] == P(c)


def test_set_select_refuses():
    t, spl, flags = tuples(5), i64(3), u8(4)
    refuses(lambda e: e.set_select(t, True, spl, flags, out=tuples(4)), "set_select: out holds fewer tuples than t")
    msg = "set_select: src must be int64 and hold len(t) entries"
    refuses(lambda e: e.set_select(t, True, spl, flags, src=i64(4)), msg)
    refuses(lambda e: e.set_select(t, True, spl, flags, src=torch.zeros(5, dtype=torch.float64)), msg)
    check_refuses_tensor(lambda e, x: e.set_select(t, True, spl, flags, src=x), i64(5))
    check_refuses_tuples(lambda e, s: e.set_select(t, True, spl, flags, out=s))
    for meth in ("set_select", "set_select_count"):
        msg = "set_select: flags must hold len(splitters) + 1 entries"
        refuses(lambda e: getattr(e, meth)(t, False, spl, u8(3)), msg)
        refuses(lambda e: getattr(e, meth)(t, False, None, u8(0)), msg)
        check_refuses_tuples(lambda e, s: getattr(e, meth)(s, False, spl, flags))
        check_refuses_tensor(lambda e, x: getattr(e, meth)(t, False, x, flags), spl)
        check_refuses_tensor(lambda e, x: getattr(e, meth)(t, False, spl, x), flags)
        check_refuses_tensor(lambda e, x: getattr(e, meth)(t, False, spl, flags, n_dev=x), i64(1))
        check_refuses_tensor(lambda e, x: getattr(e, meth)(t, False, spl, flags, count=x), i64(1))


@pytest.mark.parametrize("n,m", product(NS, MS))
@pytest.mark.parametrize("lww", [True, False])
def test_map_select(n, m, lww):
    t, val, spl, flags = tuples(n), i32(n), i64(m), u8(m + 1)
    e, rec = stub(1)
    out, out_val, count = e.map_select(t, val, lww, spl, flags)
    args1, n_src = check_composite(rec, "crdt_set_select", 8, val, val[:0], out_val, count)
    assert args1[:8] == (0 if lww else 1, T(t), n, None, P(spl) if m else None, m, P(flags), T(out))
    assert n_src == max(n, 1) and fresh_tuples(out, n) and fresh(out_val, n, I32) and count.shape == (1,)
    refuses(lambda e: e.map_select(t, i32(n + 1), lww, spl, flags), "map_select: one value per tuple")


# ---------------------------------------------------------------- two faults at once: which refusal comes first
def test_refusal_order():
    def bad(field, dtype):                       # 5 tuples, one field of another element size
        s = tuples(5)
        setattr(s, field, torch.zeros(5, dtype=dtype))
        return s
    t, n32, meta = tuples(5), i32(1), torch.zeros(1, dtype=I64, device="meta")
    rep8, tomb8 = "expected 4-byte elements, got torch.int64", "expected 1-byte elements, got torch.int64"
    refuses(lambda e: e.lww_merge_src(bad("rep", I64), t, src=i64(3)), rep8)                 # tuples, then src
    refuses(lambda e: e.set_delta(bad("rep", I64), t, True, n_src_dev=n32), rep8)            # count, tuples, n_*_dev
    refuses(lambda e: e.set_delta(bad("rep", I64), t, True, count=meta), "tensor on meta, engine on cpu")
    refuses(lambda e: e.set_compact(bad("tomb", I64), True, i32(4)), tomb8)                  # count, tuples, cut / n_dev
    refuses(lambda e: e.set_compact_count(bad("tomb", I64), True, None, count=meta), "tensor on meta, engine on cpu")
    refuses(lambda e: e.map_read(t, True, win=i64(4), keys=i32(5)), "map_read: win must be int64 and hold len(t) rows")
    refuses(lambda e: e.map_read(t, True, keys=i64(4), n_dev=n32),
            "map_read: keys / nsib hold fewer rows than t has tuples")
    refuses(lambda e: e.map_lookup(t, i64(3), True, win=i64(2), nsib=i64(3)),
            "map_lookup: win must be int64 and hold one entry per probe")
    refuses(lambda e: e.map_lookup(t, i64(3), True, nsib=i32(2), n_dev=n32),
            "map_lookup: nsib holds fewer entries than there are probes")
    refuses(lambda e: e.causal_merge(t, i32(2), bad("rep", I64), None), rep8)                # count, tuples, contexts
    refuses(lambda e: e.causal_merge_count(t, None, bad("rep", I64), None, count=meta), "tensor on meta, engine on cpu")
    refuses(lambda e: e.causal_merge_ranges(t, None, bad("rep", I64), None, i64(3), u8(3)), rep8)   # ... then flags
    apply = lambda e, t_=t, rep=2, kinds=u8(3), **kw: e.set_apply_count(t_, i64(4), rep, i64(3), kinds, True, **kw)
    refuses(lambda e: apply(e, t_=bad("rep", I64), kinds=u8(2)), "set_apply: one kind per operation key")
    refuses(lambda e: apply(e, rep=-1, n_dev=n32), "set_apply: rep is a uint32")
    refuses(lambda e: apply(e, t_=bad("rep", I64), clock_out=i32(4)), rep8)
    refuses(lambda e: e.set_select(bad("rep", I64), True, i64(3), u8(3)),
            "set_select: flags must hold len(splitters) + 1 entries")
    refuses(lambda e: e.set_select_count(bad("rep", I64), True, i32(3), u8(4)), rep8)        # tuples, then splitters
