"""CPU: the Engine's wrappers of cmap_combine / cmap_add / cmap_from_ops /
cmap_ingest over tests/engine_stub.py's stub(): which C function each would
call, with which pointers and lengths, what it refuses before any call, and
what it hands back.  No kernel runs."""
import ctypes as C

import pytest
import torch

import engine_stub as es
from crdt_amd import _lib
from crdt_amd.engine import CounterMap

COUNTED = {"crdt_cmap_combine", "crdt_cmap_add", "crdt_cmap_from_ops"}   # the last argument: the int64[1] count written


class Recorder(es.Recorder):
    """engine_stub's recorder with this family's counted calls."""

    def __call__(self, fn, *args):
        super().__call__(fn, *args)
        if fn in COUNTED and fn not in es.COUNTED:
            C.c_int64.from_address(args[-1]).value = self.k


def stub(k=0, status=0):
    e, _ = es.stub()
    e._call = rec = Recorder(k, status)
    return e, rec


def cmap(n, base=0):
    return CounterMap(torch.arange(base, base + n, dtype=torch.int64), torch.zeros(n, dtype=torch.int32),
                      torch.arange(n, dtype=torch.int64) + 3, torch.arange(n, dtype=torch.int64) + 5)


def M(a):
    if a is None:
        return None
    assert isinstance(a, _lib.crdt_cmap)
    return (a.key, a.rep, a.p, a.n)


def Mp(s):
    return tuple(t.data_ptr() or None for t in (s.key, s.rep, s.p, s.n))


def one(rec, fn):
    calls = [c for c in rec.c_calls() if c[0] == fn]
    assert len(calls) == 1, rec.calls
    return calls[0][1]


# ---------------------------------------------------------------- cmap_combine
def test_combine_passes_pointers_and_lengths_and_allocates():
    e, rec = stub(k=4)
    t, nd = cmap(9), es.i64(1)
    out, cnt = e.cmap_combine(t, n_dev=nd)
    a = one(rec, "crdt_cmap_combine")
    assert M(a[0]) == Mp(t) and a[1:5] == (9, es.P(nd), None, 0)
    assert M(a[5]) == Mp(out) and a[6] == es.P(cnt)
    assert isinstance(out, CounterMap) and len(out) == 9 and int(cnt.item()) == 4
    assert not rec.status_reads()


def test_combine_with_idx_passes_the_source_length():
    e, rec = stub()
    src_p, src_n, idx = es.i64(20), es.i64(20), es.i32(9)
    t = CounterMap(es.i64(9), es.i32(9), src_p, src_n)
    e.cmap_combine(t, idx=idx)
    a = one(rec, "crdt_cmap_combine")
    assert a[1:5] == (9, None, es.P(idx), 20)


def test_combine_trim_given_outputs_and_count_alone():
    e, rec = stub(k=4)
    out, cnt = e.cmap_combine(cmap(9), trim=True)
    assert len(out) == 4 and len(rec.status_reads()) == 1
    given, gc = cmap(9, 100), es.i64(1)
    out, cnt = e.cmap_combine(cmap(9), out=given, count=gc)
    assert out is given and cnt is gc
    e, rec = stub(k=6)
    cnt = e.cmap_combine_count(cmap(9))
    a = one(rec, "crdt_cmap_combine")
    assert a[5] is None and a[6] == es.P(cnt) and int(cnt.item()) == 6
    e, rec = stub(k=4, status=2)
    with pytest.raises(_lib.CrdtLibraryError):
        e.cmap_combine(cmap(9), trim=True)


def test_combine_refusals_come_before_any_call():
    e, rec = stub()
    t = cmap(5)
    with pytest.raises(ValueError):
        e.cmap_combine(t, out=cmap(4))                     # short out
    with pytest.raises(ValueError):
        e.cmap_combine(t, idx=es.i32(4))                   # one index per cell
    with pytest.raises(ValueError):
        e.cmap_combine(t, idx=es.i64(5))                   # indices are 4-byte
    with pytest.raises(ValueError):
        e.cmap_combine(CounterMap(t.key, t.rep, es.i64(9), es.i64(9)))   # without idx, one p per key
    with pytest.raises(ValueError):
        e.cmap_combine(CounterMap(t.key, t.rep, es.i64(9), es.i64(8)), idx=es.i32(5))
    with pytest.raises(ValueError):
        e.cmap_combine(t, count=es.i32(1))
    assert not rec.c_calls()


# ---------------------------------------------------------------- cmap_add
def test_add_passes_both_sides_and_their_device_lengths():
    e, rec = stub(k=3)
    t, d, nt, nd = cmap(8), cmap(6, 50), es.i64(1), es.i64(1)
    out, cnt = e.cmap_add(t, d, n_t_dev=nt, n_d_dev=nd)
    a = one(rec, "crdt_cmap_add")
    assert M(a[0]) == Mp(t) and a[1:3] == (8, es.P(nt)) and M(a[3]) == Mp(d) and a[4:6] == (6, es.P(nd))
    assert M(a[6]) == Mp(out) and a[7] == es.P(cnt) and len(out) == 14 and int(cnt.item()) == 3
    assert not rec.status_reads()
    cnt = e.cmap_add_count(t, d)
    assert rec.c_calls()[-1][1][6] is None and int(cnt.item()) == 3
    with pytest.raises(ValueError):
        e.cmap_add(t, d, out=cmap(13))
    with pytest.raises(ValueError):
        e.cmap_add(t, CounterMap(d.key, es.i64(6), d.p, d.n))
    assert len(rec.c_calls()) == 2


# ---------------------------------------------------------------- cmap_from_ops
def test_from_ops_passes_the_columns():
    e, rec = stub(k=5)
    k, r, dp, dn = es.i64(7), es.i32(7), es.i64(7), es.i64(7)
    out, cnt = e.cmap_from_ops(k, r, dp, dn)
    a = one(rec, "crdt_cmap_from_ops")
    assert a[:5] == (es.P(k), es.P(r), es.P(dp), es.P(dn), 7) and M(a[5]) == Mp(out) and a[6] == es.P(cnt)
    assert len(out) == 7 and int(cnt.item()) == 5 and not rec.status_reads()


def test_from_ops_of_no_operations_passes_nulls():
    e, rec = stub()
    out, cnt = e.cmap_from_ops(es.i64(0), es.i32(0), es.i64(0), es.i64(0))
    a = one(rec, "crdt_cmap_from_ops")
    assert a[:5] == (None, None, None, None, 0) and len(out) == 1


def test_from_ops_refusals_come_before_any_call():
    e, rec = stub()
    with pytest.raises(ValueError):
        e.cmap_from_ops(es.i64(7), es.i32(6), es.i64(7), es.i64(7))
    with pytest.raises(ValueError):
        e.cmap_from_ops(es.i64(7), es.i32(7), es.i64(7), es.i64(8))
    with pytest.raises(ValueError):
        e.cmap_from_ops(es.i64(7), es.i64(7), es.i64(7), es.i64(7))     # reps are 4-byte
    with pytest.raises(ValueError):
        e.cmap_from_ops(es.i64(7), es.i32(7), es.i64(7), es.i64(7), out=cmap(6))
    assert not rec.c_calls()


# ---------------------------------------------------------------- cmap_ingest
def test_ingest_is_from_ops_then_add_off_the_device_count():
    e, rec = stub(k=5)
    t, nt = cmap(8), es.i64(1)
    k, r, dp, dn = es.i64(7), es.i32(7), es.i64(7), es.i64(7)
    out, cnt = e.cmap_ingest(t, k, r, dp, dn, n_t_dev=nt)
    fns = [fn for fn, _ in rec.c_calls()]
    assert fns == ["crdt_cmap_from_ops", "crdt_cmap_add"] and not rec.status_reads()
    f, a = rec.c_calls()[0][1], rec.c_calls()[1][1]
    assert M(a[0]) == Mp(t) and a[1:3] == (8, es.P(nt))
    assert M(a[3]) == M(f[5]) and a[4] == 7 and a[5] == f[6]              # the batch, its capacity, its device count
    assert M(a[6]) == Mp(out) and len(out) == 15 and a[7] == es.P(cnt)
