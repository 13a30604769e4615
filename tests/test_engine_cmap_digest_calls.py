"""CPU: the Engine's wrappers of the counter map's range digests
(cmap_digest / cmap_select / cmap_select_count) and reconcile.cmap_round, over
tests/engine_stub.py's stub(): which C function each would call, with which
pointers and lengths, what it refuses before any call, and what it hands back.
No kernel runs."""
import ctypes as C

import pytest
import torch

import engine_stub as es
from crdt_amd import _lib, reconcile
from crdt_amd.engine import CounterMap

COUNTED = {"crdt_cmap_select", "crdt_cmap_merge", "crdt_set_digest_diff"}   # the last argument: the int64[1] count written


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
    """A recorded by-reference crdt_cmap as its four pointers (None for a NULL out)."""
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


# ---------------------------------------------------------------- cmap_digest
def test_digest_passes_pointers_and_lengths():
    e, rec = stub()
    t, sp, nd = cmap(9), es.i64(4), es.i64(1)
    h, c = e.cmap_digest(t, sp, n_dev=nd)
    a = one(rec, "crdt_cmap_digest")
    assert M(a[0]) == Mp(t) and a[1:] == (9, es.P(nd), es.P(sp), 4, es.P(h), es.P(c))
    assert h.dtype == c.dtype == torch.int64 and h.numel() == c.numel() == 5
    assert not rec.status_reads()


@pytest.mark.parametrize("sp", [None, "empty"])
def test_digest_without_splitters_passes_null(sp):
    e, rec = stub()
    t = cmap(3)
    h, c = e.cmap_digest(t, None if sp is None else es.i64(0))
    a = one(rec, "crdt_cmap_digest")
    assert a[1:5] == (3, None, None, 0) and h.numel() == c.numel() == 1


def test_digest_given_outputs_are_used_and_checked():
    e, rec = stub()
    t, sp = cmap(3), es.i64(4)
    ho, co = es.i64(5), es.i64(7)
    h, c = e.cmap_digest(t, sp, hash_out=ho, count_out=co)
    assert h is ho and c is co
    assert one(rec, "crdt_cmap_digest")[5:] == (es.P(ho), es.P(co))
    for bad in (dict(hash_out=es.i64(4)), dict(count_out=es.i64(4)), dict(hash_out=es.i32(8)),
                dict(count_out=es.i64(10)[::2])):
        with pytest.raises(ValueError):
            e.cmap_digest(t, sp, **bad)
    with pytest.raises(ValueError):
        e.cmap_digest(t, es.i32(4))                       # splitters are 8-byte
    with pytest.raises(ValueError):
        e.cmap_digest(CounterMap(t.key, es.i64(3), t.p, t.n), sp)   # rep is 4-byte
    assert len(rec.c_calls()) == 1


# ---------------------------------------------------------------- cmap_select
def test_select_passes_pointers_and_lengths_and_allocates():
    e, rec = stub(k=4)
    t, sp, fl, nd = cmap(9), es.i64(2), es.u8(3), es.i64(1)
    out, cnt = e.cmap_select(t, sp, fl, n_dev=nd)
    a = one(rec, "crdt_cmap_select")
    assert M(a[0]) == Mp(t) and a[1:6] == (9, es.P(nd), es.P(sp), 2, es.P(fl))
    assert M(a[6]) == Mp(out) and a[7] == es.P(cnt)
    assert isinstance(out, CounterMap) and len(out) == 9 and int(cnt.item()) == 4
    assert (out.key.dtype, out.rep.dtype, out.p.dtype, out.n.dtype) == (torch.int64, torch.int32, torch.int64, torch.int64)
    assert not rec.status_reads()                          # no trim: no synchronisation


def test_select_trim_reads_the_status_once_and_cuts():
    e, rec = stub(k=4)
    out, cnt = e.cmap_select(cmap(9), None, es.u8(1), trim=True)
    assert len(out) == 4 and int(cnt.item()) == 4 and len(rec.status_reads()) == 1
    assert one(rec, "crdt_cmap_select")[2:5] == (None, None, 0)
    e, rec = stub(k=4, status=2)
    with pytest.raises(_lib.CrdtLibraryError):
        e.cmap_select(cmap(9), None, es.u8(1), trim=True)


def test_select_given_out_and_count():
    e, rec = stub(k=2)
    t, given, gc = cmap(5), cmap(6, 100), es.i64(1)
    out, cnt = e.cmap_select(t, es.i64(3), es.u8(4), out=given, count=gc)
    assert out is given and cnt is gc and int(gc.item()) == 2
    a = one(rec, "crdt_cmap_select")
    assert M(a[6]) == Mp(given) and a[7] == es.P(gc)


def test_select_of_an_empty_map_still_has_a_buffer():
    e, rec = stub()
    out, cnt = e.cmap_select(cmap(0), None, es.u8(1))
    assert len(out) == 1 and one(rec, "crdt_cmap_select")[1] == 0


def test_select_refusals_come_before_any_call():
    e, rec = stub()
    t, sp = cmap(5), es.i64(3)
    with pytest.raises(ValueError):
        e.cmap_select(t, sp, es.u8(4), out=cmap(4))        # short out
    with pytest.raises(ValueError):
        e.cmap_select(t, sp, es.u8(3))                     # short flags
    with pytest.raises(ValueError):
        e.cmap_select_count(t, sp, es.u8(3))
    with pytest.raises(ValueError):
        e.cmap_select(t, sp, es.i32(4))                    # flags are bytes
    with pytest.raises(ValueError):
        e.cmap_select(t, sp, es.u8(4), count=es.i32(1))
    with pytest.raises(ValueError):
        e.cmap_select(t, sp, es.u8(8)[::2])
    assert not rec.c_calls()


def test_select_count_passes_a_null_out():
    e, rec = stub(k=7)
    t, sp, fl = cmap(9), es.i64(2), es.u8(3)
    cnt = e.cmap_select_count(t, sp, fl)
    a = one(rec, "crdt_cmap_select")
    assert M(a[0]) == Mp(t) and a[6] is None and a[7] == es.P(cnt) and int(cnt.item()) == 7
    gc = es.i64(1)
    assert e.cmap_select_count(t, sp, fl, count=gc) is gc


# ---------------------------------------------------------------- reconcile.cmap_round
def test_round_is_digests_diff_selections_and_two_merges():
    e, rec = stub(k=3)
    A, B, sp = cmap(8), cmap(6, 50), es.i64(4)
    (ma, ca), (mb, cb), flags, (ship_a, ship_b) = reconcile.cmap_round(e, A, B, sp)
    fns = [fn for fn, _ in rec.c_calls()]
    assert fns == ["crdt_cmap_digest", "crdt_cmap_digest", "crdt_set_digest_diff", "crdt_cmap_select",
                   "crdt_cmap_select", "crdt_cmap_merge", "crdt_cmap_merge"]
    assert not rec.status_reads()                          # no read-back anywhere
    calls = rec.c_calls()
    assert M(calls[0][1][0]) == Mp(A) and M(calls[1][1][0]) == Mp(B)
    assert calls[2][1][4] == 5 and calls[2][1][5] == es.P(flags) and flags.numel() == 5
    sel_a, sel_b = calls[3][1], calls[4][1]
    assert M(sel_a[0]) == Mp(A) and M(sel_b[0]) == Mp(B) and sel_a[5] == sel_b[5] == es.P(flags)
    assert sel_a[7] == es.P(ship_a) and sel_b[7] == es.P(ship_b)
    m1, m2 = calls[5][1], calls[6][1]
    # merge(A, sel(B)) at B's capacity with the selection's device count, and the mirror
    assert M(m1[0]) == Mp(A) and m1[1:3] == (8, None) and M(m1[3]) == M(sel_b[6]) and m1[4:6] == (6, es.P(ship_b))
    assert M(m2[0]) == Mp(B) and m2[1:3] == (6, None) and M(m2[3]) == M(sel_a[6]) and m2[4:6] == (8, es.P(ship_a))
    assert M(m1[6]) == Mp(ma) and M(m2[6]) == Mp(mb) and len(ma) == len(mb) == 14
    assert m1[7] == es.P(ca) and m2[7] == es.P(cb)


def test_round_of_empty_maps():
    e, rec = stub()
    (ma, ca), (mb, cb), flags, _ = reconcile.cmap_round(e, cmap(0), cmap(0), None)
    calls = rec.c_calls()
    assert calls[0][1][1:5] == (0, None, None, 0) and flags.numel() == 1
    assert calls[5][1][1] == 0 and calls[5][1][4] == 0
