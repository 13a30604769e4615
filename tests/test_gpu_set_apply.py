"""GPU: the OR-Set mutators -- a batch of local adds and removes applied to a
sorted state on the device (crdt_set_apply; csrc/setapply.hip), in the
tombstone form and the causal form, bit-exact against the numpy restatement in
tests/apply_util.py (itself held to the one-operation-at-a-time definition by
tests/test_set_apply_ref.py), hand-written answers and the engine's own merges.

A tile of the kernels is T merged items of (state, the batch's tags); a count
thread takes 4 of them, a bitmap word 64."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import apply_util as au
import causal_util as cu
from crdt_amd import _lib
from crdt_amd.engine import TupleSet, as_u64, u64_tensor

pytestmark = pytest.mark.gpu

T = 2048                       # merged items per tile
DEV_RANGE = 2                  # CRDT_DEV_RANGE
E_INVAL, E_RANGE = -1, -6
M64 = 2**64 - 1
FORMS = [False, True]          # causal?


def _u64(eng, v):
    return u64_tensor(np.asarray(v, np.uint64).reshape(-1), eng.device)


def _u8(eng, v):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.uint8))).to(eng.device)


def _assert_tuples(got, exp, msg):
    for g, e, f in zip(got, exp, cu.FIELDS):
        np.testing.assert_array_equal(g, e, err_msg=f"{msg} {f}")


def _run(eng, t, clock, rep, keys, kinds, causal, exp=None, Ts=None, n_dev=None, msg=""):
    """Tuples, src, clock_out and count == exp (default: the restatement), the
    call without src and the count-only call agree, no device flag."""
    Ts = TupleSet.from_numpy(*t, eng.device) if Ts is None else Ts
    ck, K, Kd = _u64(eng, clock), _u64(eng, keys), _u8(eng, kinds)
    exp = au.apply_ref(t, clock, rep, keys, kinds, causal) if exp is None else exp
    out, src, co, cnt = eng.set_apply(Ts, ck, rep, K, Kd, causal, n_dev=n_dev, with_src=True, trim=False)
    plain, co2, cnt2 = eng.set_apply(Ts, ck, rep, K, Kd, causal, n_dev=n_dev, trim=False)
    co3 = torch.zeros_like(ck)
    only = eng.set_apply_count(Ts, ck, rep, K, Kd, causal, n_dev=n_dev, clock_out=co3)
    k = int(cnt.item())
    assert k == len(exp[0][0]), (msg, k, len(exp[0][0]))
    assert int(cnt2.item()) == k and int(only.item()) == k, msg
    got = out.slice(k).to_numpy()
    _assert_tuples(got, exp[0], msg)
    _assert_tuples(plain.slice(k).to_numpy(), exp[0], msg + " without src")
    gsrc = src[:k].cpu().numpy()
    np.testing.assert_array_equal(gsrc, exp[1], err_msg=msg + " src")
    for c in (co, co2, co3):
        np.testing.assert_array_equal(as_u64(c), exp[2], err_msg=msg + " clock_out")
    assert eng.device_status(clear=True) == 0, msg
    return got, gsrc


# ---- 1. known answers, written by hand
# t: key 5 holds a live tag of replica 0 and a tombstoned tag of replica 1, key 7 a live tag
KA_T = cu.tup([5, 5, 7], [1, 2, 1], [0, 1, 0], [0, 1, 0])
KA_CLOCK = [3, 3]              # replica 0 applies: the operations are its events 4, 5, 6
# per sequence of three operations on one key: the (ts, tomb) of the adds' tags in the tombstone form
KA_ADDS = {"aaa": [(4, 0), (5, 0), (6, 0)], "aar": [(4, 1), (5, 1)], "ara": [(4, 1), (6, 0)], "arr": [(4, 1)],
           "raa": [(5, 0), (6, 0)], "rar": [(5, 1)], "rra": [(6, 0)], "rrr": []}


def _known(seq, key, causal):
    """The hand-written answer for `seq` on key 5 (present in t) or 6 (absent)."""
    adds = KA_ADDS[seq]
    killed = 1 if ("r" in seq and key == 5) else 0       # any remove kills the key's tags in t
    rows = []                                            # (key, ts, rep, tomb, src)
    if not (causal and killed):
        rows.append((5, 1, 0, killed, 0))
    if not causal:
        rows.append((5, 2, 1, 1, 1))                     # tombstoned in t: kept as it is / absent
    mine = [(key, ts, 0, tomb, -(ts - 4 + 1)) for ts, tomb in adds if not (causal and tomb)]
    rows += mine                                         # key 5: after (5, 2, 1); key 6: between 5 and 7
    rows.append((7, 1, 0, 0, 2))
    cols = list(zip(*rows))
    return cu.tup(*cols[:4]), np.array(cols[4], np.int64), np.array([6, 3], np.uint64)


@pytest.mark.parametrize("causal", FORMS)
def test_known_answers_three_operations_on_one_key(eng, causal):
    for seq in KA_ADDS:
        kinds = [0 if c == "a" else 1 for c in seq]
        for key in (5, 6):
            exp = _known(seq, key, causal)
            ref = au.apply_ref(KA_T, KA_CLOCK, 0, [key] * 3, kinds, causal)
            _assert_tuples(ref[0], exp[0], f"restatement {seq} {key}")
            np.testing.assert_array_equal(ref[1], exp[1])
            _run(eng, KA_T, KA_CLOCK, 0, [key] * 3, kinds, causal, exp=exp, msg=f"{seq} on {key}")


@pytest.mark.parametrize("causal", FORMS)
def test_known_answers_outside_the_state(eng, causal):
    # add below the first key, remove of an absent key, add + remove and add above the last key: events 4 .. 8
    keys, kinds = [1, 2, 9, 9, 10], [0, 1, 0, 1, 0]
    if causal:
        exp = (cu.tup([1, 5, 7, 10], [4, 1, 1, 8], [0, 0, 0, 0], [0, 0, 0, 0]), np.array([-1, 0, 2, -5], np.int64))
    else:
        exp = (cu.tup([1, 5, 5, 7, 9, 10], [4, 1, 2, 1, 6, 8], [0, 0, 1, 0, 0, 0], [0, 0, 1, 0, 1, 0]),
               np.array([-1, 0, 1, 2, -3, -5], np.int64))
    _run(eng, KA_T, KA_CLOCK, 0, keys, kinds, causal, exp=exp + (np.array([8, 3], np.uint64),))


# ---- 2. tile boundaries: seeded states, a key space small enough that tag copies and key runs cross tiles
CLOCK4 = [100, 70, 64, 90]     # every ts of the generator is <= 64: the obligation holds for each replica


@functools.lru_cache(maxsize=16)
def _state(seed, n, ks=40):
    return au.rand_state(np.random.default_rng(seed), n, ks)


@pytest.mark.parametrize("n,m", [(0, 0), (0, 5), (7, 0), (2047, 1), (2048, 1), (2049, 3), (4101, 700), (6144, 2048)])
@pytest.mark.parametrize("causal", FORMS)
def test_tile_boundaries(eng, n, m, causal):
    t = _state(31, n)
    if n >= T - 1:                                       # the generator did what the case needs
        first, tor = cu.tags(t)
        assert len(first) < n and 0 < int(t[3].sum()) < n // 5
        assert (tor != t[3][first]).any()                # copies of a tag with differing tombs
    keys, kinds = au.rand_batch(np.random.default_rng(1000 + n + m), m, 42)
    _run(eng, t, CLOCK4, 2, keys, kinds, causal, msg=f"n {n} m {m}")


@pytest.mark.parametrize("causal", FORMS)
def test_one_tag_across_three_tiles(eng, causal):
    """5000 copies of one tag, the one tombstoned copy in the first tile: the
    tag's decision sits at its last copy, two tiles on."""
    n = 5000
    for at in (0, 4999, None):
        tomb = np.zeros(n, np.uint8)
        if at is not None:
            tomb[at] = 1
        t = cu.tup(np.full(n, 9), np.full(n, 3), np.full(n, 1), tomb)
        got, src = _run(eng, t, [5, 5], 0, [9], [0], causal, msg=f"tomb at {at}")
        assert src.tolist() == ([0, -1] if not (causal and at is not None) else [-1])


# ---- 3. the look-ahead witness: a remove merged into the middle tile of its key's run
@pytest.mark.parametrize("then_add", [False, True])
@pytest.mark.parametrize("causal", FORMS)
def test_remove_reaches_the_tiles_before_and_after_it(eng, causal, then_add):
    na, nb = 4500, 500
    # key 10: 4500 distinct tags of replica 1, ts 1 .. 4500; the batch's events start at 2251
    t = cu.tup(np.r_[np.full(na, 10), np.full(nb, 20)], np.r_[1:na + 1, 1:nb + 1], np.ones(na + nb), np.zeros(na + nb))
    clock = [2250, 4500]
    keys, kinds = ([10, 10], [1, 0]) if then_add else ([10], [1])
    # in merged order the remove's event 2251 lands in tile 1 of 3: the key's tags fill tiles 0, 1 and 2
    assert 2250 // T == 1 and (na + len(keys)) // T == 2
    got, src = _run(eng, t, clock, 0, keys, kinds, causal)
    k10 = got[0] == 10
    if causal:
        assert int(k10.sum()) == (1 if then_add else 0)
    else:
        dead = got[3][k10 & (got[2] == 1)]
        assert len(dead) == na and bool(dead.all())      # every tag of the key, in the tiles before and after
    if then_add:
        mine = k10 & (got[2] == 0)
        assert got[1][mine].tolist() == [2252] and got[3][mine].tolist() == [0] and src[mine].tolist() == [-2]
    k20 = got[0] == 20
    assert int(k20.sum()) == nb and not got[3][k20].any()
    np.testing.assert_array_equal(src[k20], np.arange(na, na + nb))


# ---- 4. identities against existing device code, bit for bit
@pytest.mark.parametrize("n", [1, 777, 4101])
def test_empty_batch_is_the_merge_with_nothing(eng, n):
    t = _state(32, n)
    Ts, E = TupleSet.from_numpy(*t, eng.device), TupleSet.from_numpy(*cu.empty(), eng.device)
    ck, nk, nd = _u64(eng, CLOCK4), _u64(eng, []), _u8(eng, [])
    out, src, co, cnt = eng.set_apply(Ts, ck, 1, nk, nd, False, with_src=True, trim=False)
    mo, mc, ms = eng.orset_merge_src(Ts, E)
    k = int(cnt.item())
    assert k == int(mc.item())
    _assert_tuples(out.slice(k).to_numpy(), mo.slice(k).to_numpy(), "tombstone form")
    assert torch.equal(src[:k], ms[:k])
    np.testing.assert_array_equal(as_u64(co), np.array(CLOCK4, np.uint64))
    out, co, cnt = eng.set_apply(Ts, ck, 1, nk, nd, True, trim=False)
    mo, _, mc = eng.causal_merge(Ts, ck, E, None)
    k = int(cnt.item())
    assert k == int(mc.item())
    _assert_tuples(out.slice(k).to_numpy(), mo.slice(k).to_numpy(), "causal form")
    assert eng.device_status(clear=True) == 0


@pytest.mark.parametrize("n,m", [(5, 9), (2049, 3), (4101, 700)])
def test_adds_only_batch_is_the_merge_with_its_tags(eng, n, m):
    t = _state(33, n)
    keys = np.sort(np.random.default_rng(n + m).integers(0, 42, m).astype(np.uint64))
    Ts = TupleSet.from_numpy(*t, eng.device)
    Bs = TupleSet.from_numpy(*au.batch_tags(CLOCK4, 3, keys), eng.device)
    out, co, cnt = eng.set_apply(Ts, _u64(eng, CLOCK4), 3, _u64(eng, keys), _u8(eng, np.zeros(m)), False, trim=False)
    mo = eng.orset_merge(Ts, Bs)
    assert int(cnt.item()) == len(mo)
    _assert_tuples(out.slice(len(mo)).to_numpy(), mo.to_numpy(), "adds only")
    assert eng.device_status(clear=True) == 0


# ---- 5. the length on the device
@pytest.mark.parametrize("causal", FORMS)
def test_device_length_hides_the_tail(eng, causal):
    n_max, n = 3000, 2100
    t = _state(34, n_max)
    keys, kinds = au.rand_batch(np.random.default_rng(5), 50, 42)
    # past *n_dev: live tags of the batch's keys with high ts, and a key below all -- each would change the answer
    bad = cu.tup(np.r_[keys[:10], np.zeros(n_max - n - 10)], np.full(n_max - n, 10**6), np.full(n_max - n, 1),
                 np.zeros(n_max - n))
    whole = tuple(np.concatenate([x[:n], y]) for x, y in zip(t, bad))
    Ts = TupleSet.from_numpy(*whole, eng.device)
    head = tuple(x[:n] for x in t)
    _run(eng, head, CLOCK4, 0, keys, kinds, causal, Ts=Ts, n_dev=_u64(eng, [n]))


def _sentinels(eng, cap, nc):
    out = TupleSet(torch.full((cap,), 7, dtype=torch.int64, device=eng.device),
                   torch.full((cap,), 7, dtype=torch.int64, device=eng.device),
                   torch.full((cap,), 7, dtype=torch.int32, device=eng.device),
                   torch.full((cap,), 7, dtype=torch.uint8, device=eng.device))
    return (out, torch.full((cap,), 7, dtype=torch.int64, device=eng.device),
            torch.full((nc,), 7, dtype=torch.int64, device=eng.device))


def _assert_poisoned(eng, out, src, co, cnt):
    assert int(as_u64(cnt)[0]) == M64
    assert eng.device_status(clear=True) == DEV_RANGE
    for x in (out.key, out.ts, out.rep, out.tomb, src, co):
        assert bool((x == 7).all())


@pytest.mark.parametrize("causal", FORMS)
def test_length_out_of_range_poisons(eng, causal):
    t = _state(35, 2500)
    Ts = TupleSet.from_numpy(*t, eng.device)
    out, src, co = _sentinels(eng, 2503, 4)
    cnt = torch.zeros(1, dtype=torch.int64, device=eng.device)
    args = (Ts, _u64(eng, CLOCK4), 0, _u64(eng, [1, 2, 3]), _u8(eng, [0, 1, 0]), causal)
    eng.set_apply(*args, n_dev=_u64(eng, [2501]), out=out, src=src, clock_out=co, count=cnt, trim=False)
    _assert_poisoned(eng, out, src, co, cnt)
    cnt.zero_()
    eng.set_apply_count(*args, n_dev=_u64(eng, [2501]), clock_out=co, count=cnt)
    _assert_poisoned(eng, out, src, co, cnt)


@pytest.mark.parametrize("causal", FORMS)
def test_event_wrap_poisons(eng, causal):
    t = _state(35, 2500)
    Ts = TupleSet.from_numpy(*t, eng.device)
    out, src, co = _sentinels(eng, 2503, 4)
    cnt = torch.zeros(1, dtype=torch.int64, device=eng.device)
    clock = [100, M64 - 1, 64, 90]                       # 2^64 - 2, then three events
    args = (Ts, _u64(eng, clock), 1, _u64(eng, [1, 2, 3]), _u8(eng, [0, 1, 0]), causal)
    eng.set_apply(*args, out=out, src=src, clock_out=co, count=cnt, trim=False)
    _assert_poisoned(eng, out, src, co, cnt)
    # from 2^64 - 3 two events still fit: 2^64 - 2 and 2^64 - 1
    _run(eng, t, [100, M64 - 2, 64, 90], 1, [1, 2], [0, 0], causal, msg="the last two events")


# ---- 6. views at odd element offsets
@pytest.mark.parametrize("causal", FORMS)
def test_offset_views(eng, causal):
    n, m = 2600, 40
    t = _state(36, n)
    keys, kinds = au.rand_batch(np.random.default_rng(6), m, 42)

    def view(cols, off, cap):
        full = TupleSet.empty(cap + off + 3, eng.device)
        v = TupleSet(full.key[off:off + cap], full.ts[off:off + cap], full.rep[off:off + cap],
                     full.tomb[off:off + cap])
        if cols is not None:
            for dst, s in zip((v.key, v.ts, v.rep, v.tomb), TupleSet.from_numpy(*cols, eng.device).__dict__.values()):
                dst.copy_(s)
        return v

    Ts, O = view(t, 1, n), view(None, 3, n + m)
    assert Ts.key.data_ptr() % 16 == 8 and Ts.rep.data_ptr() % 8 == 4 and O.tomb.data_ptr() % 2 == 1
    kbuf = torch.zeros(m + 1, dtype=torch.int64, device=eng.device)
    kbuf[1:].copy_(_u64(eng, keys))
    dbuf = torch.zeros(m + 1, dtype=torch.uint8, device=eng.device)
    dbuf[1:].copy_(_u8(eng, kinds))
    sbuf = torch.zeros(n + m + 1, dtype=torch.int64, device=eng.device)
    exp = au.apply_ref(t, CLOCK4, 0, keys, kinds, causal)
    out, src, co, cnt = eng.set_apply(Ts, _u64(eng, CLOCK4), 0, kbuf[1:], dbuf[1:], causal, out=O, src=sbuf[1:],
                                      trim=False)
    k = int(cnt.item())
    assert k == len(exp[0][0])
    _assert_tuples(O.slice(k).to_numpy(), exp[0], "offset views")
    np.testing.assert_array_equal(sbuf[1:1 + k].cpu().numpy(), exp[1])
    np.testing.assert_array_equal(as_u64(co), exp[2])
    assert eng.device_status(clear=True) == 0


# ---- 7. chaining with no read-back
@pytest.mark.parametrize("causal", FORMS)
def test_map_apply_moves_the_values(eng, causal):
    n, m = 4101, 300
    t = _state(37, n)
    keys, kinds = au.rand_batch(np.random.default_rng(7), m, 42)
    val = torch.arange(n, dtype=torch.int32, device=eng.device) + 1000
    oval = -torch.arange(m, dtype=torch.int32, device=eng.device) - 1
    out, ov, co, cnt = eng.map_apply(TupleSet.from_numpy(*t, eng.device), val, _u64(eng, CLOCK4), 2, _u64(eng, keys),
                                     _u8(eng, kinds), oval, causal)
    exp, esrc, eclk = au.apply_ref(t, CLOCK4, 2, keys, kinds, causal)
    k = int(cnt.item())
    assert k == len(esrc) and (esrc >= 0).any() and (esrc < 0).any()
    _assert_tuples(out.slice(k).to_numpy(), exp, "map_apply")
    np.testing.assert_array_equal(ov[:k].cpu().numpy(), np.where(esrc >= 0, esrc + 1000, esrc).astype(np.int32))
    np.testing.assert_array_equal(as_u64(co), eclk)
    assert eng.device_status(clear=True) == 0


@pytest.mark.parametrize("causal", FORMS)
def test_set_elements_straight_off_the_apply(eng, causal):
    t = _state(38, 3000)
    keys, kinds = au.rand_batch(np.random.default_rng(8), 200, 42)
    out, co, cnt = eng.set_apply(TupleSet.from_numpy(*t, eng.device), _u64(eng, CLOCK4), 0, _u64(eng, keys),
                                 _u8(eng, kinds), causal, trim=False)
    ek, ec = eng.set_elements(out, False, n_dev=cnt)
    exp = au.apply_ref(t, CLOCK4, 0, keys, kinds, causal)[0]
    np.testing.assert_array_equal(as_u64(ek)[:int(ec.item())], cu.live_keys(exp))
    assert eng.device_status(clear=True) == 0


# ---- 8. a replica history on the device, both forms
def test_history_on_the_device(eng):
    rng = np.random.default_rng(41)
    R = 4
    tomb = [cu.empty() for _ in range(R)]
    dots = [cu.empty() for _ in range(R)]
    clock = [np.zeros(R, np.uint64) for _ in range(R)]
    dev = lambda t: TupleSet.from_numpy(*t, eng.device)
    applied = merged = 0
    for step in range(40):
        x = int(rng.integers(R))
        if rng.random() < 0.6:
            keys, kinds = au.rand_batch(rng, int(rng.integers(0, 7)), 10)
            ck, K, Kd = _u64(eng, clock[x]), _u64(eng, keys), _u8(eng, kinds)
            gt, c1, _ = eng.set_apply(dev(tomb[x]), ck, x, K, Kd, False)
            gd, c2, _ = eng.set_apply(dev(dots[x]), ck, x, K, Kd, True)
            et, _, ec = au.apply_ref(tomb[x], clock[x], x, keys, kinds, False)
            ed = au.apply_ref(dots[x], clock[x], x, keys, kinds, True)[0]
            assert torch.equal(c1, c2)
            np.testing.assert_array_equal(as_u64(c1), ec)
            applied += 1
        else:
            y = int((x + 1 + rng.integers(R - 1)) % R)
            gt = eng.orset_merge(dev(tomb[x]), dev(tomb[y]))
            gd, c1, _ = eng.causal_merge(dev(dots[x]), _u64(eng, clock[x]), dev(dots[y]), _u64(eng, clock[y]), trim=True)
            et = au.orset_merge(tomb[x], tomb[y])
            ed, _, ec, _ = cu.ref_causal(dots[x], clock[x], dots[y], clock[y])
            np.testing.assert_array_equal(as_u64(c1), ec)
            merged += 1
        gt, gd = gt.to_numpy(), gd.to_numpy()
        _assert_tuples(gt, et, f"step {step} tombstone form")
        _assert_tuples(gd, ed, f"step {step} causal form")
        _assert_tuples(cu.present(gt), gd, f"step {step} present(tombstone form) == causal form")
        tomb[x], dots[x], clock[x] = et, ed, ec
    assert applied > 10 and merged > 8
    assert eng.device_status(clear=True) == 0


# ---- 9. host errors
def test_host_errors(eng):
    t = _state(39, 1000)
    Ts, O = TupleSet.from_numpy(*t, eng.device), TupleSet.empty(1010, eng.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=eng.device)
    src = torch.zeros(1010, dtype=torch.int64, device=eng.device)
    ck, co = _u64(eng, CLOCK4), torch.zeros(4, dtype=torch.int64, device=eng.device)
    K, Kd = _u64(eng, np.arange(10)), _u8(eng, np.arange(10) % 2)
    nd = _u64(eng, [1000])
    ct, cout, cp, sp = Ts.c(), O.c(), cnt.data_ptr(), src.data_ptr()
    xc, xo, xk, xd = ck.data_ptr(), co.data_ptr(), K.data_ptr(), Kd.data_ptr()
    ref = lambda x: C.byref(x) if x is not None else None

    def raw(tt=ct, o=cout, s=sp, count=cp, form=0, n=1000, ndv=None, clock=xc, nc=4, rep=0, keys=xk, kinds=xd, m=10,
            po=xo, ctx=eng.ctx):
        eng._bind()
        with pytest.raises(_lib.CrdtError) as ei:
            _lib.call("crdt_set_apply", ctx, form, ref(tt), n, ndv, clock, nc, rep, keys, kinds, m, ref(o), s, po, count,
                      ctx=eng.ctx)
        return ei.value.status

    def fld(x, **kw):
        f = {"key": x.key.data_ptr(), "ts": x.ts.data_ptr(), "rep": x.rep.data_ptr(), "tomb": x.tomb.data_ptr()}
        f.update(kw)
        return _lib.crdt_tuples(f["key"], f["ts"], f["rep"], f["tomb"])

    assert raw(ctx=None) == E_INVAL                          # NULL ctx / t / count / clock
    assert raw(tt=None) == E_INVAL
    assert raw(count=None) == E_INVAL
    assert raw(clock=None) == E_INVAL
    assert raw(rep=4) == E_INVAL                             # rep >= n_clock
    assert raw(nc=0) == E_INVAL
    assert raw(form=2) == E_INVAL and raw(form=-1) == E_INVAL
    for f, by in (("key", 4), ("ts", 4), ("rep", 2)):
        assert raw(tt=fld(Ts, **{f: None})) == E_INVAL       # NULL fields, natural alignment
        assert raw(o=fld(O, **{f: None})) == E_INVAL
        assert raw(tt=fld(Ts, **{f: getattr(Ts, f).data_ptr() + by})) == E_INVAL
        assert raw(o=fld(O, **{f: getattr(O, f).data_ptr() + by})) == E_INVAL
    assert raw(tt=fld(Ts, tomb=None)) == E_INVAL and raw(o=fld(O, tomb=None)) == E_INVAL
    none = _lib.crdt_tuples(None, None, None, None)
    assert raw(tt=none, n=0, o=none) == E_INVAL              # out fields NULL with n_max + m > 0
    assert raw(keys=None) == E_INVAL and raw(kinds=None) == E_INVAL
    assert raw(keys=xk + 4) == E_INVAL                       # 8-byte alignment
    assert raw(clock=xc + 4) == E_INVAL
    assert raw(po=xo + 4) == E_INVAL
    assert raw(s=sp + 4) == E_INVAL
    assert raw(ndv=nd.data_ptr() + 4) == E_INVAL
    assert raw(count=cp + 4) == E_INVAL
    assert raw(o=None) == E_INVAL                            # src without out
    assert raw(o=ct) == E_INVAL                              # outputs overlapping inputs and each other
    assert raw(o=fld(O, ts=Ts.ts.data_ptr() + 8 * 999)) == E_INVAL
    assert raw(o=fld(O, key=xk + 8 * 9)) == E_INVAL
    assert raw(o=fld(O, tomb=xd + 9)) == E_INVAL
    assert raw(o=fld(O, key=xc + 8 * 3)) == E_INVAL
    assert raw(o=fld(O, key=nd.data_ptr()), ndv=nd.data_ptr()) == E_INVAL
    assert raw(o=fld(O, key=sp)) == E_INVAL
    assert raw(o=fld(O, ts=xo)) == E_INVAL
    assert raw(o=fld(O, ts=cp)) == E_INVAL
    assert raw(s=Ts.key.data_ptr()) == E_INVAL
    assert raw(s=xo) == E_INVAL
    assert raw(po=xc) == E_INVAL
    assert raw(po=xk) == E_INVAL
    assert raw(po=cp) == E_INVAL
    assert raw(count=xc) == E_INVAL
    assert raw(n=2**62, o=None, s=None) == E_RANGE
    assert raw(m=2**62, o=None, s=None) == E_RANGE
    assert raw(nc=2**32, o=None, s=None) == E_RANGE
    assert raw(n=2**61, m=2**61, o=None, s=None) == E_RANGE  # more tiles than a launch holds
    assert int(cnt.item()) == 0 and eng.device_status(clear=True) == 0
    # n_max + m == 0: nothing but the count store and the clock write
    cnt.fill_(5)
    _lib.call("crdt_set_apply", eng.ctx, 1, C.byref(none), 0, None, xc, 4, 3, None, None, 0, None, None, xo, cp,
              ctx=eng.ctx)
    assert int(cnt.item()) == 0
    np.testing.assert_array_equal(as_u64(co), np.array(CLOCK4, np.uint64))
    assert eng.device_status(clear=True) == 0
