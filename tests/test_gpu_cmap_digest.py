"""GPU: range digests of the keyed PN-Counter map (crdt_cmap_digest /
crdt_cmap_select; kernels in csrc/countermap.hpp over csrc/digest.hpp, entry
points in csrc/counters.hip) and crdt_amd.reconcile.cmap_round against the two
CPU restatements of tests/cmap_digest_util.py, bit for bit, with the device
status 0 after every exact call.

A tile is T = 2048 cells, a wave takes 8 consecutive 64-cell words (512 cells).
The hand-built cases put splitters, key runs and flagged buckets on and across
those edges and assert on the CPU that they lie where they are meant to before
the GPU runs."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cmap_digest_util as du
import cmap_util as cu
import test_gpu_cmap as t_cmap
from crdt_amd import _lib, reconcile
from crdt_amd.engine import CounterMap, as_u64, u64_tensor
from test_gpu_cmap import _cut, _dev, _eq, _n, _poisoned, _take, _up

pytestmark = pytest.mark.gpu

T = 2048
N = 3 * T + 17
DEV_RANGE = 2                  # CRDT_DEV_RANGE
E_INVAL, E_RANGE = -1, -6
M64 = 2**64 - 1
U64, U32 = np.uint64, np.uint32
LENGTHS = [0, 1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, N]
CANARY = 0x5a


# ---------------------------------------------------------------- helpers
def _sp(eng, sp):
    return u64_tensor(np.asarray(sp, dtype=U64), eng.device)


def _fl(eng, flags):
    return torch.from_numpy(np.ascontiguousarray(flags, dtype=np.uint8)).to(eng.device)


def _canary_map(eng, n):
    out = CounterMap.empty(n, eng.device)
    for x in (out.key, out.rep, out.p, out.n):
        x.fill_(CANARY)
    return out


def _untouched(out, start=0):
    return all(bool((x[start:] == CANARY).all()) for x in (out.key, out.rep, out.p, out.n))


def check_digest(eng, t, sp, Tt=None, n=None, what="digest"):
    """The digest of t (its first n cells, as a device length) two ways: allocated outputs, given
    outputs one entry longer than asked (the entry behind stays as it was)."""
    Tt = Tt or _up(eng, t)
    sp = np.asarray(sp, dtype=U64)
    m = len(sp)
    et = t if n is None else _cut(t, n)
    exp = du.digest_np(et, sp)
    assert int(exp[1].sum()) == len(et[0])
    if len(et[0]) <= 64 and m <= 64:
        assert all(np.array_equal(x, y) for x, y in zip(du.digest_d(et, sp), exp)), what + ": the restatements"
    kw = dict(n_dev=None if n is None else _dev(eng, n))
    SP = _sp(eng, sp)
    h, c = eng.cmap_digest(Tt, SP, **kw)
    assert h.numel() == c.numel() == m + 1
    for name, g, e in (("hash", h, exp[0]), ("count", c, exp[1])):
        bad = np.flatnonzero(as_u64(g) != e)
        assert bad.size == 0, f"{what}: {name} differs at buckets {bad[:5]}: got {as_u64(g)[bad[:5]]}, expected {e[bad[:5]]}"
    gh = torch.full((m + 2,), CANARY, dtype=torch.int64, device=eng.device)
    gc = torch.full((m + 2,), CANARY, dtype=torch.int64, device=eng.device)
    h2, c2 = eng.cmap_digest(Tt, SP if m else None, hash_out=gh, count_out=gc, **kw)
    assert h2 is gh and c2 is gc
    assert np.array_equal(as_u64(gh)[:m + 1], exp[0]) and np.array_equal(as_u64(gc)[:m + 1], exp[1]), what + " (given)"
    assert int(gh[m + 1]) == CANARY and int(gc[m + 1]) == CANARY, what + ": an entry past m + 1 was written"
    assert eng.device_status(clear=True) == 0, what
    return exp


def check_select(eng, t, sp, flags, Tt=None, n=None, what="select"):
    """The selection four ways: allocated output, a given output longer than t under a canary (nothing
    at or past the count is written, so nothing at or past n_max either), trim, the count alone."""
    Tt = Tt or _up(eng, t)
    sp, flags = np.asarray(sp, dtype=U64), np.asarray(flags, dtype=np.uint8)
    assert len(flags) == len(sp) + 1
    et = t if n is None else _cut(t, n)
    exp = du.select_np(et, sp, flags)
    if len(et[0]) <= 64 and len(sp) <= 64:
        assert cu.same(du.select_d(et, sp, flags), exp), what + ": the restatements"
    k = len(exp[0])
    kw = dict(n_dev=None if n is None else _dev(eng, n))
    SP, FL = _sp(eng, sp), _fl(eng, flags)
    out, cnt = eng.cmap_select(Tt, SP, FL, **kw)
    _eq(_take(out, cnt), exp, what)
    given, gc = _canary_map(eng, len(Tt) + 5), torch.full((1,), -5, dtype=torch.int64, device=eng.device)
    out2, cnt2 = eng.cmap_select(Tt, SP if len(sp) else None, FL, out=given, count=gc, **kw)
    assert out2 is given and cnt2 is gc
    _eq(_take(given, gc), exp, what + " (given outputs)")
    assert _untouched(given, k), what + ": a cell at or past the count was written"
    out3, cnt3 = eng.cmap_select(Tt, SP, FL, trim=True, **kw)
    assert len(out3) == k and _n(cnt3) == k
    _eq(out3.to_numpy(), exp, what + " (trim)")
    assert _n(eng.cmap_select_count(Tt, SP, FL, **kw)) == k, what + " (count alone)"
    assert eng.device_status(clear=True) == 0, what
    return exp


def _alternating(m):
    return (np.arange(m + 1) % 2).astype(np.uint8)


def _flag_sets(m):
    first, last = np.zeros(m + 1, np.uint8), np.zeros(m + 1, np.uint8)
    first[0], last[m] = 1, 1
    return {"all": np.ones(m + 1, np.uint8), "none": np.zeros(m + 1, np.uint8), "alternating": _alternating(m),
            "first": first, "last": last}


@functools.lru_cache(maxsize=None)
def _state():
    """N cells, about four replicas a key, the keys spread over the whole uint64 range."""
    t = cu.random_state(np.random.default_rng(21), N, N // 4)
    key = (t[0] + U64(1)) * U64((2**64 - 2) // (N // 4 + 1))   # ascending still, half of them at or above 2^63
    out = (key, t[1], t[2], t[3])
    assert cu.is_state(out) and int((key >= U64(2**63)).sum()) > N // 3
    return out


@functools.lru_cache(maxsize=None)
def _singles(n=N):
    """n keys of one cell each: cell i is key 3 i + 1."""
    t = t_cmap._runs([1] * n)
    assert t[0][5] == 16
    return t


# ---------------------------------------------------------------- 1. known answers
def test_known_answers(eng):
    cells = [((0, 0, 0, 0), 0x2130748AAAC80268), ((1, 2, 3, 4), 0xD55CCD4AEB3CCAFB),
             ((M64, 2**32 - 1, M64, M64), 0x44CE0376423ECC3B)]
    for (k, r, p, n), want in cells:
        exp = check_digest(eng, cu.state([k], [r], [p], [n]), [], what=f"h{(k, r, p, n)}")
        assert int(exp[0][0]) == want and int(exp[1][0]) == 1
    t = cu.state([0, 1, M64], [0, 2, 2**32 - 1], [0, 3, M64], [0, 4, M64])
    exp = check_digest(eng, t, [1, M64])                  # one cell a bucket
    assert exp[0].tolist() == [w for _, w in cells] and exp[1].tolist() == [1, 1, 1]
    exp = check_digest(eng, t, [])
    assert int(exp[0][0]) == sum(w for _, w in cells) % 2**64 and int(exp[1][0]) == 3
    sel = check_select(eng, t, [1, M64], [0, 1, 1])
    assert sel[0].tolist() == [1, M64] and sel[1].tolist() == [2, 2**32 - 1] and sel[3].tolist() == [4, M64]


# ---------------------------------------------------------------- 2. lengths x splitter counts
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_and_splitter_counts(eng, n):
    t = _cut(_state(), n)
    Tt = _up(eng, t)
    for m in (0, 1, 7, 255):
        sp = du.quantile_splitters(t, m)
        exp = check_digest(eng, t, sp, Tt=Tt, what=f"digest n={n} m={m}")
        if m == 255 and n >= 2047:
            assert int((exp[1] != 0).sum()) > 200         # the per-lane path: several buckets in every word
        for name, flags in _flag_sets(m).items():
            if m == 0 and name not in ("all", "none"):
                continue
            check_select(eng, t, sp, flags, Tt=Tt, what=f"select n={n} m={m} flags={name}")


# ---------------------------------------------------------------- 3. splitter kinds
def test_every_key_in_its_own_bucket(eng):
    t = _singles(2500)                                    # m >= n: 64 buckets in every word, across a tile edge
    sp = t[0].copy()
    exp = check_digest(eng, t, sp)
    assert exp[1].tolist() == [0] + [1] * 2500
    assert np.array_equal(exp[0][1:], du.h_np(t))
    sel = check_select(eng, t, sp, _alternating(2500))
    assert np.array_equal(sel[0], t[0][0::2])
    check_select(eng, t, sp, np.r_[np.zeros(2049, np.uint8), np.ones(452, np.uint8)])   # from cell 2048 on


def test_all_cells_in_one_bucket(eng):
    t = _state()                                          # 13 waves add into one entry
    lo, hi = int(t[0][0]), int(t[0][-1])
    assert lo > 0 and hi < M64
    for sp, at in (([hi + 1] * 7, 0), ([lo] * 7, 7), ([0] * 7, 7), ([M64] * 7, 0), ([lo], 1), ([hi], 0)):
        exp = check_digest(eng, t, sp, what=f"digest sp={sp[:1]}x{len(sp)}")
        want = N if sp != [hi] else N - int((t[0] == U64(hi)).sum())
        assert int(exp[1][at]) == want
        flags = np.zeros(len(sp) + 1, np.uint8)
        flags[at] = 1
        assert len(check_select(eng, t, sp, flags)[0]) == want
        assert len(check_select(eng, t, sp, 1 - flags)[0]) == N - want


def test_equal_splitters_inside_the_state(eng):
    t = _state()
    mid = int(t[0][3000])
    exp = check_digest(eng, t, [mid] * 9)
    below = int((t[0] < U64(mid)).sum())
    assert exp[1].tolist() == [below] + [0] * 8 + [N - below] and 0 < below < N
    check_select(eng, t, [mid] * 9, [0] * 9 + [1])
    check_select(eng, t, [mid] * 9, [0] + [1] * 8 + [0])  # the empty buckets alone: nothing


@pytest.mark.parametrize("at", [512, 2048])
def test_a_splitter_equal_to_the_key_at_a_wave_or_tile_edge(eng, at):
    t = _singles()
    sp = [int(t[0][at])]
    exp = check_digest(eng, t, sp, what=f"splitter at cell {at}")
    assert exp[1].tolist() == [at, N - at]                # the key itself opens the upper bucket
    assert len(check_select(eng, t, sp, [1, 0])[0]) == at
    assert int(check_select(eng, t, sp, [0, 1])[0][0]) == int(t[0][at])
    sp2 = [int(t[0][512]), int(t[0][2048])]
    assert check_digest(eng, t, sp2)[1].tolist() == [512, 1536, N - 2048]


@pytest.mark.parametrize("edge", [512, 2048])
def test_a_key_run_across_a_wave_or_tile_edge_stays_in_one_bucket(eng, edge):
    t = t_cmap._runs([1] * (edge - 4) + [8] + [1] * (N - edge - 4))
    x = int(t[0][edge])
    assert len(t[0]) == N and t[0][edge - 4] == t[0][edge + 3] == x
    assert t[0][edge - 5] != x and t[0][edge + 4] != x
    for sp, b in (([x], 1), ([x + 1], 0), ([x, x + 1], 1), ([x - 1, x, x + 1, x + 2], 2)):
        assert set(du.bucket_np(sp, t[0][edge - 4:edge + 4]).tolist()) == {b}
        exp = check_digest(eng, t, sp, what=f"run across {edge}, sp={sp}")
        if len(sp) > 1:
            assert int(exp[1][b]) == 8                    # the run alone
        flags = np.zeros(len(sp) + 1, np.uint8)
        flags[b] = 1
        sel = check_select(eng, t, sp, flags, what=f"select run across {edge}, sp={sp}")
        assert int((sel[0] == U64(x)).sum()) == 8 and sel[1][sel[0] == U64(x)].tolist() == list(range(8))
        sel = check_select(eng, t, sp, 1 - flags)
        assert int((sel[0] == U64(x)).sum()) == 0


def test_unsigned_order_and_full_width_fields(eng):
    big = 2**63
    n = 1300
    i = np.arange(n, dtype=U64)
    key = U64(big - 650 * 7) + i * U64(7)                 # 650 keys below 2^63, 650 at and above it
    rep = (U32(2**32 - 1) - (i % U64(5)).astype(U32))
    p, q = U64(M64) - i * U64(3), np.where(i % U64(2) == 0, U64(M64), U64(big) + i)
    t = (key, rep, p, q)
    assert cu.is_state(t) and int(key[650]) == big and int(rep[0]) == 2**32 - 1 and int(p[0]) == M64
    sp = [big - 7, big, big + 7, M64]
    exp = check_digest(eng, t, sp)
    assert exp[1].tolist() == [649, 1, 1, 649, 0]         # a signed comparison would put the upper half first
    sel = check_select(eng, t, sp, [0, 1, 1, 0, 1])
    assert sel[0].tolist() == [big - 7, big]
    sel = check_select(eng, t, sp, [0, 0, 0, 1, 0])
    assert len(sel[0]) == 649 and int(sel[0][0]) == big + 7


# ---------------------------------------------------------------- 4. device lengths
def test_device_lengths_below_the_buffer(eng):
    t = _state()
    for nd in (4101, 2048, 1, 0):
        pt = _poisoned(t, nd)                             # the tail breaks the order and would change every digest
        Tt = _up(eng, pt)
        for m in (0, 7, 255):
            sp = du.quantile_splitters(t, m)
            check_digest(eng, pt, sp, Tt=Tt, n=nd, what=f"digest n_dev={nd} m={m}")
            check_select(eng, pt, sp, _alternating(m) if m else [1], Tt=Tt, n=nd, what=f"select n_dev={nd} m={m}")
    check_digest(eng, t, du.quantile_splitters(t, 7), n=N)    # a count at the capacity
    check_select(eng, t, du.quantile_splitters(t, 7), _alternating(7), n=N)


@pytest.mark.parametrize("bad", [N + 1, M64])
def test_device_length_out_of_range(eng, bad):
    t = _state()
    Tt = _up(eng, t)
    sp = du.quantile_splitters(t, 63)
    SP, FL = _sp(eng, sp), _fl(eng, np.ones(64, np.uint8))
    assert eng.device_status(clear=True) == 0
    gh = torch.full((66,), CANARY, dtype=torch.int64, device=eng.device)
    gc = torch.full((66,), CANARY, dtype=torch.int64, device=eng.device)
    eng.cmap_digest(Tt, SP, n_dev=_dev(eng, bad), hash_out=gh, count_out=gc)
    assert eng.device_status(clear=True) & DEV_RANGE
    assert eng.device_status(clear=True) == 0             # read and cleared
    assert as_u64(gh)[:64].tolist() == [M64] * 64 and as_u64(gc)[:64].tolist() == [M64] * 64
    assert gh[64:].tolist() == [CANARY] * 2 and gc[64:].tolist() == [CANARY] * 2
    # a poisoned digest differs from everything, itself included
    good = eng.cmap_digest(Tt, SP)
    flags, nd = eng.digest_diff((gh[:64], gc[:64]), good)
    assert _n(nd) == 64 and bool(flags.all())
    out = _canary_map(eng, N)
    _, cnt = eng.cmap_select(Tt, SP, FL, n_dev=_dev(eng, bad), out=out)
    assert _n(cnt) == M64 and eng.device_status(clear=True) & DEV_RANGE and _untouched(out)
    assert _n(eng.cmap_select_count(Tt, SP, FL, n_dev=_dev(eng, bad))) == M64
    assert eng.device_status(clear=True) & DEV_RANGE
    check_digest(eng, t, sp, Tt=Tt)                       # the next calls are exact
    check_select(eng, t, sp, _alternating(63), Tt=Tt)


# ---------------------------------------------------------------- 5. select shapes
def test_a_flagged_bucket_ends_at_a_tile_edge(eng):
    t = _singles()
    sp = [int(t[0][1024]), int(t[0][2048]), int(t[0][4096])]
    for flags, cells in (([0, 1, 0, 0], (1024, 2048)), ([0, 0, 1, 0], (2048, 4096)), ([1, 0, 0, 0], (0, 1024)),
                         ([0, 0, 0, 1], (4096, N))):
        sel = check_select(eng, t, sp, flags, what=f"flags={flags}")
        assert np.array_equal(sel[0], t[0][cells[0]:cells[1]])


def test_offset_views_and_odd_lengths(eng):
    t = _cut(_state(), 4099)
    n, m = 4099, 37
    sp = du.quantile_splitters(t, m)
    flags = _alternating(m)
    dev = eng.device

    def off(a, by, dtype=torch.int64):
        """a's bits in a device tensor that starts ``by`` elements into its storage."""
        a = np.ascontiguousarray(a)
        buf = torch.full((len(a) + by + 3,), CANARY, dtype=dtype, device=dev)
        view = buf[by:by + len(a)]
        view.copy_(torch.from_numpy(a.view(np.int64 if dtype == torch.int64 else np.int32 if dtype == torch.int32 else np.uint8).copy()))
        assert view.storage_offset() == by and view.is_contiguous()
        return buf, view

    cols = [off(t[0], 1), off(t[1], 3, torch.int32), off(t[2], 5), off(t[3], 7)]
    Tt = CounterMap(*(v for _, v in cols))
    _, SP = off(sp, 1)
    _, FL = off(flags, 3, torch.uint8)                    # (byte flags: no alignment asked)
    hb = torch.full((m + 4,), CANARY, dtype=torch.int64, device=dev)
    cb = torch.full((m + 4,), CANARY, dtype=torch.int64, device=dev)
    h, c = eng.cmap_digest(Tt, SP, hash_out=hb[1:m + 2], count_out=cb[2:m + 3])
    exp = du.digest_np(t, sp)
    assert np.array_equal(as_u64(h), exp[0]) and np.array_equal(as_u64(c), exp[1])
    assert int(hb[0]) == CANARY and hb[m + 2:].tolist() == [CANARY] * 2
    assert cb[:2].tolist() == [CANARY] * 2 and int(cb[m + 3]) == CANARY
    ob = _canary_map(eng, n + 9)
    out = CounterMap(ob.key[3:3 + n], ob.rep[1:1 + n], ob.p[5:5 + n], ob.n[2:2 + n])
    cbuf = torch.full((3,), CANARY, dtype=torch.int64, device=dev)
    res, cnt = eng.cmap_select(Tt, SP, FL, out=out, count=cbuf[1:2])
    want = du.select_np(t, sp, flags)
    k = len(want[0])
    assert res is out and _n(cnt) == k and 0 < k < n and cbuf[::2].tolist() == [CANARY] * 2
    _eq(_cut(out.to_numpy(), k), want, "select into offset views")
    for full, view, by in ((ob.key, out.key, 3), (ob.rep, out.rep, 1), (ob.p, out.p, 5), (ob.n, out.n, 2)):
        assert bool((full[:by] == CANARY).all()) and bool((full[by + k:] == CANARY).all())
    for buf, view in cols:                                # the inputs are as they were
        assert bool((buf[:view.storage_offset()] == CANARY).all()) and bool((buf[view.storage_offset() + n:] == CANARY).all())
    assert eng.device_status(clear=True) == 0


# ---------------------------------------------------------------- 6. the round
def _round(eng, a, b, m=255):
    A, B = _up(eng, a), _up(eng, b)
    sp = du.quantile_splitters(a, m)
    SP = reconcile.key_splitters(A, m)
    assert np.array_equal(as_u64(SP), sp)
    (ma, ca), (mb, cb), flags, (ship_a, ship_b) = reconcile.cmap_round(eng, A, B, SP)
    want = du.diff_np(du.digest_np(a, sp), du.digest_np(b, sp))
    assert np.array_equal(flags.cpu().numpy(), want)
    sa, sb = du.select_np(a, sp, want), du.select_np(b, sp, want)
    assert (_n(ship_a), _n(ship_b)) == (len(sa[0]), len(sb[0]))
    assert len(ma) == len(mb) == max(len(a[0]) + len(b[0]), 1)    # (an empty map's buffer holds one slot)
    _eq(_take(ma, ca), cu.merge_np(a, b), "MA")
    _eq(_take(mb, cb), cu.merge_np(b, a), "MB")
    assert eng.device_status(clear=True) == 0
    return want, len(sa[0]), len(sb[0])


def test_round_on_a_drifted_pair(eng):
    a, b = du.drifted_pair()
    assert len(a[0]) == N and len(b[0]) == N - 3
    flags, ship_a, ship_b = _round(eng, a, b)
    assert np.flatnonzero(flags).tolist() == du.DRIFTED_FLAGGED and (ship_a, ship_b) == du.DRIFTED_SHIPPED
    _round(eng, b, a)


def test_round_in_sync_ships_nothing(eng):
    a, _ = du.drifted_pair()
    flags, ship_a, ship_b = _round(eng, a, tuple(c.copy() for c in a))
    assert not flags.any() and ship_a == ship_b == 0


def test_round_of_an_independent_pair_and_of_empty_sides(eng):
    rng = np.random.default_rng(12)
    a, b = cu.random_state(rng, N, N // 4), cu.random_state(rng, N, N // 4)
    flags, _, _ = _round(eng, a, b)
    assert int(flags.sum()) > 200
    _round(eng, a, cu.state(), m=7)
    _round(eng, cu.state(), a, m=7)
    _round(eng, cu.state(), cu.state(), m=0)


# ---------------------------------------------------------------- 7. unsorted splitters
def test_unsorted_splitters_stay_in_range(eng):
    t = _state()
    Tt = _up(eng, t)
    rng = np.random.default_rng(13)
    for m in (1, 2, 63, 1000):
        sp = rng.permutation(du.quantile_splitters(t, m))
        if m == 2:
            sp = np.sort(sp)[::-1].copy()                 # descending
        h, c = eng.cmap_digest(Tt, _sp(eng, sp))
        assert int(as_u64(c).sum(dtype=U64)) == N
        eng.cmap_select(Tt, _sp(eng, sp), _fl(eng, _alternating(m)))
        assert eng.device_status(clear=True) == 0


# ---------------------------------------------------------------- 8. refusals: before any launch
def test_host_errors(eng):
    t = _cut(_state(), 1000)
    Tt, O = _up(eng, t), CounterMap.empty(1000, eng.device)
    m = 15
    SP, FL = _sp(eng, du.quantile_splitters(t, m)), _fl(eng, np.ones(m + 1, np.uint8))
    H = torch.zeros(m + 1, dtype=torch.int64, device=eng.device)
    Cn = torch.zeros(m + 1, dtype=torch.int64, device=eng.device)
    cnt = torch.full((1,), 77, dtype=torch.int64, device=eng.device)
    ct, co = Tt.c(), O.c()
    sp, fl, hp, cp, kp = SP.data_ptr(), FL.data_ptr(), H.data_ptr(), Cn.data_ptr(), cnt.data_ptr()
    ref = lambda x: C.byref(x) if x is not None else None   # noqa: E731

    def cm(s, **kw):
        f = {"key": s.key.data_ptr(), "rep": s.rep.data_ptr(), "p": s.p.data_ptr(), "n": s.n.data_ptr()}
        f.update(kw)
        return _lib.crdt_cmap(f["key"], f["rep"], f["p"], f["n"])

    def status(fn, *args):
        eng._bind()
        with pytest.raises(_lib.CrdtError) as ei:
            _lib.call(fn, eng.ctx, *args, ctx=eng.ctx)
        return ei.value.status

    def digest(x=ct, n=1000, nd=None, s=sp, mm=m, h=hp, c=cp):
        return status("crdt_cmap_digest", ref(x), n, nd, s, mm, h, c)

    def select(x=ct, n=1000, nd=None, s=sp, mm=m, f=fl, o=co, k=kp):
        return status("crdt_cmap_select", ref(x), n, nd, s, mm, f, ref(o), k)

    # NULL outputs / flags / state; m != 0 with NULL splitters
    assert digest(h=None) == E_INVAL and digest(c=None) == E_INVAL and digest(x=None) == E_INVAL
    assert select(k=None) == E_INVAL and select(f=None) == E_INVAL and select(x=None) == E_INVAL
    assert digest(s=None) == E_INVAL and select(s=None) == E_INVAL
    # a misaligned pointer
    assert digest(s=sp + 4) == E_INVAL and digest(h=hp + 4) == E_INVAL and digest(c=cp + 4) == E_INVAL
    assert digest(nd=kp + 4) == E_INVAL
    assert select(s=sp + 4) == E_INVAL and select(k=kp + 4) == E_INVAL and select(nd=hp + 4) == E_INVAL
    for f, by in (("key", 4), ("rep", 2), ("p", 4), ("n", 4)):
        assert digest(x=cm(Tt, **{f: getattr(Tt, f).data_ptr() + by})) == E_INVAL
        assert select(x=cm(Tt, **{f: getattr(Tt, f).data_ptr() + by})) == E_INVAL
        assert select(o=cm(O, **{f: getattr(O, f).data_ptr() + by})) == E_INVAL
        # NULL cell fields with n_max != 0
        assert digest(x=cm(Tt, **{f: None})) == E_INVAL
        assert select(x=cm(Tt, **{f: None})) == E_INVAL
        assert select(o=cm(O, **{f: None})) == E_INVAL
    # any output overlapping any input or another output
    assert digest(c=hp) == E_INVAL                           # hash == count
    assert digest(c=hp + 8 * m) == E_INVAL                   # ... its last entry
    assert digest(h=Tt.key.data_ptr()) == E_INVAL and digest(c=Tt.n.data_ptr() + 8 * 999) == E_INVAL
    assert digest(h=Tt.rep.data_ptr() + 4 * 998) == E_INVAL
    assert digest(h=sp) == E_INVAL and digest(c=sp + 8 * (m - 1)) == E_INVAL
    assert digest(nd=hp) == E_INVAL
    assert select(o=ct) == E_INVAL
    assert select(o=cm(O, p=Tt.n.data_ptr() + 8 * 999)) == E_INVAL
    assert select(o=cm(O, rep=Tt.key.data_ptr() + 8 * 999 + 4)) == E_INVAL
    assert select(o=cm(O, key=O.p.data_ptr() + 8 * 999)) == E_INVAL   # two fields of out
    assert select(o=cm(O, key=sp)) == E_INVAL and select(o=cm(O, rep=fl)) == E_INVAL
    assert select(k=O.n.data_ptr()) == E_INVAL and select(k=Tt.p.data_ptr()) == E_INVAL
    assert select(k=sp) == E_INVAL and select(nd=kp) == E_INVAL
    big = torch.zeros(1024, dtype=torch.uint8, device=eng.device)
    assert select(f=big.data_ptr(), k=big.data_ptr() + 8) == E_INVAL   # the count inside the flags
    # ranges
    assert digest(mm=2**24) == E_RANGE and select(mm=2**24) == E_RANGE
    assert digest(n=2**62) == E_RANGE and select(n=2**62, o=None) == E_RANGE
    assert digest(n=2**61) == E_RANGE and select(n=2**61, o=None) == E_RANGE   # more tiles than a launch holds
    with pytest.raises(_lib.CrdtError) as ei:               # NULL ctx
        _lib.call("crdt_cmap_digest", None, C.byref(ct), 1000, None, sp, m, hp, cp)
    assert ei.value.status == E_INVAL
    with pytest.raises(ValueError):
        eng.cmap_select(Tt, SP, FL, out=CounterMap.empty(999, eng.device))
    with pytest.raises(ValueError):
        eng.cmap_digest(Tt, SP, hash_out=H[:m])
    # nothing was launched: the outputs are as they were
    assert int(cnt.item()) == 77 and not H.any() and not Cn.any() and eng.device_status(clear=True) == 0
    # n_max == 0: the digest is zeroed and the count 0, no cell read (the fields may be NULL)
    none = _lib.crdt_cmap(None, None, None, None)
    H.fill_(5)
    Cn.fill_(5)
    eng._bind()
    _lib.call("crdt_cmap_digest", eng.ctx, C.byref(none), 0, None, sp, m, hp, cp, ctx=eng.ctx)
    assert not H.any() and not Cn.any()
    _lib.call("crdt_cmap_select", eng.ctx, C.byref(none), 0, None, sp, m, fl, None, kp, ctx=eng.ctx)
    assert int(cnt.item()) == 0
    cnt.fill_(77)
    _lib.call("crdt_cmap_select", eng.ctx, C.byref(none), 0, None, None, 0, fl, C.byref(none), kp, ctx=eng.ctx)
    assert int(cnt.item()) == 0 and eng.device_status(clear=True) == 0
    check_digest(eng, t, du.quantile_splitters(t, m), Tt=Tt)
