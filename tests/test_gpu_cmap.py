"""GPU: the keyed PN-Counter map (crdt_cmap_merge / _apply / _values / _lookup /
_delta; csrc/countermap.hpp, entry points in csrc/counters.hip) against the two
CPU restatements of tests/cmap_util.py, bit for bit, with the device status 0
after every exact call.

A state is cells (key, rep, p, n) strictly ascending by (key, rep).  A tile of
the two-sided kernels is T = 2048 items of the stable merged order of (a, b),
a's copy of a shared cell first; a tile of the one-sided ones is T cells.  The
hand-built cases put shared pairs and key runs on and across those edges, and
assert on the CPU that they lie where they are meant to before the GPU runs."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmap_util as cu
from crdt_amd import _lib
from crdt_amd.engine import CounterMap, TupleSet, as_u64, u64_tensor

pytestmark = pytest.mark.gpu

T = 2048
DEV_RANGE = 2                  # CRDT_DEV_RANGE
E_INVAL, E_RANGE = -1, -6
M64 = 2**64 - 1
U64, U32 = np.uint64, np.uint32


# ---------------------------------------------------------------- helpers
def _dev(eng, v):
    return u64_tensor(np.array([v], U64), eng.device)


def _up(eng, t):
    return CounterMap.from_numpy(*t, eng.device)


def _cut(t, n):
    return tuple(x[:n] for x in t)


def _n(count):
    return int(as_u64(count)[0])


def _take(out, count):
    k = _n(count)
    assert k <= len(out)
    return _cut(out.to_numpy(), k)


def _eq(got, exp, what):
    assert len(got[0]) == len(exp[0]), f"{what}: {len(got[0])} rows, expected {len(exp[0])}"
    for name, g, e in zip(("col0", "col1", "col2", "col3"), got, exp):
        assert g.dtype == e.dtype, (what, name)
        bad = np.flatnonzero(g != e)
        assert bad.size == 0, f"{what}: {name} differs at {bad[:5]}: got {g[bad[:5]]}, expected {e[bad[:5]]}"


def _two_sided(eng, call, count_call, exp, cap, what):
    """One two-sided op four ways: allocated outputs, given outputs, trim, the count alone."""
    assert cu.is_state(exp)
    out, cnt = call()
    _eq(_take(out, cnt), exp, what)
    given, gc = CounterMap.empty(max(cap, 1), eng.device), torch.full((1,), -5, dtype=torch.int64, device=eng.device)
    out2, cnt2 = call(out=given, count=gc)
    assert out2 is given and cnt2 is gc
    _eq(_take(given, gc), exp, what + " (given outputs)")
    out3, cnt3 = call(trim=True)
    assert len(out3) == len(exp[0]) and _n(cnt3) == len(exp[0])
    _eq(out3.to_numpy(), exp, what + " (trim)")
    assert _n(count_call()) == len(exp[0]), what + " (count alone)"
    assert eng.device_status(clear=True) == 0, what


def check_merge(eng, a, b, A=None, B=None, na=None, nb=None, what="merge"):
    A, B = A or _up(eng, a), B or _up(eng, b)
    kw = dict(n_a_dev=None if na is None else _dev(eng, na), n_b_dev=None if nb is None else _dev(eng, nb))
    ea, eb = (a if na is None else _cut(a, na)), (b if nb is None else _cut(b, nb))
    exp = cu.merge_np(ea, eb)
    if len(exp[0]) <= 64:
        _eq(cu.merge_d(ea, eb), exp, what + ": the restatements")
    _two_sided(eng, lambda **k: eng.cmap_merge(A, B, **kw, **k), lambda: eng.cmap_merge_count(A, B, **kw), exp,
               len(A) + len(B), what)
    return exp


def check_delta(eng, src, dst, S=None, Dd=None, ns=None, nd=None, what="delta"):
    S, Dd = S or _up(eng, src), Dd or _up(eng, dst)
    kw = dict(n_src_dev=None if ns is None else _dev(eng, ns), n_dst_dev=None if nd is None else _dev(eng, nd))
    es, ed = (src if ns is None else _cut(src, ns)), (dst if nd is None else _cut(dst, nd))
    exp = cu.delta_np(es, ed)
    if len(es[0]) + len(ed[0]) <= 64:
        _eq(cu.delta_d(es, ed), exp, what + ": the restatements")
    _two_sided(eng, lambda **k: eng.cmap_delta(S, Dd, **kw, **k), lambda: eng.cmap_delta_count(S, Dd, **kw), exp,
               len(S), what)
    return exp


def check_apply(eng, t, rep, keys, dp, dn, Tt=None, n=None, what="apply"):
    Tt = Tt or _up(eng, t)
    keys, dp, dn = (np.asarray(x, dtype=U64) for x in (keys, dp, dn))
    ops = [u64_tensor(x, eng.device) for x in (keys, dp, dn)]
    kw = dict(n_dev=None if n is None else _dev(eng, n))
    et = t if n is None else _cut(t, n)
    exp = cu.apply_np(et, rep, keys, dp, dn)
    if len(exp[0]) <= 64:
        _eq(cu.apply_d(et, rep, keys, dp, dn), exp, what + ": the restatements")

    def count_alone():
        cnt = torch.zeros(1, dtype=torch.int64, device=eng.device)
        eng._call("crdt_cmap_apply", C.byref(Tt.c()), len(Tt), None if n is None else kw["n_dev"].data_ptr(), rep,
                  ops[0].data_ptr() if len(keys) else None, ops[1].data_ptr() if len(keys) else None,
                  ops[2].data_ptr() if len(keys) else None, len(keys), None, cnt.data_ptr())
        return cnt

    _two_sided(eng, lambda **k: eng.cmap_apply(Tt, rep, *ops, **kw, **k), count_alone, exp, len(Tt) + len(keys), what)
    return exp


def check_values(eng, t, Tt=None, n=None, what="values"):
    Tt = Tt or _up(eng, t)
    kw = dict(n_dev=None if n is None else _dev(eng, n))
    et = t if n is None else _cut(t, n)
    exp = cu.values_np(et)
    if len(et[0]) <= 64:
        _eq(cu.values_d(et), exp, what + ": the restatements")
    k = len(exp[0])

    def rows(res):
        *cols, cnt = res
        assert _n(cnt) == k, f"{what}: count {_n(cnt)}, expected {k}"
        return (as_u64(cols[0])[:k], as_u64(cols[1])[:k], as_u64(cols[2])[:k], cols[3].cpu().numpy()[:k])

    _eq(rows(eng.cmap_values(Tt, **kw)), exp, what)
    given = [torch.full((max(len(Tt), 1),), 0x5a5a, dtype=torch.int64, device=eng.device) for _ in range(4)]
    gc = torch.full((1,), -5, dtype=torch.int64, device=eng.device)
    res = eng.cmap_values(Tt, keys=given[0], p=given[1], n=given[2], value=given[3], count=gc, **kw)
    assert all(r is g for r, g in zip(res, given + [gc]))
    _eq(rows(res), exp, what + " (given outputs)")
    assert all(bool((g[k:] == 0x5a5a).all()) for g in given), what + ": rows past the count were written"
    res = eng.cmap_values(Tt, trim=True, **kw)
    assert all(c.numel() == k for c in res[:4])
    _eq(rows(res), exp, what + " (trim)")
    assert _n(eng.cmap_count_keys(Tt, **kw)) == k, what + " (count alone)"
    assert eng.device_status(clear=True) == 0, what
    return exp


def check_lookup(eng, t, probes, Tt=None, n=None, what="lookup"):
    Tt = Tt or _up(eng, t)
    probes = np.asarray(probes, dtype=U64)
    P = u64_tensor(probes, eng.device)
    kw = dict(n_dev=None if n is None else _dev(eng, n))
    et = t if n is None else _cut(t, n)
    exp = cu.lookup_np(et, probes)
    if len(et[0]) <= 64:
        assert cu.same(cu.lookup_d(et, probes), exp), what + ": the restatements"
    m = len(probes)
    val, found = eng.cmap_get(Tt, P, **kw)
    assert np.array_equal(val.cpu().numpy()[:m], exp[0]) and np.array_equal(found.cpu().numpy()[:m], exp[1]), what
    gv = torch.full((max(m, 1),), 77, dtype=torch.int64, device=eng.device)
    gf = torch.full((max(m, 1),), 7, dtype=torch.uint8, device=eng.device)
    v2, f2 = eng.cmap_get(Tt, P, value=gv, found=gf, **kw)
    assert v2 is gv and f2 is gf
    assert np.array_equal(gv.cpu().numpy()[:m], exp[0]) and np.array_equal(gf.cpu().numpy()[:m], exp[1]), what
    v3, f3 = eng.cmap_get(Tt, P, with_found=False, **kw)
    assert f3 is None and np.array_equal(v3.cpu().numpy()[:m], exp[0]), what
    assert eng.device_status(clear=True) == 0, what
    return exp


# ---------------------------------------------------------------- 1. hand-written known answers
A3 = cu.state([1, 3, 3], [0, 1, 2], [5, 7, 1], [1, 2, 1])
B3 = cu.state([2, 3, 9], [0, 1, 5], [4, 7, 2], [4, 9, 0])


def test_known_answers(eng):
    exp = check_merge(eng, A3, B3)
    _eq(exp, cu.state([1, 2, 3, 3, 9], [0, 0, 1, 2, 5], [5, 4, 7, 1, 2], [1, 4, 9, 1, 0]), "merge, typed out")
    _eq(check_merge(eng, B3, A3), exp, "merge, the other way round")
    exp = check_apply(eng, A3, 1, [2, 3, 7], [10, 1, 0], [0, 2, 0])
    _eq(exp, cu.state([1, 2, 3, 3, 7], [0, 1, 1, 2, 1], [5, 10, 8, 1, 0], [1, 0, 4, 1, 0]), "apply, typed out")
    exp = check_values(eng, A3)
    _eq(exp, (np.array([1, 3], U64), np.array([5, 8], U64), np.array([1, 3], U64), np.array([4, 5], np.int64)),
        "values, typed out")
    exp = check_lookup(eng, A3, [3, 4, 1, 3, 0])
    assert exp[0].tolist() == [5, 0, 4, 5, 0] and exp[1].tolist() == [1, 0, 1, 1, 0]
    exp = check_delta(eng, A3, B3)                       # (3, 1): p 7 == 7 and n 2 < 9, dst is ahead
    _eq(exp, cu.state([1, 3], [0, 2], [5, 1], [1, 1]), "delta(a, b), typed out")
    exp = check_delta(eng, B3, A3)                       # (3, 1): n 9 > 2 ships, with src's own p and n
    _eq(exp, B3, "delta(b, a), typed out")
    assert len(check_delta(eng, A3, A3)[0]) == 0


# ---------------------------------------------------------------- 2. unsigned witnesses
def test_unsigned_witnesses(eng):
    big = 2**63
    # a signed max would pick 5 over 2^63 + 1; a signed order would put rep 2^31 + 1 before rep 3 and key
    # 2^63 + 9 before key 9
    a = cu.state([9, 9, big + 9], [3, 2**31 + 1, 0], [big + 1, 1, 2], [5, 0, big + 7])
    b = cu.state([9, 9, big + 9], [3, 2**31 + 1, 0], [5, 3, 1], [big + 1, 0, 7])
    assert cu.is_state(a) and cu.is_state(b)
    exp = check_merge(eng, a, b)
    _eq(exp, cu.state([9, 9, big + 9], [3, 2**31 + 1, 0], [big + 1, 3, 2], [big + 1, 0, big + 7]), "merge")
    # a's cells around b's in unsigned order only
    lo, hi = cu.state([9, big + 9], [2**31 + 1, 1], [1, 1], [0, 0]), cu.state([9, big + 9], [3, 0], [2, 2], [0, 0])
    exp = check_merge(eng, lo, hi)
    assert exp[0].tolist() == [9, 9, big + 9, big + 9] and exp[1].tolist() == [3, 2**31 + 1, 0, 1]
    check_delta(eng, lo, hi)
    exp = check_delta(eng, a, b)                         # p: 2^63 + 1 > 5 ships; (9, 2^31 + 1): 1 < 3 does not
    assert exp[0].tolist() == [9, big + 9] and exp[1].tolist() == [3, 0]
    # P = (2^64 - 1) + 2 wraps to 1; N > P: a negative value
    w = cu.state([4, 4, 6, 6], [0, 1, 0, 7], [M64, 2, 1, 2], [0, 0, 10, 20])
    exp = check_values(eng, w)
    assert exp[1].tolist() == [1, 3] and exp[2].tolist() == [0, 30] and exp[3].tolist() == [1, -27]
    exp = check_lookup(eng, w, [6, 4, big + 6])
    assert exp[0].tolist() == [-27, 1, 0]
    # p + dp wraps; a decrement past 2^63
    exp = check_apply(eng, w, 1, [4, 6], [M64, big], [M64, 1])
    assert exp[2].tolist() == [M64, 1, 1, big, 2] and exp[3].tolist() == [0, M64, 10, 1, 20]
    check_apply(eng, a, 2**31 + 1, [9, big + 9], [M64, 1], [1, 1])


# ---------------------------------------------------------------- 3. empty and single-cell sides
def test_empty_and_single_sides(eng):
    e = cu.state()
    one, same_cell, other = cu.state([5], [1], [3], [4]), cu.state([5], [1], [9], [2]), cu.state([5], [0], [1], [1])
    for a, b in ((e, e), (e, one), (one, e), (one, same_cell), (same_cell, one), (one, other), (other, one),
                 (one, one)):
        check_merge(eng, a, b)
        check_delta(eng, a, b)
    for t in (e, one):
        check_values(eng, t)
        check_lookup(eng, t, [5, 6])
        check_lookup(eng, t, [])
        check_apply(eng, t, 1, [], [], [])               # m = 0
        check_apply(eng, t, 1, [5], [0], [0])            # a zero op still creates (or keeps) the cell
        check_apply(eng, t, 0, [5], [2], [1])
        check_apply(eng, t, 1, [4, 5, 6], [1, 2, 3], [0, 0, 1])
    assert len(check_apply(eng, e, 1, [5], [0], [0])[0]) == 1


# ---------------------------------------------------------------- 4. tile boundaries
def _straddle(q, ship, tail=3000):
    """(a, b), all of rep 0: q cells before the shared cell of key q, alternately a's and b's, so that a's copy is
    merged item q and b's item q + 1; behind it keys in turn shared, a's, b's.  ship: b's copy is ahead in p."""
    keys = np.arange(q + 1 + tail, dtype=U64)
    in_a = np.where(keys < q, keys % 2 == 0, (keys == q) | ((keys - q) % 3 != 2))
    in_b = np.where(keys < q, keys % 2 == 1, (keys == q) | ((keys - q) % 3 != 1))
    ka, kb = keys[in_a], keys[in_b]
    a = (ka, np.zeros(len(ka), U32), ka * U64(3) + U64(10), ka % U64(7))
    b = (kb, np.zeros(len(kb), U32), kb * U64(3) + np.where(kb % 2 == 0, 11, 9).astype(U64), kb % U64(5))
    at = int(np.searchsorted(kb, q))
    b[2][at] = a[2][int(np.searchsorted(ka, q))] + U64(1 if ship else 0)
    b[3][at] = 0
    # the CPU side: the pair sits where it is meant to
    cols, from_b, head = cu._merged(a, b)
    assert cols[0][q] == q and not from_b[q] and cols[0][q + 1] == q and from_b[q + 1] and not head[q + 1]
    assert len(head) >= q + 2 + T                        # a tile of items behind the pair
    return a, b


@pytest.mark.parametrize("q", [2047, 4095, 2046, 2048])
def test_pair_on_a_tile_boundary(eng, q):
    for ship in (True, False):
        a, b = _straddle(q, ship)
        exp = check_merge(eng, a, b, what=f"merge q={q}")
        at = int(np.searchsorted(exp[0], q))
        assert exp[2][at] == 3 * q + 10 + (1 if ship else 0)
        # delta(src = b, dst = a): dst is merged first, so the pair sits at q, q + 1
        d = check_delta(eng, b, a, what=f"delta q={q} ship={ship}")
        assert (q in d[0].tolist()) == ship
        # the other way round b's copy is merged first: the same two items
        check_delta(eng, a, b, what=f"delta, sides swapped, q={q}")
        # the batch is b's cells: the op of key q hits a's cell across the edge
        t = check_apply(eng, a, 0, b[0], b[2], b[3], what=f"apply q={q}")
        at = int(np.searchsorted(t[0], q))
        assert t[2][at] == U64(2 * (3 * q + 10) + (1 if ship else 0))


# ---------------------------------------------------------------- 5. long runs for values
def _runs(lengths, wrap=False):
    """One key per entry of lengths, with that many replicas."""
    lengths = np.asarray(lengths)
    key = np.repeat(np.arange(len(lengths), dtype=U64) * U64(3) + U64(1), lengths)
    start = np.repeat(np.cumsum(lengths) - lengths, lengths)
    rep = (np.arange(len(key)) - start).astype(U32)
    i = np.arange(len(key), dtype=U64)
    p = i * U64(2654435761) % U64(1 << 40)
    if wrap:
        p = U64(M64) - i * U64(977)
    n = (i * U64(40503) + U64(7)) % U64(1 << 41)
    t = (key, rep, p, n)
    assert cu.is_state(t)
    return t


VALUE_SHAPES = {
    "5000 replicas over 3 tiles": ([1] * 100 + [5000] + [1] * 100, (100, 5100)),
    "a run from cell 2048": ([1] * 2048 + [300] + [1] * 50, (2048, 2348)),
    "a run ending at cell 2047": ([1] * 1748 + [300] + [1] * 200, (1748, 2048)),
    "6161 single-cell keys": ([1] * 6161, None),
    "one key, 6161 replicas": ([6161], (0, 6161)),
    "runs of 2048 on the tile grid": ([2048, 2048, 1, 2047, 17], (0, 2048)),
    "a run of exactly two tiles and a cell": ([7, 4097, 5], (7, 4104)),
}


@pytest.mark.parametrize("name", sorted(VALUE_SHAPES))
def test_values_long_runs(eng, name):
    lengths, run = VALUE_SHAPES[name]
    t = _runs(lengths, wrap=name == "one key, 6161 replicas")
    if run is not None:                                  # the CPU side: the long run lies where it is meant to
        lo, hi = run
        assert t[0][lo] == t[0][hi - 1] and (lo == 0 or t[0][lo - 1] != t[0][lo])
        assert hi == len(t[0]) or t[0][hi] != t[0][hi - 1]
    exp = check_values(eng, t, what=name)
    assert len(exp[0]) == len(lengths)
    if name == "one key, 6161 replicas":                 # the partial sums wrapped
        assert sum(int(x) for x in t[2]) > 2**64 and int(exp[1][0]) == sum(int(x) for x in t[2]) % 2**64
    probes = np.concatenate([t[0][::97], t[0][::97] + U64(1)])
    check_lookup(eng, t, probes, what=name)


# ---------------------------------------------------------------- 6. random parity
def _pair(na, nb, seed=11):
    """Seeded (a, b) with a good share of a's cells in b and a shared pair across a tile edge."""
    rng = np.random.default_rng(seed)
    if na > 1 and nb > 1:
        a, b = cu.random_state(rng, na, 2000), cu.random_state(rng, nb, 2000)
    elif na == 1:                                        # a's one cell is b's cell 2047: merged items 2047 and 2048
        b = cu.random_state(rng, nb, 2000)
        a = tuple(x[2047:2048].copy() for x in b)
        a[2][0] += U64(5)
    else:                                                # b's one cell is a's cell 2047
        a = cu.random_state(rng, na, 2000)
        b = tuple(x[2047:2048].copy() for x in a)
        b[3][0] += U64(5)
    return a, b


def _assert_not_vacuous(a, b):
    cols, from_b, head = cu._merged(a, b)
    second = np.flatnonzero(~head)                       # b's copies of the shared cells, in merged order
    # a fifth of a's cells are in b; where b is too short to hold that many (a one-cell b), a fifth of b's are in a
    need = len(a[0]) if len(b[0]) >= 0.2 * len(a[0]) else len(b[0])
    assert len(second) >= 0.2 * need, "too few cells are shared"
    assert (second % T == 0).any(), "no shared pair straddles a tile boundary"


@pytest.mark.parametrize("na,nb", [(7000, 5305), (1, 6000), (6000, 1)])
def test_random_parity_two_sided(eng, na, nb):
    a, b = _pair(na, nb)
    _assert_not_vacuous(a, b)
    A, B = _up(eng, a), _up(eng, b)
    check_merge(eng, a, b, A=A, B=B)
    check_merge(eng, b, a, A=B, B=A)
    d = check_delta(eng, a, b, S=A, Dd=B)
    assert na == 1 or 0 < len(d[0]) < na                 # some of src's cells ship, some do not
    check_delta(eng, b, a, S=B, Dd=A)
    m = cu.merge_np(a, b)
    assert len(check_delta(eng, a, m, S=A)[0]) == 0      # in sync
    _eq(check_merge(eng, b, cu.delta_np(a, b), A=B), m, "merge(dst, delta) == merge(dst, src)")


def test_random_parity_apply_values_lookup(eng):
    rng = np.random.default_rng(5)
    t = cu.random_state(rng, 5461, 2000)
    keys = np.sort(rng.choice(2600, size=700, replace=False)).astype(U64)
    dp = rng.integers(0, 1 << 40, size=700, dtype=U64)
    dn = rng.integers(0, 1 << 40, size=700, dtype=U64)
    dp[::9] = M64                                        # wrapping increments
    cells = set(zip(t[0].tolist(), t[1].tolist()))
    hits = sum((int(k), 3) in cells for k in keys)
    assert 50 < hits < 650                               # the batch both updates and creates
    exp = check_apply(eng, t, 3, keys, dp, dn)
    assert len(exp[0]) == 5461 + 700 - hits
    big = _pair(7000, 5305)[0]
    v = check_values(eng, big)
    check_values(eng, exp)
    present = rng.choice(v[0], size=500)                 # with repeats
    absent = rng.choice(np.setdiff1d(np.arange(2400, dtype=U64), v[0]), size=500)
    probes = rng.permutation(np.concatenate([present, absent]))
    found = check_lookup(eng, big, probes)[1]
    assert int(found.sum()) == 500 and len(np.unique(present)) < 500


# ---------------------------------------------------------------- 7. device lengths
POISON = 0xA5A5A5A5A5A5A5A5


def _poisoned(t, n):
    """t with every cell from n on overwritten by a pattern (which also breaks the order)."""
    out = tuple(x.copy() for x in t)
    out[0][n:], out[1][n:], out[2][n:], out[3][n:] = U64(POISON), U32(0xA5A5A5A5), U64(POISON), U64(POISON)
    return out


def test_device_lengths_below_the_buffers(eng):
    a, b = _pair(6161, 6161, seed=3)
    na, nb = 4101, 4001
    _assert_not_vacuous(_cut(a, na), _cut(b, nb))
    pa, pb = _poisoned(a, na), _poisoned(b, nb)
    A, B = _up(eng, pa), _up(eng, pb)
    check_merge(eng, pa, pb, A=A, B=B, na=na, nb=nb)
    check_delta(eng, pa, pb, S=A, Dd=B, ns=na, nd=nb)
    check_delta(eng, pb, pa, S=B, Dd=A, ns=nb, nd=na)
    check_values(eng, pa, Tt=A, n=na)
    check_lookup(eng, pa, np.concatenate([a[0][::13], [U64(POISON)]]), Tt=A, n=na)
    keys = np.unique(np.concatenate([a[0][:na:11], a[0][na::7]]))
    check_apply(eng, pa, int(a[1][0]), keys, keys + U64(1), keys % U64(3), Tt=A, n=na)
    for n0, n1 in ((0, nb), (na, 0), (6161, 6161), (2048, 2048), (1, 1)):   # the range's ends; a count at the capacity
        check_merge(eng, a, b, na=n0, nb=n1)
        check_delta(eng, a, b, ns=n0, nd=n1)
    ops = np.unique(a[0][:100:3])                        # (strictly ascending: a key has several replicas' cells)
    for n0 in (0, 1, 2047, 2048, 2049, 6161):
        check_values(eng, a, n=n0)
        check_lookup(eng, a, a[0][:4200:41], n=n0)
        check_apply(eng, a, 2, ops, ops + U64(7), ops % U64(5), n=n0)


@pytest.mark.parametrize("bad", [6162, M64])
def test_device_length_out_of_range(eng, bad):
    a, b = _pair(6161, 6161, seed=3)
    A, B = _up(eng, a), _up(eng, b)
    assert eng.device_status(clear=True) == 0

    def fresh(n):
        out = CounterMap.empty(n, eng.device)
        for x in (out.key, out.rep, out.p, out.n):
            x.fill_(0x5a)
        return out

    def untouched(out):
        return all(bool((x == 0x5a).all()) for x in (out.key, out.rep, out.p, out.n))

    ops = [u64_tensor(a[0][:50], eng.device)] * 3
    for side in (0, 1):
        kw = {("n_a_dev", "n_b_dev")[side]: _dev(eng, bad)}
        dk = {("n_src_dev", "n_dst_dev")[side]: _dev(eng, bad)}
        for call, count_call, cap in (
                (lambda **k: eng.cmap_merge(A, B, **kw, **k), lambda: eng.cmap_merge_count(A, B, **kw), 12322),
                (lambda **k: eng.cmap_delta(A, B, **dk, **k), lambda: eng.cmap_delta_count(A, B, **dk), 6161)):
            out = fresh(cap)
            _, cnt = call(out=out)
            assert _n(cnt) == M64 and eng.device_status(clear=True) & DEV_RANGE and untouched(out)
            assert _n(count_call()) == M64 and eng.device_status(clear=True) & DEV_RANGE
    out = fresh(6161 + 50)
    _, cnt = eng.cmap_apply(A, 1, *ops, n_dev=_dev(eng, bad), out=out)
    assert _n(cnt) == M64 and eng.device_status(clear=True) & DEV_RANGE and untouched(out)
    cols = [torch.full((6161,), 0x5a, dtype=torch.int64, device=eng.device) for _ in range(4)]
    *_, cnt = eng.cmap_values(A, n_dev=_dev(eng, bad), keys=cols[0], p=cols[1], n=cols[2], value=cols[3])
    assert _n(cnt) == M64 and eng.device_status(clear=True) & DEV_RANGE
    assert all(bool((c == 0x5a).all()) for c in cols)
    assert _n(eng.cmap_count_keys(A, n_dev=_dev(eng, bad))) == M64 and eng.device_status(clear=True) & DEV_RANGE
    val, found = eng.cmap_get(A, u64_tensor(a[0][:300], eng.device), n_dev=_dev(eng, bad))
    assert eng.device_status(clear=True) & DEV_RANGE
    assert not val.any() and not found.any()
    check_merge(eng, a, b, A=A, B=B)                     # the next calls are exact
    check_values(eng, a, Tt=A)


def test_device_counts_chain_with_no_read_back(eng):
    a, b = _pair(7000, 5305)
    A, B = _up(eng, a), _up(eng, b)
    merged, cnt = eng.cmap_merge(A, B)                   # the merge's count is the read's length
    keys, P, N, value, kc = eng.cmap_values(merged, n_dev=cnt)
    exp = cu.values_np(cu.merge_np(a, b))
    k = _n(kc)
    _eq((as_u64(keys)[:k], as_u64(P)[:k], as_u64(N)[:k], value.cpu().numpy()[:k]), exp, "merge -> values")
    val, found = eng.cmap_get(merged, u64_tensor(exp[0][::5], eng.device), n_dev=cnt)
    assert np.array_equal(val.cpu().numpy(), exp[3][::5]) and bool(found.all())
    d, dc = eng.cmap_delta(A, B)                         # the delta's count is the merge's b length
    out, oc = eng.cmap_merge(B, d, n_b_dev=dc)
    _eq(_take(out, oc), cu.merge_np(b, a), "delta -> merge")
    assert 0 < _n(dc) < 7000
    assert eng.device_status(clear=True) == 0


# ---------------------------------------------------------------- 8. round trip
def test_three_replicas_converge(eng):
    rng = np.random.default_rng(8)
    total = {}
    states = []
    for rep in range(3):
        S, n = CounterMap.empty(1, eng.device), _dev(eng, 0)
        cpu = cu.state()
        for _ in range(2):
            keys = np.sort(rng.choice(900, size=400, replace=False)).astype(U64)
            dp = rng.integers(0, 1000, size=400, dtype=U64)
            dn = rng.integers(0, 1000, size=400, dtype=U64)
            for k, p, q in zip(keys.tolist(), dp.tolist(), dn.tolist()):
                total[k] = total.get(k, 0) + p - q
            S, n = eng.cmap_apply(S, rep, *(u64_tensor(x, eng.device) for x in (keys, dp, dn)), n_dev=n)
            cpu = cu.apply_np(cpu, rep, keys, dp, dn)
        _eq(_take(S, n), cpu, f"replica {rep} after its batches")
        states.append((S, n))
    # every replica pulls each other's delta against its own state and merges it, all on device counts
    after = []
    for i in range(3):
        S, n = states[i]
        for j in range(3):
            if j != i:
                d, dc = eng.cmap_delta(states[j][0], S, n_src_dev=states[j][1], n_dst_dev=n)
                S, n = eng.cmap_merge(S, d, n_a_dev=n, n_b_dev=dc)
        after.append(_take(S, n))
    _eq(after[1], after[0], "replica 1 == replica 0")
    _eq(after[2], after[0], "replica 2 == replica 0")
    assert cu.is_state(after[0])
    keys, _, _, value, kc = eng.cmap_values(_up(eng, after[0]), trim=True)
    assert as_u64(keys).tolist() == sorted(total)
    assert value.cpu().numpy().tolist() == [total[k] for k in sorted(total)]
    assert eng.device_status(clear=True) == 0


# ---------------------------------------------------------------- 9. refusals: before any launch
def test_host_errors(eng):
    a, b = _pair(1000, 1000, seed=2)
    A, B, O = _up(eng, a), _up(eng, b), CounterMap.empty(2000, eng.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=eng.device)
    ops = u64_tensor(a[0][:10], eng.device)
    val = torch.zeros(16, dtype=torch.int64, device=eng.device)
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

    def merge(x, y, o, count, na=1000, nb=1000):
        return status("crdt_cmap_merge", ref(x), na, None, ref(y), nb, None, ref(o), count)

    def delta(x, y, o, count, ns=1000, nd=1000):
        return status("crdt_cmap_delta", ref(x), ns, None, ref(y), nd, None, ref(o), count)

    def apply(t, o, count, n=1000, m=10, k=ops.data_ptr(), dp=ops.data_ptr(), dn=ops.data_ptr()):
        return status("crdt_cmap_apply", ref(t), n, None, 1, k, dp, dn, m, ref(o), count)

    def values(t, count, n=1000, keys=None, p=None):
        return status("crdt_cmap_values", ref(t), n, None, keys, p, None, None, count)

    def lookup(t, n=1000, m=10, probes=ops.data_ptr(), v=val.data_ptr(), f=None):
        return status("crdt_cmap_lookup", ref(t), n, None, probes, m, v, f)

    for two in (merge, delta):
        assert two(None, cb, None, cp) == E_INVAL           # NULL side / count
        assert two(ca, None, None, cp) == E_INVAL
        assert two(ca, cb, co, None) == E_INVAL
        for f in ("key", "rep", "p", "n"):                  # NULL fields with a non-zero length
            assert two(cm(A, **{f: None}), cb, None, cp) == E_INVAL
            assert two(ca, cm(B, **{f: None}), None, cp) == E_INVAL
            assert two(ca, cb, cm(O, **{f: None}), cp) == E_INVAL
        for f, by in (("key", 4), ("rep", 2), ("p", 4), ("n", 4)):   # natural alignment of every operand
            assert two(cm(A, **{f: getattr(A, f).data_ptr() + by}), cb, None, cp) == E_INVAL
            assert two(ca, cm(B, **{f: getattr(B, f).data_ptr() + by}), None, cp) == E_INVAL
            assert two(ca, cb, cm(O, **{f: getattr(O, f).data_ptr() + by}), cp) == E_INVAL
        assert two(ca, cb, ca, cp) == E_INVAL               # out overlapping an input
        assert two(ca, cb, cb, cp) == E_INVAL
        assert two(ca, cb, cm(O, p=B.n.data_ptr() + 8 * 999), cp) == E_INVAL   # ... its last element
        assert two(ca, cb, cm(O, rep=A.key.data_ptr() + 8 * 999 + 4), cp) == E_INVAL
        assert two(ca, cb, None, cp, 2**62) == E_RANGE
        assert two(ca, cb, None, cp, 1000, 2**62) == E_RANGE
        assert two(ca, cb, None, cp, 2**61, 2**61) == E_RANGE   # more tiles than a launch holds
    assert apply(None, None, cp) == E_INVAL
    assert apply(ca, co, None) == E_INVAL
    assert apply(cm(A, p=None), None, cp) == E_INVAL
    assert apply(ca, cm(O, n=None), cp) == E_INVAL
    assert apply(ca, None, cp, k=None) == E_INVAL           # NULL operation arrays with m > 0
    assert apply(ca, None, cp, dp=None) == E_INVAL
    assert apply(ca, None, cp, dn=None) == E_INVAL
    assert apply(ca, None, cp, k=ops.data_ptr() + 4) == E_INVAL
    assert apply(cm(A, rep=A.rep.data_ptr() + 2), None, cp) == E_INVAL
    assert apply(ca, ca, cp) == E_INVAL
    assert apply(ca, cm(O, key=ops.data_ptr()), cp) == E_INVAL
    assert apply(ca, None, cp, n=2**62) == E_RANGE
    assert apply(ca, None, cp, m=2**62) == E_RANGE
    assert values(None, cp) == E_INVAL
    assert values(ca, None) == E_INVAL
    assert values(cm(A, key=None), cp) == E_INVAL
    assert values(cm(A, n=A.n.data_ptr() + 4), cp) == E_INVAL
    assert values(ca, cp, keys=A.p.data_ptr()) == E_INVAL   # an output overlapping the state
    assert values(ca, cp, keys=O.key.data_ptr(), p=O.key.data_ptr() + 8 * 999) == E_INVAL   # ... or another output
    assert values(ca, cp, keys=O.key.data_ptr() + 4) == E_INVAL
    assert values(ca, cp, n=2**62) == E_RANGE
    assert lookup(None) == E_INVAL
    assert lookup(cm(A, rep=None)) == E_INVAL
    assert lookup(ca, probes=None) == E_INVAL
    assert lookup(ca, v=None) == E_INVAL
    assert lookup(ca, v=val.data_ptr() + 4) == E_INVAL
    assert lookup(ca, v=A.key.data_ptr()) == E_INVAL
    assert lookup(ca, n=2**62) == E_RANGE
    with pytest.raises(_lib.CrdtError) as ei:               # NULL ctx
        _lib.call("crdt_cmap_merge", None, C.byref(ca), 1000, None, C.byref(cb), 1000, None, None, cp)
    assert ei.value.status == E_INVAL
    with pytest.raises(_lib.CrdtError) as ei:
        eng.cmap_merge(A, B, out=CounterMap(O.key, O.rep, A.p, O.n))
    assert ei.value.status == E_INVAL
    with pytest.raises(ValueError):
        eng.cmap_merge(A, B, out=CounterMap.empty(1999, eng.device))
    assert int(cnt.item()) == 0 and eng.device_status(clear=True) == 0
    # lengths of 0: the count store alone, no side read (its fields may be NULL)
    cnt.fill_(77)
    eng._bind()
    none = _lib.crdt_cmap(None, None, None, None)
    _lib.call("crdt_cmap_merge", eng.ctx, C.byref(none), 0, None, C.byref(none), 0, None, None, cp, ctx=eng.ctx)
    assert int(cnt.item()) == 0
    cnt.fill_(77)
    _lib.call("crdt_cmap_values", eng.ctx, C.byref(none), 0, None, None, None, None, None, cp, ctx=eng.ctx)
    assert int(cnt.item()) == 0
    cnt.fill_(77)
    _lib.call("crdt_cmap_delta", eng.ctx, C.byref(none), 0, None, C.byref(ca), 1000, None, None, cp, ctx=eng.ctx)
    assert int(cnt.item()) == 0
    assert _lib.call("crdt_cmap_lookup", eng.ctx, C.byref(ca), 1000, None, None, 0, None, None, ctx=eng.ctx) == 0
    check_merge(eng, a, b, A=A, B=B)


# ---------------------------------------------------------------- the set ops still share the scaffold
def test_interleaved_with_a_set_merge(eng):
    """A counter-map call between two OR-Set merges on one context: each carves the workspace afresh."""
    from crdt_amd import synth
    sa = synth.sort_tuples_np(*synth.set_tuples(5, 0, 5000, 3000))
    sb = synth.sort_tuples_np(*synth.set_tuples(5, 1, 5000, 3000))
    SA, SB = TupleSet.from_numpy(*sa, eng.device), TupleSet.from_numpy(*sb, eng.device)
    first = eng.orset_merge(SA, SB).to_numpy()
    a, b = _pair(7000, 5305)
    check_merge(eng, a, b)
    check_values(eng, a)
    again = eng.orset_merge(SA, SB).to_numpy()
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
