"""GPU: the payload-carrying sorted set merges (crdt_lww_merge_src,
crdt_orset_merge_src) and the gather by their source indices (crdt_src_gather),
through the Engine (lww_merge_src, orset_merge_src, gather_src, lww_map_merge,
orset_map_merge).

For every case and both modes:
 (a) out / count == eng.lww_merge / eng.orset_merge of the same inputs, bit
     for bit;
 (b) src[:count] == the numpy restatement below (a then b concatenated, a
     stable lexsort by (key, ts, rep), tag runs and key runs: LWW's source is
     the first element of the last tag run of each key run, OR-Set's the first
     element of each tag run);
 (c) gathering a's and b's own key / ts / rep (LWW: and tomb) columns by src
     reproduces out's columns -- no oracle in this check; elem_size 8, 4, 1;
 (d) device_status(clear=True) == 0.

Sizes are the smallest that reach the kernels' edges: a wave is 64 merge
items, the LWW tile 4096 with a write part of 1024, the OR-Set tile 2048 with
a part of 1024 (sets.lww_parts / sets.or_parts at their defaults)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from knobs import set_knob

from crdt_amd import _lib, synth
from crdt_amd.engine import TupleSet, as_u64

pytestmark = pytest.mark.gpu

E_INVAL, E_RANGE, DEV_RANGE = -1, -6, 2
U64, U32, U8 = np.uint64, np.uint32, np.uint8


# ---------------------------------------------------------------- the restatement
def ref_src(a, b, lww):
    """Source index of every output tuple of merge(a, b), in output order."""
    na = len(a[0])
    key, ts, rep = (np.concatenate([x, y]) for x, y in zip(a[:3], b[:3]))
    if len(key) == 0:
        return np.zeros(0, np.int64)
    order = np.lexsort((rep, ts, key))                   # stable: a's copies of an equal tag before b's
    k, t, r = key[order], ts[order], rep[order]
    new_key = np.r_[True, k[1:] != k[:-1]]
    new_tag = new_key | np.r_[True, (t[1:] != t[:-1]) | (r[1:] != r[:-1])]
    tag0 = np.flatnonzero(new_tag)                       # first element of each tag run
    if lww:                                              # ... of the last tag run of each key run
        last = np.r_[new_key[tag0][1:], True]
        tag0 = tag0[last]
    pos = order[tag0].astype(np.int64)
    return np.where(pos < na, pos, -(pos - na) - 1)


def tuples(rows):
    """[(key, ts, rep, tomb), ...] in (key, ts, rep) order -> SoA numpy tuples."""
    rows = list(rows)
    t = (np.array([x[0] for x in rows], U64), np.array([x[1] for x in rows], U64),
         np.array([x[2] for x in rows], U32), np.array([x[3] for x in rows], U8))
    o = np.lexsort((t[2], t[1], t[0]))
    assert np.array_equal(o, np.arange(len(rows))), "rows must be given sorted"
    return t


EMPTY = tuples([])


def check(eng, a, b, name=""):
    """(a) - (d) for both modes; returns {lww: (out tuples, src)} (numpy)."""
    A = TupleSet.from_numpy(*a, eng.device)
    B = TupleSet.from_numpy(*b, eng.device)
    res = {}
    for lww in (True, False):
        tag = (name, "lww" if lww else "orset")
        plain = (eng.lww_merge if lww else eng.orset_merge)(A, B).to_numpy()
        out, cnt, src = (eng.lww_merge_src if lww else eng.orset_merge_src)(A, B)
        cols = [("key", A.key, B.key, out.key), ("ts", A.ts, B.ts, out.ts), ("rep", A.rep, B.rep, out.rep)]
        if lww:
            cols.append(("tomb", A.tomb, B.tomb, out.tomb))
        got = [(f, eng.gather_src(src, ca, cb, n_dev=cnt), co) for f, ca, cb, co in cols]   # no read-back so far
        c = int(cnt.item())
        assert c == len(plain[0]), (tag, c, len(plain[0]))
        for g, e, f in zip(out.slice(c).to_numpy(), plain, ("key", "ts", "rep", "tomb")):
            np.testing.assert_array_equal(g, e, err_msg=f"{tag} out.{f} vs the plain merge")
        s = src[:c].cpu().numpy()
        np.testing.assert_array_equal(s, ref_src(a, b, lww), err_msg=f"{tag} src")
        for f, g, co in got:
            assert torch.equal(g[:c], co[:c]), (tag, f, "gathered column != out's")
        assert eng.device_status(clear=True) == 0, tag
        res[lww] = (plain, s)
    return res


# ---------------------------------------------------------------- hand-built cases
def test_empty_sides(eng):
    one = tuples([(5, 1, 0, 0), (5, 2, 0, 1), (9, 1, 1, 0)])
    check(eng, EMPTY, EMPTY, "both empty")
    r = check(eng, one, EMPTY, "b empty")
    assert list(r[False][1]) == [0, 1, 2] and list(r[True][1]) == [1, 2]
    r = check(eng, EMPTY, one, "a empty")
    assert list(r[False][1]) == [-1, -2, -3] and list(r[True][1]) == [-2, -3]


def test_equal_tags_the_left_one_is_the_source(eng):
    x, y = tuples([(7, 3, 2, 0)]), tuples([(7, 3, 2, 1)])
    for a, b in ((x, y), (y, x)):                        # swapped: still the left one
        r = check(eng, a, b, "one equal tag")
        for lww in (True, False):
            assert list(r[lww][1]) == [0]
        assert r[True][0][3][0] == a[3][0]               # LWW: the left copy's tomb
        assert r[False][0][3][0] == 1                    # OR-Set: the OR


def test_copies_of_the_maximal_tag_on_both_sides(eng):
    # key 7: smaller tags, then 3 copies of its maximal tag on each side, tombs differing
    a = tuples([(3, 1, 0, 0), (7, 1, 0, 1), (7, 9, 4, 0), (7, 9, 4, 1), (7, 9, 4, 1), (8, 1, 0, 0)])
    b = tuples([(7, 2, 0, 0), (7, 9, 4, 1), (7, 9, 4, 0), (7, 9, 4, 0), (9, 5, 5, 1)])
    r = check(eng, a, b, "3 + 3 copies")
    plain, s = r[True]
    assert list(s) == [0, 2, 5, -5]                      # key 7: a's first copy
    assert plain[3][1] == 0                              # ... and its tomb
    plain, s = r[False]
    i = [j for j in range(len(s)) if (plain[0][j], plain[1][j]) == (7, 9)]
    assert len(i) == 1 and s[i[0]] == 2 and plain[3][i[0]] == 1   # a's first copy; tomb the OR (its own is 0)
    # the same tag only in b: a negative source
    a2 = tuples([(3, 1, 0, 0), (7, 1, 0, 1), (8, 1, 0, 0)])
    r = check(eng, a2, b, "only b holds the maximal tag")
    assert -2 in r[True][1] and -2 in r[False][1]
    assert list(r[True][1]) == [0, -2, 2, -5]


EDGES = (64, 1024, 2048, 4096, 8192)


def _edge_case(edge, kind, layout):
    """edge - 2 unique smaller keys (alternating sides), then one run of 5 merge
    items (positions edge - 2 .. edge + 2: across the edge) -- a key run of
    distinct tags or a tag run of copies -- then a few larger keys."""
    ra, rb = [], []
    for i in range(edge - 2):
        (ra if i % 2 == 0 else rb).append((10 + i, 1 + i % 5, i % 3, i % 2))
    K = 10 + edge
    for j in range(5):
        row = (K, 1 + j, 1, j % 2) if kind == "key" else (K, 4, 1, 1 if j in (1, 3) else 0)
        side = {"a": ra, "b": rb, "ab": ra if j % 2 == 0 else rb, "ba": rb if j % 2 == 0 else ra}[layout]
        side.append(row)
    for i in range(6):
        (ra if i % 2 == 0 else rb).append((K + 1 + i, 2, 0, 0))
    return tuples(ra), tuples(rb)


@pytest.mark.parametrize("edge", EDGES)
def test_runs_across_wave_part_and_tile_edges(eng, edge):
    for kind in ("key", "tag"):
        for layout in ("a", "b", "ab", "ba"):
            a, b = _edge_case(edge, kind, layout)
            r = check(eng, a, b, f"edge {edge} {kind} run {layout}")
            K = 10 + edge
            na_small = (edge - 2 + 1) // 2               # a's smaller keys: the run's first index on a
            nb_small = (edge - 2) // 2
            plain, s = r[True]
            w = s[np.flatnonzero(plain[0] == K)]
            assert len(w) == 1
            if kind == "key":                            # the maximal tag is the run's last item (j = 4)
                exp = {"a": na_small + 4, "b": -(nb_small + 4) - 1, "ab": na_small + 2, "ba": -(nb_small + 2) - 1}
            else:                                        # one tag: the first copy, a's when a holds one
                exp = {"a": na_small, "b": -nb_small - 1, "ab": na_small, "ba": na_small}
            assert w[0] == exp[layout], (edge, kind, layout, w[0])
            plain, s = r[False]
            w = s[np.flatnonzero(plain[0] == K)]
            if kind == "tag":
                assert list(w) == [exp[layout]] and plain[3][plain[0] == K][0] == 1


def test_one_key_holds_every_tuple(eng):
    n = 3 * 4096 + 17
    rng = np.random.default_rng(3)
    # one key, distinct tags: a key run over many tiles
    a = (np.full(n, 7, U64), np.arange(n, dtype=U64) * U64(2), np.zeros(n, U32), rng.integers(0, 2, n).astype(U8))
    b = (np.full(n, 7, U64), np.arange(n, dtype=U64) * U64(2) + U64(1), np.zeros(n, U32),
         rng.integers(0, 2, n).astype(U8))
    r = check(eng, a, b, "one key")
    assert list(r[True][1]) == [-n]                      # b's last tuple carries the maximal tag
    # one tag: the walk back (LWW) and forward (OR-Set) cross every tile and stay in range
    a = (np.full(n, 7, U64), np.full(n, 5, U64), np.full(n, 1, U32), np.r_[np.zeros(n - 1, U8), U8(1)])
    b = (np.full(n, 7, U64), np.full(n, 5, U64), np.full(n, 1, U32), np.zeros(n, U8))
    r = check(eng, a, b, "one tag")
    assert list(r[True][1]) == [0] and list(r[False][1]) == [0]
    assert r[True][0][3][0] == 0 and r[False][0][3][0] == 1
    r = check(eng, EMPTY, a, "one tag, b only")
    assert list(r[True][1]) == [-1] and list(r[False][1]) == [-1]


def test_sizes_crossed_disjoint_keys(eng):
    sizes = (1, 2047, 2048, 2049, 4097)
    rng = np.random.default_rng(11)
    for na in sizes:
        for nb in sizes:
            a = (np.arange(na, dtype=U64) * U64(2), rng.integers(0, 9, na).astype(U64), rng.integers(0, 4, na).astype(U32),
                 rng.integers(0, 2, na).astype(U8))
            b = (np.arange(nb, dtype=U64) * U64(2) + U64(1), rng.integers(0, 9, nb).astype(U64),
                 rng.integers(0, 4, nb).astype(U32), rng.integers(0, 2, nb).astype(U8))
            r = check(eng, a, b, f"{na} x {nb}")
            assert len(r[True][1]) == na + nb == len(r[False][1])


# ---------------------------------------------------------------- seeded
@functools.lru_cache(maxsize=None)
def seeded(na=200_003, nb=150_001, key_space=60_000, seed=23):
    a = synth.sort_tuples_np(*synth.set_tuples(seed, 0, na, key_space))
    b = synth.sort_tuples_np(*synth.set_tuples(seed, 1, nb, key_space))
    exp = {lww: ref_src(a, b, lww) for lww in (True, False)}
    for x in a + b + tuple(exp.values()):
        x.setflags(write=False)
    return a, b, exp


def test_seeded_both_branches(eng):
    a, b, exp = seeded()
    for lww in (True, False):                            # on the CPU, before any GPU result is looked at
        share = float((exp[lww] < 0).mean())
        print(f"{'lww' if lww else 'orset'}: {len(exp[lww])} outputs, {100 * share:.1f} % with src < 0")
        assert 0.10 <= share <= 0.90
    both = np.intersect1d(a[0], b[0]).size
    assert both > 0.5 * np.union1d(a[0], b[0]).size      # most keys occur on both sides
    check(eng, a, b, "seeded")


def _vals(n, side, kind):
    i = np.arange(n, dtype=U64)
    v = i | (U64(side) << U64(63))
    if kind == "u64":
        return torch.from_numpy(v.view(np.int64).copy())
    if kind == "16B":                                    # one 16-byte element per tuple: [n, 2] rows
        return torch.from_numpy(np.stack([v, ~v], axis=1).view(np.int64).copy())
    return torch.from_numpy(((i * U64(7) + U64(side * 3)) & U64(0x7FFF)).astype(np.int16))


@pytest.mark.parametrize("lww", [True, False])
def test_map_merges_carry_the_values(eng, lww):
    a, b, exp = seeded()
    A = TupleSet.from_numpy(*a, eng.device)
    B = TupleSet.from_numpy(*b, eng.device)
    fn = eng.lww_map_merge if lww else eng.orset_map_merge
    plain = (eng.lww_merge if lww else eng.orset_merge)(A, B).to_numpy()
    e = exp[lww]
    ia, ib = np.maximum(e, 0), np.maximum(-e - 1, 0)
    for kind in ("u64", "16B", "u16"):
        va, vb = _vals(len(A), 0, kind), _vals(len(B), 1, kind)
        out, val, cnt = fn(A, va.to(eng.device), B, vb.to(eng.device))
        c = int(cnt.item())
        assert c == len(e)
        for g, x, f in zip(out.slice(c).to_numpy(), plain, ("key", "ts", "rep", "tomb")):
            np.testing.assert_array_equal(g, x, err_msg=f"{kind} out.{f}")
        got = val[:c].cpu().numpy()
        want = np.where((e >= 0).reshape((-1,) + (1,) * (got.ndim - 1)), va.numpy()[ia], vb.numpy()[ib])
        np.testing.assert_array_equal(got, want, err_msg=kind)
        if kind == "u64":                                # val = side << 63 | index decodes to exactly src
            u = got.view(U64)
            idx = (u & U64((1 << 63) - 1)).astype(np.int64)
            np.testing.assert_array_equal(np.where(u >> U64(63) == 0, idx, -idx - 1), e)
    assert eng.device_status(clear=True) == 0


@pytest.mark.parametrize("lww", [True, False])
def test_map_merge_is_capturable(eng, lww):
    """No read-back between the merge and the gather (nor inside either): the
    whole map merge is captured in a graph -- a synchronising call would fail
    the capture -- and the replay gives the eager result."""
    a, b, exp = seeded(20_003, 15_001, 6_000, 29)
    A = TupleSet.from_numpy(*a, eng.device)
    B = TupleSet.from_numpy(*b, eng.device)
    va, vb = _vals(len(A), 0, "u64").to(eng.device), _vals(len(B), 1, "u64").to(eng.device)
    fn = eng.lww_map_merge if lww else eng.orset_map_merge
    out0, val0, cnt0 = fn(A, va, B, vb)                  # eager (the workspace is sized here)
    torch.cuda.synchronize()
    c = int(cnt0.item())
    assert c == len(exp[lww])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        out, val, cnt = fn(A, va, B, vb)
    g.replay()
    torch.cuda.synchronize()
    assert int(cnt.item()) == c
    assert torch.equal(val[:c], val0[:c]) and torch.equal(out.key[:c], out0.key[:c])
    assert torch.equal(out.tomb[:c], out0.tomb[:c])
    assert eng.device_status(clear=True) == 0


# ---------------------------------------------------------------- the diagnostic build's write shapes
def _parts_cases(eng):
    check(eng, *seeded(40_003, 30_001, 9_000, 31)[:2], "seeded, small")
    for edge in (1024, 4096):
        for layout in ("a", "b", "ab"):
            check(eng, *_edge_case(edge, "tag", layout), f"edge {edge} tag run {layout}")
            check(eng, *_edge_case(edge, "key", layout), f"edge {edge} key run {layout}")


@pytest.mark.diag
@pytest.mark.parametrize("parts", [2, 4, 8, 16])
def test_lww_src_write_parts(eng, parts):
    """k_lww_write_src at every workgroup shape (sets.lww_parts; default 4)."""
    set_knob(b"sets.lww_parts", parts)
    try:
        _parts_cases(eng)
    finally:
        set_knob(b"sets.lww_parts", 4)


@pytest.mark.diag
@pytest.mark.parametrize("parts", [1, 2, 4])
def test_orset_src_write_parts(eng, parts):
    """k_or_write_src at every workgroup shape (sets.or_parts; default 2)."""
    set_knob(b"sets.or_parts", parts)
    try:
        _parts_cases(eng)
    finally:
        set_knob(b"sets.or_parts", 2)


# ---------------------------------------------------------------- gather_src on its own
SENT = -12345


def _gather_fixture(eng, n=5000, na=3000, nb=2500, seed=5):
    rng = np.random.default_rng(seed)
    side = rng.integers(0, 2, n).astype(bool)
    src = np.where(side, rng.integers(0, na, n), -rng.integers(0, nb, n) - 1).astype(np.int64)
    ca, cb = rng.integers(0, 1 << 40, na).astype(np.int64), rng.integers(0, 1 << 40, nb).astype(np.int64)
    want = np.where(src >= 0, ca[np.maximum(src, 0)], cb[np.maximum(-src - 1, 0)])
    dev = lambda x: torch.from_numpy(x.copy()).to(eng.device)
    return src, dev(src), dev(ca), dev(cb), want


def test_gather_device_length(eng):
    src, S, CA, CB, want = _gather_fixture(eng)
    n = len(src)
    full = eng.gather_src(S, CA, CB)
    np.testing.assert_array_equal(full.cpu().numpy(), want)
    for m in (0, 1, 63, 64, 65, 257, n - 1, n):
        out = torch.full((n,), SENT, dtype=torch.int64, device=eng.device)
        eng.gather_src(S, CA, CB, n_dev=torch.tensor([m], dtype=torch.int64, device=eng.device), out=out)
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[:m], want[:m])
        assert (got[m:] == SENT).all(), m                # the rest is untouched
    assert eng.device_status(clear=True) == 0
    for m in (n + 1, -1):                                # n_max + 1 and 2^64 - 1: nothing written, DEV_RANGE
        out = torch.full((n,), SENT, dtype=torch.int64, device=eng.device)
        eng.gather_src(S, CA, CB, n_dev=torch.tensor([m], dtype=torch.int64, device=eng.device), out=out)
        assert eng.device_status(clear=True) == DEV_RANGE
        assert (out.cpu().numpy() == SENT).all()
        assert eng.device_status(clear=True) == 0        # cleared


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.int32, torch.int64, "16B"])
def test_gather_indices_outside_their_side(eng, dtype):
    src, S, CA, CB, want = _gather_fixture(eng, seed=6)
    n, na, nb = len(src), CA.numel(), CB.numel()
    if dtype == "16B":
        conv = lambda x: torch.stack([x, x + 1], dim=1).contiguous()
    else:
        conv = lambda x: x.to(dtype)
    ca, cb = conv(CA), conv(CB)
    wt = torch.where((S >= 0).reshape((-1,) + (1,) * (ca.dim() - 1)), ca[S.clamp(min=0)], cb[(-S - 1).clamp(min=0)])
    bad = src.copy()
    bad[100], bad[4001] = na, -(nb + 1)                  # one past each side
    out = torch.full_like(wt, 77)
    eng.gather_src(torch.from_numpy(bad).to(eng.device), ca, cb, out=out)
    assert eng.device_status(clear=True) == DEV_RANGE
    keep = torch.ones(n, dtype=torch.bool, device=eng.device)
    keep[100] = keep[4001] = False
    assert torch.equal(out[keep], wt[keep])              # every other element written
    assert (out[~keep] == 77).all()                      # the two left as they were
    assert eng.device_status(clear=True) == 0


def _raw(eng, fn, *args):
    eng._bind()
    return getattr(_lib.lib(), fn)(eng.ctx, *args)


def test_gather_host_errors(eng):
    src, S, CA, CB, want = _gather_fixture(eng)
    n, na, nb = len(src), CA.numel(), CB.numel()
    out = torch.full((n + 2,), SENT, dtype=torch.int64, device=eng.device)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    raw = lambda *a: _raw(eng, "crdt_src_gather", *a)
    assert raw(p(S), n, None, p(CA), na, p(CB), nb, p(out), 8) == 0
    for es in (0, 3, 5, 12, 32):
        assert raw(p(S), n, None, p(CA), na, p(CB), nb, p(out), es) == E_INVAL
    assert raw(None, n, None, p(CA), na, p(CB), nb, p(out), 8) == E_INVAL
    assert raw(p(S), n, None, p(CA), na, p(CB), nb, None, 8) == E_INVAL
    assert raw(p(S), n, None, None, na, p(CB), nb, p(out), 8) == E_INVAL      # a NULL side with a length
    assert raw(p(S), n, None, p(CA), na, None, nb, p(out), 8) == E_INVAL
    assert raw(p(S, 4), n - 1, None, p(CA), na, p(CB), nb, p(out), 8) == E_INVAL   # misaligned src
    assert raw(p(S), n, None, p(CA), na, p(CB), nb, p(out, 4), 8) == E_INVAL       # ... out
    assert raw(p(S), n, None, p(CA, 2), na - 1, p(CB), nb, p(out), 4) == E_INVAL   # ... a column
    assert raw(p(S), n, None, p(CA), na, p(CB, 8), nb - 1, p(out), 16) == E_INVAL
    assert raw(p(S), n, None, p(CA), na, p(CB), nb, p(CA), 8) == E_INVAL           # out overlaps a column
    assert raw(p(S), n, None, p(CA), na, p(CB), nb, p(CB, 8 * (nb - 1)), 8) == E_INVAL
    assert raw(p(S), n, None, p(CA), na, p(CB), nb, p(S, 8 * (n - 1)), 8) == E_INVAL   # ... src
    assert raw(p(S), 2**62, None, p(CA), na, p(CB), nb, p(out), 8) == E_RANGE
    assert raw(None, 0, None, None, 0, None, 0, None, 8) == 0                     # n_max == 0: nothing launched
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out[:n].cpu().numpy(), want)                    # only the first call wrote
    assert (out[n:] == SENT).all()
    assert eng.device_status(clear=True) == 0


@pytest.mark.parametrize("fn", ["crdt_lww_merge_src", "crdt_orset_merge_src"])
def test_merge_src_host_errors(eng, fn):
    a, b, _ = seeded(20_003, 15_001, 6_000, 29)
    A = TupleSet.from_numpy(*a, eng.device)
    B = TupleSet.from_numpy(*b, eng.device)
    na, nb = len(A), len(B)
    out = TupleSet.empty(na + nb, eng.device)
    src = torch.empty(na + nb + 1, dtype=torch.int64, device=eng.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=eng.device)
    ca, cb, co = A.c(), B.c(), out.c()
    raw = lambda s: _raw(eng, fn, C.byref(ca), na, C.byref(cb), nb, C.byref(co), s, C.c_void_p(cnt.data_ptr()))
    assert raw(None) == E_INVAL
    assert raw(C.c_void_p(src.data_ptr() + 4)) == E_INVAL                         # misaligned
    assert raw(C.c_void_p(A.key.data_ptr())) == E_INVAL                           # overlaps an input
    assert raw(C.c_void_p(B.ts.data_ptr() + 8 * (nb - 1))) == E_INVAL
    assert raw(C.c_void_p(B.tomb.data_ptr() & ~7)) == E_INVAL
    assert raw(C.c_void_p(out.key.data_ptr())) == E_INVAL                         # ... or out
    assert raw(C.c_void_p(out.rep.data_ptr() + 4 * (na + nb - 2))) == E_INVAL
    torch.cuda.synchronize()
    assert int(cnt.item()) == 0                                                   # nothing ran
    assert raw(C.c_void_p(src.data_ptr() + 8)) == 0                               # any 8-byte aligned offset is fine
    assert _raw(eng, fn, C.byref(ca), 0, C.byref(cb), 0, C.byref(co), None, C.c_void_p(cnt.data_ptr())) == 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == 0                                                   # both sides empty: NULL src is fine
    assert eng.device_status(clear=True) == 0
