"""GPU: the map reads -- each member key's winning tuple, its sibling count and
the batched point lookup (crdt_map_read, crdt_map_lookup; csrc/mapread.hip)
against the numpy closed form of tests/map_read_util.py, every output compared
bit for bit and written into views inside canary buffers.

Tile = 2048 tuples (four waves of eight 64-tuple mask words).  The hand-built
cases put the run whose decision crosses an edge at a tile edge (2048), and
again at a word edge (64) and at a wave edge (512) inside tile 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from crdt_amd import _lib, synth
from crdt_amd.engine import TupleSet, as_u64, u64_tensor
from map_read_util import ref_lookup, ref_map_read

pytestmark = pytest.mark.gpu

T = 2048                       # tuples per tile
NC = 3 * T + 10                # the hand-built states
DEV_RANGE = 2                  # CRDT_DEV_RANGE
E_INVAL = -1                   # CRDT_E_INVAL
M64 = 2**64 - 1
G = 64                         # canary elements each side of an output view
CANARY = 0x5a
EDGES = [T, 64, 512]
MODES = [True, False]


class Guarded:
    def __init__(self, n, dtype, dev):
        self.n = n
        self.buf = torch.full((n + 2 * G,), CANARY, dtype=dtype, device=dev)
        self.view = self.buf[G:G + n]

    def check(self, k, what):
        """Nothing but the first k entries of the view was written."""
        b = self.buf.cpu().numpy()
        assert (b[:G] == CANARY).all() and (b[G + k:] == CANARY).all(), f"{what}: a write outside the first {k} outputs"
        return b[G:G + k]


def _count(c):
    return int(as_u64(c)[0])


def _sets(n, ks):
    return synth.sort_tuples_np(*synth.set_tuples(31 + n, 0, n, ks))


def _read(eng, Td, lww, exp, what, with_keys=True, with_nsib=True, n_dev=None):
    """One crdt_map_read into canary-guarded views == exp, bit for bit."""
    n = len(Td)
    keys = Guarded(n, torch.int64, eng.device) if with_keys else None
    nsib = Guarded(n, torch.int32, eng.device) if with_nsib else None
    win = Guarded(n, torch.int64, eng.device)
    k_, w_, s_, cnt = eng.map_read(Td, lww, n_dev=n_dev, with_keys=with_keys, with_nsib=with_nsib,
                                   keys=keys.view if keys else None, win=win.view, nsib=nsib.view if nsib else None)
    assert (k_ is None) == (not with_keys) and (s_ is None) == (not with_nsib), what
    k = len(exp[0])
    assert _count(cnt) == k, (what, _count(cnt), k)
    np.testing.assert_array_equal(win.check(k, what + " win"), exp[1], err_msg=what + " win")
    if with_keys:
        np.testing.assert_array_equal(keys.check(k, what + " keys").view(np.uint64), exp[0], err_msg=what + " keys")
    if with_nsib:
        np.testing.assert_array_equal(nsib.check(k, what + " nsib").view(np.uint32), exp[2], err_msg=what + " nsib")


def _lookup(eng, Td, lww, exp, probes, what, with_nsib=True, n_dev=None):
    m = len(probes)
    win = Guarded(m, torch.int64, eng.device)
    nsib = Guarded(m, torch.int32, eng.device) if with_nsib else None
    eng.map_lookup(Td, u64_tensor(probes, eng.device), lww, n_dev=n_dev, with_nsib=with_nsib, win=win.view,
                   nsib=nsib.view if nsib else None)
    ew, es = ref_lookup(exp, probes)
    np.testing.assert_array_equal(win.check(m, what + " lookup win"), ew, err_msg=what + " lookup win")
    if with_nsib:
        np.testing.assert_array_equal(nsib.check(m, what + " lookup nsib").view(np.uint32), es, err_msg=what + " lookup nsib")


def _probes(t, rng):
    """Every key of the state, keys below its minimum and above its maximum,
    keys in the gaps, and duplicates, shuffled."""
    ks = np.unique(t[0])
    lo, hi = (int(ks[0]), int(ks[-1])) if len(ks) else (5, 5)
    extra = [0, max(lo - 1, 0), max(lo - 2, 0), min(hi + 1, M64), min(hi + 2, M64), M64]
    gaps = ks[:-1] + (ks[1:] - ks[:-1]) // np.uint64(2) if len(ks) > 1 else ks[:0]
    p = np.concatenate([ks, ks[::3], gaps, np.array(extra, np.uint64)]).astype(np.uint64)
    return p[rng.permutation(len(p))]


def _both(eng, t, what, lookups=True):
    """Both modes: the read with every output, and the lookup of the state's keys and their surroundings."""
    Td = TupleSet.from_numpy(*t, eng.device)
    res = {}
    for lww in MODES:
        exp = ref_map_read(*t, lww)
        w = f"{what} lww={lww}"
        _read(eng, Td, lww, exp, w)
        if lookups:
            _lookup(eng, Td, lww, exp, _probes(t, np.random.default_rng(7)), w)
        res[lww] = exp
    assert eng.device_status(clear=True) == 0
    return res


def _row(exp, key):
    i = int(np.searchsorted(exp[0], np.uint64(key)))
    assert i < len(exp[0]) and exp[0][i] == key, f"key {key} is not a member"
    return int(exp[1][i]), int(exp[2][i])


def _absent(exp, key):
    i = int(np.searchsorted(exp[0], np.uint64(key)))
    return not (i < len(exp[0]) and exp[0][i] == key)


# ---- 1. sizes x key spaces, both modes, every combination of optional outputs
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 4097, 8193, 100_000])
def test_sizes_and_key_spaces(eng, n):
    rng = np.random.default_rng(n)
    for ks in (1, 7, max(1, n // 3), 10**9):
        t = _sets(n, ks)
        Td = TupleSet.from_numpy(*t, eng.device)
        for lww in MODES:
            exp = ref_map_read(*t, lww)
            for with_keys in (True, False):
                for with_nsib in (True, False):
                    _read(eng, Td, lww, exp, f"n={n} ks={ks} lww={lww} keys={with_keys} nsib={with_nsib}", with_keys, with_nsib)
            if n:
                for with_nsib in (True, False):
                    _lookup(eng, Td, lww, exp, _probes(t, rng), f"n={n} ks={ks} lww={lww}", with_nsib)
    assert eng.device_status(clear=True) == 0


def test_grid_is_not_trivial():
    """The seeded states hold multi-valued keys and winners followed by dead tuples of their key."""
    t = _sets(100_000, 100_000 // 3)
    keys, win, nsib = ref_map_read(*t, False)
    assert (nsib > 1).sum() > len(keys) // 2
    nxt = np.minimum(win + 1, len(t[0]) - 1)
    assert ((t[0][nxt] == keys) & (nxt > win)).sum() > 1000


# ---- 2. hand-built cases: `U` is the edge's unit -- "tile k" below is tuples [k U, (k + 1) U)
def _ordinary(n=NC):
    """n single-tuple keys 10 i (distinct tags), every third tombstoned."""
    i = np.arange(n)
    return ((10 * i).astype(np.uint64), (1000 + i).astype(np.uint64), (i % 5).astype(np.uint32),
            (i % 3 == 0).astype(np.uint8))


def _one_key(t, lo, hi):
    """Tuples [lo, hi) become one key, 10 lo, with distinct ascending tags."""
    t[0][lo:hi] = 10 * lo
    t[2][lo:hi] = 0


def _one_tag(t, lo, hi):
    """Tuples [lo, hi) become copies of the tag of tuple lo."""
    t[1][lo:hi] = t[1][lo]
    t[2][lo:hi] = t[2][lo]


@pytest.mark.parametrize("U", EDGES)
def test_winner_tiles_before_the_key_end(eng, U):
    """One key from tile 0 to tile 3: a live tag, then the winner -- its first
    copy in tile 0, copies running into tile 1 -- then only dead tags through
    tile 2, the key end in tile 3."""
    t = _ordinary()
    lo, hi = U - 6, 3 * U + 4
    _one_key(t, lo, hi)
    _one_tag(t, lo + 1, U + 3)
    t[3][lo:U + 3] = 0
    t[3][U + 3:hi] = 1
    res = _both(eng, t, f"winner far, U={U}")
    assert _row(res[False], 10 * lo) == (lo + 1, 2)
    assert _absent(res[True], 10 * lo)                   # LWW: the maximal tag is dead


@pytest.mark.parametrize("U", EDGES)
@pytest.mark.parametrize("live", [False, True])
def test_tag_over_the_edge_decided_by_the_copy_before_it(eng, U, live):
    """A tag with one copy as the last tuple of a tile and its run's end as the
    first tuple of the next.  The copy before the edge tombstoned: the carried
    tomb-OR kills the next tile's first tag end, and the winner falls back to
    an earlier tag.  Both copies live: that tag wins, from its first copy."""
    t = _ordinary()
    lo, hi = U - 4, U + 3
    _one_key(t, lo, hi)
    _one_tag(t, U - 1, U + 1)
    t[3][lo:hi] = [0, 1, 1, 0 if live else 1, 0, 1, 1]
    res = _both(eng, t, f"tag over the edge, U={U} live={live}")
    assert _row(res[False], 10 * lo) == ((U - 1, 2) if live else (lo, 1))


@pytest.mark.parametrize("U", EDGES)
def test_long_tag_over_many_tiles(eng, U):
    """One tag from tile 0 through tile 2: alive it wins from its first copy,
    tiles before its end; with a single tombstoned copy in tile 0 it is dead
    and the key's earlier tag wins."""
    for dead in (False, True):
        t = _ordinary()
        lo, hi = U - 5, 2 * U + 9
        _one_key(t, lo, hi)
        _one_tag(t, lo + 2, hi - 1)
        t[3][lo:hi] = 0
        t[3][hi - 1] = 1                                 # the key's maximal tag: dead
        t[3][lo + 3] = 1 if dead else 0
        res = _both(eng, t, f"long tag, U={U} dead={dead}")
        assert _row(res[False], 10 * lo) == ((lo + 1, 2) if dead else (lo + 2, 3))


@pytest.mark.parametrize("U", EDGES)
def test_siblings_counted_across_tiles(eng, U):
    """A key with live tags in every tile, dead ones between, some tags in two copies."""
    t = _ordinary()
    lo, hi = 5, 3 * U + 5
    _one_key(t, lo, hi)
    i = np.arange(lo, hi)
    t[3][lo:hi] = (i % 7 != 0).astype(np.uint8)
    for e in (U, 2 * U, 3 * U):                          # a two-copy tag over each edge, live at U and 3 U
        _one_tag(t, e - 1, e + 1)
        t[3][e - 1:e + 1] = 0 if e != 2 * U else (0, 1)
    res = _both(eng, t, f"siblings, U={U}")
    win, nsib = _row(res[False], 10 * lo)
    assert nsib == len({(a, b) for a, b, c in zip(t[1][lo:hi], t[2][lo:hi], t[3][lo:hi])}
                       - {(a, b) for a, b, c in zip(t[1][lo:hi], t[2][lo:hi], t[3][lo:hi]) if c})
    assert nsib >= 3 * U // 7 - 3 and win >= 3 * U - 1


@pytest.mark.parametrize("U", EDGES)
def test_member_after_three_tiles_of_dead_tuples(eng, U):
    t = _ordinary()
    t[3][:3 * U] = 1
    t[3][3 * U] = 0
    t[3][3 * U + 1:] = 1
    res = _both(eng, t, f"member after dead tiles, U={U}")
    for lww in MODES:
        assert len(res[lww][0]) == 1 and _row(res[lww], 10 * 3 * U) == (3 * U, 1)


@pytest.mark.parametrize("U", EDGES)
def test_non_member_keys_between_members(eng, U):
    """Multi-tuple keys that are not members (every tag dead, one by a single
    tombstoned copy) between member keys, over each edge."""
    t = _ordinary()
    for e in (U, 2 * U, 3 * U):
        _one_key(t, e - 9, e - 5)                        # a member: two live tags
        t[3][e - 9:e - 5] = [0, 1, 0, 1]
        _one_key(t, e - 5, e + 2)                        # not a member, over the edge
        _one_tag(t, e - 2, e + 1)
        t[3][e - 5:e + 2] = [1, 1, 1, 0, 0, 1, 1]
        _one_key(t, e + 2, e + 5)                        # a member again
        t[3][e + 2:e + 5] = [1, 0, 1]
    res = _both(eng, t, f"non-members between, U={U}")
    for e in (U, 2 * U, 3 * U):
        assert _row(res[False], 10 * (e - 9)) == (e - 7, 2)
        assert _absent(res[False], 10 * (e - 5))
        assert _row(res[False], 10 * (e + 2)) == (e + 3, 1)


def test_one_key_across_many_tiles(eng):
    """One key of 20000 tuples in two-copy tags: the winner and the sibling
    count of a key whose run is ten tiles long."""
    n = 20_000
    key = np.zeros(n, np.uint64)
    ts = np.repeat(np.arange(n // 2, dtype=np.uint64), 2)
    rep = np.zeros(n, np.uint32)
    for mod in (3, 5):
        t = (key, ts, rep, (np.arange(n) % mod == 0).astype(np.uint8))
        res = _both(eng, t, f"one key, mod={mod}")
        assert len(res[False][0]) == 1 and res[False][2][0] > 1000


# ---- 3. the device length
def test_shorter_device_length(eng):
    """Only the first *n_dev tuples are read: cut inside a key's run, inside a
    tag's run and at tile edges, what lies past the cut would change the rows."""
    t = _ordinary(2 * T + 40)
    _one_key(t, T - 6, T + 6)
    _one_tag(t, T - 2, T + 2)
    t[3][T - 6:T + 6] = [1, 0, 1, 1, 0, 0, 0, 1, 1, 1, 0, 1]
    Td = TupleSet.from_numpy(*t, eng.device)
    for nd in (0, 1, T - 5, T - 1, T, T + 1, T + 2, T + 5, 2 * T, 2 * T + 39):
        n_dev = torch.tensor([nd], dtype=torch.int64, device=eng.device)
        cut = tuple(x[:nd] for x in t)
        for lww in MODES:
            exp = ref_map_read(*cut, lww)
            _read(eng, Td, lww, exp, f"n_dev={nd} lww={lww}", n_dev=n_dev)
            _lookup(eng, Td, lww, exp, _probes(t, np.random.default_rng(nd)), f"n_dev={nd} lww={lww}", n_dev=n_dev)
    assert eng.device_status(clear=True) == 0


def test_device_length_out_of_range(eng):
    t = _sets(5000, 300)
    Td = TupleSet.from_numpy(*t, eng.device)
    probes = u64_tensor(np.unique(t[0]), eng.device)
    for bad in (len(t[0]) + 1, -1):                      # (-1: the ~0 a failed call leaves as its count)
        n_dev = torch.tensor([bad], dtype=torch.int64, device=eng.device)
        for lww in MODES:
            keys, win, nsib = (Guarded(5000, d, eng.device) for d in (torch.int64, torch.int64, torch.int32))
            _, _, _, cnt = eng.map_read(Td, lww, n_dev=n_dev, keys=keys.view, win=win.view, nsib=nsib.view)
            assert _count(cnt) == M64
            for g in (keys, win, nsib):
                g.check(0, "read, n_dev out of range")
            assert eng.device_status(clear=True) == DEV_RANGE
            w, s = eng.map_lookup(Td, probes, lww, n_dev=n_dev, with_nsib=True)
            assert (w.cpu().numpy() == -1).all() and (s.cpu().numpy() == 0).all()
            assert eng.device_status(clear=True) == DEV_RANGE


def test_read_chained_off_a_merge_count(eng):
    a, b = _sets(3000, 500), synth.sort_tuples_np(*synth.set_tuples(31 + 3000, 1, 2500, 500))
    A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
    out, cnt = eng.orset_merge(A, B, trim=False)
    keys, win, nsib, c = eng.map_read(out, False, n_dev=cnt, with_nsib=True)
    k = int(cnt.item())
    m = tuple(x.cpu().numpy()[:k] for x in (out.key, out.ts, out.rep, out.tomb))
    m = (m[0].view(np.uint64), m[1].view(np.uint64), m[2].view(np.uint32), m[3])
    exp = ref_map_read(*m, False)
    r = _count(c)
    assert r == len(exp[0]) and 0 < r < k < len(out)
    np.testing.assert_array_equal(as_u64(keys)[:r], exp[0])
    np.testing.assert_array_equal(win.cpu().numpy()[:r], exp[1])
    np.testing.assert_array_equal(nsib.cpu().numpy()[:r].view(np.uint32), exp[2])
    assert eng.device_status(clear=True) == 0


# ---- 4. lookups at the edges of the call
def test_lookup_of_nothing_and_in_nothing(eng):
    t = _sets(300, 40)
    Td = TupleSet.from_numpy(*t, eng.device)
    empty = TupleSet.from_numpy(*(x[:0] for x in t), eng.device)
    none = torch.empty(0, dtype=torch.int64, device=eng.device)
    for lww in MODES:
        w, s = eng.map_lookup(Td, none, lww, with_nsib=True)           # m = 0
        assert w.numel() == 0 and s.numel() == 0
        _lookup(eng, empty, lww, ref_map_read(*(x[:0] for x in t), lww), _probes(t, np.random.default_rng(1)),
                f"empty state lww={lww}")
        assert _lib.call("crdt_map_lookup", eng.ctx, 0 if lww else 1, C.byref(Td.c()), len(Td), None, None, 0, None, None) == 0
    assert eng.device_status(clear=True) == 0


# ---- 5. round trips: puts and deletes on two replicas, merged, read as a map
@pytest.mark.parametrize("causal", [False, True])
def test_put_delete_merge_get(eng, causal):
    rng = np.random.default_rng(11 + causal)
    dev = eng.device
    KS = 60

    def batch(m):
        keys = np.sort(rng.integers(1, KS, m)).astype(np.uint64)
        kinds = (rng.random(m) < 0.35).astype(np.uint8)
        vals = rng.integers(1, 1 << 40, m).astype(np.int64)
        return keys, kinds, vals

    def model_apply(tags, clock, rep, keys, kinds, vals):
        for i in range(len(keys)):
            k, ev = int(keys[i]), clock[rep] + 1 + i
            if kinds[i] == 0:
                tags[(k, ev, rep)] = [int(vals[i]), 0]
            else:
                for g in [g for g in tags if g[0] == k]:
                    if causal:
                        del tags[g]
                    else:
                        tags[g][1] = 1
        clock[rep] += len(keys)

    def dev_apply(state, val, clock, rep, keys, kinds, vals):
        out, oval, clock_out, cnt = eng.map_apply(state, val, clock, rep, u64_tensor(keys, dev),
                                                  torch.from_numpy(kinds).to(dev), torch.from_numpy(vals).to(dev), causal)
        k = int(cnt.item())
        return out.slice(k), oval[:k].contiguous(), clock_out

    # replica 0 applies a batch; replica 1 starts from a copy of the result; each applies two more
    empty = TupleSet.from_numpy(*(np.zeros(0, d) for d in (np.uint64, np.uint64, np.uint32, np.uint8)), dev)
    s0, v0, c0 = empty, torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    m0, mc0 = {}, [0, 0]
    b = batch(80)
    s0, v0, c0 = dev_apply(s0, v0, c0, 0, *b)
    model_apply(m0, mc0, 0, *b)
    s1, v1, c1 = s0, v0, c0
    m1, mc1 = {g: list(x) for g, x in m0.items()}, list(mc0)
    for _ in range(2):
        b = batch(50)
        s0, v0, c0 = dev_apply(s0, v0, c0, 0, *b)
        model_apply(m0, mc0, 0, *b)
        b = batch(50)
        s1, v1, c1 = dev_apply(s1, v1, c1, 1, *b)
        model_apply(m1, mc1, 1, *b)
    merged, mval, cnt = eng.orset_map_merge(s0, v0, s1, v1)
    model = {}
    for g in set(m0) | set(m1):
        x, y = m0.get(g), m1.get(g)
        model[g] = [(x or y)[0], (x[1] if x else 0) | (y[1] if y else 0)]
    want = {}                                            # key -> (its greatest live tag, that tag's value, live tags)
    for (k, ev, rep), (val, dead) in model.items():
        if not dead:
            cur = want.get(k)
            want[k] = ((ev, rep), val, 1) if cur is None else (max(cur[0], (ev, rep)), val if (ev, rep) > cur[0] else cur[1], cur[2] + 1)
    assert 5 < len(want) < KS - 1 and any(w[2] > 1 for w in want.values())

    keys, vals, c = eng.map_values(merged, mval, False, n_dev=cnt)
    r = _count(c)
    assert r == len(want)
    gk, gv = as_u64(keys)[:r], vals.cpu().numpy()[:r]
    assert [int(x) for x in gk] == sorted(want)
    assert [int(x) for x in gv] == [want[k][1] for k in sorted(want)]
    _, _, nsib, _ = eng.map_read(merged, False, n_dev=cnt, with_nsib=True)
    assert [int(x) for x in nsib.cpu().numpy()[:r]] == [want[k][2] for k in sorted(want)]

    probes = np.arange(0, KS + 3, dtype=np.uint64)
    probes = np.concatenate([probes, probes[::4]])
    k = int(cnt.item())
    got = eng.map_get(merged.slice(k), mval[:k].contiguous(), u64_tensor(probes, dev), -7, False)
    assert [int(x) for x in got.cpu().numpy()] == [want[int(p)][1] if int(p) in want else -7 for p in probes]
    assert eng.device_status(clear=True) == 0           # a missing key raises nothing


# ---- 6. argument errors
def test_argument_errors(eng):
    n = 256
    t = _sets(n, 40)
    Td = TupleSet.from_numpy(*t, eng.device)
    dev = eng.device
    i64 = lambda k=n: torch.zeros(k + 1, dtype=torch.int64, device=dev)
    i32 = lambda k=n: torch.zeros(k + 1, dtype=torch.int32, device=dev)
    keys, win, nsib, cnt, probes = i64(), i64(), i32(), i64(0), i64()
    ct = Td.c()

    p = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr())

    def status(fn, *args):
        eng._bind()
        try:
            return _lib.call(fn, *args)
        except _lib.CrdtError as e:
            return e.status

    def read(mode=1, tt=ct, n_max=n, keys=keys, win=win, nsib=nsib, cnt=cnt, ctx=eng.ctx):
        return status("crdt_map_read", ctx, mode, C.byref(tt) if tt is not None else None, n_max, None, p(keys),
                      p(win), p(nsib), p(cnt))

    def lookup(mode=1, tt=ct, n_max=n, probes=probes, m=n, win=win, nsib=nsib):
        return status("crdt_map_lookup", eng.ctx, mode, C.byref(tt) if tt is not None else None, n_max, None,
                      p(probes), m, p(win), p(nsib))

    assert read() == 0 and lookup() == 0
    assert read(keys=None, nsib=None) == 0 and lookup(nsib=None) == 0
    null = _lib.crdt_tuples(None, None, None, None)
    assert read(tt=null, n_max=0, keys=None, win=None, nsib=None) == 0       # an empty call needs no outputs
    odd = _lib.crdt_tuples(ct.key + 4, ct.ts, ct.rep, ct.tomb)
    for mode in (0, 1):
        assert read(mode, tt=None) == E_INVAL and lookup(mode, tt=None) == E_INVAL
        assert read(mode, cnt=None) == E_INVAL
        assert read(mode, win=None) == E_INVAL and lookup(mode, win=None) == E_INVAL
        assert lookup(mode, probes=None) == E_INVAL
        assert read(mode, tt=null) == E_INVAL and lookup(mode, tt=null) == E_INVAL
        assert read(mode, tt=odd) == E_INVAL and lookup(mode, tt=odd) == E_INVAL
        # misaligned
        assert read(mode, keys=keys.data_ptr() + 4) == E_INVAL and read(mode, win=win.data_ptr() + 4) == E_INVAL
        assert read(mode, nsib=nsib.data_ptr() + 2) == E_INVAL
        assert lookup(mode, probes=probes.data_ptr() + 4) == E_INVAL and lookup(mode, win=win.data_ptr() + 4) == E_INVAL
        assert lookup(mode, nsib=nsib.data_ptr() + 2) == E_INVAL
        # overlapping: an output with the state, an output with another, the lookup's outputs with its probes
        assert read(mode, keys=Td.key) == E_INVAL and read(mode, win=Td.ts) == E_INVAL and read(mode, nsib=Td.rep) == E_INVAL
        assert read(mode, keys=win) == E_INVAL and read(mode, nsib=win) == E_INVAL and read(mode, nsib=keys) == E_INVAL
        assert read(mode, win=win.data_ptr() + 8, keys=win) == E_INVAL
        assert lookup(mode, win=Td.key) == E_INVAL and lookup(mode, nsib=Td.rep) == E_INVAL
        assert lookup(mode, win=probes) == E_INVAL and lookup(mode, nsib=probes) == E_INVAL and lookup(mode, nsib=win) == E_INVAL
    assert read(2) == E_INVAL and lookup(-1) == E_INVAL
    assert read(ctx=None) == E_INVAL
    assert read(n_max=2**62) == -6 and lookup(n_max=2**62) == -6        # CRDT_E_RANGE
    eng.sync()
    assert eng.device_status(clear=True) == 0
