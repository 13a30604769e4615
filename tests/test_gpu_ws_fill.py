"""GPU: no kernel depends on what its scratch held before the call.

Every device entry point carves its scratch out of the context's workspace
(ws_reserve, csrc/capi.hip); the sharded protocols keep a second arena per
member (scratch_reserve, csrc/shard.hip).  The rest of the suite shares one
engine and runs in a fixed order, so each op finds there what the test before
it left -- the same bytes on every run.  Here every family that touches the
workspace runs

1. under the diagnostic build's ``ctx.ws_fill``: the whole workspace is set
   to 0x00, 0xFF or 0xA5 before EVERY engine call of the case (``Filling``
   reserves 64 MiB in front of each, which is what fills, and holds
   ``ctx.ws_filled_mb`` to have advanced by as much), and
2. in shrink-and-swap sequences on one engine with no reserve in between
   (any build): five tiles, two and a partial, none, one element, another
   family whose carve lays other arrays over the first's, the first again --
   a previous call's real counts and bitmaps pass every range check.

Every output -- tuples, device counts, source indices, contexts, flags -- is
compared bit for bit with the CPU oracle (oracle/) or the numpy restatements of
the family's own test module, never with another GPU run, and the device
status must stay 0.  The rows, their kernel files and shapes are
tests/ws_fill_table.py; a new kernel's scratch is expected to pass here.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import apply_util as au
import test_gpu_codec as t_codec
import test_gpu_counters as t_cnt
import test_gpu_d2_planned as t_d2
import test_gpu_local_apply as t_local
import test_gpu_map_read as t_map
import test_gpu_population as t_pop
import test_gpu_refmerge as t_ref
import test_gpu_seg as t_seg
import test_gpu_set_apply as t_apply
import test_gpu_set_causal as t_causal
import test_gpu_set_causal_ranges as t_cr
import test_gpu_set_compact as t_compact
import test_gpu_set_delta as t_delta
import test_gpu_set_digest as t_dig
import test_gpu_set_read as t_read
import test_gpu_set_src as t_src
import test_gpu_shard_loopback as t_loop
import test_gpu_sort as t_sort
from crdt_amd import _lib, refmerge, shard, synth
from crdt_amd.engine import TupleSet, as_u64, u64_tensor
from knobs import set_knob
from map_read_util import ref_map_read
from oracle import oracle
from refmerge_util import assert_batch_matches_oracle, oracle_merge
from test_shard_gloo import rank_sets, stable_rank_merge
from ws_fill_table import LT, N_DEV, N_SET, N_SORT, NA, NB, ROWS, SEQUENCES, T

pytestmark = pytest.mark.gpu

RESERVE = 64 << 20             # far above what any row needs: no row grows the workspace
FILLS = [0x00, -1, 0xFF, 0xA5]  # 0x00 first: the bytes a fresh allocation usually holds
FIELDS = ("key", "ts", "rep", "tomb")
MODES = (True, False)
M64 = 2**64 - 1


def _filled_mb():
    return _lib.get_option(b"ctx.ws_filled_mb")


class Filling:
    """The engine, with every call made through it started from a freshly
    filled workspace: crdt_ctx_reserve in front of the call (under
    ctx.ws_fill >= 0 it sets every byte of the workspace; the counter must
    show it did).  The engine's own nested calls (a gather chained behind its
    merge) are one call."""
    _PLAIN = {"device_status", "check_device", "sync", "reserve", "close"}

    def __init__(self, eng, fill):
        self._eng, self._fill, self.fills = eng, fill, 0

    def fill_now(self):
        before = _filled_mb()
        self._eng.reserve(RESERVE)
        if self._fill >= 0:
            assert _filled_mb() - before >= RESERVE >> 20, "crdt_ctx_reserve filled nothing"
        self.fills += 1

    def __getattr__(self, name):
        v = getattr(self._eng, name)
        if not callable(v) or name in self._PLAIN or (name.startswith("_") and name != "_call"):
            return v

        def call(*a, **k):
            self.fill_now()
            return v(*a, **k)
        return call


@pytest.fixture(scope="module", autouse=True)
def _fill_off_after_the_module():
    yield
    if _lib.is_diag():
        _lib.set_option(b"ctx.ws_fill", -1)


@pytest.fixture
def filling(eng, fill):
    set_knob(b"ctx.ws_fill", fill)       # the product build: -1 is a plain parity run, the others skip
    try:
        yield Filling(eng, fill)
    finally:
        if _lib.is_diag():
            _lib.set_option(b"ctx.ws_fill", -1)


# ---------------------------------------------------------------- shared inputs and comparisons
def _dev(e, t):
    return TupleSet.from_numpy(*t, e.device)


def _n_dev(e, n):
    return u64_tensor(np.array([n], np.uint64), e.device)


def _cut(t, n):
    return tuple(np.ascontiguousarray(x[:n]) for x in t)


def _same(got, exp, what):
    for g, x, f in zip(got, exp, FIELDS):
        np.testing.assert_array_equal(g, x, err_msg=f"{what} {f}")


def _merge(lww):
    return oracle.lww_merge if lww else oracle.orset_merge


@functools.lru_cache(maxsize=64)
def _side(seed, side, n, ks=3000):
    return tuple(np.ascontiguousarray(x) for x in synth.sort_tuples_np(*synth.set_tuples(seed, side, n, ks)))


@functools.lru_cache(maxsize=64)
def _state(seed, n, ks=900):
    """One sorted state of n tuples that holds copies of a tag (both sides of a pair, cut)."""
    a, b = _side(seed, 0, n, ks), _side(seed, 1, n, ks)
    both = synth.sort_tuples_np(*(np.concatenate([x, y]) for x, y in zip(a, b)))
    return _cut(both, n)


@functools.lru_cache(maxsize=64)
def _merged(seed, na, nb, lww):
    return _merge(lww)(_side(seed, 0, na), _side(seed, 1, nb))


# ---------------------------------------------------------------- the families: fam(e, size, seed)
def fam_merge(e, n, seed=71, sides=None):
    na, nb = sides if sides else (n - n // 3, n // 3)
    a, b = _side(seed, 0, na), _side(seed, 1, nb)
    A, B = _dev(e, a), _dev(e, b)
    for lww in MODES:
        exp = _merged(seed, na, nb, lww)
        out, cnt = (e.lww_merge if lww else e.orset_merge)(A, B, trim=False)
        k = int(cnt.item())
        assert k == len(exp[0]), (lww, k, len(exp[0]))
        _same(out.slice(k).to_numpy(), exp, f"merge lww={lww}")
    assert e.device_status() == 0


def fam_merge_src(e, n, seed=72, sides=None, vals=False):
    na, nb = sides if sides else (n - n // 3, n // 3)
    a, b = _side(seed, 0, na), _side(seed, 1, nb)
    A, B = _dev(e, a), _dev(e, b)
    av, bv = np.arange(na, dtype=np.int64) * 3 + 1, -np.arange(nb, dtype=np.int64) * 5 - 2
    for lww in MODES:
        exp, esrc = _merged(seed, na, nb, lww), t_src.ref_src(a, b, lww)
        if vals:
            out, oval, cnt = (e.lww_map_merge if lww else e.orset_map_merge)(
                A, torch.from_numpy(av).to(e.device), B, torch.from_numpy(bv).to(e.device))
        else:
            out, cnt, src = (e.lww_merge_src if lww else e.orset_merge_src)(A, B)
        k = int(cnt.item())
        assert k == len(exp[0]), (lww, k, len(exp[0]))
        _same(out.slice(k).to_numpy(), exp, f"merge_src lww={lww}")
        if vals:
            ev = np.where(esrc >= 0, av[np.maximum(esrc, 0)] if na else 0, bv[np.maximum(-esrc - 1, 0)] if nb else 0)
            np.testing.assert_array_equal(oval[:k].cpu().numpy(), ev, err_msg=f"values lww={lww}")
        else:
            np.testing.assert_array_equal(src[:k].cpu().numpy(), esrc, err_msg=f"src lww={lww}")
    assert e.device_status() == 0


def fam_tuples_merge(e, n, seed=73, sides=None):
    na, nb = sides if sides else (n - n // 3, n // 3)
    a, b = _side(seed, 0, na), _side(seed, 1, nb)
    _same(e.tuples_merge(_dev(e, a), _dev(e, b)).to_numpy(), stable_rank_merge([a, b]), "tuples_merge")
    assert e.device_status() == 0


def fam_set_read(e, n, seed=31, n_dev=None):
    t = _state(seed, n)
    Td, nd = _dev(e, t), None if n_dev is None else _n_dev(e, n_dev)
    seen = t if n_dev is None else _cut(t, n_dev)
    for lww in MODES:
        exp = t_read.ref_elements(*seen, lww)
        keys, cnt = e.set_elements(Td, lww, n_dev=nd)
        card = e.set_cardinality(Td, lww, n_dev=nd)
        k = int(cnt.item())
        assert k == len(exp) == int(card.item()), (lww, k, len(exp), int(card.item()))
        np.testing.assert_array_equal(as_u64(keys)[:k], exp, err_msg=f"elements lww={lww}")
        probes = np.concatenate([exp[::3], exp[::3] + np.uint64(1), np.array([0, M64], np.uint64)])
        got = e.keys_contain(keys, u64_tensor(probes, e.device), n_dev=cnt).cpu().numpy()
        np.testing.assert_array_equal(got, np.isin(probes, exp).astype(np.uint8), err_msg=f"contains lww={lww}")
    assert e.device_status() == 0


def fam_map_read(e, n, seed=32, n_dev=None):
    t = _state(seed, n)
    Td, nd = _dev(e, t), None if n_dev is None else _n_dev(e, n_dev)
    seen = t if n_dev is None else _cut(t, n_dev)
    for lww in MODES:
        exp = ref_map_read(*seen, lww)
        t_map._read(e, Td, lww, exp, f"map_read lww={lww}", n_dev=nd)
        t_map._lookup(e, Td, lww, exp, t_map._probes(seen, np.random.default_rng(7)), f"map_lookup lww={lww}", n_dev=nd)
    assert e.device_status() == 0


def fam_set_delta(e, n, seed=33, sides=None, n_dev=None):
    ns, nd_ = sides if sides else (n - n // 3, n // 3)
    src, dst = _side(seed, 1, ns), _side(seed, 0, nd_)
    if n_dev is None:
        t_delta._check(e, src, dst)
    else:
        t_delta._check(e, _cut(src, n_dev[0]), _cut(dst, n_dev[1]), S=_dev(e, src), Dd=_dev(e, dst),
                       ns_dev=_n_dev(e, n_dev[0]), nd_dev=_n_dev(e, n_dev[1]))


def fam_set_compact(e, n, seed=34, n_dev=None):
    t = _state(seed, n)
    seen = t if n_dev is None else _cut(t, n_dev)
    res = t_compact._check(e, seen, t_compact.CUT, Td=_dev(e, t), n_dev=None if n_dev is None else _n_dev(e, n_dev),
                           src_ref=False)                 # (src_ref would compare with a GPU merge_src)
    for lww in MODES:
        m = _merge(lww)(seen, t_compact._empty())
        esrc = t_src.ref_src(seen, t_src.EMPTY, lww)[t_compact._keep(m, t_compact.CUT)]
        np.testing.assert_array_equal(res[lww][1], esrc, err_msg=f"compact src lww={lww}")


def fam_set_digest(e, n, seed=35, n_dev=None):
    t = _state(seed, n)
    seen = t if n_dev is None else _cut(t, n_dev)
    t_dig._check(e, seen, t_dig._splitters(seen, 63), Td=_dev(e, t), n_dev=None if n_dev is None else _n_dev(e, n_dev))


def fam_set_select(e, n, seed=36, n_dev=None):
    t = _state(seed, n)
    seen = t if n_dev is None else _cut(t, n_dev)
    sp, flags = t_dig._splitters(seen, 63), (np.arange(64) % 3 != 1).astype(np.uint8)
    Td, Sd = _dev(e, t), t_dig._sp_dev(e, sp)
    Fd, nd = torch.from_numpy(flags).to(e.device), None if n_dev is None else _n_dev(e, n_dev)
    for lww in MODES:
        m = t_dig.canon(seen, lww)
        keep = flags[t_dig.buckets(sp, m[0])] != 0
        exp, esrc = tuple(x[keep] for x in m), t_src.ref_src(seen, t_src.EMPTY, lww)[keep]
        out, src, cnt = e.set_select(Td, lww, Sd, Fd, n_dev=nd, with_src=True)
        only = e.set_select_count(Td, lww, Sd, Fd, n_dev=nd)
        k = int(as_u64(cnt)[0])
        assert k == len(exp[0]) == int(as_u64(only)[0]), (lww, k, len(exp[0]))
        _same(tuple(x[:k] for x in out.to_numpy()), exp, f"select lww={lww}")
        np.testing.assert_array_equal(src.cpu().numpy()[:k], esrc, err_msg=f"select src lww={lww}")
    assert e.device_status() == 0


def fam_causal_merge(e, n, seed=37, sides=None):
    na, nb = sides if sides else (n - n // 3, n // 3)
    t_causal._check(e, _side(seed, 0, na, 2**40), t_causal._ctx(1), _side(seed, 1, nb, 2**40), t_causal._ctx(2))


def fam_set_apply(e, n, seed=38, n_dev=None):
    m = min(700, n)
    t = t_apply._state(seed, n - m)
    seen = t if n_dev is None else _cut(t, n_dev)
    keys, kinds = au.rand_batch(np.random.default_rng(1000 + n), m, 42)
    for causal in t_apply.FORMS:
        t_apply._run(e, seen, t_apply.CLOCK4, 2, keys, kinds, causal, Ts=_dev(e, t),
                     n_dev=None if n_dev is None else _n_dev(e, n_dev), msg=f"apply causal={causal}")


@functools.lru_cache(maxsize=16)
def _unsorted(seed, n, words):
    rng = np.random.default_rng(seed)
    if words == 1:                                           # (the field ranges of tests/test_gpu_sort.py)
        return synth.set_tuples(seed, 1, n, max(1, n // 2))
    kb, tb, rb = (40, 30, 10) if words == 2 else (64, 64, 32)
    u64 = lambda bits: rng.integers(0, 2**bits - 1, n, dtype=np.uint64, endpoint=True)
    key, ts = u64(kb), u64(tb)
    if n > 200:
        key[:100] = key[100:200]                             # key ties
    return key, ts, rng.integers(0, 2**rb, n, dtype=np.uint64).astype(np.uint32), rng.integers(0, 2, n, dtype=np.uint8)


def fam_sort(e, n, seed=39):
    for words in (1, 2, 3):
        if n:
            t_sort._check(e, _unsorted(seed, n, words))


def fam_merge_unsorted(e, n, seed=40, sides=None):
    na, nb = sides if sides else (n, max(n - 1000, 0) if n > 1000 else n // 2)
    ua, ub = synth.set_tuples(seed, 0, na, 3000), synth.set_tuples(seed, 1, nb, 3000)
    A, B = _dev(e, ua), _dev(e, ub)
    for lww in MODES:
        out, cnt = (e.lww_merge_unsorted if lww else e.orset_merge_unsorted)(A, B, trim=False)
        t_d2._same(out, cnt, t_d2._expect(lww, ua, ub))
    assert e.device_status() == 0


def fam_refmerge(e, n, seed=11, kv=False):
    """n: the merge items of one replica (L and R of n // 2 entries each)."""
    if n < 2:                                                # empty replicas / one entry, through the packer
        reps = [({}, {}), ({}, {})] if n == 0 else [({7: {"a": "1"}}, {}), ({}, {9: {"b": "x"}})]
        for (diff, remote), (d_gpu, s_gpu) in zip(reps, refmerge.merge_batch(e, reps)):
            d_or, s_or = oracle_merge(diff, remote)
            assert list(d_gpu) == list(d_or) and s_gpu == s_or
        assert e.device_status() == 0
        return
    h = _packed(seed, 3, n // 2)
    if kv:
        out, plain, kvo = t_ref._run_kv(e, h)
        assert_batch_matches_oracle(h, out)
        assert_batch_matches_oracle(h, plain)
        t_ref._assert_kv_output(h, out, plain, kvo)
    else:
        assert_batch_matches_oracle(h, e.refmerge_batch(refmerge.to_device(h, e.device)))
    assert e.device_status() == 0


@functools.lru_cache(maxsize=8)
def _packed(seed, replicas, entries):
    return synth.refmerge_packed(seed, replicas, entries)


FAMILIES = {     # id -> (fam, the tile its sizes are counted in)
    "lww_orset_merge": (fam_merge, LT), "merge_src": (fam_merge_src, LT), "set_read": (fam_set_read, T),
    "map_read": (fam_map_read, T), "set_delta": (fam_set_delta, T), "set_compact": (fam_set_compact, T),
    "set_digest": (fam_set_digest, T), "set_select": (fam_set_select, T), "causal_merge": (fam_causal_merge, T),
    "set_apply": (fam_set_apply, T), "sort_tuples": (fam_sort, 4096), "merge_unsorted": (fam_merge_unsorted, 4096),
    "refmerge_batch": (fam_refmerge, LT),
}


# ---------------------------------------------------------------- the rows that are not one family call
def row_digest_diff(e):
    rng = np.random.default_rng(3)
    n = 1000
    h, c = rng.integers(0, 2**63, n).astype(np.uint64), rng.integers(0, 100, n).astype(np.uint64)
    h2, c2 = h.copy(), c.copy()
    at = rng.choice(n, 37, replace=False)
    h2[at[:20]] += np.uint64(1)
    c2[at[20:]] += np.uint64(1)
    d = lambda x, y: (u64_tensor(x, e.device), u64_tensor(y, e.device))
    f, nd = e.digest_diff(d(h, c), d(h2, c2))
    np.testing.assert_array_equal(f.cpu().numpy(), ((h != h2) | (c != c2)).astype(np.uint8))
    assert int(nd.item()) == 37 and e.device_status() == 0


def row_causal_ranges(e):
    a, b = _side(41, 0, NA, 2**40), _side(41, 1, NB, 2**40)
    seen = _cut(b, N_DEV)
    sp = t_cr._quantiles(np.sort(np.concatenate([a[0], seen[0]])), 7)
    flags = (np.arange(8) % 2 == 0).astype(np.uint8)
    t_cr._check(e, a, t_cr._ctx(1), seen, t_cr._ctx(2), sp, flags, B=_dev(e, b), nb_dev=_n_dev(e, N_DEV))


def row_planned(e):
    ua, ub = synth.set_tuples(43, 0, N_SORT, 3000), synth.set_tuples(43, 1, N_SORT - 1000, 3000)
    A, B = _dev(e, ua), _dev(e, ub)
    for lww in MODES:
        plan = e.set_merge_plan(lww, A, B, widen=True)       # ... and every call below starts from a fill
        out = TupleSet.empty(len(A) + len(B), e.device)
        cnt = torch.zeros(1, dtype=torch.int64, device=e.device)
        e.merge_unsorted_planned(lww, plan, A, B, out, cnt)
        t_d2._same(out, cnt, t_d2._expect(lww, ua, ub))
    assert e.device_status() == 0


def row_fold(e):
    for rows, nodes in ((300, 64), (300, 63)):
        t_cnt.test_fold_matches_oracle(e, rows, nodes)
    assert e.device_status() == 0


def row_stable_cut(e):
    for rows, nodes in ((300, 64), (300, 63)):
        a = synth.counters(9, 4, rows * nodes).reshape(rows, nodes)
        np.testing.assert_array_equal(as_u64(e.vclock_stable_cut(u64_tensor(a, e.device))), a.min(axis=0))
    assert e.device_status() == 0


def row_counter_values(e):
    for rows, nodes in ((300, 64), (33, 7)):
        t_cnt.test_pncounter_value_and_join(e, rows, nodes)
    assert e.device_status() == 0


def row_refmerge_pull(e):
    """Every replica's R is a peer's L read in place, its key slots re-based:
    the oracle merges replica p's L with replica q's L as R."""
    d, kv, pull, q = t_ref._pull_batch(e, seed=19, P=12)
    h = synth.refmerge_packed(19, 12, 2000)
    out = e.refmerge_batch(d, kv=kv, pull=pull)
    assert e.device_status() == 0
    off = out["off"].cpu().numpy()
    l_off, l_kv, kk = h["l_off"], h["l_kv"], h["kv_key"].view(np.uint32).astype(np.int64)
    for p in range(12):
        lb, le, rb, re_ = int(l_off[p]), int(l_off[p + 1]), int(l_off[q[p]]), int(l_off[q[p] + 1])
        key = kk - p * 62
        key[int(l_kv[rb]):int(l_kv[re_])] = kk[int(l_kv[rb]):int(l_kv[re_])] - int(q[p]) * 62
        o_ts, o_or, o_src, kind, sstr, ssum = oracle.refmerge_packed(
            h["l_ts"][lb:le], h["l_origin"][lb:le], l_kv[lb:le + 1].astype(np.uint32), h["l_ts"][rb:re_],
            l_kv[rb:re_ + 1].astype(np.uint32), key.astype(np.uint32), h["kv_val"].view(np.uint32), h["str_bytes"],
            h["str_off"], 62)
        x, y = int(off[p]), int(off[p + 1])
        np.testing.assert_array_equal(out["ts"][x:y].cpu().numpy(), o_ts)
        np.testing.assert_array_equal(out["origin"][x:y].cpu().numpy(), o_or)
        np.testing.assert_array_equal(out["src"][x:y].cpu().numpy(), np.where(o_src >= 0, o_src + lb, o_src - rb))
        sl = slice(p * 62, (p + 1) * 62)
        np.testing.assert_array_equal(out["st_kind"][sl].cpu().numpy(), kind)
        np.testing.assert_array_equal(out["st_str"][sl].cpu().numpy().view(np.uint32)[kind == 1], sstr[kind == 1])
        np.testing.assert_array_equal(out["st_sum"][sl].cpu().numpy()[kind == 2], ssum[kind == 2])


def row_refmerge_delta(e):
    h = _packed(14, 3, (3 * LT + 200) // 2)
    d = refmerge.to_device(h, e.device)
    st = e.replay_state_init(d)
    assert_batch_matches_oracle(h, e.refmerge_delta(d, st))
    assert e.device_status() == 0


def _first_replicas(h, P):
    """The first P replicas of a packed batch (the kv arena and the strings stay whole)."""
    nl, nr = int(h["l_off"][P]), int(h["r_off"][P])
    return dict(h, replicas=P, n_slots=P * 62, l_off=h["l_off"][:P + 1], l_ts=h["l_ts"][:nl], l_origin=h["l_origin"][:nl],
                l_kv=h["l_kv"][:nl + 1], r_off=h["r_off"][:P + 1], r_ts=h["r_ts"][:nr], r_kv=h["r_kv"][:nr + 1])


def _row_refmerge_plan(e, replicas):
    h = _packed(23, (1 << 16) + 1, 12)                       # kSmallPlan + 1 replicas, one tile each
    h = h if replicas == h["replicas"] else _first_replicas(h, replicas)
    out = e.refmerge_batch(refmerge.to_device(h, e.device))
    assert_batch_matches_oracle(h, out, replicas=list(range(0, replicas, 997)) + [replicas - 1])
    off = out["off"].cpu().numpy()
    assert off[0] == 0 and np.all(np.diff(off) >= np.diff(h["l_off"]))
    assert e.device_status() == 0


def row_seg_ops(e):
    t_seg.test_counts_to_offsets(e, N_SET)
    t_seg.test_seg_offsets_and_gather2(e, N_SET, 2)
    t_seg.test_seg_copy2_delta(e, 0, 700, 40)
    t_seg.test_seg_copy2_delta(e, 1, 700, 40)
    assert e.device_status() == 0


def row_gossip_decode(e):
    e.fill_now()                                             # (codec.decode calls the library on the context itself)
    t_codec.test_decode_matches_host_ingest(e)
    assert e.device_status() == 0


def row_population(e):
    e.fill_now()                                             # (so do the population's rounds)
    for draw in ("random", "reference"):
        t_pop.test_population_rounds_match_reference_simulation(e, 1, draw)
    assert e.device_status() == 0


class _Members:
    """shard.Comm.loopback(0, 3): sync (which fills every member's scratch)
    and a reserve on every member's context in front of each protocol call."""

    def __init__(self, e):
        self.e, self.comm = e, shard.Comm.loopback(0, 3)

    def fill_now(self):
        torch.cuda.synchronize()
        before = _filled_mb()
        self.comm.sync()
        for i in range(self.comm.members):
            ctx = C.c_void_p()
            self.comm._call("crdt_shard_member_ctx", i, C.byref(ctx))
            _lib.call("crdt_ctx_reserve", ctx, RESERVE, ctx=ctx)
        if self.e._fill >= 0:
            assert _filled_mb() - before >= self.comm.members * (RESERVE >> 20), "the member contexts were not filled"


def row_shard_set_merge_local(e):
    m = _Members(e)
    try:
        sets = [rank_sets(11, r, na, nb, 4000) for r, (na, nb) in enumerate(t_loop._local_sizes(3, "empty_sides"))]
        A = [TupleSet.from_numpy(*s[0], "cuda:0") for s in sets]
        B = [TupleSet.from_numpy(*s[1], "cuda:0") for s in sets]
        pa, pb = stable_rank_merge([s[0] for s in sets]), stable_rank_merge([s[1] for s in sets])
        for lww in MODES:
            exp = _merge(lww)(pa, pb)
            m.fill_now()
            for g in m.comm.set_merge_local(A, B, lww=lww, gather=True):
                _same(g.to_numpy(), exp, f"gather lww={lww}")
            m.fill_now()
            mine = m.comm.set_merge_local(A, B, lww=lww, gather=False)
            _same([np.concatenate([x.to_numpy()[f] for x in mine]) for f in range(4)], exp, f"ranges lww={lww}")
            m.fill_now()
            outs, counts = m.comm.set_merge_local_dev(A, B, lww=lww)
            m.comm.sync()
            dev = [o.slice(int(c.item())).to_numpy() for o, c in zip(outs, counts)]
            _same([np.concatenate([d[f] for d in dev]) for f in range(4)], exp, f"device counts lww={lww}")
    finally:
        m.comm.close()


def row_shard_refmerge(e):
    m = _Members(e)
    try:
        m.fill_now()
        t_loop.test_refmerge_ts_range_shards(m.comm, e._eng)
    finally:
        m.comm.close()


def _both(fam, **kw):
    """The row's shape, then one side empty and the other a single tuple."""
    def run(e):
        fam(e, NA + NB, sides=(NA, NB), **kw)
    return run


def _one(fam, **kw):
    def run(e):
        fam(e, 1, sides=(0, 1), **kw)
        fam(e, 1, sides=(1, 0), **kw)
    return run


def _host_then_one(fam):
    def run(e):
        fam(e, N_SET)
        fam(e, 1)
    return run


def _seq(*runs):
    def run(e):
        for r in runs:
            r(e)
    return run


RUN = {
    "lww_orset_merge": _both(fam_merge), "lww_orset_merge_one": _one(fam_merge),
    "merge_src": _both(fam_merge_src), "merge_src_one": _one(fam_merge_src),
    "map_merge": _both(fam_merge_src, vals=True),
    "tuples_merge": _seq(_both(fam_tuples_merge), lambda e: fam_tuples_merge(e, 1, sides=(0, 1))),
    "set_read": _host_then_one(fam_set_read), "set_read_ndev": lambda e: fam_set_read(e, N_SET, n_dev=N_DEV),
    "map_read": _host_then_one(fam_map_read), "map_read_ndev": lambda e: fam_map_read(e, N_SET, n_dev=N_DEV),
    "set_delta": _seq(_both(fam_set_delta), _one(fam_set_delta)),
    "set_delta_ndev": lambda e: fam_set_delta(e, 0, sides=(NA, NB), n_dev=(N_DEV, N_DEV - 100)),
    "set_compact": _host_then_one(fam_set_compact), "set_compact_ndev": lambda e: fam_set_compact(e, N_SET, n_dev=N_DEV),
    "set_digest": _seq(_host_then_one(fam_set_digest), lambda e: fam_set_digest(e, N_SET, n_dev=N_DEV)),
    "digest_diff": row_digest_diff,
    "set_select": _seq(_host_then_one(fam_set_select), lambda e: fam_set_select(e, N_SET, n_dev=N_DEV)),
    "reconcile_round_lww": lambda e: t_dig.test_reconcile_round(e, True),
    "reconcile_round_orset": lambda e: t_dig.test_reconcile_round(e, False),
    "causal_merge": _seq(_both(fam_causal_merge), lambda e: fam_causal_merge(e, 1, sides=(0, 1))),
    "causal_merge_ranges": row_causal_ranges,
    "set_apply": _seq(lambda e: fam_set_apply(e, N_SET), lambda e: fam_set_apply(e, N_SET, n_dev=N_DEV)),
    "sort_tuples": lambda e: fam_sort(e, N_SORT),
    "merge_unsorted": _seq(lambda e: fam_merge_unsorted(e, N_SORT), lambda e: fam_merge_unsorted(e, 1, sides=(0, 1))),
    "merge_unsorted_planned": row_planned,
    "gcounter_fold": row_fold, "vclock_stable_cut": row_stable_cut, "counter_values": row_counter_values,
    "refmerge_batch": lambda e: fam_refmerge(e, 3 * LT + 200),
    "refmerge_batch_kv": lambda e: fam_refmerge(e, 3 * LT + 200, kv=True),
    "refmerge_pull": row_refmerge_pull, "refmerge_delta": row_refmerge_delta,
    "refmerge_small_plan": lambda e: _row_refmerge_plan(e, 1 << 16),
    "refmerge_large_plan": lambda e: _row_refmerge_plan(e, (1 << 16) + 1),
    "refmerge_lds_overflow": t_ref.test_many_keys_per_replica_matches_oracle,
    "seg_ops": row_seg_ops,
    "local_apply": lambda e: t_local.test_local_apply_matches_restatement(e, 1),
    "gossip_decode": row_gossip_decode,
    "population_round": row_population,
    "shard_set_merge_local": row_shard_set_merge_local, "shard_refmerge": row_shard_refmerge,
}
assert list(RUN) == [r[0] for r in ROWS], "tests/ws_fill_table.py and RUN name the same rows, in one order"


@pytest.mark.diag
@pytest.mark.parametrize("row", list(RUN))
@pytest.mark.parametrize("fill", FILLS, ids=lambda f: "off" if f < 0 else f"0x{f:02X}")   # (the outer loop: 0x00 first)
def test_op_under_fill(filling, fill, row):
    RUN[row](filling)
    assert filling.fills > 0 or row.startswith("shard_")
    assert filling.device_status() == 0


# ---------------------------------------------------------------- 3. stale but plausible scratch
@pytest.mark.parametrize("first,other", SEQUENCES, ids=[f"{a}-{b}" for a, b in SEQUENCES])
def test_shrink_and_swap(eng, first, other):
    """One engine, no reserve in between: what each call finds in its carve is
    what the call before it left there."""
    fam, tile = FAMILIES[first]
    fam2, tile2 = FAMILIES[other]
    fam(eng, 5 * tile, seed=51)
    fam(eng, 2 * tile + 9, seed=52)
    fam(eng, 0, seed=53)
    fam(eng, 1, seed=54)
    fam2(eng, 2 * tile2 + 9, seed=55)
    fam(eng, 5 * tile, seed=56)
    assert eng.device_status() == 0
