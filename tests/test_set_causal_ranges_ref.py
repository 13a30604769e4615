"""CPU: the numpy restatement of the range-restricted causal merge
(tests/causal_ranges_util.py), the reference tests/test_gpu_set_causal_ranges.py
holds the GPU to, checked over seeded replica histories: a digest round --
flag the buckets whose canonical tuples differ, select them on either side,
merge each whole state with the other side's selection -- gives both replicas
causal_merge(A, B) and its context.  And the suite discriminates: the plain
causal merge of a whole state with a selection does not."""
import numpy as np
import pytest

from causal_ranges_util import canon, ideal_flags, np_select, ref_causal_ranges
from causal_util import FIELDS, History, cat, ctx_max, empty, present, ref_causal, tup

SEED_SETS = [tuple(range(s, s + 6)) for s in (100, 200, 300, 400)]       # 24 seeds
STEPS = 250


def _eq(got, exp, msg):
    for g, e, f in zip(got, exp, FIELDS):
        np.testing.assert_array_equal(g, e, err_msg=f"{msg} {f}")


def _splitters(rng, a, b):
    """m = 0, or up to 9 ascending values around the history's keys (0 .. 11):
    equal neighbours and splitters equal to keys come up all the time; one in
    four draws takes every splitter from the keys held."""
    m = int(rng.integers(0, 10))
    if m == 0:
        return np.zeros(0, np.uint64)
    held = np.concatenate([a[0], b[0]])
    if len(held) and rng.random() < 0.25:
        return np.sort(rng.choice(held, m)).astype(np.uint64)
    return np.sort(rng.integers(0, 14, m)).astype(np.uint64)


@pytest.mark.parametrize("seeds", SEED_SETS)
def test_round_is_the_causal_merge(seeds):
    merges = partial = naive_wrong = with_m0 = with_equal = with_key = 0
    for seed in seeds:
        h = History(seed)
        rng = np.random.default_rng(seed + 7)
        for _ in range(STEPS):
            op, x, y = h.step()
            if op != "merge":
                continue
            merges += 1
            A, ca, B, cb = h.dots[x], h.clock[x], h.dots[y], h.clock[y]
            sp = _splitters(rng, A, B)
            with_m0 += len(sp) == 0
            with_equal += bool(len(sp) > 1 and (sp[1:] == sp[:-1]).any())
            with_key += bool(np.isin(sp, np.concatenate([A[0], B[0]])).any())
            flags = ideal_flags(A, B, sp)
            assert len(flags) == len(sp) + 1
            sel_a, _ = np_select(A, sp, flags)
            sel_b, _ = np_select(B, sp, flags)
            right, _, ctx, _ = ref_causal(A, ca, B, cb)
            ma, _, ctx_ma = ref_causal_ranges(A, ca, sel_b, cb, sp, flags)
            mb, _, ctx_mb = ref_causal_ranges(B, cb, sel_a, ca, sp, flags)
            _eq(ma, right, f"seed {seed}: A with sel(B)")
            _eq(mb, right, f"seed {seed}: B with sel(A)")
            np.testing.assert_array_equal(ctx_ma, ctx)
            np.testing.assert_array_equal(ctx_mb, ctx)
            if 0 < int(flags.sum()) < len(flags):
                partial += 1
                naive = ref_causal(A, ca, sel_b, cb)[0]
                if len(naive[0]) != len(right[0]) or any(not np.array_equal(g, e) for g, e in zip(naive, right)):
                    naive_wrong += 1
            h.dots[x], h.clock[x] = ma, ctx_ma
    assert merges > 50 * len(seeds)
    assert partial >= 1 and naive_wrong >= 1, (merges, partial, naive_wrong)
    assert with_m0 >= 1 and with_equal >= 1 and with_key >= 1


def test_identities():
    """Every flag set: ref_causal, source indices included; no flag set: a's
    present tags, whatever b and the contexts hold."""
    h = History(5)
    for _ in range(200):
        op, x, y = h.step()
        if op == "merge":
            h.tomb[x], h.clock[x] = ref_causal_tomb(h, x, y)
    a, ca, b, cb = h.tomb[0], h.clock[0], h.tomb[1], h.clock[1]
    assert int(a[3].sum()) and int(b[3].sum())
    for sp in (np.zeros(0, np.uint64), np.array([3, 3, 7], np.uint64)):
        ones, zeros = np.ones(len(sp) + 1, np.uint8), np.zeros(len(sp) + 1, np.uint8)
        exp, esrc, ectx, _ = ref_causal(a, ca, b, cb)
        got, src, ctx = ref_causal_ranges(a, ca, b, cb, sp, ones)
        _eq(got, exp, "all flags")
        np.testing.assert_array_equal(src, esrc)
        np.testing.assert_array_equal(ctx, ectx)
        got, src, ctx = ref_causal_ranges(a, ca, b, cb, sp, zeros)
        _eq(got, present(a), "no flag")
        assert bool((src >= 0).all())
        _eq((a[0][src], a[1][src], a[2][src], a[3][src]), got, "src names a's live first copies")
        np.testing.assert_array_equal(ctx, ectx)


def ref_causal_tomb(h, x, y):
    """The tombstone-form merge of replicas x and y in numpy: the union of the
    tags, tombs OR-ed (canon of the concatenation), and the joined clock."""
    return canon(cat(h.tomb[x], h.tomb[y]))[0], ctx_max(h.clock[x], h.clock[y])


def test_rule_by_hand():
    """Buckets (-inf, 5), [5, 8), [8, inf) with only the middle one flagged.
    Key 5 equals a splitter and belongs to the upper (flagged) bucket."""
    sp, flags = np.array([5, 8], np.uint64), np.array([0, 1, 0], np.uint8)
    a = tup([1, 2, 2, 5, 6, 9], [1, 2, 2, 3, 4, 5], [0, 1, 1, 0, 0, 0], [0, 0, 1, 0, 0, 0])
    b = tup([2, 3, 5, 7, 9, 9], [2, 9, 3, 8, 5, 5], [1, 1, 0, 1, 0, 0], [0, 0, 1, 0, 1, 1])
    ca, cb = np.array([9, 0], np.uint64), np.array([9, 9], np.uint64)
    # key 1: a only, covered by cb, unflagged -> kept (the plain merge drops it)
    # key 2: tombstoned on a, live on b, unflagged -> absent (no revival; the plain merge keeps it: not covered by ca)
    # key 3: b only, unflagged -> ignored (the plain merge keeps it: rep 1 is not covered by ca)
    # key 5: flagged; present in a, tombstoned on b and covered by cb -> dropped
    # key 6: flagged; a only, covered by cb -> dropped
    # key 7: flagged; b only, not covered by ca -> kept, from b
    # key 9: unflagged; present in a, tombstoned on b -> kept, from a
    out, src, ctx = ref_causal_ranges(a, ca, b, cb, sp, flags)
    _eq(out, tup([1, 7, 9], [1, 8, 5], [0, 1, 0], [0, 0, 0]), "rule")
    np.testing.assert_array_equal(src, [0, -4, 5])
    np.testing.assert_array_equal(ctx, [9, 9])
    plain = ref_causal(a, ca, b, cb)[0]
    np.testing.assert_array_equal(plain[0], [2, 3, 7])
    np.testing.assert_array_equal(ideal_flags(a, b, sp), [1, 1, 1])
    np.testing.assert_array_equal(ideal_flags(a, a, sp), [0, 0, 0])
    sel, ssrc = np_select(a, sp, flags)
    _eq(sel, tup([5, 6], [3, 4], [0, 0], [0, 0]), "select")
    np.testing.assert_array_equal(ssrc, [3, 4])
    out, src, _ = ref_causal_ranges(empty(), None, b, cb, None, np.array([0], np.uint8))
    assert len(out[0]) == 0 and len(src) == 0
