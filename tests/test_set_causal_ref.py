"""CPU: the numpy restatement of the causal OR-Set merge (tests/causal_util.py),
the reference tests/test_gpu_set_causal.py holds the GPU to, checked against the
oracle's tombstone-form OR-Set merge over seeded replica histories and for the
algebra the header promises: commutative, associative, idempotent."""
import numpy as np
import pytest

from causal_util import FIELDS, History, cat, ctx_max, empty, live_keys, present, ref_causal, tup
from oracle import oracle


def _eq(got, exp, msg):
    for g, e, f in zip(got, exp, FIELDS):
        np.testing.assert_array_equal(g, e, err_msg=f"{msg} {f}")


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_history_in_both_forms(seed):
    """The causal state's dots are the live tags of the tombstone-form state at
    every replica after every step, and every dot stays covered by its own
    replica's context."""
    h = History(seed)
    merges = 0
    for _ in range(300):
        op, x, y = h.step()
        if op == "merge":
            merges += 1
            # what a merge of the tombstone-form replicas keeps alive, before either form of x is set
            both, _, _, _ = ref_causal(h.tomb[x], h.clock[x], h.tomb[y], h.clock[y])
            merged = oracle.orset_merge(h.tomb[x], h.tomb[y])
            _eq(both, present(merged), "tombstone-form operands")
            dots, _, ctx, _ = ref_causal(h.dots[x], h.clock[x], h.dots[y], h.clock[y])
            back, _, ctx2, _ = ref_causal(h.dots[y], h.clock[y], h.dots[x], h.clock[x])
            _eq(dots, back, "commutative")
            np.testing.assert_array_equal(ctx, ctx2)
            h.tomb[x], h.dots[x], h.clock[x] = merged, dots, ctx
        for r in range(h.n):
            _eq(h.dots[r], present(h.tomb[r]), f"replica {r} after {op}")
            d = h.dots[r]
            assert bool((d[1] <= h.clock[r][d[2].astype(np.int64)]).all())
    assert merges > 50 and any(len(d[0]) for d in h.dots)
    assert any(int(t[3].sum()) for t in h.tomb)


def test_algebra():
    h = History(7, keys=6)
    for _ in range(200):
        op, x, y = h.step()
        if op == "merge":
            dots, _, ctx, _ = ref_causal(h.dots[x], h.clock[x], h.dots[y], h.clock[y])
            h.tomb[x], h.dots[x], h.clock[x] = oracle.orset_merge(h.tomb[x], h.tomb[y]), dots, ctx
    s = [(h.dots[r], h.clock[r]) for r in range(3)]
    m = lambda p, q: ref_causal(p[0], p[1], q[0], q[1])[::2]
    left, right = m(m(s[0], s[1]), s[2]), m(s[0], m(s[1], s[2]))
    _eq(left[0], right[0], "associative")
    np.testing.assert_array_equal(left[1], right[1])
    for p in s:
        _eq(m(p, p)[0], p[0], "idempotent")
    assert len(left[0][0]) > 0


def test_rule_by_hand():
    a = tup([1, 2, 3, 4, 4], [5, 5, 5, 5, 5], [0, 0, 0, 1, 1], [0, 0, 0, 0, 1])
    b = tup([1, 3, 4, 9], [5, 5, 5, 2], [0, 0, 1, 2], [0, 1, 0, 0])
    # key 1: both; key 2: a only, b's context covers it; key 3: a present, b tombstoned and covered;
    # key 4: a tombstoned, b present, a's context does not cover rep 1; key 9: b only, rep past a's context
    out, src, ctx, kinds = ref_causal(a, np.array([9], np.uint64), b, np.array([5, 0, 0], np.uint64))
    _eq(out, tup([1, 4, 9], [5, 5, 2], [0, 1, 2], [0, 0, 0]), "rule")
    np.testing.assert_array_equal(src, [0, -3, -4])
    np.testing.assert_array_equal(ctx, [9, 0, 0])
    assert kinds == {"both": 1, "a_kept": 0, "a_dropped": 2, "b_kept": 2, "b_dropped": 0, "absent": 0}
    np.testing.assert_array_equal(ctx_max(None, None), np.zeros(0, np.uint64))
    np.testing.assert_array_equal(live_keys(cat(a, b)), [1, 2, 9])
    assert len(ref_causal(empty(), None, empty(), None)[0][0]) == 0
