"""CPU: the two restatements of combine / add / from_ops in
tests/cmap_ingest_util.py agree, give typed-out known answers, and obey the
laws that make an unsorted log a valid way to build counter-map state."""
import numpy as np
import pytest

import cmap_ingest_util as iu
import cmap_util as cu

U64, U32 = np.uint64, np.uint32
M64 = 2**64 - 1


def eq(x, y):
    return cu.same(x, y)


# ---------------------------------------------------------------- known answers
def test_known_answers_typed_out():
    ops = iu.log([5, 3, 5, 3, 5, 9], [1, 0, 1, 2, 0, 1], [1, 2, 10, 4, 7, 0], [0, 1, 2, 0, 0, 0])
    exp = cu.state([3, 3, 5, 5, 9], [0, 2, 0, 1, 1], [2, 4, 7, 11, 0], [1, 0, 0, 2, 0])
    assert eq(iu.from_ops_d(ops), exp) and eq(iu.from_ops_np(ops), exp)      # (9, 1): zero sums keep the cell
    srt = iu.sorted_log(ops)
    assert iu.is_sorted(srt) and not cu.is_state(srt)
    assert eq(iu.combine_d(srt), exp) and eq(iu.combine_np(srt), exp)
    t = cu.state([3, 5, 7], [0, 1, 0], [1, 1, 1], [5, 5, 5])
    d = cu.state([3, 5, 8], [0, 0, 2], [2, 3, 0], [1, 0, 0])
    exp = cu.state([3, 5, 5, 7, 8], [0, 0, 1, 0, 2], [3, 3, 1, 1, 0], [6, 0, 5, 5, 0])
    assert eq(iu.add_d(t, d), exp) and eq(iu.add_np(t, d), exp)


def test_sums_wrap():
    ops = iu.log([4, 4], [1, 1], [M64, 2], [2**63, 2**63])                    # (2^64 - 1) + 2 = 1
    exp = cu.state([4], [1], [1], [0])
    assert eq(iu.from_ops_d(ops), exp) and eq(iu.from_ops_np(ops), exp)
    assert eq(iu.combine_d(ops), exp) and eq(iu.combine_np(ops), exp)
    t, d = cu.state([4], [1], [M64], [1]), cu.state([4], [1], [2], [M64])
    assert eq(iu.add_d(t, d), cu.state([4], [1], [1], [0])) and eq(iu.add_np(t, d), cu.state([4], [1], [1], [0]))


def test_orders_are_unsigned():
    big = 2**63
    ops = iu.log([big + 1, 1, 1, big + 1], [0, 2**31 + 5, 3, 0], [1, 2, 3, 4], [0, 0, 0, 0])
    exp = cu.state([1, 1, big + 1], [3, 2**31 + 5, 0], [3, 2, 5], [0, 0, 0])
    assert eq(iu.from_ops_d(ops), exp) and eq(iu.from_ops_np(ops), exp)


def test_indexed_combine():
    keys = iu.log([2, 2, 6], [0, 0, 1], [0, 0, 0], [0, 0, 0])
    src = (np.array([10, 20, 30, 40], U64), np.array([1, 2, 3, 4], U64))
    exp = cu.state([2, 6], [0, 1], [50, 20], [5, 2])
    assert eq(iu.combine_d(keys, [3, 0, 1], src), exp) and eq(iu.combine_np(keys, [3, 0, 1], src), exp)
    exp = cu.state([2, 6], [0, 1], [40, 20], [4, 2])                          # index 4 is out of range: contributes 0
    assert eq(iu.combine_d(keys, [3, 4, 1], src), exp) and eq(iu.combine_np(keys, [3, 4, 1], src), exp)


# ---------------------------------------------------------------- the restatements agree
@pytest.mark.parametrize("m,keys,big", [(0, 1, False), (1, 1, False), (300, 10, False), (300, 10, True), (500, 400, True)])
def test_restatements_agree(m, keys, big):
    rng = np.random.default_rng(m + keys)
    ops = iu.random_log(rng, m, keys, big=big)
    st = iu.from_ops_np(ops)
    assert cu.is_state(st) and eq(iu.from_ops_d(ops), st)
    srt = iu.sorted_log(ops)
    assert eq(iu.combine_d(srt), st) and eq(iu.combine_np(srt), st)
    keyed = iu.perm(ops, np.lexsort((ops[1], ops[0])))
    idx = np.lexsort((ops[1], ops[0]))
    assert eq(iu.combine_np(keyed, idx, (ops[2], ops[3])), st) and eq(iu.combine_d(keyed, idx, (ops[2], ops[3])), st)
    other = iu.from_ops_np(iu.random_log(rng, 200, keys, big=big))
    assert eq(iu.add_d(st, other), iu.add_np(st, other))


# ---------------------------------------------------------------- laws
@pytest.fixture(scope="module")
def a_log():
    return iu.random_log(np.random.default_rng(77), 1200, 60, reps=4, big=True)


def test_from_ops_ignores_the_order(a_log):
    rng = np.random.default_rng(1)
    exp = iu.from_ops_np(a_log)
    assert len(exp[0]) < 300                             # heavy repeats
    for _ in range(3):
        assert eq(iu.from_ops_np(iu.perm(a_log, rng.permutation(1200))), exp)
    assert eq(iu.from_ops_np(iu.perm(a_log, np.arange(1199, -1, -1))), exp)


def test_from_ops_of_a_concatenation_is_add(a_log):
    x, y = tuple(c[:500] for c in a_log), tuple(c[500:] for c in a_log)
    assert eq(iu.from_ops_np(iu.cat(x, y)), iu.add_np(iu.from_ops_np(x), iu.from_ops_np(y)))
    assert eq(iu.from_ops_np(a_log), iu.add_np(iu.from_ops_np(a_log), cu.state()))


def test_values_of_from_ops_are_the_plain_sums(a_log):
    total = {}
    for k, _, dp, dn in zip(*a_log):
        p, n = total.get(int(k), (0, 0))
        total[int(k)] = ((p + int(dp)) % 2**64, (n + int(dn)) % 2**64)
    keys, P, N, value = cu.values_np(iu.from_ops_np(a_log))
    assert keys.tolist() == sorted(total)
    assert P.tolist() == [total[k][0] for k in sorted(total)] and N.tolist() == [total[k][1] for k in sorted(total)]
    assert value.tolist() == [cu._as_i64(total[k][0] - total[k][1]) for k in sorted(total)]


def test_add_of_one_replicas_batch_is_apply():
    rng = np.random.default_rng(5)
    t = cu.random_state(rng, 400, 100)
    keys = np.sort(rng.choice(160, size=90, replace=False)).astype(U64)
    dp, dn = rng.integers(0, 2**64 - 1, size=90, dtype=U64), rng.integers(0, 1 << 40, size=90, dtype=U64)
    batch = iu.from_ops_np((keys, np.full(90, 3, U32), dp, dn))
    assert eq(batch, (keys, np.full(90, 3, U32), dp, dn))                 # already a state
    assert eq(iu.add_np(t, batch), cu.apply_np(t, 3, keys, dp, dn))
    assert eq(iu.add_d(t, batch), cu.apply_d(t, 3, keys, dp, dn))


def test_split_by_replica_and_apply_in_any_order(a_log):
    t = cu.random_state(np.random.default_rng(6), 150, 60, reps=4)
    t = (t[0] * U64(7) + U64(3), t[1], t[2], t[3])       # the log's key space, so that cells are shared
    exp = iu.add_np(t, iu.from_ops_np(a_log))
    assert len(exp[0]) < 150 + len(iu.from_ops_np(a_log)[0])
    for order in ((0, 1, 2, 3), (3, 1, 0, 2), (2, 3, 1, 0)):
        s = t
        for r in order:
            part = tuple(c[a_log[1] == r] for c in a_log)
            b = iu.combine_np(iu.sorted_log(part))
            assert cu.is_state(b) and (b[1] == r).all()
            s = cu.apply_np(s, r, b[0], b[2], b[3])
        assert eq(s, exp)


def test_combine_of_a_state_is_the_identity():
    t = cu.random_state(np.random.default_rng(9), 500, 100)
    assert eq(iu.combine_np(t), t) and eq(iu.combine_d(t), t)
    assert eq(iu.combine_np(cu.state()), cu.state())
    assert eq(iu.combine_np(iu.expand(t, 3)), (t[0], t[1], t[2] * U64(3), t[3] * U64(3)))
