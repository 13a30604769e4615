"""CPU: the two restatements of the keyed PN-Counter map in tests/cmap_util.py
(dict-based, the definition; vectorised numpy) agree on seeded inputs, and the
definition satisfies the laws the type promises: the merge is a join, applies
on different replicas converge under it, the value is the plain sum of every
increment minus every decrement, and the delta is the smallest state that
brings dst up to merge(dst, src)."""
import numpy as np
import pytest

import cmap_util as cu

SEEDS = [1, 2, 3]


def _states(seed, sizes=(300, 260, 190), key_space=90):
    rng = np.random.default_rng(seed)
    out = [cu.random_state(rng, n, key_space) for n in sizes]
    # extremes: values near 2^64, so that sums wrap and a signed max would differ
    for t in out:
        t[2][::7] = np.uint64(2**64 - 1) - rng.integers(0, 5, size=len(t[2][::7]), dtype=np.uint64)
        t[3][::11] = np.uint64(2**63) + rng.integers(0, 5, size=len(t[3][::11]), dtype=np.uint64)
    return out


def _batch(rng, m, key_space):
    keys = np.sort(rng.choice(key_space, size=m, replace=False)).astype(np.uint64)
    dp = rng.integers(0, 1 << 40, size=m, dtype=np.uint64)
    dn = rng.integers(0, 1 << 40, size=m, dtype=np.uint64)
    return keys, dp, dn


@pytest.mark.parametrize("seed", SEEDS)
def test_restatements_agree(seed):
    a, b, c = _states(seed)
    rng = np.random.default_rng(100 + seed)
    assert cu.is_state(a) and cu.is_state(b) and cu.is_state(c)
    shared = set(cu.to_dict(a)) & set(cu.to_dict(b))
    assert len(shared) > 20                               # the merge meets equal cells
    for x, y in ((a, b), (b, a), (a, cu.state()), (cu.state(), b), (cu.state(), cu.state()), (a, a)):
        assert cu.same(cu.merge_d(x, y), cu.merge_np(x, y))
        assert cu.same(cu.delta_d(x, y), cu.delta_np(x, y))
    for t in (a, cu.state()):
        for m in (0, 1, 40):
            keys, dp, dn = _batch(rng, m, 120)
            dp[::3] = np.uint64(2**64 - 1)                # p + dp wraps
            got = cu.apply_np(t, 3, keys, dp, dn)
            assert cu.same(cu.apply_d(t, 3, keys, dp, dn), got) and cu.is_state(got)
    for t in (a, c, cu.state()):
        assert cu.same(cu.values_d(t), cu.values_np(t))
        probes = rng.integers(0, 130, size=200).astype(np.uint64)
        assert cu.same(cu.lookup_d(t, probes), cu.lookup_np(t, probes))
    keys, P, N, value = cu.values_d(a)
    assert (value < 0).any() and (value > 0).any()


@pytest.mark.parametrize("seed", SEEDS)
def test_merge_is_a_join(seed):
    a, b, c = _states(seed)
    assert cu.same(cu.merge_d(a, b), cu.merge_d(b, a))
    assert cu.same(cu.merge_d(cu.merge_d(a, b), c), cu.merge_d(a, cu.merge_d(b, c)))
    assert cu.same(cu.merge_d(a, a), a)
    assert cu.same(cu.merge_d(cu.merge_d(a, b), b), cu.merge_d(a, b))
    assert cu.is_state(cu.merge_d(a, b))


@pytest.mark.parametrize("seed", SEEDS)
def test_applies_converge_and_sum(seed):
    rng = np.random.default_rng(200 + seed)
    base = cu.state()
    total = {}
    x = y = base
    for rep, who in ((1, "x"), (2, "y"), (1, "x"), (2, "y")):
        keys, dp, dn = _batch(rng, 30, 50)
        for k, p, n in zip(keys, dp, dn):
            total[int(k)] = total.get(int(k), 0) + int(p) - int(n)
        if who == "x":
            x = cu.apply_d(x, rep, keys, dp, dn)
        else:
            y = cu.apply_d(y, rep, keys, dp, dn)
    xy, yx = cu.merge_d(x, y), cu.merge_d(y, x)
    assert cu.same(xy, yx)
    keys, _, _, value = cu.values_d(xy)
    assert [int(k) for k in keys] == sorted(total)
    assert [int(v) for v in value] == [total[k] for k in sorted(total)]


@pytest.mark.parametrize("seed", SEEDS)
def test_delta_is_the_smallest_catch_up(seed):
    src, dst, _ = _states(seed)
    d = cu.delta_d(src, dst)
    want = cu.merge_d(dst, src)
    assert len(d[0]) > 0 and len(d[0]) < len(src[0])     # some cells ship, some do not
    assert cu.same(cu.merge_d(dst, d), want)
    for i in range(len(d[0])):                           # every cell of the delta is needed
        less = tuple(np.delete(c, i) for c in d)
        assert not cu.same(cu.merge_d(dst, less), want), i
    assert len(cu.delta_d(src, src)[0]) == 0
    assert len(cu.delta_d(src, want)[0]) == 0
