"""CPU: the numpy restatement of crdt_set_apply (tests/apply_util.py) checked
against itself: the closed form the kernels compute equals the definition, one
operation at a time, and in a seeded replica history the two forms of the
OR-Set stay in lockstep under apply and merge."""
import numpy as np
import pytest

import apply_util as au
import causal_util as cu


def _eq(got, exp, msg):
    for g, e, f in zip(got, exp, cu.FIELDS):
        np.testing.assert_array_equal(g, e, err_msg=f"{msg} {f}")
        assert g.dtype == e.dtype, (msg, f)


@pytest.mark.parametrize("causal", [False, True])
def test_closed_form_is_the_sequential_definition(causal):
    rng = np.random.default_rng(20)
    for case in range(150):
        n, m = int(rng.integers(0, 40)), int(rng.integers(0, 9))
        t = au.rand_state(rng, n, key_space=6, reps=3, ts_space=8, p_tomb=0.2, p_dup=0.3)
        clock = np.array([8, 8, 8], np.uint64) + rng.integers(0, 5, 3).astype(np.uint64)
        rep = int(rng.integers(3))
        keys, kinds = au.rand_batch(rng, m, 8)           # keys below, inside and above the state's
        exp, esrc, eclk = au.apply_seq(t, clock, rep, keys, kinds, causal)
        got, gsrc, gclk = au.apply_ref(t, clock, rep, keys, kinds, causal)
        _eq(got, exp, f"case {case}")
        np.testing.assert_array_equal(gsrc, esrc, err_msg=f"case {case} src")
        np.testing.assert_array_equal(gclk, eclk, err_msg=f"case {case} clock")


def test_every_three_operation_sequence_on_one_key():
    t = cu.tup([5, 5, 7], [1, 2, 1], [0, 1, 0], [0, 1, 0])
    clock = np.array([3, 3], np.uint64)
    for bits in range(8):
        kinds = np.array([(bits >> j) & 1 for j in range(3)], np.uint8)
        for key in (5, 6):
            keys = np.full(3, key, np.uint64)
            for causal in (False, True):
                exp = au.apply_seq(t, clock, 0, keys, kinds, causal)
                got = au.apply_ref(t, clock, 0, keys, kinds, causal)
                _eq(got[0], exp[0], f"{bits} {key} {causal}")
                np.testing.assert_array_equal(got[1], exp[1])


def test_forms_stay_in_lockstep_through_a_history():
    rng = np.random.default_rng(21)
    R = 4
    tomb = [cu.empty() for _ in range(R)]
    dots = [cu.empty() for _ in range(R)]
    clock = [np.zeros(R, np.uint64) for _ in range(R)]
    applied = merged = 0
    for step in range(120):
        x = int(rng.integers(R))
        if rng.random() < 0.6:
            keys, kinds = au.rand_batch(rng, int(rng.integers(0, 7)), 10)
            tomb[x], _, c1 = au.apply_ref(tomb[x], clock[x], x, keys, kinds, False)
            dots[x], _, c2 = au.apply_ref(dots[x], clock[x], x, keys, kinds, True)
            np.testing.assert_array_equal(c1, c2)
            clock[x] = c1
            applied += 1
        else:
            y = int((x + 1 + rng.integers(R - 1)) % R)
            tomb[x] = au.orset_merge(tomb[x], tomb[y])
            dots[x], _, ctx, _ = cu.ref_causal(dots[x], clock[x], dots[y], clock[y])
            clock[x] = ctx
            merged += 1
        for z in range(R):
            _eq(cu.present(tomb[z]), dots[z], f"step {step} replica {z}")
            for s in (tomb[z], dots[z]):                 # the obligation: a state's context covers its own tags
                assert bool(cu.covered(s[1], s[2], clock[z]).all()), (step, z)
    assert applied > 30 and merged > 30
    assert any(len(d[0]) for d in dots) and any(int(t[3].sum()) for t in tomb)
