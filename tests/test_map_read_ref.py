"""CPU: the host restatements of the map read (tests/map_read_util.py) agree
with each other and with what was there before the read -- the closed form the
GPU tests compare against == a literal per-key dictionary interpreter; its
keys == the member keys of the oracle's merge with an empty side; its win ==
the composition of compaction, LWW pick and index composition."""
import numpy as np
import pytest

from crdt_amd import synth
from map_read_util import composed_win, interp_map_read, ref_map_read, with_copies
from oracle import oracle

SIZES = [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 4097, 8193, 100_000]


def _sets(n, ks):
    return synth.sort_tuples_np(*synth.set_tuples(31 + n, 0, n, ks))


def _key_spaces(n):
    return (1, 7, max(1, n // 3), 10**9)


def _same(a, b, what):
    for x, y, f in zip(a, b, ("keys", "win", "nsib")):
        assert x.dtype == y.dtype, (what, f, x.dtype, y.dtype)
        np.testing.assert_array_equal(x, y, err_msg=f"{what} {f}")


@pytest.mark.parametrize("n", SIZES)
def test_closed_form_equals_interpreter(n):
    for ks in _key_spaces(n):
        t = _sets(n, ks)
        for lww in (True, False):
            _same(ref_map_read(*t, lww), interp_map_read(*t, lww), f"n={n} ks={ks} lww={lww}")


@pytest.mark.parametrize("n,ks", [(1, 1), (65, 7), (2049, 3), (2049, 600), (8193, 40), (8193, 2700)])
def test_closed_form_equals_interpreter_with_copies(n, ks):
    """1 to 4 copies of every tag, mixed tombs within a tag: the first copy's
    tomb (LWW) and the tomb-OR (OR-Set) differ."""
    t = with_copies(_sets(n, ks), np.random.default_rng(n + ks))
    first_differs = 0
    for lww in (True, False):
        got = ref_map_read(*t, lww)
        _same(got, interp_map_read(*t, lww), f"copies n={n} ks={ks} lww={lww}")
        first_differs += len(got[0])
    if n > 1000:
        a, b = ref_map_read(*t, True), ref_map_read(*t, False)
        assert not np.array_equal(a[1], b[1])             # the two modes disagree somewhere: the cases are not trivial
        assert (b[2] > 1).any()


@pytest.mark.parametrize("n", [65, 2049, 8193, 100_000])
def test_keys_are_the_oracle_merge_members(n):
    for ks in _key_spaces(n):
        t = _sets(n, ks)
        empty = tuple(x[:0] for x in t)
        for lww in (True, False):
            k, _, _, tomb = (oracle.lww_merge if lww else oracle.orset_merge)(t, empty)
            np.testing.assert_array_equal(ref_map_read(*t, lww)[0], np.unique(k[tomb == 0]), err_msg=f"n={n} ks={ks} lww={lww}")


@pytest.mark.parametrize("n", [0, 1, 65, 2049, 8193, 100_000])
def test_win_is_the_composition_of_the_earlier_calls(n):
    rng = np.random.default_rng(n)
    for ks in _key_spaces(n):
        for t in (_sets(n, ks), with_copies(_sets(n, ks), rng)):
            for lww in (True, False):
                keys, win, nsib = ref_map_read(*t, lww)
                np.testing.assert_array_equal(win, composed_win(t, lww), err_msg=f"n={n} ks={ks} lww={lww}")
                np.testing.assert_array_equal(t[0][win], keys)
                assert (nsib >= 1).all()
