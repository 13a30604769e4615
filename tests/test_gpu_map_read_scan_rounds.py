"""GPU: the map read (crdt_map_read; csrc/mapread.hip) where the one-workgroup
tile scan changes rounds (k_tile_scan, csrc/settile.hpp; tests/
test_gpu_settile_scan_rounds.py has the set-state ops there).

Every state has 2049 tiles of T tuples: two full rounds of 1024 and a third of
one tile.  The key whose winner depends on what the previous tile carries sits
on the round edge -- a tag with one copy in tile 1023, the last of round 0, and
one in tile 1024 -- or its deciding tag runs from tile 1023 across all of round
1 into tile 2048.  At rounds of 16384 the same states run in one round on the
product build.  Expectations are the numpy closed form, compared bit for bit,
the outputs being views inside canary buffers."""
import numpy as np
import pytest

from crdt_amd.engine import TupleSet, u64_tensor
from knobs import set_knob
from map_read_util import ref_map_read
from test_gpu_map_read import _lookup, _read, _row

pytestmark = [pytest.mark.gpu, pytest.mark.diag]

T = 2048                       # tuples per tile
TILES = 2049
N = TILES * T
E = 1024 * T                   # the first tuple of tile 1024 = of round 1 at rounds of 1024
E2 = 2048 * T                  # the first tuple of tile 2048 = of round 2
ROUNDS = [16384, 1024]


@pytest.fixture(params=ROUNDS)
def rounds(request, eng):
    try:
        set_knob("settile.scan_round", request.param)
        yield request.param
    finally:
        set_knob("settile.scan_round", 16384)


def _ordinary(n=N):
    """n single-tuple keys 10 i with distinct tags, every third tombstoned."""
    i = np.arange(n, dtype=np.uint64)
    return 10 * i, 1000 + i, (i % 5).astype(np.uint32), (i % 3 == 0).astype(np.uint8)


def _one_key(t, lo, hi):
    t[0][lo:hi] = 10 * lo
    t[2][lo:hi] = 0


def _one_tag(t, lo, hi):
    t[1][lo:hi] = t[1][lo]
    t[2][lo:hi] = t[2][lo]


def _check(eng, t, what, probes):
    Td = TupleSet.from_numpy(*t, eng.device)
    res = {}
    for lww in (False, True):
        exp = ref_map_read(*t, lww)
        _read(eng, Td, lww, exp, f"{what} lww={lww}")
        _read(eng, Td, lww, exp, f"{what} lww={lww}, win alone", with_keys=False, with_nsib=False)
        _lookup(eng, Td, lww, exp, np.asarray(probes, np.uint64), f"{what} lww={lww}")
        res[lww] = exp
    assert eng.device_status(clear=True) == 0
    return res


@pytest.mark.parametrize("live", [False, True])
def test_winner_decided_over_the_round_edge(eng, rounds, live):
    """Key 10 (E - 3): a live tag, a dead one, a tag with a copy in tile 1023
    and one in tile 1024, dead tags.  The copy in tile 1023 tombstoned: tile
    1024 alone sees a live tag, the carry kills it and the winner falls back to
    tuple E - 3.  Both copies live: the tag wins from its first copy, E - 1."""
    t = _ordinary()
    lo, hi = E - 3, E + 3
    _one_key(t, lo, hi)
    _one_tag(t, E - 1, E + 1)
    t[3][lo:hi] = [0, 1, 0 if live else 1, 0, 1, 1]
    res = _check(eng, t, f"round edge, live={live}", [10 * lo, 10 * (lo - 1), 10 * hi, 10 * lo + 1])
    assert _row(res[False], 10 * lo) == ((E - 1, 2) if live else (lo, 1))


@pytest.mark.parametrize("dead", [True, False])
def test_winner_decided_by_a_tag_spanning_round_1(eng, rounds, dead):
    """One tag from tile 1023 across all of round 1 into tile 2048, its only
    tombstone the first copy: dead, and the key's winner is the tag before it,
    in tile 1023; alive it wins from its first copy, 1025 tiles before its end."""
    t = _ordinary()
    lo, hi = E - 7, E2 + 9
    _one_key(t, lo, hi)
    _one_tag(t, E - 5, E2 + 7)
    t[3][lo:hi] = 0
    t[3][lo + 1] = 1
    t[3][E - 5] = 1 if dead else 0
    t[3][E2 + 7:hi] = 1
    res = _check(eng, t, f"spanning tag, dead={dead}", [10 * lo, 10 * (lo - 1), 10 * hi])
    assert _row(res[False], 10 * lo) == ((lo, 1) if dead else (E - 5, 2))
