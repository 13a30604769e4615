"""The witness populations of the vector-clock classify tests
(tests/lanegroup_util.py), checked without a GPU: what they cover is counted
from the arrays themselves, and every deliberately wrong host classifier
below is reported wrong on at least one pair.

Why this file exists: three of the mutants -- ">= is violated" read from the
last column only, a low-32-bit compare, a signed compare -- agree with the
reference on synth.vclock_pairs at every shape of test_vclock_matches_oracle,
since that generator's clocks differ by one and b > a occurs in the last
column only (the last test here pins that, and that the two other simple
mutants, "<= is violated" from the last column only and a high-32-bit
compare, are the ones that generator does catch).  A classify kernel with one
of the three faults passed the suite.
"""
import numpy as np
import pytest

import lanegroup_util as L
from lanegroup_util import AFTER, BEFORE, CANARY, CONCURRENT, EQUAL

from crdt_amd import synth
from oracle import oracle

VECTOR_NODES = [128, 64, 32]
GENERIC_NODES = [1, 3, 65, 513]
PARITY_SHAPES = [(1, 128), (7, 128), (20_000, 128), (5000, 64), (3000, 32), (1000, 100), (100, 1), (50, 3), (10, 513)]


# ---------------------------------------------------------------- mutants
def _from_violations(nle, nge):
    return L.classes(~nle.any(axis=1), ~nge.any(axis=1))


def _masked(keep):
    """Only the columns keep(nodes) selects are compared."""
    def classify(a, b):
        m = keep(a.shape[1])
        return _from_violations((a > b) & m, (a < b) & m)
    return classify


def _cols(sel):
    def keep(nodes):
        m = np.zeros(nodes, bool)
        m[sel(nodes)] = True
        return m
    return keep


def m_ge_last_only(a, b):
    nge = a < b
    nge[:, :-1] = False
    return _from_violations(a > b, nge)


def m_le_last_only(a, b):
    nle = a > b
    nle[:, :-1] = False
    return _from_violations(nle, a < b)


def m_low32(a, b):
    m = np.uint64(0xFFFFFFFF)
    return L.classify_ref(a & m, b & m)


def m_high32(a, b):
    s = np.uint64(32)
    return L.classify_ref(a >> s, b >> s)


def m_signed(a, b):
    x, y = a.view(np.int64), b.view(np.int64)
    return _from_violations(x > y, x < y)


def m_neighbour(a, b):
    """A pair also sees the violations of pair p ^ 1."""
    nle, nge = (a > b).any(axis=1), (a < b).any(axis=1)
    q = np.minimum(np.arange(len(nle)) ^ 1, len(nle) - 1)
    return L.classes(~(nle | nle[q]), ~(nge | nge[q]))


def m_last_slot_equal(slots):
    def classify(a, b):
        out = L.classify_ref(a, b)
        out[slots - 1::slots] = EQUAL
        return out
    return classify


def m_sweep_copy(sweep):
    """Entries at p >= one sweep hold what entry p - sweep holds."""
    def classify(a, b):
        out = L.classify_ref(a, b)
        out[sweep:] = out[:-sweep].copy()
        return out
    return classify


def m_tail_canary(rows_per_load):
    """The rows of a ragged last wave-load are never written."""
    def classify(a, b):
        out = L.classify_ref(a, b)
        tail = len(out) % rows_per_load
        if tail:
            out[-tail:] = CANARY
        return out
    return classify


SYNTH_BLIND = {"ge from the last column": m_ge_last_only, "low 32 bits": m_low32, "signed": m_signed}
SYNTH_SEEN = {"le from the last column": m_le_last_only, "high 32 bits": m_high32}


def mutants(nodes, slots):
    """name -> classifier, the mutants that are wrong at this node count."""
    out = {"high 32 bits": m_high32, "low 32 bits": m_low32, "signed": m_signed,
           "even columns skipped": _masked(_cols(lambda n: slice(1, None, 2))),
           "column 0 dropped": _masked(_cols(lambda n: slice(1, None))),
           "last column dropped": _masked(_cols(lambda n: slice(0, n - 1))),
           "neighbour pair leaks": m_neighbour, "last slot left EQUAL": m_last_slot_equal(slots)}
    if nodes > 1:                                   # at one node these three are the reference itself
        out["ge from the last column"] = m_ge_last_only
        out["le from the last column"] = m_le_last_only
        out["odd columns skipped"] = _masked(_cols(lambda n: slice(0, None, 2)))
    if nodes > 64:
        out["first 64 columns only"] = _masked(_cols(lambda n: slice(0, 64)))
    if nodes in L.VCLOCK_VECTOR_NODES and nodes < 128:
        out["ragged tail left at the canary"] = m_tail_canary(64 // (nodes // 2))
    return out


@pytest.fixture(scope="module")
def population():
    cache = {}

    def get(nodes):
        if nodes not in cache:
            a, b = L.witness_pairs(nodes, L.witness_slots(nodes), seed=nodes)
            a.setflags(write=False)
            b.setflags(write=False)
            cache[nodes] = (a, b, L.classify_ref(a, b))
        return cache[nodes]

    yield get
    cache.clear()


# ---------------------------------------------------------------- the population
@pytest.mark.parametrize("nodes", VECTOR_NODES + GENERIC_NODES)
def test_population_covers_every_column_slot_and_kind(population, nodes):
    slots = L.witness_slots(nodes)
    if nodes in VECTOR_NODES:
        assert slots == 64 // (nodes // 2) * 32
    a, b, exp = population(nodes)
    assert a.shape == b.shape and a.shape[1] == nodes and a.dtype == b.dtype == np.uint64
    np.testing.assert_array_equal(oracle.vclock_classify(a, b), exp)
    np.testing.assert_array_equal(L.classify_ref(b, a), L.SWAP[exp])
    # the background: a == b, at least 2^32, room above for every delta
    same = a == b
    assert (a[same] >= np.uint64(2**32)).all() and (a[same] < np.uint64(2**62)).all()
    ndiff = (~same).sum(axis=1)
    p = np.arange(len(exp))
    for cls, a_higher in ((BEFORE, False), (AFTER, True)):
        one = np.nonzero((exp == cls) & (ndiff == 1))[0]
        col = (~same)[one].argmax(axis=1)
        lo, hi = (b, a) if a_higher else (a, b)
        kind = L.kind_of(lo[one, col], hi[one, col])
        assert (kind >= 0).all()
        seen = np.zeros((nodes, slots), bool)
        seen[col, p[one] % slots] = True
        assert seen.all(), f"class {cls}: (column, slot) without a single-column witness: {np.argwhere(~seen)[:4]}"
        kinds = np.zeros((nodes, L.KINDS), bool)
        kinds[col, kind] = True
        assert kinds.all(), f"class {cls}: (column, kind) never planted: {np.argwhere(~kinds)[:4]}"
    counts = np.bincount(exp, minlength=4)
    per = nodes * slots
    if nodes > 1:
        assert (counts > 0).all()
        assert counts[CONCURRENT] == 4 * per and counts[BEFORE] == counts[AFTER] == per + nodes
        # CONCURRENT on two columns: every column as the a > b side, with a
        # partner in its own 16-byte vector (even nodes) and one outside it
        two = np.nonzero((exp == CONCURRENT) & (ndiff == 2))[0]
        ca, cb = (a > b)[two].argmax(axis=1), (a < b)[two].argmax(axis=1)
        assert (np.bincount(ca, minlength=nodes) >= 3 * slots).all()
        if nodes % 2 == 0:
            assert set(ca[(ca ^ 1) == cb]) == set(range(nodes))
        if nodes > 3:
            assert set(ca[(ca ^ 1) != cb]) == set(range(nodes))
        # near misses: b > a everywhere but one column, every column once per slot
        near = np.nonzero(ndiff == nodes)[0]
        assert (exp[near] == CONCURRENT).all() and ((a > b)[near].sum(axis=1) == 1).all()
        seen = np.zeros((nodes, slots), bool)
        seen[(a > b)[near].argmax(axis=1), near % slots] = True
        assert seen.all() or nodes == 2                   # at two nodes a near miss is an ordinary CONCURRENT pair
    else:
        assert counts[CONCURRENT] == 0 and counts[EQUAL] > 0 and counts[BEFORE] == counts[AFTER] == per + nodes
    if nodes == 128:
        assert len(exp) - 3 * 2 * nodes - 3 == 24_576     # six blocks of 128 x 32
    # isolated witnesses: EQUAL on both sides of a single-column witness
    iso = np.nonzero((exp[1:-1] != EQUAL) & (exp[:-2] == EQUAL) & (exp[2:] == EQUAL))[0] + 1
    assert len(iso) >= 2 * nodes - 2
    assert set((~same)[iso].argmax(axis=1)) == set(range(nodes))
    assert len(exp) % 4 == 3                              # a ragged last wave-load at 2 and 4 pairs per load


@pytest.mark.parametrize("nodes", VECTOR_NODES + GENERIC_NODES)
def test_every_mutant_is_caught(population, nodes):
    a, b, exp = population(nodes)
    assert L.check_population(a, b, L.classify_ref) == 0
    assert L.check_population(a, b, oracle.vclock_classify) == 0
    survivors = [name for name, m in mutants(nodes, L.witness_slots(nodes)).items() if L.check_population(a, b, m) == 0]
    assert not survivors, f"nodes {nodes}: mutants the population does not catch: {survivors}"


@pytest.mark.parametrize("nodes", VECTOR_NODES + [3])
def test_sweep_copy_mutant_is_caught_by_the_dense_population(nodes):
    """The sweep tests' population, at the size an 8-CU device would give it
    (256 CUs for the one-pair-per-wave kernel, whose sweep is small anyway):
    a result that repeats the sweep before it is wrong, every class and delta
    kind occurs, and each pair's class hangs on one column (two for CONCURRENT)."""
    cus = 8 if nodes in L.VCLOCK_VECTOR_NODES else 256
    pairs = L.sweep_rows(L.vclock_geometry(1 << 20, nodes, cus, 32, 1))
    g = L.vclock_geometry(pairs, nodes, cus, 32, 1)
    L.assert_sweeps(g)
    a, b = L.dense_pairs(nodes, pairs, seed=nodes)
    exp = L.classify_ref(a, b)
    np.testing.assert_array_equal(oracle.vclock_classify(a, b), exp)
    counts = np.bincount(exp, minlength=4)
    assert (np.abs(counts / pairs - 0.25) < 0.05).all(), counts
    ndiff = (a != b).sum(axis=1)
    np.testing.assert_array_equal(ndiff, np.array([0, 1, 1, 2])[exp])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    kinds = L.kind_of(lo[a != b], hi[a != b])
    assert set(kinds) == set(range(L.KINDS))
    assert L.check_population(a, b, m_sweep_copy(g.sweep)) > pairs // 4
    assert L.check_population(a, b, m_sweep_copy(2 * g.sweep)) > 0
    if g.rows_per_load > 1:
        assert L.check_population(a, b, m_tail_canary(g.rows_per_load)) == pairs % g.rows_per_load > 0
    assert not (a[g.sweep:] == a[:-g.sweep]).all(axis=1).any()


# ---------------------------------------------------------------- the geometry
def test_vclock_geometry_known_values():
    """256 CUs.  Product defaults (U = 32, one block per CU): 1024 waves."""
    g = L.vclock_geometry(100_000, 128, 256, 32, 1)
    assert (g.kernel, g.grid, g.waves, g.rows_per_load, g.rows_per_iter, g.sweep) == ("vector", 256, 1024, 1, 32, 32_768)
    assert (g.full_sweeps, g.partial) == (3, 100_000 - 3 * 32_768)
    g = L.vclock_geometry(100_000, 64, 256, 32, 1)
    assert (g.kernel, g.rows_per_load, g.rows_per_iter, g.sweep) == ("vector", 2, 64, 65_536)
    g = L.vclock_geometry(100_000, 32, 256, 32, 1)
    assert (g.kernel, g.rows_per_load, g.rows_per_iter, g.sweep) == ("vector", 4, 128, 131_072)
    # no vector kernel at 16 nodes, none for a misaligned operand: one pair per wave
    for nodes, aligned in ((16, True), (100, True), (128, False), (32, False)):
        g = L.vclock_geometry(100_000, nodes, 256, 32, 1, aligned=aligned)
        assert (g.kernel, g.rows_per_load, g.rows_per_iter, g.sweep) == ("generic", 1, 1, 1024)
    # U = 1: a sweep is 1024 pairs at 128 nodes; two blocks per CU double it
    assert L.vclock_geometry(100_000, 128, 256, 1, 1).sweep == 1024
    assert L.vclock_geometry(100_000, 128, 256, 1, 2).sweep == 2048
    assert L.vclock_geometry(100_000, 32, 256, 1, 1).sweep == 4096
    # launch_vc's default arm
    assert [L.vclock_unroll(v) for v in (1, 2, 4, 8, 16, 32, 3, 64)] == [1, 2, 4, 8, 16, 32, 4, 4]
    # below the cap: one wave per pair's worth of lanes, a single sweep
    g = L.vclock_geometry(1000, 100, 256, 32, 1)
    assert (g.grid, g.waves, g.full_sweeps, g.partial) == (250, 1000, 1, 0)
    g = L.vclock_geometry(7, 128, 256, 32, 1)
    assert (g.grid, g.sweep, g.full_sweeps) == (2, 256, 0)
    # the sweep tests' sizes: 2 sweeps + 3 wave-loads + 1
    for nodes, pairs in ((128, 65_540), (32, 262_157), (3, 2052)):
        g = L.vclock_geometry(1 << 20, nodes, 256, 32, 1)
        assert L.sweep_rows(g) == pairs
        L.assert_sweeps(L.vclock_geometry(pairs, nodes, 256, 32, 1))
    with pytest.raises(AssertionError):
        L.assert_sweeps(L.vclock_geometry(20_000, 128, 256, 32, 1))      # the largest ordinary parity shape
    assert "sweep 2 + 4" in L.vclock_geometry(65_540, 128, 256, 32, 1).where(65_540)


def test_rowsum_geometry_known_values():
    """256 CUs x 8 blocks: 8192 waves, 64 / (nodes / 2) rows per wave-load."""
    for nodes, rpl in ((128, 1), (64, 2), (32, 4), (16, 8)):
        g = L.rowsum_geometry(1 << 20, nodes, 256)
        assert (g.kernel, g.grid, g.waves, g.rows_per_load, g.rows_per_iter, g.sweep) == \
            ("vector", 2048, 8192, rpl, rpl, 8192 * rpl)
        rows = L.sweep_rows(g)
        assert rows == 2 * 8192 * rpl + 3 * rpl + 1
        L.assert_sweeps(L.rowsum_geometry(rows, nodes, 256))
    for nodes, aligned in ((5, True), (8, True), (200, True), (64, False), (128, False)):
        g = L.rowsum_geometry(1 << 20, nodes, 256, aligned=aligned)
        assert (g.kernel, g.sweep) == ("generic", 8192)
    g = L.rowsum_geometry(5000, 64, 256)                                  # the largest shape of the parity tests
    assert (g.grid, g.full_sweeps) == (1250, 0)
    assert L.order_map_sweep(2 * 4096 * 256 + 3) == 4096 * 256 and L.order_map_sweep(1006) == 1024


# ---------------------------------------------------------------- why the file exists
def test_three_mutants_pass_the_synthetic_pairs():
    """On synth.vclock_pairs three mutants make no mistake at any shape of
    test_vclock_matches_oracle: b > a occurs in the last column only, and no
    two cells differ by more than one.  (The generator's CONCURRENT pairs put
    a > b in another column and its values' high halves are equal, so it does
    catch the two other simple mutants.)"""
    seen = {name: 0 for name in SYNTH_SEEN}
    for pairs, nodes in PARITY_SHAPES:
        a, b = synth.vclock_pairs(21, pairs, nodes)
        assert not (b > a)[:, :-1].any()
        assert (np.maximum(a, b) - np.minimum(a, b)).max() <= 1
        for name, m in SYNTH_BLIND.items():
            assert L.check_population(a, b, m) == 0, (name, pairs, nodes)
        for name, m in SYNTH_SEEN.items():
            seen[name] += L.check_population(a, b, m)
    assert all(seen.values()), seen
