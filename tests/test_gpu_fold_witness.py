"""GPU: the column-max fold (crdt_gcounter_fold, crdt_shard_fold_max_u64)
and the join's knob variants against populations in which one skipped or
over-read row changes the answer.

synth.counters plants 2^64-1 in ~1/4096 of the cells, so at the sizes that
reach the fold's second unrolled step every column's maximum is that
constant and a fold that skips rows still passes.  Here every planted 2^64-1
is zeroed (the background: distinct, untied column maxima, asserted) and
witness rounds write one value per column, all >= 2^63, distinct, one of
them 2^64-1, into the rows the launch geometry makes critical (tests/fold_util.py):
row 0, 1, rows-2, rows-1, the end of the last full unrolled step, both ends
of every remainder stride, every 8-way shard cut -1/0/+1, and seeded random
rows.  The fold must return exactly the witnesses, and the background's fold
again once they are restored.  Row counts come from the device's CU count
and the fold knobs; each test asserts that its shape still runs the unrolled
loop twice and the remainder loop for a whole and a partial stride.
"""
import numpy as np
import pytest
import torch
from fold_util import (Population, fold_geometry, join_geometry, join_rows, pow2_rows, run_rounds,
                       shard_cuts, shard_witnesses, special_rows, witness_schedule, witness_values)
from knobs import set_knob

from crdt_amd import _lib, shard
from crdt_amd.engine import as_u64
from oracle import oracle

pytestmark = pytest.mark.gpu

EDGE = np.array([0, 1, 2**63 - 1, 2**63, 2**64 - 2, 2**64 - 1], dtype=np.uint64)


def _cus(eng) -> int:
    return torch.cuda.get_device_properties(eng.device).multi_processor_count


def _fold_knobs():
    return _lib.get_option(b"fold.unroll"), _lib.get_option(b"fold.blocks_per_cu")


@pytest.fixture(scope="module")
def pops(eng):
    """Populations shared by the tests of this module, keyed by shape."""
    cache = {}

    def get(rows, nodes, misaligned=False):
        key = (rows, nodes, misaligned)
        if key not in cache:
            cache[key] = Population(eng, rows, nodes, misaligned=misaligned)
        return cache[key]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


def _pow2_case(eng, pops, nodes):
    """The pow2 shape for the knobs in force, its geometry (preconditions asserted) and schedule."""
    unroll, bpc = _fold_knobs()
    cus = _cus(eng)
    rows = pow2_rows(nodes, cus, bpc)
    g = fold_geometry(rows, nodes, cus, unroll, bpc)
    assert g.path == "pow2" and g.grid == cus * bpc
    assert g.full_steps >= 2, "the unrolled loop must run at least twice"
    assert g.rem_part > 0 and (g.rem_full >= 1 or unroll == 1), "remainder: one whole stride and a partial one"
    pop = pops(rows, nodes)
    assert pop.t.data_ptr() % 16 == 0
    cuts = shard_cuts(rows)
    sched = witness_schedule(rows, nodes, special_rows(rows, g, cuts), seed=nodes)
    return pop, g, cuts, sched


def _zero_identity(pop):
    """A column all zero but a 1 in its last row folds to 1, an all-zero one to 0."""
    t, exp = pop.t, pop.bg.copy()
    keep = t[:, :2].clone()
    try:
        t[:, 0] = 0
        t[-1, 0] = 1
        exp[0] = 1
        if pop.nodes > 1:
            t[:, 1] = 0
            exp[1] = 0
        np.testing.assert_array_equal(pop.fold(), exp)
    finally:
        t[:, :2] = keep
    np.testing.assert_array_equal(pop.fold(), pop.bg)


# ---------------------------------------------------------------- 1. witness populations
@pytest.mark.parametrize("nodes", [2, 4, 16, 64, 256, 512])
def test_pow2_fold_witnesses(eng, pops, nodes):
    pop, g, cuts, sched = _pow2_case(eng, pops, nodes)
    np.testing.assert_array_equal(pop.fold(), pop.bg)
    run_rounds(pop, sched, lambda: [pop.fold()], oracle_rounds=(f"row {pop.rows - 1}", "random 0"))
    _zero_identity(pop)


@pytest.mark.parametrize("case", ["63", "1024", "3", "64-misaligned"])
def test_generic_fold_witnesses(eng, pops, case):
    cus = _cus(eng)
    grid = 4 * cus
    nodes, rows = {"63": (63, 2 * grid + 5), "1024": (1024, grid + 1), "3": (3, 2 * grid + 5),
                   "64-misaligned": (64, 2 * grid + 5)}[case]
    mis = case.endswith("misaligned")
    pop = pops(rows, nodes, mis)
    if mis:                                               # contiguous, not 16-byte aligned: the generic kernel
        assert pop.t.is_contiguous() and pop.t.data_ptr() % 16 == 8
    g = fold_geometry(rows, nodes, cus, *_fold_knobs(), aligned=not mis)
    assert g.path == "generic" and g.grid == grid < rows, "the row loop of a block must run more than once"
    assert g.full_steps >= 1 and g.rem_part > 0
    np.testing.assert_array_equal(pop.fold(), pop.bg)
    sched = witness_schedule(rows, nodes, special_rows(rows, g, shard_cuts(rows)), seed=nodes)
    run_rounds(pop, sched, lambda: [pop.fold()], oracle_rounds=(f"row {rows - 1}", "random 0"))
    _zero_identity(pop)


# ---------------------------------------------------------------- 2. over-read and shard paths
def test_prefix_fold_excludes_the_row_after_it(eng, pops):
    """fold(t[:k]) of a prefix of a larger allocation: a witness in row k-1
    is in it, a larger one in row k is not (k at a stride boundary and odd)."""
    pop, g, _, _ = _pow2_case(eng, pops, 64)
    cols = np.arange(64)
    inside, outside = witness_values(64, 3, base=64), witness_values(64, 5)
    assert (outside > inside).all() and (inside > pop.bg).all()
    for k in (g.stride_rows * (g.unroll + 1), g.stride_rows * g.unroll + 777):
        assert 1 < k < pop.rows and (k % g.stride_rows == 0 or k % 2 == 1)
        saved = pop.host[k, cols].copy()
        try:
            pop.put(np.full(64, k), cols, outside)
            exp = oracle.gcounter_fold(pop.host[:k])
            assert (exp < inside).all()
            np.testing.assert_array_equal(as_u64(eng.gcounter_fold(pop.t[:k])), exp, err_msg=f"prefix {k}")
            saved1 = pop.host[k - 1, cols].copy()
            try:
                pop.put(np.full(64, k - 1), cols, inside)
                np.testing.assert_array_equal(as_u64(eng.gcounter_fold(pop.t[:k])), inside, err_msg=f"prefix {k}")
            finally:
                pop.put(np.full(64, k - 1), cols, saved1)
        finally:
            pop.put(np.full(64, k), cols, saved)
    np.testing.assert_array_equal(pop.fold(), pop.bg)


def test_each_shard_fold_equals_the_oracle_of_its_slice(eng, pops):
    """fold_util.shard_witnesses: every shard's last row (even columns) and
    first row (odd columns) carry witnesses, and the row just outside either
    end of a shard holds a larger value in its columns.  Each slice's fold ==
    the oracle's fold of that slice alone == that shard's own witnesses, and
    every witness shows in exactly one shard's result."""
    pop, _, cuts, _ = _pow2_case(eng, pops, 64)
    writes = shard_witnesses(cuts, 64)
    for r, cc, v in writes:
        assert (v > pop.bg[cc]).all() and (v >= np.uint64(2**63)).all()
    saved = [(r, cc, pop.host[r, cc].copy()) for r, cc, _ in writes]
    try:
        for r, cc, v in writes:
            pop.put(np.full(len(cc), r), cc, v)
        parts = [as_u64(eng.gcounter_fold(pop.t[cuts[r]:cuts[r + 1]])) for r in range(8)]
        for r in range(8):
            np.testing.assert_array_equal(parts[r], oracle.gcounter_fold(pop.host[cuts[r]:cuts[r + 1]]),
                                          err_msg=f"shard {r}")
            for row, cc, v in writes:                     # its own witnesses, nothing from a neighbour
                if cuts[r] <= row < cuts[r + 1]:
                    np.testing.assert_array_equal(parts[r][cc], v, err_msg=f"shard {r}, row {row}")
        stack = np.stack(parts)
        for row, cc, v in writes:                         # a witness shows in exactly one shard's result
            assert ((stack[:, cc] == v[None, :]).sum(axis=0) == 1).all(), f"row {row}"
        whole = oracle.gcounter_fold(pop.host)
        np.testing.assert_array_equal(np.maximum.reduce(parts), whole)
        np.testing.assert_array_equal(pop.fold(), whole)
    finally:
        for r, cc, v in saved:
            pop.put(np.full(len(cc), r), cc, v)
    np.testing.assert_array_equal(pop.fold(), pop.bg)


def _comm_schedule(pop, cuts):
    """Row 0, the last row, and the cut rounds: column c's witness at cut 1 + c % 7, offset -1 / 0 / +1."""
    nodes = pop.nodes
    inner = np.array(cuts[1:8], np.int64)
    rounds = [("row 0", np.zeros(nodes, np.int64)), (f"row {pop.rows - 1}", np.full(nodes, pop.rows - 1, np.int64))]
    rounds += [(f"cuts{d:+d}", inner[np.arange(nodes) % 7] + d) for d in (-1, 0, 1)]
    return [(name, rr, witness_values(nodes, k)) for k, (name, rr) in enumerate(rounds)]


@pytest.mark.parametrize("path", ["loopback8", "init_rank", "create"])
def test_fold_max_transports_see_every_witness(eng, pops, path):
    pop, _, cuts, _ = _pow2_case(eng, pops, 64)
    if path == "loopback8":
        c = shard.Comm.loopback(0, 8)
        shards = [pop.t[cuts[r]:cuts[r + 1]] for r in range(8)]
    else:
        c = shard.Comm.init_rank(eng) if path == "init_rank" else shard.Comm.create([0])
        shards = [pop.t]

    def fold():
        torch.cuda.synchronize()                          # the member streams are the library's own
        outs = c.fold_max(shards)
        c.sync()
        torch.cuda.synchronize()
        return [as_u64(o) for o in outs]

    try:
        assert len(fold()) == (8 if path == "loopback8" else 1)
        run_rounds(pop, _comm_schedule(pop, cuts), fold, oracle_rounds=("cuts+0",))
    finally:
        c.close()


# ---------------------------------------------------------------- 3. knob variants
FOLD_VARIANTS = ([("fold.unroll", v) for v in (1, 2, 4, 8, 16)] + [("fold.nontemporal", v) for v in (0, 1)]
                 + [("fold.blocks_per_cu", v) for v in (1, 2, 4)])
JOIN_VARIANTS = ([("join.unroll", v) for v in (1, 2, 4, 8)] + [("join.nontemporal", v) for v in (0, 1)]
                 + [("join.blocks_per_cu", v) for v in (1, 2, 8)])


@pytest.mark.diag
@pytest.mark.parametrize("knob,value", FOLD_VARIANTS)
def test_fold_knob_variant_witnesses(eng, pops, knob, value):
    before = _lib.get_option(knob.encode())
    try:
        set_knob(knob, value)
        assert _lib.get_option(knob.encode()) == value
        pop, _, _, sched = _pow2_case(eng, pops, 64)      # geometry and rows for the knob in force
        np.testing.assert_array_equal(pop.fold(), pop.bg)
        run_rounds(pop, sched, lambda: [pop.fold()], oracle_rounds=("random 0",))
        _zero_identity(pop)
    finally:
        set_knob(knob, before)


@pytest.mark.diag
def test_fold_unroll_32_is_refused(eng):
    """crdt_gcounter_fold instantiates unroll 1, 2, 4, 8, 16: the validator
    accepts no other value (the product build refuses every name)."""
    before = _lib.get_option(b"fold.unroll")
    with pytest.raises(_lib.CrdtError):
        _lib.set_option(b"fold.unroll", 32)
    assert _lib.get_option(b"fold.unroll") == before


@pytest.fixture(scope="module")
def join_inputs(eng):
    cache = {}

    def get(rows, nodes):
        if (rows, nodes) not in cache:
            ta, tb = eng.synth_counters(13, 1, rows, nodes), eng.synth_counters(13, 2, rows, nodes)
            cache[(rows, nodes)] = (ta, tb, as_u64(ta).reshape(-1), as_u64(tb).reshape(-1))
        return cache[(rows, nodes)]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


@pytest.mark.diag
@pytest.mark.parametrize("knob,value", JOIN_VARIANTS)
def test_join_knob_variant_exact(eng, join_inputs, knob, value):
    """k_join through two unrolled steps, a whole and a partial remainder
    stride, and k_join_tail (odd element count) == np.maximum.  All 36 EDGE
    pairs ride through each of the three last elements -- both lanes of the
    last full vector and the odd tail element -- three pairs per join, the
    assignment rotated over three passes.  The whole output is compared on
    the host once per pass and on the device (against the uploaded
    np.maximum) in every join."""
    nodes = 63
    before = _lib.get_option(knob.encode())
    try:
        set_knob(knob, value)
        assert _lib.get_option(knob.encode()) == value
        unroll, bpc, cus = _lib.get_option(b"join.unroll"), _lib.get_option(b"join.blocks_per_cu"), _cus(eng)
        rows = join_rows(nodes, cus, unroll, bpc)
        n = rows * nodes
        g = join_geometry(n, cus, unroll, bpc)
        assert n % 2 == 1 and g.grid == cus * bpc and g.full_steps >= 2
        assert g.rem_part > 0 and (g.rem_full >= 1 or unroll == 1)
        ta, tb, a, b = join_inputs(rows, nodes)
        pairs = [(x, y) for x in EDGE for y in EDGE]
        keep = a[n - 3:].copy(), b[n - 3:].copy()
        exp_dev = torch.from_numpy(np.maximum(a, b).view(np.int64)).to(eng.device)
        seen = [set(), set(), set()]
        try:
            for rot in range(3):
                for k in range(0, len(pairs), 3):         # elements n-3, n-2: the last full vector; n-1: the tail
                    slot = [pairs[k + (s + rot) % 3] for s in range(3)]
                    for s in range(3):
                        seen[s].add(slot[s])
                    a[n - 3:] = [p[0] for p in slot]
                    b[n - 3:] = [p[1] for p in slot]
                    ta.view(-1)[n - 3:] = torch.from_numpy(a[n - 3:].view(np.int64).copy()).to(eng.device)
                    tb.view(-1)[n - 3:] = torch.from_numpy(b[n - 3:].view(np.int64).copy()).to(eng.device)
                    exp_dev[n - 3:] = torch.from_numpy(np.maximum(a[n - 3:], b[n - 3:]).view(np.int64)).to(eng.device)
                    out = eng.gcounter_join(ta, tb).view(-1)
                    np.testing.assert_array_equal(as_u64(out[n - 3:]), np.maximum(a[n - 3:], b[n - 3:]),
                                                  err_msg=f"EDGE pairs {slot}")
                    assert torch.equal(out, exp_dev), f"pass {rot}, pairs {k}..{k + 2}"
                    if k == 0:
                        np.testing.assert_array_equal(as_u64(out), np.maximum(a, b), err_msg=f"pass {rot}")
            assert all(len(s) == len(pairs) for s in seen)
        finally:
            a[n - 3:], b[n - 3:] = keep
            ta.view(-1)[n - 3:] = torch.from_numpy(a[n - 3:].view(np.int64).copy()).to(eng.device)
            tb.view(-1)[n - 3:] = torch.from_numpy(b[n - 3:].view(np.int64).copy()).to(eng.device)
    finally:
        set_knob(knob, before)


# ---------------------------------------------------------------- 5. one large-offset case
BIG_ROWS, BIG_NODES = 2**26 + 16_387, 64                  # 34.4 GB: just past 16-byte vector index 2^31
BIG_MASK = 2**62 - 1


@pytest.fixture(scope="module")
def big(eng):
    """Device-only population: synth counters & (2^62-1), the cells that
    became 2^62-1 (the planted edges) zeroed so no column folds to a constant."""
    hold = [eng.synth_counters(2024, 7, BIG_ROWS, BIG_NODES)]
    try:
        hold[0].bitwise_and_(BIG_MASK)
        for r0 in range(0, BIG_ROWS, 1 << 23):
            s = hold[0][r0:r0 + (1 << 23)]
            s.masked_fill_(s == BIG_MASK, 0)
        torch.cuda.synchronize()
        yield hold
    finally:
        hold.clear()
        torch.cuda.empty_cache()


def test_fold_past_vector_index_2_31(eng, big):
    """One witness round on 2^26 + 16,387 rows x 64: witnesses in the rows at
    byte offsets 2^32 .. 2^35 and the rows after them, around 16-byte vector
    index 2^31, and in the last row.  The expectation is torch's signed
    column amax of each 8-way slice (exact: the background is < 2^62)."""
    t = big[0]
    rows, nodes, row_bytes = BIG_ROWS, BIG_NODES, BIG_NODES * 8
    assert rows * nodes // 2 > 2**31 and rows * row_bytes > 2**35
    cuts = shard_cuts(rows)
    bg_parts = [t[cuts[r]:cuts[r + 1]].amax(dim=0).cpu().numpy().view(np.uint64) for r in range(8)]
    bg = np.maximum.reduce(bg_parts)
    assert (bg < BIG_MASK).all() and len(np.unique(bg)) == nodes, "the background folds to a constant"
    stack = np.stack(bg_parts)                            # a slice's expectation is no other slice's
    assert all(len(np.unique(stack[:, c])) == 8 for c in range(nodes)), "slice maxima tied across slices"
    wrows = []
    for p in (32, 33, 34, 35):
        wrows += [2**p // row_bytes, 2**p // row_bytes + 1]
    wrows += [2**31 // (nodes // 2) - 1, 2**31 // (nodes // 2), 2**31 // (nodes // 2) + 1, rows - 1]
    wrows = sorted(set(wrows))
    assert wrows[-1] == rows - 1 and all(0 <= r < rows for r in wrows) and len(wrows) == 10
    vals = witness_values(nodes, 0)
    rr = np.array([wrows[c % len(wrows)] for c in range(nodes)])
    for r in wrows:
        cc = np.nonzero(rr == r)[0]
        t[r, torch.as_tensor(cc, device=t.device)] = torch.from_numpy(vals[cc].view(np.int64).copy()).to(t.device)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(as_u64(eng.gcounter_fold(t)), vals, err_msg="whole fold")
    shards = [t[cuts[r]:cuts[r + 1]] for r in range(8)]
    for r in range(8):
        exp = bg_parts[r].copy()
        mine = (rr >= cuts[r]) & (rr < cuts[r + 1])
        exp[mine] = vals[mine]
        np.testing.assert_array_equal(as_u64(eng.gcounter_fold(shards[r])), exp, err_msg=f"slice {r}")
    c = shard.Comm.loopback(0, 8)
    try:
        torch.cuda.synchronize()
        outs = c.fold_max(shards)
        c.sync()
        for r, o in enumerate(outs):
            np.testing.assert_array_equal(as_u64(o), vals, err_msg=f"loopback rank {r}")
    finally:
        c.close()
    c = shard.Comm.init_rank(eng)
    try:
        np.testing.assert_array_equal(as_u64(c.fold_max([t])[0]), vals, err_msg="init_rank")
    finally:
        c.close()
