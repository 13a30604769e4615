"""GPU: the causal-stability cut of a vector-clock population
(crdt_vclock_stable_cut, csrc/stable.hip; Comm.stable_cut) against
numpy.min(axis=0) on uint64, on populations in which one skipped or over-read
row changes the answer.

The kernels are the column-MIN twins of the fold's, at the fold's product
shape (unroll 8, one workgroup per CU, compile-time), so tests/fold_util.py's
geometry describes them too.  A fold_util.Population is made discriminating
for a minimum: the top bit is set in every background cell (all >= 2^63: a
signed minimum prefers a background cell, and no cell is zero), and witness
rounds write one distinct value < 2^63 per column into the rows the launch
geometry makes critical -- both ends, the end of the last full unrolled step,
both ends of every remainder stride, seeded random rows.  The cut must return
exactly the witnesses, and the background's minimum again once they are
restored."""
import numpy as np
import pytest
import torch
from fold_util import Population, fold_geometry, pow2_rows, shard_cuts, special_rows, witness_schedule

from crdt_amd import _lib, shard, synth
from crdt_amd.engine import TupleSet, as_u64, u64_tensor
from oracle import oracle

pytestmark = pytest.mark.gpu

UNROLL, BPC = 8, 1             # the compile-time shape of k_cut_pow2's launch (csrc/stable.hip)
H = 2**63
M64 = 2**64 - 1
E_INVAL = -1


def _cus(eng) -> int:
    return torch.cuda.get_device_properties(eng.device).multi_processor_count


class MinPopulation:
    """A fold_util.Population with bit 63 set in every cell, and its column minimum."""

    def __init__(self, eng, rows, nodes, misaligned=False):
        self.pop = Population(eng, rows, nodes, misaligned=misaligned)
        self.pop.t.bitwise_or_(torch.iinfo(torch.int64).min)
        self.pop.host |= np.uint64(H)
        self.eng, self.rows, self.nodes, self.t, self.host = eng, rows, nodes, self.pop.t, self.pop.host
        self.bg = self.host.min(axis=0)
        assert (self.host >= np.uint64(H)).all() and (self.bg >= np.uint64(H)).all()

    def cut(self):
        return as_u64(self.eng.vclock_stable_cut(self.t))

    def check(self, msg=""):
        np.testing.assert_array_equal(self.cut(), self.host.min(axis=0), err_msg=msg)


def _witnesses(nodes, k):
    """`nodes` distinct values < 2^63 (so below every background cell),
    rotated by k; one of them 2^63 - 1 and, from two nodes on, one of them 1."""
    v = (np.arange(nodes, dtype=np.uint64) + np.uint64(k)) % np.uint64(nodes)
    return np.where(v == 0, np.uint64(H - 1), v * np.uint64(0x9E3779B1) + np.uint64(1) - np.uint64(0x9E3779B1))


def _run_rounds(mp, sched):
    cols = np.arange(mp.nodes)
    for k, (name, rr, _) in enumerate(sched):
        vals = _witnesses(mp.nodes, k)
        assert (vals < np.uint64(H)).all() and len(np.unique(vals)) == mp.nodes
        saved = mp.host[rr, cols].copy()
        try:
            mp.pop.put(rr, cols, vals)
            np.testing.assert_array_equal(mp.cut(), vals, err_msg=f"witness round '{name}'")
        finally:
            mp.pop.put(rr, cols, saved)
        np.testing.assert_array_equal(mp.cut(), mp.bg, err_msg=f"after restoring round '{name}'")


def _extremes(mp):
    """A column whose minimum is 0 (one zero cell, in the last row), and one all 2^64 - 1."""
    t = mp.t
    keep = t[:, :2].clone()
    exp = mp.bg.copy()
    try:
        t[-1, 0] = 0
        exp[0] = 0
        if mp.nodes > 1:
            t[:, 1] = -1
            exp[1] = M64
        np.testing.assert_array_equal(mp.cut(), exp)
    finally:
        t[:, :2] = keep
    np.testing.assert_array_equal(mp.cut(), mp.bg)


@pytest.mark.parametrize("nodes", [2, 64, 128, 512])
def test_pow2_witnesses(eng, nodes):
    cus = _cus(eng)
    rows = pow2_rows(nodes, cus, BPC)
    g = fold_geometry(rows, nodes, cus, UNROLL, BPC)
    assert g.path == "pow2" and g.grid == cus * BPC
    assert g.full_steps >= 2 and g.rem_full >= 1 and g.rem_part > 0
    mp = MinPopulation(eng, rows, nodes)
    assert mp.t.data_ptr() % 16 == 0
    mp.check("background")
    _run_rounds(mp, witness_schedule(rows, nodes, special_rows(rows, g, shard_cuts(rows)), seed=nodes))
    _extremes(mp)


@pytest.mark.parametrize("case", ["3", "63", "1024", "64-misaligned"])
def test_generic_witnesses(eng, case):
    cus = _cus(eng)
    grid = 4 * cus
    nodes, rows = {"3": (3, 2 * grid + 5), "63": (63, 2 * grid + 5), "1024": (1024, grid + 1),
                   "64-misaligned": (64, 2 * grid + 5)}[case]
    mis = case.endswith("misaligned")
    mp = MinPopulation(eng, rows, nodes, misaligned=mis)
    if mis:                                               # contiguous, 8 bytes past a 16-byte boundary
        assert mp.t.is_contiguous() and mp.t.data_ptr() % 16 == 8
    g = fold_geometry(rows, nodes, cus, UNROLL, BPC, aligned=not mis)
    assert g.path == "generic" and g.grid == grid < rows
    assert g.full_steps >= 1 and g.rem_part > 0
    mp.check("background")
    _run_rounds(mp, witness_schedule(rows, nodes, special_rows(rows, g, shard_cuts(rows)), seed=nodes))
    _extremes(mp)


@pytest.mark.parametrize("nodes", [1, 3, 64, 1024])
def test_one_row_and_none(eng, nodes):
    row = np.random.default_rng(nodes).integers(0, M64, (1, nodes), dtype=np.uint64, endpoint=True)
    row[0, 0] = M64
    t = u64_tensor(row, eng.device)
    np.testing.assert_array_equal(as_u64(eng.vclock_stable_cut(t)), row[0])
    out = torch.full((nodes,), 0x5a, dtype=torch.int64, device=eng.device)
    with pytest.raises(_lib.CrdtError) as ei:             # no replica: no cut (it would be all-ones)
        eng.vclock_stable_cut(t[:0], out=out)
    assert ei.value.status == E_INVAL
    assert bool((out == 0x5a).all())
    if nodes == 1:
        with pytest.raises(_lib.CrdtError) as ei:         # nodes == 0, as the fold
            eng.vclock_stable_cut(t[:, :0].contiguous())
        assert ei.value.status == E_INVAL
    assert eng.device_status(clear=True) == 0


@pytest.mark.parametrize("members", [2, 3, 8])
def test_comm_stable_cut(eng, members):
    nodes, rows = 64, 1000 * members + 37
    host = np.random.default_rng(members).integers(0, M64, (rows, nodes), dtype=np.uint64, endpoint=True)
    host[:, 0] = M64                                      # a column all-ones, one with a zero, one >= 2^63
    host[rows // 2, 1] = 0
    host[:, 2] |= np.uint64(H)
    t = u64_tensor(host, eng.device)
    empty = members // 2                                  # that member holds no row
    bounds = [int(b) for b in np.linspace(0, rows, members)]      # members - 1 uneven pieces
    pieces = [t[bounds[j]:bounds[j + 1]] for j in range(members - 1)]
    shards = pieces[:empty] + [t[:0]] + pieces[empty:]
    assert shards[empty].shape[0] == 0 and sum(s.shape[0] for s in shards) == rows
    c = shard.Comm.loopback(0, members)
    try:
        torch.cuda.synchronize()
        outs = c.stable_cut(shards)
        assert len(outs) == members
        for i, o in enumerate(outs):
            np.testing.assert_array_equal(as_u64(o), host.min(axis=0), err_msg=f"member {i}")
        np.testing.assert_array_equal(as_u64(eng.vclock_stable_cut(t)), host.min(axis=0))
        with pytest.raises(ValueError):
            c.stable_cut([t[:0]] * members)
    finally:
        c.close()


def test_cut_feeds_the_compaction(eng):
    """Clocks over 64 nodes -> vclock_stable_cut -> set_compact of a synthetic state == numpy."""
    rows, nodes = 3000, 64
    clocks = np.random.default_rng(11).integers(2**19, 2**20, (rows, nodes), dtype=np.uint64)
    clocks[rows - 1, 5] = 0                               # node 5: some replica has seen nothing of it
    cut = as_u64(eng.vclock_stable_cut(u64_tensor(clocks, eng.device)))
    np.testing.assert_array_equal(cut, clocks.min(axis=0))
    t = tuple(np.ascontiguousarray(x) for x in synth.sort_tuples_np(*synth.set_tuples(2024, 0, 20000, 3000)))
    Td = TupleSet.from_numpy(*t, eng.device)
    empty = tuple(x[:0] for x in t)
    for lww in (True, False):
        m = (oracle.lww_merge if lww else oracle.orset_merge)(t, empty)
        key, ts, rep, tomb = m
        keep = ~((tomb == 1) & (rep < nodes) & (ts <= clocks.min(axis=0)[np.minimum(rep, nodes - 1)]))
        assert 0 < (~keep).sum() and (keep & (tomb == 1)).sum() > 0
        out, cnt = eng.set_compact(Td, lww, eng.vclock_stable_cut(u64_tensor(clocks, eng.device)))
        k = int(as_u64(cnt)[0])
        assert k == int(keep.sum())
        for g, e in zip(out.to_numpy(), m):
            np.testing.assert_array_equal(g[:k], e[keep])
    assert eng.device_status(clear=True) == 0
