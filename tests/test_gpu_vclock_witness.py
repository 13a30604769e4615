"""GPU: crdt_vclock_classify against populations in which every pair's class
hangs on one column (tests/lanegroup_util.py), == plain numpy on the host.

synth.vclock_pairs puts every b > a in the last column and never lets two
cells differ by more than one, so a kernel that reads ">= is violated" from
the last lane only, compares 32 bits or compares as signed passes every
parity test built on it (tests/test_lanegroup_witness_table.py).  Here each
(column, pair position) of a wave iteration carries a BEFORE-only and an
AFTER-only witness whose values differ in the high half only, across the
sign bit, or by 2^64 - 1; CONCURRENT pairs split over one 16-byte vector,
over the two halves of the row and over neighbouring columns; and EQUAL pairs
sit between witnesses.  The vector kernels (32 / 64 / 128 nodes), the generic
kernel (other node counts, and the vector widths on operands 8 bytes off a
16-byte boundary), ragged tails, a third grid-stride sweep and every
vclock.pairs_per_wave x vclock.blocks_per_cu shape run it.  Sizes come from
the device's CU count and the knobs in force, and each test asserts that its
shape still reaches the loop it is there for.

Every call writes into a view at an odd byte offset of a larger buffer: the
view is prefilled with 0xFF (no class), its surroundings with 0xAB, so an
entry the kernel never wrote, or wrote out of place, is seen.
"""
import numpy as np
import pytest
import torch
from knobs import set_knob

import lanegroup_util as L
from crdt_amd import _lib
from oracle import oracle

pytestmark = pytest.mark.gpu

PAD_FRONT, PAD_BACK = 13, 67                  # bytes of 0xAB around the output view; an odd offset
GENERIC_NODES = [1, 2, 3, 16, 63, 65, 100, 127, 129, 256, 513]


def _cus(eng) -> int:
    return torch.cuda.get_device_properties(eng.device).multi_processor_count


def _knobs():
    return _lib.get_option(b"vclock.pairs_per_wave"), _lib.get_option(b"vclock.blocks_per_cu")


def _geometry(eng, pairs, nodes, aligned=True) -> L.LaneGeometry:
    return L.vclock_geometry(pairs, nodes, _cus(eng), *_knobs(), aligned=aligned)


def _device(eng, host: np.ndarray, misaligned: bool = False) -> torch.Tensor:
    """host uint64 [pairs, nodes] on the device: a fresh allocation, or a
    contiguous view 8 bytes into one (fold_util.Population's trick)."""
    src = torch.from_numpy(host.view(np.int64))
    if not misaligned:
        t = src.to(eng.device)
        assert t.data_ptr() % 16 == 0
        return t
    flat = torch.empty(host.size + 2, dtype=torch.int64, device=eng.device)
    assert flat.data_ptr() % 16 == 0
    t = flat[1:1 + host.size].view(host.shape)
    t.copy_(src)
    assert t.is_contiguous() and t.data_ptr() % 16 == 8
    return t


def classify(eng, ta, tb) -> np.ndarray:
    """eng.vclock_classify into a canary-guarded view; the view's bytes."""
    pairs = ta.shape[0]
    buf = torch.full((PAD_FRONT + pairs + PAD_BACK,), 0xAB, dtype=torch.uint8, device=eng.device)
    view = buf[PAD_FRONT:PAD_FRONT + pairs]
    view.fill_(L.CANARY)
    assert pairs == 0 or view.data_ptr() % 2 == 1
    got = eng.vclock_classify(ta, tb, out=view)
    assert got.data_ptr() == view.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:PAD_FRONT] == 0xAB).all(), "bytes before cls were written"
    assert (host[PAD_FRONT + pairs:] == 0xAB).all(), "bytes after cls were written"
    return host[PAD_FRONT:PAD_FRONT + pairs]


def expect(got: np.ndarray, exp: np.ndarray, g: L.LaneGeometry, what: str) -> None:
    """Whole arrays; the first mismatch is named relative to the sweep boundaries."""
    assert got.shape == exp.shape
    bad = np.nonzero(got != exp)[0]
    if len(bad):
        p = int(bad[0])
        unwritten = int((got == L.CANARY).sum())
        pytest.fail(f"{what}: {len(bad)} of {len(exp)} pairs wrong ({unwritten} never written); first at "
                    f"{g.where(p)}: got {got[p]}, expected {exp[p]}")


class Pairs:
    """One population on the host and on the device, with its reference
    (numpy, checked against the oracle once) and aligned prefixes of it."""

    def __init__(self, eng, a: np.ndarray, b: np.ndarray):
        self.eng, self.a, self.b = eng, a, b
        self.exp = L.classify_ref(a, b)
        np.testing.assert_array_equal(oracle.vclock_classify(a, b, threads=8), self.exp, err_msg="oracle vs numpy")
        self.ta, self.tb = _device(eng, a), _device(eng, b)
        self.pairs, self.nodes = a.shape

    def run(self, pairs=None, what="") -> None:
        pairs = self.pairs if pairs is None else pairs
        assert pairs <= self.pairs
        ta, tb = self.ta[:pairs], self.tb[:pairs]
        assert ta.is_contiguous() and ta.data_ptr() % 16 == 0 and tb.data_ptr() % 16 == 0
        g = _geometry(self.eng, pairs, self.nodes)
        expect(classify(self.eng, ta, tb), self.exp[:pairs], g, f"{what} nodes {self.nodes}, pairs {pairs}")


@pytest.fixture(scope="module")
def witness(eng):
    """The single-witness population of each node count, shared by the tests of this module."""
    cache = {}

    def get(nodes) -> Pairs:
        if nodes not in cache:
            cache[nodes] = Pairs(eng, *L.witness_pairs(nodes, L.witness_slots(nodes), seed=nodes))
        return cache[nodes]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def dense(eng):
    """The dense random-class population of each node count, regenerated
    larger when a test (a knob variant with a longer sweep) needs more pairs."""
    cache = {}

    def get(nodes, pairs) -> Pairs:
        if nodes not in cache or cache[nodes].pairs < pairs:
            cache.pop(nodes, None)
            cache[nodes] = Pairs(eng, *L.dense_pairs(nodes, pairs, seed=1000 + nodes))
        return cache[nodes]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 1. the vector kernels
@pytest.mark.parametrize("nodes", [32, 64, 128])
def test_vector_kernel_single_witness(eng, witness, nodes):
    pop = witness(nodes)
    g = _geometry(eng, pop.pairs, nodes)
    assert g.kernel == "vector" and L.witness_slots(nodes) == g.rows_per_load * 32 >= g.rows_per_iter
    assert pop.pairs % 4 == 3 and (nodes == 128 or pop.pairs % g.rows_per_load != 0)      # a ragged last wave-load
    assert (np.bincount(pop.exp, minlength=4) > 0).all()
    pop.run(what="single witness")
    expect(classify(eng, pop.tb, pop.ta), L.SWAP[pop.exp], g, f"classify(b, a), nodes {nodes}")


# ---------------------------------------------------------------- 2. the generic kernel
@pytest.mark.parametrize("nodes", GENERIC_NODES)
def test_generic_kernel_single_witness(eng, witness, nodes):
    """A short row, exactly one 64-lane stride, a stride plus one, several
    strides with a ragged end, and a vector width (16) that has no kernel."""
    pop = witness(nodes)
    g = _geometry(eng, pop.pairs, nodes)
    assert g.kernel == "generic" and g.rows_per_iter == 1
    assert (np.bincount(pop.exp, minlength=4)[:3] > 0).all() and ((pop.exp == L.CONCURRENT).any() or nodes == 1)
    pop.run(what="single witness")
    expect(classify(eng, pop.tb, pop.ta), L.SWAP[pop.exp], g, f"classify(b, a), nodes {nodes}")


@pytest.mark.parametrize("which", ["a", "b", "both"])
@pytest.mark.parametrize("nodes", [32, 64, 128])
def test_misaligned_operand_takes_the_generic_kernel(eng, witness, nodes, which):
    """a, b or both start 8 bytes into a 16-byte-aligned allocation: vec ==
    false, the generic kernel at a vector width."""
    pop = witness(nodes)
    ta = _device(eng, pop.a, misaligned=True) if which in ("a", "both") else pop.ta
    tb = _device(eng, pop.b, misaligned=True) if which in ("b", "both") else pop.tb
    assert (ta.data_ptr() % 16 == 8) == (which in ("a", "both")) and (tb.data_ptr() % 16 == 8) == (which in ("b", "both"))
    assert ta.data_ptr() % 16 in (0, 8) and tb.data_ptr() % 16 in (0, 8)
    g = _geometry(eng, pop.pairs, nodes, aligned=False)
    assert g.kernel == "generic"
    expect(classify(eng, ta, tb), pop.exp, g, f"misaligned {which}, nodes {nodes}")


# ---------------------------------------------------------------- 3. tails and sweeps
def _tail_sizes(g: L.LaneGeometry):
    """1, PPW - 1, PPW, PPW + 1 and every remainder modulo the pairs of a
    wave-load, after one and after three whole iterations of a wave."""
    ppw, ppl = g.rows_per_iter, g.rows_per_load
    sizes = {1, ppw - 1, ppw, ppw + 1}
    for base in (ppw, 3 * ppw):
        sizes |= {base + r for r in range(ppl)}
    sizes |= {2 * ppl + r for r in range(ppl)}
    return sorted(s for s in sizes if s > 0)


def _run_tails(eng, dense, nodes):
    g = _geometry(eng, 1, nodes)
    sizes = _tail_sizes(g)
    assert {s % g.rows_per_load for s in sizes} == set(range(g.rows_per_load))
    assert {1, g.rows_per_iter, g.rows_per_iter + 1} <= set(sizes)
    pop = dense(nodes, max(sizes))
    for pairs in sizes:
        pop.run(pairs, what="tail")


def _run_sweeps(eng, dense, nodes):
    pairs = L.sweep_rows(_geometry(eng, 1, nodes))
    g = _geometry(eng, pairs, nodes)
    L.assert_sweeps(g)                                    # 2 full sweeps, 3 wave-loads and 1 pair
    assert pairs == 2 * g.sweep + 3 * g.rows_per_load + 1 and g.waves == 4 * _cus(eng) * _knobs()[1]
    pop = dense(nodes, pairs)
    exp = pop.exp[:pairs]
    # a sweep that repeated the one before it would be wrong on most pairs
    assert (exp[g.sweep:] != exp[:-g.sweep]).mean() > 0.5
    pop.run(pairs, what="sweeps")


@pytest.mark.parametrize("nodes", [32, 64, 128])
def test_vector_kernel_tails(eng, dense, nodes):
    assert _geometry(eng, 1, nodes).kernel == "vector"
    _run_tails(eng, dense, nodes)


@pytest.mark.parametrize("nodes", [128, 32, 3])
def test_third_sweep_of_the_grid(eng, dense, nodes):
    """pairs = 2 sweeps + 3 wave-loads + 1: every wave runs its loop twice,
    the first waves a third time, and the last wave-load is ragged."""
    assert _geometry(eng, 1, nodes).kernel == ("generic" if nodes == 3 else "vector")
    _run_sweeps(eng, dense, nodes)


# ---------------------------------------------------------------- 4. degenerate calls
@pytest.mark.parametrize("nodes", [128, 32, 65])
def test_same_tensor_on_both_sides_is_equal(eng, witness, nodes):
    pop = witness(nodes)
    got = classify(eng, pop.ta, pop.ta)
    expect(got, np.zeros(pop.pairs, np.uint8), _geometry(eng, pop.pairs, nodes), f"classify(a, a), nodes {nodes}")


@pytest.mark.parametrize("nodes", [128, 3])
def test_no_pairs_writes_nothing(eng, nodes):
    ta = torch.empty(0, nodes, dtype=torch.int64, device=eng.device)
    assert classify(eng, ta, ta.clone()).size == 0        # and the 0xAB on either side is intact


# ---------------------------------------------------------------- 5. knob variants
@pytest.mark.diag
@pytest.mark.parametrize("blocks_per_cu", [1, 2])
@pytest.mark.parametrize("pairs_per_wave", L.VCLOCK_UNROLLS)
def test_knob_variant(eng, witness, dense, pairs_per_wave, blocks_per_cu):
    """Every k_vclock<NODES, U> launch_vc instantiates (4 through its
    default arm) at one and two blocks per CU: the single-witness population,
    the tails and a third sweep, sized for the knobs in force."""
    before = _knobs()
    try:
        set_knob("vclock.pairs_per_wave", pairs_per_wave)
        set_knob("vclock.blocks_per_cu", blocks_per_cu)
        assert _knobs() == (pairs_per_wave, blocks_per_cu)
        for nodes in (128, 32):
            g = _geometry(eng, 1 << 30, nodes)
            assert g.kernel == "vector" and g.rows_per_iter == g.rows_per_load * pairs_per_wave
            assert g.sweep == _cus(eng) * blocks_per_cu * 4 * g.rows_per_iter
            witness(nodes).run(what=f"U={pairs_per_wave} bpc={blocks_per_cu} single witness")
            _run_tails(eng, dense, nodes)
            _run_sweeps(eng, dense, nodes)
    finally:
        set_knob("vclock.pairs_per_wave", before[0])
        set_knob("vclock.blocks_per_cu", before[1])
