"""GPU: the row sums behind crdt_gcounter_value / crdt_pncounter_value
(k_rowsum<NODES>, k_rowsum_generic) and the ordered-int64 maps, at the shapes
where a lane-group kernel goes wrong, == plain numpy on the host.

The inputs are full-range random uint64 (not synth.counters, whose cells are
mostly below 2^20): dropping a column, or half of one, changes the wrapped
sum.  Every vector width runs every remainder of rows modulo the rows of a
wave-load and a third grid-stride sweep; the generic kernel runs short,
one-stride, ragged and long rows, a third sweep, and the vector widths on
operands 8 bytes off a 16-byte boundary.  Row counts come from the device's
CU count (tests/lanegroup_util.py) and each test asserts the loop it is there
for is reached.  Every call writes into a view inside a buffer prefilled with
a value the reference does not produce, so an entry never written, or one
written outside the view, is seen.
"""
import numpy as np
import pytest
import torch

import lanegroup_util as L
from crdt_amd.engine import as_u64
from oracle import oracle

pytestmark = pytest.mark.gpu

FILL = 0x5AA5_C33C_0FF0_9669                  # the canary; asserted absent from every reference
PAD = 5                                       # int64 entries of canary on either side of the view
EDGE = np.array([0, 1, 2**63 - 1, 2**63, 2**64 - 2, 2**64 - 1], dtype=np.uint64)
FORMS = ["gcounter", "pncounter"]


def _cus(eng) -> int:
    return torch.cuda.get_device_properties(eng.device).multi_processor_count


def _device(eng, host: np.ndarray, misaligned: bool = False) -> torch.Tensor:
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


def _guarded(eng, n: int):
    buf = torch.full((PAD + n + PAD,), FILL, dtype=torch.int64, device=eng.device)
    return buf, buf[PAD:PAD + n]


def _unguard(buf, n: int, what: str) -> np.ndarray:
    host = buf.cpu().numpy()
    assert (host[:PAD] == FILL).all(), f"{what}: entries before out were written"
    assert (host[PAD + n:] == FILL).all(), f"{what}: entries after out were written"
    return host[PAD:PAD + n]


def value(eng, form: str, tp, tn, rows: int = None) -> np.ndarray:
    """crdt_gcounter_value(p) or crdt_pncounter_value(p, n) on the first `rows` rows, through eng._call."""
    rows = tp.shape[0] if rows is None else rows
    nodes = tp.shape[1]
    buf, view = _guarded(eng, rows)
    if form == "gcounter":
        eng._call("crdt_gcounter_value", tp.data_ptr(), rows, nodes, view.data_ptr())
    else:
        eng._call("crdt_pncounter_value", tp.data_ptr(), tn.data_ptr(), view.data_ptr(), rows, nodes)
    return _unguard(buf, rows, f"{form}, rows {rows}, nodes {nodes}")


def expect(got: np.ndarray, exp: np.ndarray, g: L.LaneGeometry, what: str) -> None:
    assert exp.dtype == np.int64 and got.shape == exp.shape
    assert (exp != FILL).all(), "the canary is a value of the reference: pick another"
    bad = np.nonzero(got != exp)[0]
    if len(bad):
        r = int(bad[0])
        pytest.fail(f"{what}: {len(bad)} of {len(exp)} rows wrong ({int((got == FILL).sum())} never written); "
                    f"first at {g.where(r)}: got {got[r]}, expected {exp[r]}")


class Counters:
    """Full-range random P and N [rows, nodes] on the host and the device,
    and both references (numpy; the PN one checked against the oracle once)."""

    def __init__(self, eng, rows: int, nodes: int, misalign=()):
        rng = np.random.default_rng(7919 * nodes + rows)
        self.eng, self.rows, self.nodes = eng, rows, nodes
        self.p = rng.integers(0, 2**64, size=(rows, nodes), dtype=np.uint64)
        self.n = rng.integers(0, 2**64, size=(rows, nodes), dtype=np.uint64)
        assert (self.p >= np.uint64(2**63)).any() and (self.p >> np.uint64(32)).any()
        self.aligned = not misalign
        self.tp = _device(eng, self.p, "p" in misalign)
        self.tn = _device(eng, self.n, "n" in misalign)
        self.exp = {"gcounter": L.rowsum_ref(self.p), "pncounter": L.rowsum_ref(self.p, self.n)}
        np.testing.assert_array_equal(oracle.pncounter_value(self.p, self.n), self.exp["pncounter"],
                                      err_msg="oracle vs numpy")

    def geometry(self, form: str, rows: int = None) -> L.LaneGeometry:
        # the G form never looks at N: only P's alignment picks its kernel
        aligned = self.tp.data_ptr() % 16 == 0 and (form == "gcounter" or self.tn.data_ptr() % 16 == 0)
        return L.rowsum_geometry(self.rows if rows is None else rows, self.nodes, _cus(self.eng), aligned)

    def run(self, form: str, rows: int = None, what: str = "") -> None:
        rows = self.rows if rows is None else rows
        got = value(self.eng, form, self.tp, self.tn, rows)
        expect(got, self.exp[form][:rows], self.geometry(form, rows), f"{what} {form}, rows {rows}, nodes {self.nodes}")


@pytest.fixture(scope="module")
def counters(eng):
    cache = {}

    def get(rows, nodes, misalign=()) -> Counters:
        key = (rows, nodes, tuple(misalign))
        if key not in cache:
            cache[key] = Counters(eng, rows, nodes, misalign)
        return cache[key]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 1. vector widths
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nodes", [16, 32, 64, 128])
def test_vector_rowsum_every_remainder(eng, counters, nodes, form):
    """rows = 1 .. two wave-loads + 1, and every remainder around the rows one block holds."""
    rpl = 64 // (nodes // 2)
    sizes = sorted(set(range(1, 2 * rpl + 2)) | {4 * rpl + r for r in range(-1, rpl + 1)})
    assert {s % rpl for s in sizes} == set(range(rpl))
    c = counters(max(sizes), nodes)
    for rows in sizes:
        g = c.geometry(form, rows)
        assert g.kernel == "vector" and g.rows_per_load == rpl
        c.run(form, rows, what="remainder")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nodes", [16, 32, 64, 128])
def test_vector_rowsum_third_sweep(eng, counters, nodes, form):
    rows = L.sweep_rows(L.rowsum_geometry(1, nodes, _cus(eng)))
    c = counters(rows, nodes)
    g = c.geometry(form)
    assert g.kernel == "vector" and g.cap == 8 * _cus(eng)
    L.assert_sweeps(g)                                    # 2 full sweeps, 3 wave-loads and 1 row
    c.run(form, what="sweeps")


# ---------------------------------------------------------------- 2. the generic kernel
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nodes", [1, 5, 63, 65, 200, 1024])
def test_generic_rowsum(eng, counters, nodes, form):
    """Short rows, one 64-lane stride less one and plus one, ragged and whole
    multiples of the stride; at 5 nodes a third sweep of the grid."""
    rows = L.sweep_rows(L.rowsum_geometry(1, nodes, _cus(eng))) if nodes == 5 else 259
    c = counters(rows, nodes)
    g = c.geometry(form)
    assert g.kernel == "generic" and g.rows_per_iter == 1
    if nodes == 5:
        L.assert_sweeps(g)
    c.run(form, what="generic")
    c.run(form, 1, what="generic")


@pytest.mark.parametrize("case", ["gcounter-p", "pncounter-p", "pncounter-n", "pncounter-pn"])
@pytest.mark.parametrize("nodes", [64, 128])
def test_misaligned_rowsum_takes_the_generic_kernel(eng, counters, nodes, case):
    form, mis = case.split("-")
    c = counters(259, nodes, tuple(mis))
    assert (c.tp.data_ptr() % 16 == 8) == ("p" in mis) and (c.tn.data_ptr() % 16 == 8) == ("n" in mis)
    assert c.geometry(form).kernel == "generic"
    c.run(form, what=f"misaligned {mis}")


# ---------------------------------------------------------------- 3. wrap and sign
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nodes", [128, 16, 5])
def test_rowsum_wraps_and_goes_negative(eng, nodes, form):
    """Rows of all 2^64 - 1 (the G sum wraps to -nodes as int64); rows with
    sum(p) < sum(n), whose int64 value is negative and equals the wrapped
    numpy difference; rows of EDGE values against zero and against each other."""
    rng = np.random.default_rng(nodes)
    rows = 37
    p = rng.integers(0, 2**64, size=(rows, nodes), dtype=np.uint64)
    n = rng.integers(0, 2**64, size=(rows, nodes), dtype=np.uint64)
    p[0:4], n[0:4] = np.uint64(L.U64_MAX), np.array([[0], [1], [L.U64_MAX], [2**63]], dtype=np.uint64)
    p[4:8] = rng.integers(0, 2**40, size=(4, nodes), dtype=np.uint64)          # sum(p) < sum(n), no wrap in either
    n[4:8] = p[4:8] + rng.integers(1, 2**20, size=(4, nodes), dtype=np.uint64)
    p[8:14], n[8:14] = EDGE[:, None], 0
    p[14:20], n[14:20] = 0, EDGE[:, None]
    p[20:26], n[20:26] = EDGE[:, None], EDGE[::-1, None]
    exp_g, exp_pn = L.rowsum_ref(p), L.rowsum_ref(p, n)
    assert (exp_g[0:4] == -nodes).all() and exp_pn[0] == -nodes and exp_pn[2] == 0
    assert (exp_pn[4:8] < 0).all() and (exp_pn[4:8] > -(2**30)).all()
    assert [int(v) for v in exp_pn[4:8]] == [int(a) - int(b) for a, b in zip(p[4:8].astype(object).sum(1), n[4:8].astype(object).sum(1))]
    np.testing.assert_array_equal(oracle.pncounter_value(p, n), exp_pn)
    tp, tn = _device(eng, p), _device(eng, n)
    g = L.rowsum_geometry(rows, nodes, _cus(eng))
    assert g.kernel == ("generic" if nodes == 5 else "vector")
    expect(value(eng, form, tp, tn), exp_g if form == "gcounter" else exp_pn, g, f"wrap and sign, {form}, nodes {nodes}")


def test_engine_wrappers_agree(eng, counters):
    """eng.gcounter_value / eng.pncounter_value (fresh outputs) == the guarded calls' reference."""
    c = counters(259, 64)
    np.testing.assert_array_equal(eng.gcounter_value(c.tp).cpu().numpy(), c.exp["gcounter"])
    np.testing.assert_array_equal(eng.pncounter_value(c.tp, c.tn).cpu().numpy(), c.exp["pncounter"])


# ---------------------------------------------------------------- 4. ordered maps
def test_ordered_maps_third_sweep(eng):
    """n = 2 x 4096 x 256 + 3: two sweeps of the capped grid and a tail.  The
    six EDGE values sit on both sides of each sweep boundary; the forward map
    == x ^ 2^63 as int64, its signed order is the unsigned order, and the
    round trip is exact.  Both outputs are guarded views."""
    n = 2 * L.ORDER_MAP_CAP * 256 + 3
    sweep = L.order_map_sweep(n)
    assert sweep == L.ORDER_MAP_CAP * 256 and n // sweep == 2 and n % sweep == 3
    rng = np.random.default_rng(64)
    x = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    idx = []
    for cut in (sweep, 2 * sweep):
        after = min(6, n - cut)                           # the tail holds three elements
        x[cut - 6:cut] = EDGE
        x[cut:cut + after] = EDGE[::-1][:after]
        idx += list(range(cut - 6, cut + after))
    x[0], x[n - 1] = np.uint64(2**63), np.uint64(2**63 - 1)
    idx = np.array(idx + [0, n - 1])
    assert set(x[idx]) == set(EDGE) and len(idx) == 12 + 9 + 2
    exp = (x ^ np.uint64(2**63)).view(np.int64)
    assert (exp != FILL).all() and (x.view(np.int64) != FILL).all()
    tx = torch.from_numpy(x.view(np.int64)).to(eng.device)

    buf, view = _guarded(eng, n)
    assert eng.u64_to_ordered_i64(tx, out=view).data_ptr() == view.data_ptr()
    y = _unguard(buf, n, "u64_to_ordered_i64")
    bad = np.nonzero(y != exp)[0]
    assert not len(bad), f"{len(bad)} wrong, first at {bad[0]} = sweep {bad[0] // sweep} + {bad[0] % sweep}"
    ux, sy = x[idx], y[idx]
    np.testing.assert_array_equal(ux[:, None] < ux[None, :], sy[:, None] < sy[None, :])
    ty = view.clone()

    buf, view = _guarded(eng, n)
    assert eng.ordered_i64_to_u64(ty, out=view).data_ptr() == view.data_ptr()
    back = _unguard(buf, n, "ordered_i64_to_u64")
    bad = np.nonzero(back.view(np.uint64) != x)[0]
    assert not len(bad), f"round trip: {len(bad)} wrong, first at {bad[0]} = sweep {bad[0] // sweep} + {bad[0] % sweep}"
    np.testing.assert_array_equal(as_u64(eng.ordered_i64_to_u64(eng.u64_to_ordered_i64(tx[:1006]))), x[:1006])
