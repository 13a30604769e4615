"""GPU: crdt_tuples_sort on inputs and outputs that start mid-allocation.

Every tensor test_gpu_sort.py passes is a fresh allocation (256-byte
aligned), so launch_minmax always takes k_sort_minmax<true>.  Here `in` is a
view 1..4 elements into a larger buffer (1, 3: key / ts off a 16-byte
boundary; 2: rep at 8 modulo 16; 4: aligned again), `out` a view at another
offset, and everything around both is a canary pattern extreme in every
field (tests/d2_util.py): a minmax or upsweep that reads one element outside
`in` changes the plan or pulls a canary into the output, a store outside
`out` lands on one.  Bit-exact against numpy's lexsort; the form and the
minmax variant of every case are checked in tests/test_d2_case_table.py."""
import numpy as np
import pytest
from knobs import set_knob

import d2_util as U

pytestmark = pytest.mark.gpu

KNOB_CASE = U.SORT_KNOB_CASE


@pytest.fixture(scope="module")
def expected():
    """numpy's lexsort of every input, once per (kind, n)."""
    return {(k, n): U.np_sorted(U.sort_input(k, n)) for k, n in {(c.kind, c.n) for c in U.SORT_CASES}}


def _run(eng, case, expected):
    t = case.tuples()
    IN, in_back = U.view_set(eng, t, case.off)
    OUT, out_back = U.out_set(eng, case.n, case.off_out)
    assert U.minmax_vec(IN) == case.mm_vec, "test setup: the view is not in the case's alignment class"
    got = eng.sort_tuples(IN, out=OUT).to_numpy()
    assert eng.device_status() == 0
    for g, e, f in zip(got, expected[case.kind, case.n], U.FIELDS):
        np.testing.assert_array_equal(g, e, err_msg=f)
    U.assert_canaries_intact(in_back, whole=True, what="in")
    U.assert_canaries_intact(out_back, what="out")


@pytest.mark.parametrize("case", U.SORT_CASES, ids=lambda c: c.id)
def test_sort_offset_views(eng, expected, case):
    _run(eng, case, expected)


@pytest.mark.diag
@pytest.mark.parametrize("knob,value,default", [("sort.xcd_tiles", 0, 1), ("sort.mm_blocks_per_cu", 16, 1)])
def test_sort_knob_variants_on_a_view(eng, expected, knob, value, default):
    """The scatter without the per-XCD tile ranges, and the minmax grid at 16
    workgroups per CU: the 12 289-tuple one-word sort on an offset view."""
    try:
        set_knob(knob, value)
        _run(eng, KNOB_CASE, expected)
    finally:
        set_knob(knob, default)
