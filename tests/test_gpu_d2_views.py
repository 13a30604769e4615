"""GPU: the fused D2 merges (crdt_{lww,orset}_merge_unsorted and their planned
forms) across host predicate x form, on sides and outputs that start
mid-allocation.

sort.hip picks its kernel chain from the plan's form and from d2_vec (key /
ts 16-, rep 8-, tomb 2-byte aligned, an even na); the rest of the suite
passes fresh, even-length allocations, so the non-vector chains -- the
scalar k_sort_minmax, the scalar composing upsweep reading p.in2, k_lww_table
behind one radix pass, two passes + k_chunk_bounds + k_or_chunk -- run only
by accident there.  Here every form (tests/d2_util.py's generators) runs in
every alignment class, the sides and `out` being views inside buffers of a
canary pattern extreme in every field: a read outside a side moves the plan
or surfaces in the output, a store outside `out` lands on a canary.

Expected: the oracle's merge of the numpy-lexsorted host sides, bit for bit
in all four fields and the count -- test_gpu_merge_unsorted.py's
expectation.  tests/test_d2_case_table.py checks without a GPU that every
case here takes the form and predicate class it is named for; the drift
guard below ties plan_shape to the device's k_sort_plan."""
import numpy as np
import pytest
import torch
from knobs import set_knob

import d2_util as U
from crdt_amd.engine import TupleSet, as_u64
from oracle import oracle

pytestmark = pytest.mark.gpu

REF = {"lww": oracle.lww_merge, "orset": oracle.orset_merge}
KNOB_CASES = U.D2_KNOB_CASES


@pytest.fixture(scope="module")
def expect():
    """The oracle's merge of one (mode, A, B), computed once and shared."""
    memo = {}

    def get(key, mode, a, b):
        if (key, mode) not in memo:
            memo[key, mode] = REF[mode](U.np_sorted(a), U.np_sorted(b))
        return memo[key, mode]
    return get


def _same(got, exp, what=""):
    assert len(got[0]) == len(exp[0]), f"{what} count"
    for g, e, f in zip(got, exp, U.FIELDS):
        np.testing.assert_array_equal(g, e, err_msg=f"{what} {f}")


def _merge(eng, case, expect):
    """The case's merge on its views == the oracle; canaries and inputs intact.  Returns the output."""
    a, b = case.sides()
    A, a_back = U.view_set(eng, a, case.off_a)
    B, b_back = U.view_set(eng, b, case.off_b)
    OUT, out_back = U.out_set(eng, case.na + case.nb, case.off_out)
    assert U.is_vec(A, B) == case.vec and U.minmax_vec(A, B) == case.mm_vec, \
        "test setup: the views are not in the case's alignment class"
    fn = eng.lww_merge_unsorted if case.mode == "lww" else eng.orset_merge_unsorted
    got = fn(A, B, out=OUT).to_numpy()
    assert eng.device_status() == 0
    _same(got, expect((case.gen, case.na, case.nb), case.mode, a, b), case.id)
    U.assert_canaries_intact(a_back, whole=True, what="a")
    U.assert_canaries_intact(b_back, whole=True, what="b")
    U.assert_canaries_intact(out_back, what="out")
    return got


@pytest.mark.parametrize("case", U.D2_CASES, ids=lambda c: c.id)
def test_d2_views(eng, expect, case):
    _merge(eng, case, expect)


@pytest.mark.parametrize("mode", U.MODE_NAMES)
@pytest.mark.parametrize("gen", list(U.GENS))
def test_plan_shape_matches_the_device_plan(eng, gen, mode):
    """Drift guard: d2_util.plan_shape == k_sort_plan's exact plan, read out
    of crdt_set_merge_plan's blob -- on fresh allocations (the vector minmax)
    and on views at (3, 5) inside canaries (the scalar one: a partial that
    took in one element outside a view changes the widths)."""
    a, b = U.gen_sides(gen)
    exp = U.plan_shape(a, b, mode)
    assert U.form_of(exp, mode) == U.FORMS[gen, mode]
    lww = mode == "lww"
    A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
    VA, _ = U.view_set(eng, a, 3)
    VB, _ = U.view_set(eng, b, 5)
    assert U.minmax_vec(A, B) and not U.minmax_vec(VA, VB), "test setup: alignment"
    for X, Y in ((A, B), (VA, VB)):
        got = U.blob_shape(eng.set_merge_plan(lww, X, Y, widen=False))
        assert got == (0 if lww else 1, len(a[0]), len(b[0]), exp)
    wide = U.blob_shape(eng.set_merge_plan(lww, VA, VB, widen=True))[3]
    assert wide == U.plan_shape(a, b, mode, widen=True)
    assert eng.device_status() == 0


@pytest.mark.parametrize("case", U.PLANNED_CASES, ids=lambda c: c.id)
def test_planned_on_inputs_aligned_unlike_the_plans(eng, expect, case):
    """d2_vec comes from each call's inputs, not from the plan: a plan made
    on fresh allocations (even na: the vector chain; odd na: the scalar one),
    run on them and then on views at offsets (1, 3) holding a permutation of
    the data with fresh tombs -- the scalar chain under a plan whose passes
    check every tuple against it (the upsweep's range word)."""
    lww = case.mode == "lww"
    a, b = case.sides()
    fa, fb = case.fresh_sides()
    na, nb = len(a[0]), len(b[0])
    A, B = TupleSet.from_numpy(*a, eng.device), TupleSet.from_numpy(*b, eng.device)
    VA, va_back = U.view_set(eng, fa, U.PLANNED_OFFS[0])
    VB, vb_back = U.view_set(eng, fb, U.PLANNED_OFFS[1])
    assert U.is_vec(A, B) == (not case.odd) and not U.is_vec(VA, VB), "test setup: alignment"
    plan = eng.set_merge_plan(lww, A, B, widen=True)
    shape = U.blob_shape(plan)[3]
    assert shape == U.plan_shape(a, b, case.mode, widen=True) and U.form_of(shape, case.mode) == case.form
    OUT, out_back = U.out_set(eng, na + nb, 3)
    cnt = torch.zeros(1, dtype=torch.int64, device=eng.device)
    runs = ((A, B, expect((case.gen, na, nb), case.mode, a, b), "aligned"),
            (VA, VB, expect((case.gen, na, nb, "fresh"), case.mode, fa, fb), "views"))
    for X, Y, exp, what in runs:
        cnt.fill_(-7)
        eng.merge_unsorted_planned(lww, plan, X, Y, OUT, cnt)
        torch.cuda.synchronize()
        assert eng.device_status() == 0, what
        n = int(as_u64(cnt)[0])
        assert n != 2**64 - 1 and n == len(exp[0]), what
        _same(OUT.slice(n).to_numpy(), exp, what)
        U.assert_canaries_intact(out_back, what=f"out ({what})")
    U.assert_canaries_intact(va_back, whole=True, what="a")
    U.assert_canaries_intact(vb_back, whole=True, what="b")


KNOBS = [("sort.vec_up", 0, 1), ("sort.xcd_tiles", 0, 1), ("sort.mm_blocks_per_cu", 2, 1),
         ("sort.mm_blocks_per_cu", 16, 1)]


@pytest.mark.diag
@pytest.mark.parametrize("case", KNOB_CASES, ids=lambda c: c.id)
@pytest.mark.parametrize("knob,value,default", KNOBS)
def test_d2_sort_knob_variants(eng, expect, knob, value, default, case):
    """sort.vec_up = 0 (aligned inputs forced down the scalar chain),
    sort.xcd_tiles = 0 and sort.mm_blocks_per_cu = 2 / 16 on an aligned
    even-na and an offset case: == the default's result and the oracle."""
    base = _merge(eng, case, expect)
    try:
        set_knob(knob, value)
        got = _merge(eng, case, expect)
    finally:
        set_knob(knob, default)
    _same(got, base, "against the default")
