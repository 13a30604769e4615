"""The case table of the sort / D2 view tests (tests/d2_util.py), checked
without a GPU: every case test_gpu_sort_views.py and test_gpu_d2_views.py
run takes the form it is named for (plan_shape, the numpy restatement of
k_sort_plan) and sits in the predicate class it is named for (is_vec /
minmax_vec on 256-byte-aligned base addresses plus the case's offsets).  A
generator or size change that moves a case onto another kernel chain fails
here, not silently on the GPU."""
import numpy as np
import pytest

import d2_util as U

ALL_FORMS = {"lww_table_u32", "lww_table_u64", "or_chunks", "radix_1w", "radix_2w", "radix_3w"}
CLASSES = {"vec_0_0", "vec_4_4", "vec_mm_scalar_2_2", "odd_na_0_0", "off_1_0", "off_0_1", "off_3_5"}


def _sides(case):
    return U.fake_set(case.na, case.off_a, base=0x7F0000000000), U.fake_set(case.nb, case.off_b, base=0x7F1000000000)


@pytest.mark.parametrize("kbits,tbits,lww,orset", [
    (11, 20, "radix_1w", "radix_1w"), (12, 20, "lww_table_u32", "radix_1w"), (16, 20, "lww_table_u32", "or_chunks"),
    (23, 20, "lww_table_u32", "or_chunks"), (24, 20, "radix_1w", "or_chunks"), (25, 20, "radix_1w", "or_chunks"),
    (26, 20, "radix_1w", "radix_1w"), (20, 23, "lww_table_u32", "or_chunks"), (20, 24, "lww_table_u64", "or_chunks"),
    (16, 40, "lww_table_u64", "or_chunks"), (22, 34, "lww_table_u64", "or_chunks"), (23, 33, "radix_1w", "or_chunks"),
    (17, 40, "radix_2w", "radix_2w")])
def test_plan_shape_thresholds(kbits, tbits, lww, orset):
    """The limits of the dense-key forms: LWW tables at 12..23 key bits with
    tags (and marker) of <= 32 bits, 12..22 with wider ones; OR-Set chunks at
    16..25 key bits; both on one-word composites only."""
    rng = np.random.default_rng(kbits)
    a = U._fields(rng, 1000, kbits, tbits, 6)
    b = U._fields(rng, 900, kbits, tbits, 6)
    words = (kbits + tbits + 6 + 2 + 63) // 64
    assert U.form_of(U.plan_shape(a, b, "lww"), "lww") == lww
    assert U.form_of(U.plan_shape(a, b, "orset"), "orset") == orset
    assert U.form_of(U.plan_shape(a, b, "lww", lww_table=0), "lww") == f"radix_{words}w"
    assert U.form_of(U.plan_shape(a, b, "orset", or_table=0), "orset") == f"radix_{words}w"


def test_plan_shape_config_d_and_chunk_density():
    """Config D's fields: 23 + 20 + 6 + 2 = 51 bits; LWW one pass on the
    key's top byte and 15-bit u32 tables, OR-Set two passes and 2^9-key
    chunks; key bits + one more digit without the chunks (4 passes); more
    than 1280 tuples per chunk on average keeps OR-Set off its chunks."""
    rng = np.random.default_rng(1)
    a, b = U._fields(rng, 700, 23, 20, 6), U._fields(rng, 700, 23, 20, 6)
    assert U.plan_shape(a, b, "lww") == U.Shape(23, 20, 6, 2, 51, 1, 43, 1, 15, 4)
    assert U.plan_shape(a, b, "orset") == U.Shape(23, 20, 6, 2, 51, 1, 35, 2, 9, 4)
    assert U.plan_shape(a, b, "orset", or_table=0) == U.Shape(23, 20, 6, 2, 51, 1, 19, 4, 0, 0)
    assert U.plan_shape(a, b, "orset", key_only=0, or_table=0) == U.Shape(23, 20, 6, 2, 51, 1, 0, 7, 0, 0)
    assert U.plan_shape(a, None, "sort") == U.Shape(23, 20, 6, 1, 50, 1, 0, 7, 0, 0)
    c, d = U._fields(rng, 1280 * 128, 16, 20, 6), U._fields(rng, 2, 16, 20, 6)
    assert U.form_of(U.plan_shape(c, U.cut(d, 0), "orset"), "orset") == "or_chunks"
    assert U.form_of(U.plan_shape(c, U.cut(d, 1), "orset"), "orset") == "radix_1w"
    one = tuple(x[:1] for x in a)
    assert U.plan_shape(one, None, "sort") == U.Shape(0, 0, 0, 1, 1, 1, 0, 1, 0, 0)


def test_predicates_clause_by_clause():
    n = 1000
    al = U.fake_set(n, 0)
    assert U.is_vec(al, al) and U.minmax_vec(al, al)
    assert not U.is_vec(al, al, vec_up=0)
    assert not U.is_vec(U.fake_set(n + 1, 0), al) and U.is_vec(al, U.fake_set(n + 1, 0))      # only na's parity
    for offs, vec, mm in (((1, 0, 0, 0), False, False), ((0, 1, 0, 0), False, False), ((2, 2, 0, 0), True, True),
                          ((0, 0, 1, 0), False, False), ((0, 0, 2, 0), True, False), ((0, 0, 4, 0), True, True),
                          ((0, 0, 0, 1), False, True), ((0, 0, 0, 2), True, True)):
        for A, B in ((U.fake_set(n, offs), al), (al, U.fake_set(n, offs))):
            assert U.is_vec(A, B) == vec, offs
            assert U.minmax_vec(A, B) == mm, offs
    bad = U.fake_set(0, 1)                                   # an empty side's pointers do not count
    assert U.is_vec(bad, al) and U.is_vec(al, bad) and U.minmax_vec(bad, al) and U.minmax_vec(al, bad)
    assert U.minmax_vec(al) and not U.minmax_vec(U.fake_set(n, 2))


@pytest.mark.parametrize("case", U.D2_CASES, ids=lambda c: c.id)
def test_d2_case_takes_its_form_and_class(case):
    a, b = case.sides()
    assert len(a[0]) == case.na and len(b[0]) == case.nb and 0 < case.na + case.nb <= 25_000
    assert U.form_of(U.plan_shape(a, b, case.mode), case.mode) == case.form
    A, B = _sides(case)
    assert U.is_vec(A, B) == case.vec
    assert U.minmax_vec(A, B) == case.mm_vec
    assert case.off_out in (1, 3)
    if case.cls.startswith("vec_"):
        assert case.na % 2 == 0 and case.vec
    if case.cls == "odd_na_0_0":                             # the parity clause alone
        assert case.na % 2 == 1 and U.is_vec(U.fake_set(case.na + 1, 0), B)
    if case.cls.startswith("only_"):                         # exactly one clause of d2_vec
        assert case.na % 2 == 0
        assert sum(1 for off in (case.off_a, case.off_b) for x in U._offs4(off) if x) == 1
        assert U.is_vec(U.fake_set(case.na, 0), U.fake_set(case.nb, 0))
    if case.cls.startswith("empty_"):
        assert (case.na == 0) != (case.nb == 0)
        side, off = (A, case.off_a) if case.na else (B, case.off_b)
        assert not U.minmax_vec(side) and off in (1, 3)      # the non-empty side is misaligned


def test_d2_table_is_complete():
    """Every form under every alignment class in both modes; the
    single-clause cases on two dense generators; both parities of nb beside
    an empty A."""
    assert {c.form for c in U.D2_CASES} == ALL_FORMS
    assert len({c.id for c in U.D2_CASES}) == len(U.D2_CASES)
    for gen in U.GENS:
        for mode in U.MODE_NAMES:
            mine = [c for c in U.D2_CASES if c.gen == gen and c.mode == mode]
            assert CLASSES <= {c.cls for c in mine}
            empties = [c for c in mine if c.cls.startswith("empty_")]
            assert any(c.nb == 0 for c in empties)
            assert {c.nb % 2 for c in empties if c.na == 0} == {0, 1}
            only = {c.cls for c in mine if c.cls.startswith("only_")}
            assert only == ({"only_tomb_off", "only_rep_off", "only_ts_off"} if gen in U.DENSE else set())
    for form, mode in set((f, m) for (_, m), f in U.FORMS.items()):   # form x class, whichever generator gives the form
        assert CLASSES <= {c.cls for c in U.D2_CASES if c.form == form and c.mode == mode}, (form, mode)
    assert {U.FORMS[g, "lww"] for g in U.DENSE} == {"lww_table_u32", "lww_table_u64"}
    assert {U.FORMS[g, "orset"] for g in U.DENSE} == {"or_chunks"}


def test_d2_generators_hold_what_the_forms_need():
    for gen in U.GENS:
        a, b = U.gen_sides(gen)
        both = set(zip(*(x.tolist() for x in a[:3]))) & set(zip(*(x.tolist() for x in b[:3])))
        assert len(both) >= 400                              # cross-side equal tags ...
        ta = dict(zip(zip(*(x.tolist() for x in a[:3])), a[3].tolist()))
        tb = dict(zip(zip(*(x.tolist() for x in b[:3])), b[3].tolist()))
        assert sum(1 for t in both if ta[t] != tb[t]) >= 100  # ... with differing tombs
    # keys10 / OR-Set: the key-and-digit sort leaves groups of equal sorted
    # bits for or_run_dedup (s0 > 0), some longer than its 32-tuple
    # element-wise limit (the LDS rank-sort)
    a, b = U.gen_sides("keys10")
    sh = U.plan_shape(a, b, "orset")
    assert sh.s0 == 14 and sh.tw == 0 and sh.b0 + sh.br == 8
    key = np.concatenate([a[0], b[0]])
    ts = np.concatenate([a[1], b[1]])
    grp = (key - key.min()) << np.uint64(20) | (ts - ts.min()) >> np.uint64(sh.s0 - 8)
    sizes = np.unique(grp, return_counts=True)[1]
    assert (sizes > 32).sum() >= 6 and sizes.max() <= 3072
    # dense16_wide_ts / OR-Set: tags over 32 bits (the chunk kernel's wide entries)
    sh = U.plan_shape(*U.gen_sides("dense16_wide_ts"), "orset")
    assert sh.b0 + sh.br + sh.bt > 32


@pytest.mark.parametrize("case", U.PLANNED_CASES, ids=lambda c: c.id)
def test_planned_case_takes_its_form_and_classes(case):
    a, b = case.sides()
    fa, fb = case.fresh_sides()
    assert len(a[0]) % 2 == (1 if case.odd else 0)
    wide = U.plan_shape(a, b, case.mode, widen=True)
    assert U.form_of(wide, case.mode) == case.form
    for x, y in zip(a[:3] + b[:3], fa[:3] + fb[:3]):         # the fresh inputs stay inside the plan
        assert x.min() == y.min() and x.max() == y.max() and len(x) == len(y)
    assert not np.array_equal(a[3], fa[3])
    na, nb = len(a[0]), len(b[0])
    assert U.is_vec(U.fake_set(na, 0), U.fake_set(nb, 0)) == (not case.odd)
    assert U.minmax_vec(U.fake_set(na, 0), U.fake_set(nb, 0))
    oa, ob = U.PLANNED_OFFS
    assert not U.is_vec(U.fake_set(na, oa), U.fake_set(nb, ob))
    assert not U.minmax_vec(U.fake_set(na, oa), U.fake_set(nb, ob))


def test_planned_table_is_complete():
    assert {(c.gen, c.mode, c.odd) for c in U.PLANNED_CASES} == {
        (g, m, o) for g in ("dense17", "two_words") for m in U.MODE_NAMES for o in (False, True)}
    assert {c.form for c in U.PLANNED_CASES} == {"lww_table_u32", "or_chunks", "radix_2w"}


@pytest.mark.parametrize("case", U.SORT_CASES, ids=lambda c: c.id)
def test_sort_case_takes_its_form_and_class(case):
    t = case.tuples()
    assert len(t[0]) == case.n
    assert U.form_of(U.plan_shape(t, None, "sort"), "sort") == case.form
    assert U.minmax_vec(U.fake_set(case.n, case.off)) == case.mm_vec
    assert case.off_out != case.off and case.off_out in (1, 2, 3, 4)


def test_sort_table_is_complete():
    for off in (1, 2, 3, 4):
        mine = [c for c in U.SORT_CASES if c.off == off]
        assert {c.n for c in mine if c.kind == "1w"} == {1, 2, 4095, 4097, 12_289}
        assert {(c.kind, c.n) for c in mine if c.kind != "1w"} == {("2w", 12_289), ("3w", 12_289)}
    assert {c.off for c in U.SORT_CASES if c.mm_vec} == {4}


def test_knob_cases_take_their_classes():
    """The sort-knob variants run an aligned even-na and an offset dense17
    case; sort.vec_up = 0 sends the aligned one down the scalar chain."""
    assert [c.cls for c in U.D2_KNOB_CASES] == ["vec_0_0", "off_3_5", "vec_0_0", "off_3_5"]
    assert {(c.gen, c.mode) for c in U.D2_KNOB_CASES} == {("dense17", "lww"), ("dense17", "orset")}
    for c in U.D2_KNOB_CASES:
        assert c in U.D2_CASES
        assert not U.is_vec(*_sides(c), vec_up=0)
    assert U.SORT_KNOB_CASE in U.SORT_CASES
