"""CPU: the two restatements of the counter map's range digests in
tests/cmap_digest_util.py agree with each other, with the known answers of the
hash, and with the laws the reconciliation round rests on."""
import numpy as np
import pytest

import cmap_digest_util as du
import cmap_util as cu
from crdt_amd import synth

U64, U32 = np.uint64, np.uint32
M64 = du.M64
N = 3 * 2048 + 17


def _same_digest(x, y):
    return all(np.array_equal(a, b) and a.dtype == b.dtype == U64 for a, b in zip(x, y))


def _state(seed, n=300, ks=90):
    return cu.random_state(np.random.default_rng(seed), n, ks)


# ---------------------------------------------------------------- known answers
def test_known_answers():
    assert du.sm(0) == 0xE220A8397B1DCDAF
    assert du.h(0, 0, 0, 0) == 0x2130748AAAC80268
    assert du.h(1, 2, 3, 4) == 0xD55CCD4AEB3CCAFB
    assert du.h(M64, 2**32 - 1, M64, M64) == 0x44CE0376423ECC3B
    t = cu.state([0, 1, M64], [0, 2, 2**32 - 1], [0, 3, M64], [0, 4, M64])
    assert du.h_np(t).tolist() == [0x2130748AAAC80268, 0xD55CCD4AEB3CCAFB, 0x44CE0376423ECC3B]
    assert int(du.sm_np([0])[0]) == 0xE220A8397B1DCDAF


def test_sm_is_the_projects_splitmix64():
    xs = np.array([0, 1, 2**63, M64, 0x9E3779B97F4A7C15], dtype=U64)
    assert [int(synth.splitmix64(int(x))) for x in xs] == [du.sm(int(x)) for x in xs] == du.sm_np(xs).tolist()


# ---------------------------------------------------------------- the restatements
@pytest.mark.parametrize("seed,m", [(1, 0), (2, 1), (3, 7), (4, 63), (5, 400)])
def test_restatements_agree(seed, m):
    t = _state(seed)
    rng = np.random.default_rng(seed + 100)
    sp = np.sort(rng.integers(0, 95, size=m).astype(U64))     # repeats: empty buckets; some above every key
    d = du.digest_d(t, sp)
    assert _same_digest(d, du.digest_np(t, sp))
    assert int(d[1].sum()) == len(t[0])
    flags = rng.integers(0, 2, size=m + 1).astype(np.uint8)
    assert cu.same(du.select_d(t, sp, flags), du.select_np(t, sp, flags))
    other = _state(seed + 50)
    assert np.array_equal(du.diff_d(d, du.digest_d(other, sp)), du.diff_np(d, du.digest_np(other, sp)))


def test_unsigned_buckets_and_fields():
    big = 2**63
    t = cu.state([5, big - 1, big, big + 7, M64], [2**32 - 1, 0, 2**31, 1, 2**32 - 1], [M64, 1, big, 0, M64],
                 [M64, big + 1, 0, M64, M64 - 1])
    assert cu.is_state(t)
    sp = np.array([big, big + 7, M64], dtype=U64)
    assert du.bucket_np(sp, t[0]).tolist() == [0, 0, 1, 2, 3] == [du.bucket_d(sp, k) for k in t[0]]
    assert _same_digest(du.digest_d(t, sp), du.digest_np(t, sp))
    assert du.digest_np(t, sp)[1].tolist() == [2, 1, 1, 1]


def test_one_bucket_and_empty_state():
    t = _state(7)
    hs, cs = du.digest_np(t, [])
    assert hs.shape == cs.shape == (1,) and int(cs[0]) == len(t[0])
    assert int(hs[0]) == sum(du.h(*c) for c in zip(*t)) & M64
    e = cu.state()
    assert _same_digest(du.digest_d(e, [3, 9]), du.digest_np(e, [3, 9]))
    assert du.digest_np(e, [3, 9])[0].tolist() == [0, 0, 0] and du.digest_np(e, [3, 9])[1].tolist() == [0, 0, 0]
    assert len(du.select_np(e, [3], [1, 1])[0]) == 0


def test_a_finer_cut_sums_to_the_coarser():
    t = _state(8, n=2000, ks=600)
    fine = du.quantile_splitters(t, 63)
    coarse = fine[7::8]                                   # every 8th splitter: buckets of 8 fine ones
    hf, cf = du.digest_np(t, fine)
    hc, cc = du.digest_np(t, coarse)
    assert len(hc) == 8
    with np.errstate(over="ignore"):
        assert np.array_equal(np.add.reduceat(hf, np.arange(0, 64, 8)), hc)
    assert np.array_equal(np.add.reduceat(cf, np.arange(0, 64, 8)), cc)


# ---------------------------------------------------------------- diff and select
def test_equal_states_flag_nothing_and_one_raise_flags_its_bucket():
    t = _state(9, n=1500, ks=500)
    sp = du.quantile_splitters(t, 31)
    d = du.digest_np(t, sp)
    assert not du.diff_np(d, du.digest_np(tuple(c.copy() for c in t), sp)).any()
    for at in (0, 700, 1499):
        u = tuple(c.copy() for c in t)
        u[2][at] += U64(1)
        flags = du.diff_np(d, du.digest_np(u, sp))
        assert np.flatnonzero(flags).tolist() == [int(du.bucket_np(sp, t[0][at:at + 1])[0])]
        assert du.digest_np(u, sp)[1].tolist() == d[1].tolist()      # the counts agree: the hash alone tells


def test_select_all_and_none():
    t = _state(10)
    sp = du.quantile_splitters(t, 15)
    assert cu.same(du.select_np(t, sp, np.ones(16, np.uint8)), t)
    assert cu.same(du.select_d(t, sp, np.ones(16, np.uint8)), t)
    none = du.select_np(t, sp, np.zeros(16, np.uint8))
    assert all(len(c) == 0 for c in none) and [c.dtype for c in none] == [c.dtype for c in t]


def test_a_keys_cells_share_a_bucket():
    t = _state(11, n=700, ks=90)                          # about 8 replicas a key
    sp = du.quantile_splitters(t, 127)                    # a step of 6 cells: below a key's run
    b = du.bucket_np(sp, t[0])
    heads = np.flatnonzero(np.r_[True, t[0][1:] != t[0][:-1]])
    assert all(len(set(b[i:j].tolist())) == 1 for i, j in zip(heads, np.r_[heads[1:], len(b)]))
    assert (du.digest_np(t, sp)[1] == 0).any()            # repeated keys among the splitters: empty buckets


# ---------------------------------------------------------------- the round's law
def test_merge_with_the_selection_is_the_merge():
    a, b = du.drifted_pair()
    assert len(a[0]) == N and len(b[0]) == N - 3 and cu.is_state(a) and cu.is_state(b)
    sp = du.quantile_splitters(a, 255)
    flags = du.diff_np(du.digest_np(a, sp), du.digest_np(b, sp))
    # known answers of drifted_pair(seed=24) under 255 quantile splitters: the 5 raised and 3 dropped
    # cells fall into 8 different buckets of 256
    assert np.flatnonzero(flags).tolist() == du.DRIFTED_FLAGGED
    assert np.array_equal(flags, du.diff_d(du.digest_np(a, sp), du.digest_np(b, sp)))
    sa, sb = du.select_np(a, sp, flags), du.select_np(b, sp, flags)
    assert (len(sa[0]), len(sb[0])) == du.DRIFTED_SHIPPED
    m = cu.merge_np(a, b)
    assert cu.same(cu.merge_np(a, sb), m)
    assert cu.same(cu.merge_np(b, sa), cu.merge_np(b, a)) and cu.same(cu.merge_np(b, a), m)
    assert not cu.same(m, a) and not cu.same(m, b)


def test_an_independent_pair_flags_every_bucket():
    rng = np.random.default_rng(12)
    a, b = cu.random_state(rng, N, N // 4), cu.random_state(rng, N, N // 4)
    sp = du.quantile_splitters(a, 255)
    da, db = du.digest_np(a, sp), du.digest_np(b, sp)
    occupied = (da[1] != 0) | (db[1] != 0)
    assert np.array_equal(du.diff_np(da, db) != 0, occupied) and int(occupied.sum()) > 200
    flags = du.diff_np(da, db)
    assert cu.same(cu.merge_np(a, du.select_np(b, sp, flags)), cu.merge_np(a, b))
