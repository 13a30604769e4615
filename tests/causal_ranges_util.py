"""The range-restricted causal OR-Set merge (crdt_orset_merge_causal_ranges)
restated in numpy on top of tests/causal_util.py, with the digest machinery it
is used with in exact form: buckets, an ideal digest diff (a bucket is flagged
iff the canonical tuples differ -- what the 64-bit digests say up to a
collision) and the selection.  Host only: nothing here touches a GPU.

Buckets are crdt_set_digest's: bucket(key) = #{ j : splitters[j] <= key },
unsigned, len(splitters) + 1 of them."""
import numpy as np

from causal_util import ctx_max, ref_causal, tags


def u64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64))


def bucket(key, splitters):
    sp = u64([] if splitters is None else splitters)
    return np.searchsorted(sp, u64(key), side="right")


def pick(t, idx):
    return tuple(np.ascontiguousarray(x[idx]) for x in t)


def canon(t):
    """(tuples, first): merge(t, {}) of an OR-Set state -- each tag once, tomb
    the OR over its copies -- and the index in t of each tag's first copy."""
    first, tor = tags(t)
    return (t[0][first], t[1][first], t[2][first], tor), first


def np_select(t, splitters, flags):
    """crdt_set_select in OR-Set mode: (tuples, src)."""
    c, first = canon(t)
    keep = np.asarray(flags)[bucket(c[0], splitters)] != 0
    return pick(c, keep), first[keep].astype(np.int64)


def ideal_flags(a, b, splitters):
    """uint8[m + 1]: 1 where the canonical tuples of a and b differ in the bucket."""
    m = 0 if splitters is None else len(splitters)
    flags = np.zeros(m + 1, np.uint8)
    (ca, _), (cb, _) = canon(a), canon(b)
    ba, bb = bucket(ca[0], splitters), bucket(cb[0], splitters)
    na, nb = np.bincount(ba, minlength=m + 1), np.bincount(bb, minlength=m + 1)
    flags[na != nb] = 1
    oa, ob = np.concatenate([[0], np.cumsum(na)]), np.concatenate([[0], np.cumsum(nb)])
    for k in np.flatnonzero((na == nb) & (na > 0)):         # (sorted by key: a bucket is a contiguous slice)
        sa, sb = slice(oa[k], oa[k + 1]), slice(ob[k], ob[k + 1])
        if any(not np.array_equal(x[sa], y[sb]) for x, y in zip(ca, cb)):
            flags[k] = 1
    return flags


def ref_causal_ranges(a, ca, b, cb, splitters, flags):
    """(tuples, src, ctx_out): in flagged buckets ref_causal of the two sides'
    tuples there; in unflagged ones a's present tags, b's tuples dropped; the
    pieces in key order, src mapped back to positions in a and b."""
    flags = np.asarray(flags)
    fa, fb = flags[bucket(a[0], splitters)] != 0, flags[bucket(b[0], splitters)] != 0
    ia_f, ia_u, ib_f = np.flatnonzero(fa), np.flatnonzero(~fa), np.flatnonzero(fb)
    out_f, src_f, _, _ = ref_causal(pick(a, ia_f), ca, pick(b, ib_f), cb)
    from_a, at = src_f >= 0, np.empty(len(src_f), np.int64)
    at[from_a] = ia_f[src_f[from_a]]
    at[~from_a] = -(ib_f[-(src_f[~from_a] + 1)] + 1)
    src_f = at
    au = pick(a, ia_u)
    first, tor = tags(au)
    i = first[tor == 0]
    out_u = (au[0][i], au[1][i], au[2][i], np.zeros(len(i), np.uint8))
    src_u = ia_u[i].astype(np.int64)
    out = tuple(np.concatenate([x, y]) for x, y in zip(out_f, out_u))
    src = np.concatenate([src_f, src_u])
    o = np.lexsort((out[2], out[1], out[0]))
    return tuple(np.ascontiguousarray(x[o]) for x in out), src[o], ctx_max(ca, cb)
