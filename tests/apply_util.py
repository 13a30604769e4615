"""crdt_set_apply restated in numpy, twice: one operation at a time (the
definition) and in closed form (what the kernels compute), on top of
tests/causal_util.py.  Host only: nothing here touches a GPU.

A state is (key, ts, rep, tomb) numpy arrays sorted by (key, ts, rep), copies
of a tag in any order and number; a clock row / causal context a uint64 array.
Operation i of replica rep is its event clock[rep] + 1 + i, add (kind 0) and
remove (kind != 0) alike."""
import numpy as np

import causal_util as cu


def canon(t, causal):
    """(tuples, src): each tag once in ascending order with src = the index of
    its first copy; tombstone form tomb = the OR over the copies, causal form
    the tags with tomb-OR 0 alone, tomb 0."""
    first, tor = cu.tags(t)
    if causal:
        first, tor = first[tor == 0], tor[tor == 0]
    return (t[0][first], t[1][first], t[2][first], tor.astype(np.uint8)), first.astype(np.int64)


def apply_seq(t, clock, rep, keys, kinds, causal):
    """The definition: (tuples, src, clock_out), the batch applied one
    operation at a time to the canonical form of t."""
    (k, s, r, m), src = canon(t, causal)
    rows = [[int(a), int(b), int(c), int(d), int(e)] for a, b, c, d, e in zip(k, s, r, m, src)]
    ts0 = int(clock[rep])
    for i, (key, kind) in enumerate(zip(keys, kinds)):
        key = int(key)
        if kind == 0:
            rows.append([key, ts0 + 1 + i, int(rep), 0, -(i + 1)])
        elif causal:
            rows = [x for x in rows if x[0] != key]
        else:
            for x in rows:
                if x[0] == key:
                    x[3] = 1
    rows.sort(key=lambda x: (x[0], x[1], x[2]))
    cols = list(zip(*rows)) if rows else [[], [], [], [], []]
    out = cu.tup(np.array(cols[0], dtype=np.uint64), np.array(cols[1], dtype=np.uint64), cols[2], cols[3])
    clock_out = np.array(clock, dtype=np.uint64)
    clock_out[rep] = np.uint64(ts0 + len(keys))
    return out, np.array(cols[4], dtype=np.int64), clock_out


def apply_ref(t, clock, rep, keys, kinds, causal):
    """The closed form, vectorised: a tag of t dies iff the batch holds a
    remove of its key, the tag of add i iff a remove of its key sits at an
    index > i; the survivors' sorted union.  (tuples, src, clock_out)."""
    keys = np.asarray(keys, dtype=np.uint64)
    kinds = np.asarray(kinds, dtype=np.uint8)
    m = len(keys)
    clock = np.asarray(clock, dtype=np.uint64)
    ts0 = clock[rep]
    (k, s, r, tm), src = canon(t, causal)
    rm = kinds != 0
    removed = np.unique(keys[rm])
    hit = np.isin(k, removed)
    # the last remove of each operation's key (sorted keys: a suffix maximum inside the key's run)
    idx = np.arange(m, dtype=np.int64)
    last = np.full(m, -1, np.int64)
    if m:
        run = np.concatenate([[0], np.cumsum(keys[1:] != keys[:-1])])
        best = np.full(int(run[-1]) + 1, -1, np.int64)
        np.maximum.at(best, run[rm], idx[rm])
        last = best[run]
    add = ~rm
    dead_add = last[add] > idx[add]
    ak = keys[add]
    ats = (ts0 + np.uint64(1) + idx[add].astype(np.uint64)).astype(np.uint64)
    arep = np.full(int(add.sum()), rep, np.uint32)
    asrc = -(idx[add] + 1)
    if causal:
        keep_s, keep_a = ~hit, ~dead_add
        tomb_s, tomb_a = np.zeros(len(k), np.uint8), np.zeros(len(ak), np.uint8)
    else:
        keep_s, keep_a = np.ones(len(k), bool), np.ones(len(ak), bool)
        tomb_s, tomb_a = (tm | hit).astype(np.uint8), dead_add.astype(np.uint8)
    K = np.concatenate([k[keep_s], ak[keep_a]])
    S = np.concatenate([s[keep_s], ats[keep_a]])
    R = np.concatenate([r[keep_s], arep[keep_a]])
    M = np.concatenate([tomb_s[keep_s], tomb_a[keep_a]])
    X = np.concatenate([src[keep_s], asrc[keep_a]])
    o = np.lexsort((R, S, K))
    clock_out = clock.copy()
    clock_out[rep] = ts0 + np.uint64(m)
    return cu.tup(K[o], S[o], R[o], M[o]), X[o].astype(np.int64), clock_out


def batch_tags(clock, rep, keys):
    """The tags an adds-only batch inserts, as a sorted state (tomb 0)."""
    keys = np.asarray(keys, dtype=np.uint64)
    ts = np.uint64(clock[rep]) + np.uint64(1) + np.arange(len(keys), dtype=np.uint64)
    return cu.sort(cu.tup(keys, ts, np.full(len(keys), rep, np.uint32), np.zeros(len(keys), np.uint8)))


def orset_merge(a, b):
    """crdt_orset_merge restated: each tag of either side once, tomb = the OR over all its copies."""
    return canon(cu.cat(a, b), False)[0]


def rand_batch(rng, m, key_space, p_remove=0.4):
    """m seeded operations over [0, key_space): sorted keys (repeats likely), kinds."""
    keys = np.sort(rng.integers(0, key_space, m).astype(np.uint64))
    kinds = (rng.random(m) < p_remove).astype(np.uint8)
    return keys, kinds


def rand_state(rng, n, key_space, reps=4, ts_space=64, p_tomb=0.1, p_dup=0.15):
    """n seeded sorted tuples: about p_tomb tombstoned, about p_dup of them a
    second copy of another tuple's tag with its own tomb."""
    if n == 0:
        return cu.empty()
    nd = int(n * p_dup)
    nu = n - nd
    key = rng.integers(0, key_space, nu).astype(np.uint64)
    ts = rng.integers(1, ts_space + 1, nu).astype(np.uint64)
    rep = rng.integers(0, reps, nu).astype(np.uint32)
    pick = rng.integers(0, nu, nd)
    key, ts, rep = np.concatenate([key, key[pick]]), np.concatenate([ts, ts[pick]]), np.concatenate([rep, rep[pick]])
    tomb = (rng.random(n) < p_tomb).astype(np.uint8)
    o = rng.permutation(n)                               # copies of a tag in any order
    return cu.sort(cu.tup(key[o], ts[o], rep[o], tomb[o]))
