"""Counter-map state from increment logs (crdt_cmap_combine / _add /
_from_ops) restated twice on the CPU, in tests/cmap_util.py's forms.

A log is four numpy columns (key uint64, rep uint32, dp uint64, dn uint64) in
any order, with repeats.  The ``*_d`` functions are the definition: a dict, one
cell or one operation at a time, Python integers mod 2^64.  The ``*_np``
functions are vectorised (np.lexsort, np.add.reduceat on uint64, which wraps).
tests/test_cmap_ingest_ref.py holds the two to each other; the GPU tests
compare the kernels with them bit for bit.
"""
import numpy as np

import cmap_util as cu

M64 = cu.M64
U64, U32 = np.uint64, np.uint32


def log(key=(), rep=(), dp=(), dn=()):
    return cu.state(key, rep, dp, dn)


def is_sorted(t):
    """Ascending by (key, rep), unsigned, repeats allowed."""
    cells = [(int(k), int(r)) for k, r in zip(t[0], t[1])]
    return all(x <= y for x, y in zip(cells, cells[1:]))


# ---------------------------------------------------------------- the definition
def from_ops_d(ops):
    out = {}
    for k, r, dp, dn in zip(*ops):
        p, n = out.get((int(k), int(r)), (0, 0))
        out[(int(k), int(r))] = ((p + int(dp)) % M64, (n + int(dn)) % M64)
    return cu.from_dict(out)


def combine_d(t, idx=None, src=None):
    """t sorted with repeats; with idx, position i contributes src = (p, n) at
    idx[i], 0 when the index is at or past len(src[0])."""
    p, n = (t[2], t[3]) if src is None else src
    out = {}
    for i, (k, r) in enumerate(zip(t[0], t[1])):
        j = i if idx is None else int(idx[i])
        dp, dn = (int(p[j]), int(n[j])) if j < len(p) else (0, 0)
        a, b = out.get((int(k), int(r)), (0, 0))
        out[(int(k), int(r))] = ((a + dp) % M64, (b + dn) % M64)
    return cu.from_dict(out)


def add_d(t, d):
    out = cu.to_dict(t)
    for cell, (p, n) in cu.to_dict(d).items():
        a, b = out.get(cell, (0, 0))
        out[cell] = ((a + p) % M64, (b + n) % M64)
    return cu.from_dict(out)


# ---------------------------------------------------------------- vectorised
def _reduce(key, rep, p, n):
    """Columns already in (key, rep) order -> one cell per run."""
    if len(key) == 0:
        return cu.state()
    head = np.ones(len(key), dtype=bool)
    head[1:] = (key[1:] != key[:-1]) | (rep[1:] != rep[:-1])
    at = np.flatnonzero(head)
    return key[at], rep[at], np.add.reduceat(p, at).astype(U64), np.add.reduceat(n, at).astype(U64)


def combine_np(t, idx=None, src=None):
    key, rep = np.asarray(t[0], U64), np.asarray(t[1], U32)
    if idx is None:
        p, n = np.asarray(t[2], U64), np.asarray(t[3], U64)
    else:
        idx = np.asarray(idx, dtype=np.int64)
        ok = idx < len(src[0])
        at = np.where(ok, idx, 0)
        p = np.where(ok, np.asarray(src[0], U64)[at] if len(src[0]) else U64(0), U64(0)).astype(U64)
        n = np.where(ok, np.asarray(src[1], U64)[at] if len(src[1]) else U64(0), U64(0)).astype(U64)
    return _reduce(key, rep, p, n)


def from_ops_np(ops):
    key, rep, dp, dn = (np.asarray(ops[0], U64), np.asarray(ops[1], U32), np.asarray(ops[2], U64),
                        np.asarray(ops[3], U64))
    order = np.lexsort((rep, key))
    return _reduce(key[order], rep[order], dp[order], dn[order])


def add_np(t, d):
    return cu._combine(t, d, np.add)                     # (uint64 sums wrap)


# ---------------------------------------------------------------- seeded inputs
def random_log(rng, m, key_space, reps=4, big=False):
    """m operations over key_space keys and ``reps`` replicas (heavy repeats when
    m >> key_space * reps); big: amounts over the whole of uint64, so sums wrap."""
    key = rng.integers(0, key_space, size=m, dtype=np.uint64) * U64(7) + U64(3)
    rep = rng.integers(0, reps, size=m, dtype=np.uint64).astype(U32)
    hi = (1 << 64) - 1 if big else 1 << 40
    dp = rng.integers(0, hi, size=m, dtype=np.uint64)
    dn = rng.integers(0, hi, size=m, dtype=np.uint64)
    return key, rep, dp, dn


def cat(x, y):
    return tuple(np.concatenate([a, b]) for a, b in zip(x, y))


def perm(ops, order):
    return tuple(np.ascontiguousarray(c[order]) for c in ops)


def sorted_log(ops):
    """The log stably ordered by (key, rep): combine's input form."""
    return perm(ops, np.lexsort((ops[1], ops[0])))


def expand(t, copies):
    """Each cell of t ``copies`` times in a row: runs of equal (key, rep)."""
    return tuple(np.repeat(c, copies) for c in t)
