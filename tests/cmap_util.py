"""The keyed PN-Counter map (crdt_cmap_*) restated twice on the CPU.

A state is four numpy columns (key uint64, rep uint32, p uint64, n uint64),
strictly ascending by (key, rep).  The ``*_d`` functions are the definition:
dict-based, one cell or one operation at a time, Python integers mod 2^64.
The ``*_np`` functions are vectorised numpy.  tests/test_cmap_ref.py holds the
two to each other; the GPU tests compare the kernels with them bit for bit.
"""
import numpy as np

M64 = 1 << 64
U64, U32 = np.uint64, np.uint32


def state(key=(), rep=(), p=(), n=()):
    return (np.asarray(key, dtype=U64), np.asarray(rep, dtype=U32), np.asarray(p, dtype=U64),
            np.asarray(n, dtype=U64))


def is_state(t):
    """Strictly ascending by (key, rep), unsigned."""
    cells = [(int(k), int(r)) for k, r in zip(t[0], t[1])]
    return all(x < y for x, y in zip(cells, cells[1:]))


def same(x, y):
    return len(x) == len(y) and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(x, y))


# ---------------------------------------------------------------- the definition
def to_dict(t):
    return {(int(k), int(r)): (int(p), int(n)) for k, r, p, n in zip(*t)}


def from_dict(d):
    cells = sorted(d)
    return state([c[0] for c in cells], [c[1] for c in cells], [d[c][0] for c in cells], [d[c][1] for c in cells])


def merge_d(a, b):
    out = to_dict(a)
    for cell, (p, n) in to_dict(b).items():
        if cell in out:
            out[cell] = (max(out[cell][0], p), max(out[cell][1], n))
        else:
            out[cell] = (p, n)
    return from_dict(out)


def apply_d(t, rep, op_key, op_dp, op_dn):
    out = to_dict(t)
    for k, dp, dn in zip(op_key, op_dp, op_dn):
        p, n = out.get((int(k), int(rep)), (0, 0))
        out[(int(k), int(rep))] = ((p + int(dp)) % M64, (n + int(dn)) % M64)
    return from_dict(out)


def _as_i64(x):
    x %= M64
    return x - M64 if x >= 1 << 63 else x


def values_d(t):
    """(keys, P, N, value): one row per distinct key, in key order."""
    rows = {}
    for (k, _), (p, n) in sorted(to_dict(t).items()):
        P, N = rows.get(k, (0, 0))
        rows[k] = ((P + p) % M64, (N + n) % M64)
    keys = sorted(rows)
    return (np.asarray(keys, dtype=U64), np.asarray([rows[k][0] for k in keys], dtype=U64),
            np.asarray([rows[k][1] for k in keys], dtype=U64),
            np.asarray([_as_i64(rows[k][0] - rows[k][1]) for k in keys], dtype=np.int64))


def lookup_d(t, probes):
    keys, _, _, value = values_d(t)
    rows = {int(k): int(v) for k, v in zip(keys, value)}
    return (np.asarray([rows.get(int(x), 0) for x in probes], dtype=np.int64),
            np.asarray([1 if int(x) in rows else 0 for x in probes], dtype=np.uint8))


def delta_d(src, dst):
    d = to_dict(dst)
    out = {}
    for cell, (p, n) in to_dict(src).items():
        if cell not in d or p > d[cell][0] or n > d[cell][1]:
            out[cell] = (p, n)
    return from_dict(out)


# ---------------------------------------------------------------- vectorised
def _merged(a, b):
    """Both sides in the stable merged order, a first on an equal cell:
    (columns, from_b, starts a run of equal cells)."""
    cols = [np.concatenate([x, y]) for x, y in zip(a, b)]
    from_b = np.concatenate([np.zeros(len(a[0]), dtype=bool), np.ones(len(b[0]), dtype=bool)])
    order = np.lexsort((cols[1], cols[0]))               # stable: by key, then rep, then a before b
    cols = [c[order] for c in cols]
    from_b = from_b[order]
    head = np.ones(len(order), dtype=bool)
    head[1:] = (cols[0][1:] != cols[0][:-1]) | (cols[1][1:] != cols[1][:-1])
    return cols, from_b, head


def _combine(a, b, op):
    cols, _, head = _merged(a, b)
    if len(head) == 0:
        return state()
    at = np.flatnonzero(head)
    return (cols[0][at], cols[1][at], op.reduceat(cols[2], at).astype(U64), op.reduceat(cols[3], at).astype(U64))


def merge_np(a, b):
    return _combine(a, b, np.maximum)


def apply_np(t, rep, op_key, op_dp, op_dn):
    op_key = np.asarray(op_key, dtype=U64)
    batch = (op_key, np.full(len(op_key), rep, dtype=U32), np.asarray(op_dp, dtype=U64), np.asarray(op_dn, dtype=U64))
    return _combine(t, batch, np.add)                   # (uint64 sums wrap)


def values_np(t):
    key, _, p, n = t
    if len(key) == 0:
        return np.zeros(0, U64), np.zeros(0, U64), np.zeros(0, U64), np.zeros(0, np.int64)
    head = np.ones(len(key), dtype=bool)
    head[1:] = key[1:] != key[:-1]
    at = np.flatnonzero(head)
    P, N = np.add.reduceat(p, at).astype(U64), np.add.reduceat(n, at).astype(U64)
    return key[at], P, N, (P - N).view(np.int64)


def lookup_np(t, probes):
    keys, _, _, value = values_np(t)
    probes = np.asarray(probes, dtype=U64)
    if len(keys) == 0:
        return np.zeros(len(probes), np.int64), np.zeros(len(probes), np.uint8)
    at = np.minimum(np.searchsorted(keys, probes), len(keys) - 1)
    found = keys[at] == probes
    return np.where(found, value[at], 0).astype(np.int64), found.astype(np.uint8)


def delta_np(src, dst):
    cols, from_src, head = _merged(dst, src)
    if len(head) == 0:
        return state()
    paired = from_src & ~head                            # dst's copy of the cell sits just before it
    prev_p, prev_n = np.roll(cols[2], 1), np.roll(cols[3], 1)
    ship = from_src & (~paired | (cols[2] > prev_p) | (cols[3] > prev_n))
    return tuple(c[ship] for c in cols)


# ---------------------------------------------------------------- seeded inputs
def random_state(rng, n, key_space, reps=8):
    """n distinct cells with keys below key_space and reps below ``reps``, p and n below 2^40."""
    assert n <= key_space * reps
    cells = rng.choice(key_space * reps, size=n, replace=False)
    cells.sort()
    key, rep = (cells // reps).astype(U64), (cells % reps).astype(U32)
    p = rng.integers(0, 1 << 40, size=n, dtype=np.uint64)
    q = rng.integers(0, 1 << 40, size=n, dtype=np.uint64)
    return key, rep, p, q
