"""Range digests of the keyed PN-Counter map (crdt_cmap_digest /
crdt_cmap_select) restated twice on the CPU, in the style of cmap_util.py.

A state is four numpy columns (key uint64, rep uint32, p uint64, n uint64),
strictly ascending by (key, rep).  m ascending uint64 splitters cut the key
space into m + 1 buckets, bucket(key) = #{ j : splitters[j] <= key }, unsigned.
With sm = SplitMix64's output function the hash of a cell is

    h(key, rep, p, n) = sm( sm( sm( sm(key) ^ rep ) ^ p ) ^ n )

hash[b] is the sum mod 2^64 of h over the cells in bucket b, count[b] their
number; select(t, flags) is the cells of t whose bucket is flagged, in order,
unchanged.  The ``*_d`` functions are the definition: one cell at a time,
Python integers.  The ``*_np`` functions are vectorised numpy.
tests/test_cmap_digest_ref.py holds the two to each other; the GPU tests
compare the kernels with them bit for bit.
"""
import numpy as np

M64 = (1 << 64) - 1
U64, U32 = np.uint64, np.uint32


# ---------------------------------------------------------------- the definition
def sm(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def h(key, rep, p, n):
    return sm(sm(sm(sm(int(key)) ^ int(rep)) ^ int(p)) ^ int(n))


def bucket_d(splitters, key):
    return sum(1 for s in splitters if int(s) <= int(key))


def digest_d(t, splitters):
    """(hash, count): uint64 arrays of len(splitters) + 1 entries."""
    splitters = [int(s) for s in splitters]
    hs, cs = [0] * (len(splitters) + 1), [0] * (len(splitters) + 1)
    for key, rep, p, n in zip(*t):
        b = bucket_d(splitters, key)
        hs[b] = (hs[b] + h(key, rep, p, n)) & M64
        cs[b] += 1
    return np.asarray(hs, dtype=U64), np.asarray(cs, dtype=U64)


def select_d(t, splitters, flags):
    splitters = [int(s) for s in splitters]
    keep = [i for i, key in enumerate(t[0]) if flags[bucket_d(splitters, key)] != 0]
    return tuple(np.asarray([c[i] for i in keep], dtype=c.dtype) for c in t)


def diff_d(da, db):
    """uint8 flags: 1 where the hashes or the counts differ."""
    return np.asarray([1 if (int(x) != int(y) or int(c) != int(d)) else 0
                       for x, c, y, d in zip(da[0], da[1], db[0], db[1])], dtype=np.uint8)


# ---------------------------------------------------------------- vectorised
def sm_np(x):
    x = np.asarray(x, dtype=U64)
    with np.errstate(over="ignore"):
        x = x + U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
    return x ^ (x >> U64(31))


def h_np(t):
    key, rep, p, n = t
    return sm_np(sm_np(sm_np(sm_np(key) ^ rep.astype(U64)) ^ p) ^ n)


def bucket_np(splitters, key):
    return np.searchsorted(np.asarray(splitters, dtype=U64), np.asarray(key, dtype=U64), side="right")


def digest_np(t, splitters):
    nb = len(splitters) + 1
    b = bucket_np(splitters, t[0])
    hs = np.zeros(nb, dtype=U64)
    with np.errstate(over="ignore"):
        np.add.at(hs, b, h_np(t))                        # (uint64 sums wrap)
    return hs, np.bincount(b, minlength=nb).astype(U64)


def select_np(t, splitters, flags):
    keep = np.asarray(flags)[bucket_np(splitters, t[0])] != 0
    return tuple(c[keep] for c in t)


def diff_np(da, db):
    return ((da[0] != db[0]) | (da[1] != db[1])).astype(np.uint8)


def quantile_splitters(t, m):
    """crdt_amd.reconcile.key_splitters on the CPU: every ceil(n / (m + 1))-th key."""
    n = len(t[0])
    if n == 0 or m == 0:
        return np.zeros(m, dtype=U64)
    step = -(-n // (m + 1))
    return t[0][np.minimum(np.arange(1, m + 1) * step, n - 1)]


# ---------------------------------------------------------------- the pair of the round tests
# known answers of drifted_pair() at its defaults under quantile_splitters(A, 255), worked out with digest_d
DRIFTED_FLAGGED = [1, 23, 56, 83, 112, 169, 203, 218]   # the buckets that differ
DRIFTED_SHIPPED = (201, 198)                            # cells A and B select from them


def drifted_pair(n=3 * 2048 + 17, raised=5, dropped=3, seed=24):
    """(A, B): A a seeded state of n cells over n // 4 keys; B is A with
    ``raised`` cells' p raised by 1 and ``dropped`` other cells missing."""
    import cmap_util as cu
    rng = np.random.default_rng(seed)
    a = cu.random_state(rng, n, max(1, n // 4))
    at = rng.choice(n, size=raised + dropped, replace=False)
    b = tuple(c.copy() for c in a)
    b[2][at[:raised]] += U64(1)
    keep = np.ones(n, dtype=bool)
    keep[at[raised:]] = False
    return a, tuple(c[keep] for c in b)
