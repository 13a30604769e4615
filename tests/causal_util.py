"""The causal OR-Set merge (crdt_orset_merge_causal) restated in numpy, and a
small seeded replica history in both forms of the OR-Set, for
tests/test_gpu_set_causal.py.  Host only: nothing here touches a GPU.

A causal state is (tuples, context); tuples are (key, ts, rep, tomb) numpy
arrays sorted by (key, ts, rep), a context a uint64 array.  Side X holds a tag
present iff it holds a copy and none of its copies is tombstoned; a tag is
covered by a context v iff rep < len(v) and ts <= v[rep] (unsigned)."""
import numpy as np

DT = (np.uint64, np.uint64, np.uint32, np.uint8)
FIELDS = ("key", "ts", "rep", "tomb")


def tup(key, ts, rep, tomb):
    return tuple(np.ascontiguousarray(np.asarray(x, dtype=d)) for x, d in zip((key, ts, rep, tomb), DT))


def empty():
    return tuple(np.zeros(0, d) for d in DT)


def sort(t):
    o = np.lexsort((t[2], t[1], t[0]))                   # stable
    return tuple(np.ascontiguousarray(x[o]) for x in t)


def cat(*ts):
    return sort(tuple(np.concatenate([t[f] for t in ts]) for f in range(4)))


def tags(t):
    """Distinct tags of sorted tuples: (first index of each tag run, tomb-OR of each run)."""
    key, ts, rep, tomb = t
    n = len(key)
    new = np.ones(n, bool)
    new[1:] = (key[1:] != key[:-1]) | (ts[1:] != ts[:-1]) | (rep[1:] != rep[:-1])
    first = np.flatnonzero(new)
    tor = np.zeros(len(first), np.uint8)
    if n:
        np.maximum.at(tor, np.cumsum(new) - 1, (tomb != 0).astype(np.uint8))
    return first, tor


def covered(ts, rep, ctx):
    ctx = np.zeros(0, np.uint64) if ctx is None else np.asarray(ctx, dtype=np.uint64)
    ok = rep.astype(np.uint64) < np.uint64(len(ctx))
    v = np.zeros(len(ts), np.uint64)
    v[ok] = ctx[rep[ok].astype(np.int64)]
    return ok & (ts <= v)


def ctx_max(ca, cb):
    ca = np.zeros(0, np.uint64) if ca is None else np.asarray(ca, dtype=np.uint64)
    cb = np.zeros(0, np.uint64) if cb is None else np.asarray(cb, dtype=np.uint64)
    out = np.zeros(max(len(ca), len(cb)), np.uint64)
    out[:len(ca)] = ca
    out[:len(cb)] = np.maximum(out[:len(cb)], cb)
    return out


def present(t):
    """The present tags of a side, each once, tomb 0."""
    first, tor = tags(t)
    i = first[tor == 0]
    return t[0][i], t[1][i], t[2][i], np.zeros(len(i), np.uint8)


def ref_causal(a, ca, b, cb):
    """(tuples, src, ctx_out, kinds): the surviving tags in ascending order with
    tomb 0; per tag the first copy on a side that holds it present, a before b
    (>= 0 an index into a, else -(j + 1) for b's j); the merged context; and how
    many distinct tags met each case of the rule."""
    fa, ta = tags(a)
    fb, tb = tags(b)
    k = np.concatenate([a[0][fa], b[0][fb]])
    t = np.concatenate([a[1][fa], b[1][fb]])
    r = np.concatenate([a[2][fa], b[2][fb]])
    side = np.concatenate([np.zeros(len(fa), np.uint8), np.ones(len(fb), np.uint8)])
    pres = np.concatenate([ta == 0, tb == 0])
    first = np.concatenate([fa, fb]).astype(np.int64)
    o = np.lexsort((side, r, t, k))
    k, t, r, side, pres, first = k[o], t[o], r[o], side[o], pres[o], first[o]
    n = len(o)
    new = np.ones(n, bool)
    new[1:] = (k[1:] != k[:-1]) | (t[1:] != t[:-1]) | (r[1:] != r[:-1])
    gid = np.cumsum(new) - 1
    ng = int(new.sum())
    pa, pb = np.zeros(ng, bool), np.zeros(ng, bool)
    ia, ib = np.zeros(ng, np.int64), np.zeros(ng, np.int64)
    ma, mb = side == 0, side == 1
    pa[gid[ma]] = pres[ma]
    ia[gid[ma]] = first[ma]
    pb[gid[mb]] = pres[mb]
    ib[gid[mb]] = first[mb]
    gk, gt, gr = k[new], t[new], r[new]
    cova, covb = covered(gt, gr, ca), covered(gt, gr, cb)
    keep = (pa & pb) | (pa & ~covb) | (pb & ~cova)
    src = np.where(pa, ia, -(ib + 1))
    kinds = {"both": int((pa & pb).sum()), "a_kept": int((pa & ~pb & ~covb).sum()),
             "a_dropped": int((pa & ~pb & covb).sum()), "b_kept": int((pb & ~pa & ~cova).sum()),
             "b_dropped": int((pb & ~pa & cova).sum()), "absent": int((~pa & ~pb).sum())}
    out = (gk[keep], gt[keep], gr[keep], np.zeros(int(keep.sum()), np.uint8))
    return out, src[keep], ctx_max(ca, cb), kinds


def live_keys(t):
    """crdt_set_elements of an OR-Set state: the keys with a live tag."""
    return np.unique(present(t)[0])


class History:
    """A seeded history of `replicas` OR-Set replicas kept in both forms.  An
    add at replica r is r's next event e: the tag (key, e, r).  A remove of a
    key tombstones the replica's tags of it (tombstone form) or deletes them
    (causal form) and is no event.  clock[x][r] = the events of r that x has
    seen.  `merge(x, y)` is left to the caller, who sets both forms of x."""

    def __init__(self, seed, replicas=4, keys=12):
        self.rng = np.random.default_rng(seed)
        self.n = replicas
        self.keys = keys
        self.tomb = [empty() for _ in range(replicas)]   # tombstone form
        self.dots = [empty() for _ in range(replicas)]   # causal form (tomb all 0)
        self.clock = [np.zeros(replicas, np.uint64) for _ in range(replicas)]

    def add(self, x, key):
        self.clock[x][x] += np.uint64(1)
        one = tup([key], [self.clock[x][x]], [x], [0])
        self.tomb[x] = cat(self.tomb[x], one)
        self.dots[x] = cat(self.dots[x], one)

    def remove(self, x, key):
        k, t, r, m = self.tomb[x]
        self.tomb[x] = (k, t, r, np.where(k == key, 1, m).astype(np.uint8))
        keep = self.dots[x][0] != key
        self.dots[x] = tuple(np.ascontiguousarray(f[keep]) for f in self.dots[x])

    def step(self):
        """One random step: ("add" | "remove", x, key) applied, or ("merge", x, y) for the caller."""
        u = self.rng.random()
        x = int(self.rng.integers(self.n))
        if u < 0.45:
            key = int(self.rng.integers(self.keys))
            self.add(x, key)
            return "add", x, key
        if u < 0.70:
            key = int(self.rng.integers(self.keys))
            self.remove(x, key)
            return "remove", x, key
        y = int((x + 1 + self.rng.integers(self.n - 1)) % self.n)
        return "merge", x, y
