"""The map read (crdt_map_read / crdt_map_lookup) restated twice on the host:
a numpy closed form, which the GPU tests compare against bit for bit, and a
literal per-key dictionary interpreter of the same contract, which the CPU
tests hold the closed form to.

The contract (include/crdt_amd.h).  t sorted ascending by (key, ts, rep),
copies of one tag in any order and number.
  OR-Set : a tag is live iff none of its copies is tombstoned; a key is a
           member iff it has a live tag; its winner is its greatest live tag;
           nsib = the number of its distinct live tags.
  LWW    : a key's winner is its maximal tag; the key is a member iff the tomb
           of that tag's FIRST copy is 0; nsib = 1.
One row per member key, ascending: (key, win = the index in t of the first
copy of the winner tag, nsib saturating at 2^32 - 1)."""
import numpy as np

SAT = 2**32 - 1


def _empty():
    return np.zeros(0, np.uint64), np.zeros(0, np.int64), np.zeros(0, np.uint32)


def ref_map_read(key, ts, rep, tomb, lww):
    """(keys uint64, win int64, nsib uint32): the closed form."""
    n = len(key)
    if n == 0:
        return _empty()
    tag_new = np.ones(n, bool)
    tag_new[1:] = (key[1:] != key[:-1]) | (ts[1:] != ts[:-1]) | (rep[1:] != rep[:-1])
    first = np.flatnonzero(tag_new)                      # the first index of each tag
    tkey = key[first]
    key_new = np.ones(len(first), bool)
    key_new[1:] = tkey[1:] != tkey[:-1]
    key_last = np.ones(len(first), bool)                 # the tag is its key's last
    key_last[:-1] = key_new[1:]
    if lww:
        w = first[key_last]
        keep = tomb[w] == 0
        w = w[keep]
        return key[w].astype(np.uint64), w.astype(np.int64), np.ones(len(w), np.uint32)
    tor = np.maximum.reduceat(tomb, first)               # the tomb-OR per tag
    live = tor == 0
    kid = np.cumsum(key_new) - 1                         # the key each tag belongs to
    nk = int(kid[-1]) + 1
    nsib = np.bincount(kid[live], minlength=nk)
    last_live = np.full(nk, -1, np.int64)                # per key, its last live tag (tags ascend within a key)
    lt = np.flatnonzero(live)
    last_live[kid[lt]] = lt                              # later assignments win: ascending tag order
    member = nsib > 0
    keys = tkey[key_last][member]
    win = first[last_live[member]]
    return keys.astype(np.uint64), win.astype(np.int64), np.minimum(nsib[member], SAT).astype(np.uint32)


def interp_map_read(key, ts, rep, tomb, lww):
    """The same rows from a literal per-key dictionary: key -> {tag: [first
    index, first copy's tomb, tomb-OR]}, read key by key."""
    state = {}
    for i in range(len(key)):
        tags = state.setdefault(int(key[i]), {})
        g = (int(ts[i]), int(rep[i]))
        if g in tags:
            tags[g][2] |= int(tomb[i])
        else:
            tags[g] = [i, int(tomb[i]), int(tomb[i])]
    keys, win, nsib = [], [], []
    for k in sorted(state):
        tags = state[k]
        if lww:
            f, first_tomb, _ = tags[max(tags)]
            if first_tomb == 0:
                keys.append(k), win.append(f), nsib.append(1)
            continue
        live = [g for g in tags if tags[g][2] == 0]
        if live:
            keys.append(k), win.append(tags[max(live)][0]), nsib.append(min(len(live), SAT))
    return np.array(keys, np.uint64), np.array(win, np.int64), np.array(nsib, np.uint32)


def ref_lookup(rows, probes):
    """(win, nsib) of each probe from a read's rows: the key's row, or (-1, 0)."""
    keys, win, nsib = rows
    probes = np.asarray(probes, np.uint64)
    w = np.full(len(probes), -1, np.int64)
    s = np.zeros(len(probes), np.uint32)
    if len(keys):
        i = np.minimum(np.searchsorted(keys, probes), len(keys) - 1)
        hit = keys[i] == probes
        w[hit] = win[i[hit]]
        s[hit] = nsib[i[hit]]
    return w, s


def np_compact(t, lww, drop_dead):
    """crdt_set_compact restated: (tuples, src) of merge(t, {}) -- OR-Set: every
    distinct tag with its tomb-OR; LWW: every key's maximal tag with its first
    copy's tomb -- without the dead tuples when ``drop_dead`` (a cut that makes
    every tag stable); src = the index in t of the first copy."""
    key, ts, rep, tomb = t
    n = len(key)
    if n == 0:
        return tuple(x[:0] for x in t), np.zeros(0, np.int64)
    tag_new = np.ones(n, bool)
    tag_new[1:] = (key[1:] != key[:-1]) | (ts[1:] != ts[:-1]) | (rep[1:] != rep[:-1])
    first = np.flatnonzero(tag_new)
    if lww:
        tkey = key[first]
        last = np.ones(len(first), bool)
        last[:-1] = tkey[1:] != tkey[:-1]
        src = first[last]
        tb = tomb[src]
    else:
        src = first
        tb = np.maximum.reduceat(tomb, first)
    if drop_dead:
        src, tb = src[tb == 0], tb[tb == 0]
    return (key[src], ts[src], rep[src], tb.astype(np.uint8)), src.astype(np.int64)


def composed_win(t, lww):
    """What a caller composes from the calls that were there before the read:
    OR-Set -- compact under an all-2^64-1 cut (the live tags), an LWW
    compaction of that (each key's greatest), the two source-index arrays
    composed; LWW -- one compaction and the members among its rows."""
    if lww:
        c, src = np_compact(t, True, False)
        return src[c[3] == 0]
    c, src1 = np_compact(t, False, True)
    _, src2 = np_compact(c, True, False)
    return src1[src2]


def with_copies(t, rng, max_copies=4, p_tomb=0.3):
    """Every tuple of t repeated 1 .. max_copies times (the copies of one tag
    stay adjacent, so the order holds), the copies' tombs drawn afresh for a
    share of the tags: mixed tombs within a tag."""
    key, ts, rep, tomb = t
    c = rng.integers(1, max_copies + 1, len(key))
    out = [np.repeat(x, c) for x in (key, ts, rep, tomb)]
    flip = (rng.random(len(out[3])) < p_tomb).astype(np.uint8)
    out[3] = (out[3] ^ flip).astype(np.uint8)
    return tuple(out)
