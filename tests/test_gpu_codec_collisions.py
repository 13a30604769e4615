"""GPU: string interning (crdt_strtab, csrc/codec.hip) under hash collisions,
probe chains that wrap round the table's end, rehashes and the hashes 0 and
0xFFFFFFFF -- the cases seeded data never produces (two of a few hundred
strings share a 32-bit hash with probability ~1e-5).

Two distinct strings that receive one id merge into one CurrentState entry
and nothing faults, so every input here is built from the collider fixture
(tests/golden/strtab_colliders.json; its properties are asserted without a
GPU by tests/test_strtab_colliders.py): full hash32 collisions of every
length class tab_claim compares differently (<= 7 bytes: the short form
beside a resolved entry; <= 8: one packed word against a pending claimer or
an arena string; >= 9: the byte walk), strings whose home entry is the
table's last or first one, and the two extreme hashes.

The expectation is always the Python list the test built its input from,
never another call into the library.  After EVERY call (_Tab.accept):
  (a) len(table) == the number of distinct strings accepted so far;
  (b) strings() has no duplicates and its set is the expected set;
  (c) every returned id (kv_key - slot_base, kv_val, intern's ids) resolves
      through strings() to exactly the bytes presented at that position;
  (d) strings()[:n_before] is unchanged: ids of earlier calls never move;
  (e) the new strings' ids are exactly n_before .. n_after - 1.
Id order inside one call follows the claim races, so ids are compared through
the strings they resolve to.

Table sizes.  tab_reserve gives a table pow2_at_least(4 * (n + pairs of the
call)) entries (1024 at the least) whenever 2 * (n + pairs) exceeds its
size.  Every call here keeps n + pairs <= 16384 (MAX_LOAD, asserted per call
by a model of that rule), so no table exceeds 65536 entries and the
fixture's `last` / `first` strings (low 16 hash bits all set / all clear)
have the last / first entry as their home whatever size is reached.

kBodyFull cannot be reached through the ABI: tab_reserve sizes both tables
for every pair of a call before the claim pass runs, so tab_claim always
finds an empty entry.  There is no test (and no failpoint) for it.

Every test runs under each decode form (codec.small) and each claim form
(codec.short_tab): the default pair on the product build, the others in the
diagnostic child suite (tests/test_gpu_diag_build.py).
"""
import numpy as np
import pytest
from knobs import set_knob

from codec_util import _decode, _raw_body, fnv1a, load_colliders
from crdt_amd import codec
from crdt_amd.engine import Engine
from crdt_amd.server import Server
from oracle import pyref

pytestmark = [pytest.mark.gpu, pytest.mark.diag]

MAX_LOAD = 16384                                       # interned strings + pairs of a call, per table

C = load_colliders()
CLUSTER = C["cluster"]
PAIRS = C["pairs"]
SHORT_PAIRS = [(a, b) for a, b in PAIRS if len(a) == len(b) <= 7]
LAST, FIRST = C["last"], C["first"]
ZERO, ONES = C["extreme"][0], C["extreme"][0xFFFFFFFF]
EXTREME = ZERO + ONES
SETS = {"cluster": CLUSTER, "pairs": [s for p in PAIRS for s in p], "last": LAST, "first": FIRST, "extreme": EXTREME}
EVERY = [s for ss in SETS.values() for s in ss]
GROUPS = [CLUSTER] + [list(p) for p in PAIRS]          # strings of one hash32 each


@pytest.fixture(params=[(s, t) for s in (1, 0, 2, 3) for t in (3, 0, 1, 2, 4)],
                ids=lambda p: f"small{p[0]}-short_tab{p[1]}", autouse=True)
def variant(request, eng):
    """codec.small: 1 the product's choice by size, 0 multi-pass, 2 one-pass,
    3 one-pass coalesced.  codec.short_tab: 0 the byte walk for every
    candidate, 1 short forms, 2 - 4 the two-home-entries fast path with one,
    two and three pairs per thread (256 / 512 / 768 pairs per workgroup)."""
    try:
        set_knob(b"codec.small", request.param[0])
        set_knob(b"codec.short_tab", request.param[1])
        yield request.param
    finally:
        set_knob(b"codec.small", 1)
        set_knob(b"codec.short_tab", 3)


class _Tab:
    """A string table and the Python list its strings() must equal."""

    def __init__(self, eng, *cap):
        self.tab = codec.StrTab(eng, *cap)
        self.want = []                                 # strings() after the last call, checked by accept()
        self.H = 1024                                  # tab_reserve's rule, restated

    def accept(self, presented, ids, more):
        """After a call that presented `presented` (bytes, in position order)
        and returned `ids` for them, reserving room for `more` strings."""
        n0 = len(self.want)
        assert n0 + more <= MAX_LOAD
        if 2 * (n0 + more) > self.H:
            self.H = max(1024, 1 << (4 * (n0 + more) - 1).bit_length())
        assert self.H <= 65536
        new = set(presented) - set(self.want)
        ss = self.tab.strings()
        assert len(self.tab) == n0 + len(new)                                        # (a)
        assert len(set(ss)) == len(ss) and set(ss) == set(self.want) | new           # (b)
        ids = np.asarray(ids, np.int64)
        assert len(ids) == len(presented) and ids.min(initial=0) >= 0 and ids.max(initial=0) < len(ss)
        bad = [(i, s, ss[j]) for i, (s, j) in enumerate(zip(presented, ids.tolist())) if ss[j] != s]
        assert not bad, bad[:4]                                                      # (c)
        assert ss[:n0] == self.want                                                  # (d)
        assert {j for s, j in zip(presented, ids.tolist()) if s in new} == set(range(n0, len(ss)))   # (e)
        self.want = ss
        return ids


def _intern(t, strs):
    strs = list(strs)
    return t.accept(strs, t.tab.intern(strs).astype(np.int64), len(strs))


def _dec(eng, K, V, bodies):
    """One crdt_gossip_decode of bodies = [[(key, value), ...], ...], one pair
    per entry (so the order flags do not apply): every body decodes on the
    device, and both tables pass accept().  Returns (key ids, value ids)."""
    raw = [_raw_body([(i + 1, [kv]) for i, kv in enumerate(b)]) for b in bodies]
    dec, st, kk, kv = _decode(eng, raw, K.tab, V.tab)
    assert st.tolist() == [0] * len(bodies), st
    flat = [(bi, k, v) for bi, b in enumerate(bodies) for k, v in b]
    n = len(flat)
    assert dec["r_kv"].cpu().numpy().tolist() == list(range(3, 3 + n + 1))           # kv_base 3, one pair per entry
    for a in (kk, kv):                                                                # nothing outside [3, 3 + n)
        assert a[:3].tolist() == [-1] * 3 and a[3 + n] == -1
    kid = kk[3:3 + n].astype(np.int64) - 1000 * np.array([bi for bi, _, _ in flat], np.int64)
    kid = K.accept([k for _, k, _ in flat], kid, n)
    vid = V.accept([v for _, _, v in flat], kv[3:3 + n].astype(np.int64), n)
    return kid, vid


def _fill_key(b, i):
    """Filler keys, one per (body, position): 7 bytes (a short form), 8 (one
    word) and 20 (the byte walk) in turn."""
    return (b"f%d%05d" % (b, i), b"g%d%06d" % (b, i), b"filler-key-%d-%07d" % (b, i))[i % 3]


def _fill_val(i):
    """Filler values: a few strings many pairs share (pending duplicates)."""
    return b"v%d" % (i % 7) if i % 4 else b"a-longer-value-%d" % (i % 5)


def _fillers(tag, n):
    return [(b"%s%04d" % (tag, i), b"%s-%05d" % (tag, i), b"%s-long-%08d" % (tag, i))[i % 3] for i in range(n)]


def _layout(n_bodies, n):
    return [[(_fill_key(b, i), _fill_val(i)) for i in range(n)] for b in range(n_bodies)]


# ------------------------------------------------------------ StrTab.intern
def test_intern_whole_cluster(eng):
    t = _Tab(eng)
    _intern(t, CLUSTER)
    assert len(t.tab) == len(CLUSTER)
    _intern(t, CLUSTER[::-1])                                          # found again, each under its own id
    assert eng.device_status(clear=True) == 0


@pytest.mark.parametrize("name", list(SETS))
def test_intern_each_set(eng, name):
    t = _Tab(eng)
    _intern(t, SETS[name])
    assert len(t.tab) == len(SETS[name])
    assert eng.device_status(clear=True) == 0


def test_intern_every_string_three_times(eng):
    """Each collider twice at adjacent positions (one wave) and a third time
    more than 768 positions on (another claim workgroup in every form)."""
    strs = [x for s in EVERY for x in (s, s)] + _fillers(b"t", 800) + EVERY
    third = {s: i for i, s in enumerate(strs)}                         # last position of each
    assert all(third[s] - (2 * j + 1) > 768 for j, s in enumerate(EVERY))
    t = _Tab(eng)
    ids = _intern(t, strs)
    assert len(t.tab) == len(EVERY) + 800
    for j, s in enumerate(EVERY):
        assert ids[2 * j] == ids[2 * j + 1] == ids[third[s]]
    assert eng.device_status(clear=True) == 0


def test_intern_empty_string_with_extreme_hashes(eng):
    t = _Tab(eng)
    _intern(t, [b""] + EXTREME + [b""])
    assert len(t.tab) == 1 + len(EXTREME)
    _intern(t, EXTREME[::-1] + [b""])
    assert eng.device_status(clear=True) == 0


# ------------------------------------- pending against each other, one decode
def _positions(mode, g, m):
    """(body, pair index) of the first and the second appearance of member m
    of group g."""
    if mode == "adjacent":          # neighbours; both appearances inside one 32-pair block: one wave
        return (0, 32 * g + m), (0, 32 * g + 16 + m)
    if mode == "waves":             # 64 apart: another wave (of the same workgroup while within 256 / 512 / 768)
        return (0, g + 64 * m), (0, g + 64 * (m + 10))
    if mode == "workgroups":        # >= 1600 apart: another claim workgroup in every form (at most 768 pairs each)
        return (0, 1600 * (m % 2) + 8 * g + m // 2), (0, 1600 * ((m + 1) % 2) + 200 + 8 * g + m // 2)
    assert mode == "bodies"         # another body of the same call
    return (m % 3, 8 * g + m // 3), ((m + 1) % 3, 200 + 8 * g + m // 3)


@pytest.mark.parametrize("mode,n_bodies,n", [("adjacent", 1, 600), ("waves", 1, 1300), ("workgroups", 1, 2000),
                                             ("bodies", 3, 400)])
def test_decode_colliders_pending_against_each_other(eng, mode, n_bodies, n):
    """Fresh tables, so every string of the call is pending: a collider meets
    its hash in an entry claimed by another pair of the same call and is told
    apart (or recognised, its second appearance) through the body's own
    bytes.  Each collider is the key AND the value of its pair: the key and
    the value table each see the whole cluster and every pair."""
    bodies = _layout(n_bodies, n)
    used = {}
    for g, group in enumerate(GROUPS):
        for m, s in enumerate(group):
            for b, i in _positions(mode, g, m):
                assert (b, i) not in used and i < n
                used[(b, i)] = s
                bodies[b][i] = (s, s)
    if mode == "workgroups":
        for g, group in enumerate(GROUPS):
            assert abs(_positions(mode, g, 0)[0][1] - _positions(mode, g, 1)[0][1]) >= 1600
    K, V = _Tab(eng), _Tab(eng)
    _dec(eng, K, V, bodies)
    assert set(s for g in GROUPS for s in g) <= set(K.want) and set(s for g in GROUPS for s in g) <= set(V.want)
    assert eng.device_status(clear=True) == 0


# --------------------------------------------------------------- across calls
def test_decode_colliders_across_calls(eng):
    """Call 1 interns one half of every pair / cluster; call 2 presents the
    other half (compared against resolved entries of its own hash) and the
    first half again; a third, identical call interns nothing."""
    half1 = [s for g in GROUPS for s in g[0::2]]
    half2 = [s for g in GROUPS for s in g[1::2]]
    K, V = _Tab(eng), _Tab(eng)
    b1 = _layout(1, 300)
    for i, s in enumerate(half1):
        b1[0][5 * i + 1] = (s, s)
    k1, v1 = _dec(eng, K, V, b1)
    id1 = {s: (int(k1[5 * i + 1]), int(v1[5 * i + 1])) for i, s in enumerate(half1)}
    b2 = _layout(1, 300)
    for i, s in enumerate(half2 + half1):
        b2[0][5 * i + 2] = (s, s)
    n_k, n_v = len(K.want), len(V.want)
    k2, v2 = _dec(eng, K, V, b2)
    # (new filler keys too: those of the positions that held the first half in call 1)
    assert len(K.want) == n_k + len(half2) + len(half1) and len(V.want) == n_v + len(half2)
    for i, s in enumerate(half1):                                      # the first half keeps its ids
        assert (int(k2[5 * (len(half2) + i) + 2]), int(v2[5 * (len(half2) + i) + 2])) == id1[s]
    for i, s in enumerate(half2):                                      # the second half got new ones
        assert k2[5 * i + 2] >= n_k and v2[5 * i + 2] >= n_v
    n_k, n_v = len(K.want), len(V.want)
    k3, v3 = _dec(eng, K, V, b2)
    assert (len(K.want), len(V.want)) == (n_k, n_v)
    assert np.array_equal(k2, k3) and np.array_equal(v2, v3)
    assert eng.device_status(clear=True) == 0


# ---------------------------------------------------------------- wrap-around
@pytest.mark.parametrize("order", ["first_then_last", "last_then_first"])
def test_probe_chain_wraps_from_last_entry_to_entry_0(eng, order):
    """A tiny table (1024 entries, never grown here).  `first` occupies
    entries 0 ..; the chain of `last` starts at entry 1023 and runs over them.
    In the other order `last` fills 1023, 0, 1, .. and `first` finds its home
    taken by strings that wrapped."""
    a, b = (FIRST, LAST) if order == "first_then_last" else (LAST, FIRST)
    assert all(fnv1a(s) & 1023 == 1023 for s in LAST) and all(fnv1a(s) & 1023 == 0 for s in FIRST)
    K, V = _Tab(eng, 4, 64), _Tab(eng, 4, 64)
    _intern(K, a)
    _intern(V, a)
    _dec(eng, K, V, [[(s, s) for s in b]])
    n_k, n_v = len(K.want), len(V.want)
    assert n_k == n_v == len(a) + len(b)
    k1, v1 = _dec(eng, K, V, [[(s, t) for s, t in zip(a + b, b + a)]])   # both sets again: nothing new
    assert (len(K.want), len(V.want)) == (n_k, n_v)
    assert K.H == V.H == 1024
    assert eng.device_status(clear=True) == 0


# --------------------------------------------------------------------- rehash
def test_colliders_keep_their_ids_across_rehashes(eng):
    """Every collider interned into a tiny table, which then grows twice (the
    sizes by tab_reserve's rule: 1024 -> 4096 -> 16384 entries): k_rehash
    re-inserts by hash alone and rewrites the short forms.  After each growth
    a decode of every collider as key and value resolves to the first ids."""
    K, V = _Tab(eng, 4, 64), _Tab(eng, 4, 64)
    body = [[(s, s) for s in EVERY]]
    k0, v0 = _dec(eng, K, V, body)
    sizes = [K.H]
    for tag, n in ((b"p", 600), (b"q", 3000)):
        _intern(K, _fillers(tag, n))
        _intern(V, _fillers(tag, n))
        sizes.append(K.H)
        assert K.H == V.H
        n_k, n_v = len(K.want), len(V.want)
        k1, v1 = _dec(eng, K, V, body)
        assert (len(K.want), len(V.want)) == (n_k, n_v)
        assert np.array_equal(k0, k1) and np.array_equal(v0, v1)
        assert K.H == sizes[-1]                                        # the decode itself did not grow it
    assert sizes == [1024, 4096, 16384]
    assert eng.device_status(clear=True) == 0


# ---------------------------------------------------- half-resolved fast path
def test_short_pairs_with_one_side_unresolved(eng):
    """Pairs of key <= 7 and value <= 7 bytes (codec.short_tab 2 - 4 probe
    both home entries at once and resolve the pair there only when BOTH
    match).  a_i / b_i collide: b_i, interned one call after a_i, sits one
    probe past their common home entry."""
    A = [a for a, _ in SHORT_PAIRS]
    B = [b for _, b in SHORT_PAIRS]
    assert len(A) >= 12
    K, V = _Tab(eng, 4, 64), _Tab(eng, 4, 64)
    _intern(K, A[0:6])
    _intern(V, A[6:12])
    _intern(K, B[0:3])
    _intern(V, B[6:9])
    body = [
        (A[3], b"nv1"), (B[0], b"nv2"),                    # only the key is interned (at home / one probe on)
        (b"nk1", A[9]), (b"nk2", B[6]),                    # only the value is interned
        (B[1], A[10]), (A[4], B[7]), (B[2], B[8]),         # both interned, one / the other / both one probe on
        (A[5], A[11]),                                     # both at home: resolved by the fast path
        (b"nk3", b"nv3"),                                  # neither
        (B[3], B[9]),                                      # neither, and both home entries hold the collider
        (A[3], B[9]), (B[3], A[9]),                        # pending collider on one side, resolved on the other
    ]
    assert all(len(k) <= 7 and len(v) <= 7 for k, v in body)
    n_k, n_v = len(K.want), len(V.want)
    k1, v1 = _dec(eng, K, V, [body])
    assert len(K.want) == n_k + 4 and len(V.want) == n_v + 4          # nk1-3, B[3]; nv1-3, B[9]
    k2, v2 = _dec(eng, K, V, [body])                                    # all resolved now
    assert len(K.want) == n_k + 4 and len(V.want) == n_v + 4
    assert np.array_equal(k1, k2) and np.array_equal(v1, v2)
    assert eng.device_status(clear=True) == 0


# ------------------------------------------------------------- extreme hashes
@pytest.mark.parametrize("id0", ["zero", "ones"])
def test_extreme_hashes_as_keys_and_values(eng, id0):
    """hash32 0 with id 0 is the all-zero entry word; hash32 0xFFFFFFFF
    entries differ from the empty entry only in their low word."""
    z = (ZERO if id0 == "zero" else ONES)[0]
    assert fnv1a(z) == (0 if id0 == "zero" else 0xFFFFFFFF)
    K, V = _Tab(eng, 4, 64), _Tab(eng, 4, 64)
    k, v = _dec(eng, K, V, [[(z, z)]])
    assert k.tolist() == [0] and v.tolist() == [0]
    body = [(s, t) for s, t in zip(EXTREME, EXTREME[1:] + EXTREME[:1])] + [(z, z), (b"", z), (z, b"")]
    k1, v1 = _dec(eng, K, V, [body])                                    # same call: pending against each other
    assert len(K.want) == len(V.want) == len(EXTREME) + 1
    assert k1[len(EXTREME)] == 0 and v1[len(EXTREME)] == 0              # z kept id 0
    k2, v2 = _dec(eng, K, V, [body[::-1], body])                        # across calls: all resolved
    assert len(K.want) == len(V.want) == len(EXTREME) + 1
    assert np.array_equal(k2[len(body):], k1) and np.array_equal(v2[len(body):], v1)
    assert eng.device_status(clear=True) == 0


# ----------------------------------------------------------------- end to end
def _sig(diff):
    return [[t, "local" if isinstance(v, pyref.Command) else "remote"] for t, v in sorted(diff.items())]


def test_server_merge_keeps_colliding_keys_apart(eng):
    """A device-resident Server pulls binary bodies whose keys and values
    collide (altarage / zinke, declinate / macallums, a same-length pair of
    <= 7 bytes), then merges: CurrentState and the Diff == the Python
    restatement of merge() (oracle/pyref.py) on the same dicts."""
    (a, b), (a2, b2) = [(x.decode(), y.decode()) for x, y in SHORT_PAIRS[:2]]
    # A context's Servers share its key and value tables, and the session's
    # context may know these strings from an earlier test: in a context of its
    # own the colliders of the first pull meet as pending claims, those of the
    # second meet resolved entries.
    own = Engine(0)
    try:
        s = Server(own, 8080)
        s.Diff.Put(10 ** 6, {"seed": "0"})                 # the merge walk inserts remote entries below a local one
        diff = {10 ** 6: {"seed": "0"}}
        pulls = [
            {1: {"altarage": "costarring"}, 2: {"zinke": "liquid"}, 3: {a: a2}, 4: {b: b2},
             5: {"declinate": "macallums", "macallums": "declinate"},
             6: {"altarage": "liquid", "zinke": "costarring", a: b2, b: a2}},
            {7: {"zinke": "zinkes", "altarage": "altarages"}, 8: {b: a, a: b}, 9: {"declinate": "5", "macallums": "-3"},
             10: {"declinate": "7", "macallums": "1", "liquid": "altarage", "costarring": "zinke"}},
        ]
        for remote in pulls:
            peer = Server(None, 9100)
            for t, kv in remote.items():
                peer.Diff.Put(t, kv)
            st, body = peer.GossipBinary()
            peer.close()
            assert st == 200 and s.IngestBinary(body) == 0
            s.merge()
            diff, state = pyref.merge(diff, remote)
            assert s.CurrentState == state
            assert s.DiffSignature == _sig(diff)
            for x, y in (("altarage", "zinke"), ("declinate", "macallums"), (a, b)):
                assert x in state and y in state and state[x] != state[y]   # (the restatement: separate entries)
        s.close()
        assert own.device_status(clear=True) == 0
    finally:
        own.close()
    assert eng.device_status(clear=True) == 0
