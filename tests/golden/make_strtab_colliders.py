#!/usr/bin/env python3
"""Writes tests/golden/strtab_colliders.json: byte strings that collide under
the device string tables' hash (crdt_strtab, csrc/codec.hip: 32-bit FNV-1a,
offset basis 2166136261, prime 16777619), for the collision / wrap-around
tests of the interning (tests/test_strtab_colliders.py,
tests/test_gpu_codec_collisions.py).

FNV-1a is invertible byte by byte (the prime is odd: h' = ((h ^ b) * P) mod
2^32  <=>  h = (h' * P^-1 mod 2^32) ^ b), so a string with a chosen hash is
found by meeting in the middle: the states after PREFIX + one of the 40^4
four-byte words over a 40-character alphabet (forward) against the states
from which two trailing bytes reach the target (backward, 65536 of them):
about 40^4 * 2^16 / 2^32 = 39 matches per prefix.  Prefixes are arbitrary
bytes (NUL and 0xFF among them), the inverted bytes take any value.

Pure Python / numpy, a fixed enumeration order, no randomness: running it
again reproduces the committed file byte for byte.  Strings are hex-encoded.

  cluster  >= 8 strings with ONE hash32: two of 4 bytes, two of 6, one of 7,
           one of 8, two of 9, one of 12, one of 33
  pairs    the four English pairs, same-length pairs of 4 .. 7 bytes, one
           of 8 and one of 11 bytes
  last     hash & 0xFFFF == 0xFFFF: home entry = the last entry of every
           table of up to 65536 entries (lengths 4 .. 20)
  first    hash & 0xFFFF == 0: home entry 0 (lengths 4 .. 20)
  extreme  hash32 == 0x00000000 and == 0xFFFFFFFF (6 and 9 bytes)
"""
import json
import os

import numpy as np

BASIS, PRIME, M32 = 2166136261, 16777619, 0xFFFFFFFF
PRIME_INV = pow(PRIME, -1, 1 << 32)
ALPHABET = b"abcdefghijklmnopqrstuvwxyz0123456789-_.:"
assert len(ALPHABET) == 40 and len(set(ALPHABET)) == 40

ENGLISH = [(b"costarring", b"liquid"), (b"declinate", b"macallums"), (b"altarage", b"zinke"),
           (b"altarages", b"zinkes")]


def fnv1a(s: bytes, h: int = BASIS) -> int:
    for b in s:
        h = ((h ^ b) * PRIME) & M32
    return h


_IDX = np.arange(40 ** 4, dtype=np.int64)
_ALPHA = np.frombuffer(ALPHABET, np.uint8).astype(np.uint64)
_COLS = [_ALPHA[(_IDX // 40 ** (3 - k)) % 40] for k in range(4)]      # word i = base-40 digits of i, big end first


def word(i: int) -> bytes:
    return bytes(ALPHABET[(i // 40 ** (3 - k)) % 40] for k in range(4))


def forward(prefix: bytes) -> np.ndarray:
    """hash32 state after prefix + word(i), for every i (uint64 array, values < 2^32)."""
    h = np.full(40 ** 4, fnv1a(prefix), np.uint64)
    for c in _COLS:
        h = ((h ^ c) * np.uint64(PRIME)) & np.uint64(M32)
    return h


def low16(prefix: bytes, want: int, count: int):
    """The first `count` strings prefix + word(i), by i, whose hash has low 16 bits == want."""
    hit = np.flatnonzero((forward(prefix) & np.uint64(0xFFFF)) == np.uint64(want))
    assert len(hit) >= count, (prefix, want, len(hit))
    return [prefix + word(int(i)) for i in hit[:count]]


def reach(prefix: bytes, target: int, count: int):
    """The first `count` strings prefix + word(i) + b1 b2 with hash32 == target,
    in byte-string order."""
    b2 = np.arange(256, dtype=np.uint64)
    s1 = ((np.uint64(target) * np.uint64(PRIME_INV)) & np.uint64(M32)) ^ b2          # state before b2
    b1 = np.arange(256, dtype=np.uint64)
    s0 = ((s1[None, :] * np.uint64(PRIME_INV)) & np.uint64(M32)) ^ b1[:, None]       # [b1, b2]: state before b1
    back = s0.ravel()
    fw = forward(prefix)
    out = []
    for i in np.flatnonzero(np.isin(fw, back)):
        for j in np.flatnonzero(back == fw[i]):
            out.append(prefix + word(int(i)) + bytes([int(j) // 256, int(j) % 256]))
    out.sort()
    assert len(out) >= count, (prefix, hex(target), len(out))
    for s in out[:count]:
        assert fnv1a(s) == target
    return out[:count]


def word_pairs(count: int):
    """The first `count` colliding pairs of four-byte words, by (hash, index)."""
    fw = forward(b"")
    order = np.argsort(fw, kind="stable")
    same = np.flatnonzero(fw[order][1:] == fw[order][:-1])
    assert len(same) >= count
    return [(word(int(order[p])), word(int(order[p + 1]))) for p in same[:count]]


def build():
    wp = word_pairs(12)
    # same-length pairs of 4 .. 7 bytes: colliding words stay colliding under a common suffix
    suffix = [b"", b"", b"", b"0", b"\x00", b"\xff", b"xy", b"\x00\x00", b"\xff\x00", b"-12", b"\x00\xff\x00", b"zzz"]
    short_pairs = [(a + s, b + s) for (a, b), s in zip(wp, suffix)]
    # ... and of 8 and 11 bytes (one packed word; the byte walk)
    more = word_pairs(15)[13:]
    long_pairs = [(a + s, b + s) for (a, b), s in zip(more, [b"\x00\xff89", b"-suffix"])]
    # the cluster: the hash of one more colliding word pair, reached from other prefixes
    ca, cb = word_pairs(13)[12]
    target = fnv1a(ca)
    cluster = [ca, cb]                                                   # two of 4 bytes
    cluster += reach(b"", target, 2)                                     # two of 6
    cluster += reach(b"\x00", target, 1)                                 # one of 7
    cluster += reach(b"\xff\x00", target, 1)                             # one of 8
    cluster += reach(b"\x00\xff\x7f", target, 2)                         # two of 9
    cluster += reach(b"\xff\xff\x00\x00k=", target, 1)                   # one of 12
    cluster += reach(b"\x00\xff" + b"a long collider prefix...", target, 1)   # one of 33
    last, first = [], []
    for dst, want in ((last, 0xFFFF), (first, 0)):
        dst += low16(b"", want, 8)                                       # 4 bytes
        dst += low16(b"\x00", want, 4)                                   # 5
        dst += low16(b"\xff\x00\x01", want, 4)                           # 7
        dst += low16(b"\x00\x00\xff\xff", want, 4)                       # 8
        dst += low16(b"\xffkey:", want, 6)                               # 9
        dst += low16(b"\x00sixteen byte pre", want, 2)                   # 20
    extreme = {}
    for t in (0x00000000, 0xFFFFFFFF):
        extreme["%08x" % t] = reach(b"", t, 2) + reach(b"\x00\xffz", t, 2)   # two of 6, two of 9
    return target, cluster, ENGLISH + short_pairs + long_pairs, last, first, extreme


def check(target, cluster, pairs, last, first, extreme):
    assert len(cluster) >= 8 and len(set(cluster)) == len(cluster)
    assert all(fnv1a(s) == target for s in cluster)
    assert sorted(map(len, cluster)) == [4, 4, 6, 6, 7, 8, 9, 9, 12, 33]
    assert any(0 in s for s in cluster) and any(255 in s for s in cluster)
    for a, b in pairs:
        assert a != b and fnv1a(a) == fnv1a(b), (a, b)
    assert sum(len(a) == len(b) <= 7 for a, b in pairs) >= 8
    for s in last:
        assert fnv1a(s) & 0xFFFF == 0xFFFF
    for s in first:
        assert fnv1a(s) & 0xFFFF == 0
    assert len(set(last)) == len(last) >= 24 and len(set(first)) == len(first) >= 24
    for t, ss in extreme.items():
        assert all(fnv1a(s) == int(t, 16) for s in ss)
        assert any(len(s) <= 7 for s in ss) and any(len(s) >= 9 for s in ss)
    every = cluster + [s for p in pairs for s in p] + last + first + [s for ss in extreme.values() for s in ss]
    assert len(set(every)) == len(every)                                 # the sets may be mixed freely
    assert b"" not in every


def render() -> str:
    """The fixture file's text."""
    target, cluster, pairs, last, first, extreme = build()
    check(target, cluster, pairs, last, first, extreme)
    H = lambda s: s.hex()
    doc = {
        "hash": {"name": "FNV-1a 32", "offset_basis": BASIS, "prime": PRIME},
        "cluster": {"hash32": "%08x" % target, "strings": [H(s) for s in cluster]},
        "pairs": [[H(a), H(b)] for a, b in pairs],
        "last": [H(s) for s in last],
        "first": [H(s) for s in first],
        "extreme": {t: [H(s) for s in ss] for t, ss in extreme.items()},
    }
    return json.dumps(doc, indent=1) + "\n"


if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "strtab_colliders.json")
    with open(out, "w") as f:
        f.write(render())
    print(out)
