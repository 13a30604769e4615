"""The collider fixture of the device string tables (crdt_strtab,
csrc/codec.hip), checked without a GPU.

tests/golden/strtab_colliders.json (written by make_strtab_colliders.py)
holds byte strings chosen by their 32-bit FNV-1a hash: full collisions, home
entries at the two ends of the table, the hashes 0 and 0xFFFFFFFF.  The GPU
tests (tests/test_gpu_codec_collisions.py) rely on those properties; here
every hash is recomputed by a restatement written in this file, so a stale or
hand-edited fixture -- or a changed hash in codec.hip -- fails here and the
GPU tests never run vacuously.  The body builder those tests use and the host
decode are checked against the plain Python dicts the bodies were built from.
"""
import importlib.util
import os
import re

from codec_util import _raw_body, fnv1a, load_colliders
from crdt_amd.server import Server

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

C = load_colliders()

ENGLISH = [(b"costarring", b"liquid"), (b"declinate", b"macallums"), (b"altarage", b"zinke"),
           (b"altarages", b"zinkes")]


def _fnv1a(s: bytes) -> int:
    h = 0x811C9DC5                                     # 2166136261
    for b in s:
        h ^= b
        h = (h * 0x01000193) % (1 << 32)               # 16777619
    return h


def _every():
    return (C["cluster"] + [s for p in C["pairs"] for s in p] + C["last"] + C["first"] +
            [s for ss in C["extreme"].values() for s in ss])


def test_fixture_properties():
    cl = C["cluster"]
    assert len(cl) >= 8 and len(set(cl)) == len(cl)
    assert {_fnv1a(s) for s in cl} == {C["cluster_hash"]}
    by_len = {}
    for s in cl:
        by_len.setdefault(len(s), []).append(s)
    short = {n: v for n, v in by_len.items() if n <= 7}
    assert any(len(v) >= 2 for v in short.values()) and len(short) >= 2    # two of one length <= 7, one of another
    assert 8 in by_len                                                     # the last single-word compare
    assert any(n >= 9 and len(v) >= 2 for n, v in by_len.items())          # two for the byte walk
    assert any(n >= 33 for n in by_len)
    assert any(0 in s for s in cl) and any(0xFF in s for s in cl)
    assert C["pairs"][:4] == ENGLISH
    for a, b in C["pairs"]:
        assert a != b and _fnv1a(a) == _fnv1a(b), (a, b)
    assert sum(1 for a, b in C["pairs"] if len(a) == len(b) <= 7) >= 8
    for name, low in (("last", 0xFFFF), ("first", 0)):
        ss = C[name]
        assert len(ss) >= 24 and len(set(ss)) == len(ss)
        assert all(_fnv1a(s) & 0xFFFF == low for s in ss), name
        assert any(len(s) <= 7 for s in ss) and any(len(s) == 8 for s in ss) and any(len(s) >= 9 for s in ss)
    assert set(C["extreme"]) == {0x00000000, 0xFFFFFFFF}
    for h, ss in C["extreme"].items():
        assert len(ss) >= 2 and all(_fnv1a(s) == h for s in ss)
        assert any(len(s) <= 7 for s in ss) and any(len(s) >= 9 for s in ss)
    # one string never sits in two sets, and none is empty: the GPU tests mix
    # the sets in one table (as keys, as values) and add b"" themselves
    every = _every()
    assert len(set(every)) == len(every) and b"" not in every
    assert all(fnv1a(s) == _fnv1a(s) for s in every)                       # the helper the GPU tests use


def test_codec_hash_is_the_fixtures_hash():
    """hash32 and hash32_short in codec.hip still are FNV-1a with the offset
    basis and prime the fixture was made for.  If this fails the hash changed:
    change make_strtab_colliders.py (and the restatements here and in
    codec_util.py) to the new hash and regenerate strtab_colliders.json."""
    assert C["hash"] == {"name": "FNV-1a 32", "offset_basis": 2166136261, "prime": 16777619}
    with open(os.path.join(ROOT, "crdt_amd", "csrc", "codec.hip")) as f:
        src = f.read()
    for fn in ("hash32", "hash32_short"):
        m = re.search(r"uint32_t %s\([^)]*\)\s*\{(.*?)\n\}" % fn, src, re.S)
        assert m, f"{fn} not found in codec.hip"
        body = m.group(1)
        assert "2166136261u" in body and "16777619u" in body, f"{fn}: regenerate tests/golden/strtab_colliders.json"
        assert re.search(r"\(h \^ .*\) \* 16777619u", body), f"{fn}: xor, then multiply (FNV-1a)"


def test_fixture_regenerates_byte_for_byte():
    spec = importlib.util.spec_from_file_location("make_strtab_colliders",
                                                  os.path.join(GOLDEN, "make_strtab_colliders.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(GOLDEN, "strtab_colliders.json")) as f:
        assert f.read() == gen.render()


def _dec(b: bytes) -> str:
    return b.decode("utf-8", "surrogateescape")        # as Server's maps present Go's byte strings


def test_host_ingest_of_collider_bodies():
    """Binary bodies built from the collider sets (codec_util._raw_body, the
    builder of the GPU tests) through the host decode: RemoteDiff == the
    dicts the bodies were built from, colliding keys as separate members."""
    every = _every()
    # one pair per entry: every collider as a key, its set's next string as the value
    single = {i + 1: {s: every[(i + 1) % len(every)]} for i, s in enumerate(every)}
    # whole sets as the keys of one entry (keys ascending, as the wire form has them)
    multi = {1000 + i: {s: ss[(j + 1) % len(ss)] for j, s in enumerate(ss)}
             for i, ss in enumerate([C["cluster"], [s for p in C["pairs"] for s in p], C["last"], C["first"],
                                     C["extreme"][0] + C["extreme"][0xFFFFFFFF] + [b""]])}
    for want in (single, multi, {**single, **multi}):
        body = _raw_body([(t, sorted(kv.items())) for t, kv in sorted(want.items())])
        host = Server(None, 9000)
        assert host.IngestBinary(body) == 0
        assert host.RemoteDiff.Keys() == sorted(want)
        for t, kv in want.items():
            got, found = host.RemoteDiff.Get(t)
            assert found and got == {_dec(k): _dec(v) for k, v in kv.items()}, t
            assert len(got) == len(kv)                                     # colliders stay apart
        host.close()
