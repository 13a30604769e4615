"""CPU: the range-digest entry points (crdt_set_digest, crdt_set_digest_diff,
crdt_set_select) are declared in include/crdt_amd.h, carried by
crdt_amd._lib.SIGNATURES with matching argument counts, surfaced by the Engine
(set_digest, digest_diff, set_select, set_select_count, map_select) and
crdt_amd.reconcile (key_splitters, reconcile_round), and bound by the Go files
(SetDigest, SetDigestDiff, SetSelect).  Symbol export and the NULL-context
rejection are test_capi.py's, over every SIGNATURES entry."""
import glob
import os
import re

import pytest

from crdt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"crdt_set_digest": 9, "crdt_set_digest_diff": 8, "crdt_set_select": 11}


@pytest.mark.parametrize("name", sorted(ARGS))
def test_header_declares(name):
    with open(os.path.join(ROOT, "include", "crdt_amd.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.M | re.S)
    assert m, name
    assert len(m.group(1).split(",")) == ARGS[name]


@pytest.mark.parametrize("name", sorted(ARGS))
def test_signatures_carry(name):
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name][1]) == ARGS[name]


def test_header_spells_out_the_hash():
    """A host in any language must be able to reproduce the digest."""
    with open(os.path.join(ROOT, "include", "crdt_amd.h")) as f:
        hdr = f.read()
    for c in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB"):
        assert c in hdr, c


def test_python_surface():
    from crdt_amd import reconcile
    from crdt_amd.engine import Engine
    for name in ("set_digest", "digest_diff", "set_select", "set_select_count", "map_select"):
        assert callable(getattr(Engine, name)), name
    assert callable(reconcile.key_splitters) and callable(reconcile.reconcile_round)


def test_go_binding_defines_the_calls():
    src = ""
    for p in sorted(glob.glob(os.path.join(ROOT, "go", "crdt", "*.go"))):
        with open(p) as f:
            src += f.read()
    for fn in ("SetDigest", "SetDigestDiff", "SetSelect"):
        assert re.search(r"^func " + fn + r"\(", src, flags=re.M), fn
    for c in ARGS:
        assert "C." + c + "(" in src, c
