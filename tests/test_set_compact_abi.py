"""CPU: the tombstone-compaction entry points (crdt_set_compact,
crdt_vclock_stable_cut) are declared in include/crdt_amd.h, carried by
crdt_amd._lib.SIGNATURES with matching argument counts, surfaced by the Engine
(set_compact, set_compact_count, map_compact, vclock_stable_cut) and
Comm.stable_cut, and bound by the Go files (StableCut, SetCompact,
SetCompactCount).  Symbol export and the NULL-context rejection are
test_capi.py's, over every SIGNATURES entry."""
import glob
import os
import re

import pytest

from crdt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"crdt_set_compact": 10, "crdt_vclock_stable_cut": 5}


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


def test_python_surface():
    from crdt_amd.engine import Engine
    from crdt_amd.shard import Comm
    for name in ("set_compact", "set_compact_count", "map_compact", "vclock_stable_cut"):
        assert callable(getattr(Engine, name)), name
    assert callable(Comm.stable_cut)


def test_go_binding_defines_the_calls():
    src = ""
    for p in sorted(glob.glob(os.path.join(ROOT, "go", "crdt", "*.go"))):
        with open(p) as f:
            src += f.read()
    for fn in ("StableCut", "SetCompact", "SetCompactCount"):
        assert re.search(r"^func " + fn + r"\(", src, flags=re.M), fn
    assert "C.crdt_set_compact(" in src and "C.crdt_vclock_stable_cut(" in src
