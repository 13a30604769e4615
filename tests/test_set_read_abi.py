"""CPU: the set-read entry points (crdt_set_elements, crdt_u64_contains) are
declared in include/crdt_amd.h with their mode constants, carried by
crdt_amd._lib.SIGNATURES with matching argument counts, and bound by the Go
files (SetElements, SetCardinality, KeysContain).  Symbol export and the
NULL-context rejection are test_capi.py's, over every SIGNATURES entry."""
import glob
import os
import re

from crdt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "crdt_amd.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_header_declares_the_set_reads():
    hdr = _header()
    for name, nargs in (("crdt_set_elements", 7), ("crdt_u64_contains", 7)):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.M | re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
    assert re.search(r"^#define\s+CRDT_SET_LWW\s+0\s*$", hdr, flags=re.M)
    assert re.search(r"^#define\s+CRDT_SET_ORSET\s+1\s*$", hdr, flags=re.M)


def test_signatures_carry_the_set_reads():
    for name in ("crdt_set_elements", "crdt_u64_contains"):
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == 7, name


def test_python_surface():
    from crdt_amd import shard
    from crdt_amd.engine import Engine
    for name in ("set_elements", "set_cardinality", "keys_contain"):
        assert callable(getattr(Engine, name)), name
    assert callable(shard.set_cardinality)


def test_go_binding_defines_the_set_reads():
    src = ""
    for p in sorted(glob.glob(os.path.join(ROOT, "go", "crdt", "*.go"))):
        with open(p) as f:
            src += f.read()
    for fn in ("SetElements", "SetCardinality", "KeysContain"):
        assert re.search(r"^func " + fn + r"\(", src, flags=re.M), fn
    assert "C.crdt_set_elements(" in src and "C.crdt_u64_contains(" in src
    assert "C.CRDT_SET_LWW" in src and "C.CRDT_SET_ORSET" in src
