"""CPU: the set-delta entry point (crdt_set_delta) is declared in
include/crdt_amd.h, carried by crdt_amd._lib.SIGNATURES with a matching
argument count, surfaced by the Engine (set_delta, set_delta_count) and bound
by the Go files (SetDelta, SetDeltaCount).  Symbol export and the NULL-context
rejection are test_capi.py's, over every SIGNATURES entry."""
import glob
import os
import re

from crdt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_set_delta():
    with open(os.path.join(ROOT, "include", "crdt_amd.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"^int\s+crdt_set_delta\s*\(([^;]*?)\)\s*;", hdr, flags=re.M | re.S)
    assert m
    assert len(m.group(1).split(",")) == 10


def test_signatures_carry_the_set_delta():
    assert "crdt_set_delta" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["crdt_set_delta"][1]) == 10


def test_python_surface():
    from crdt_amd.engine import Engine
    for name in ("set_delta", "set_delta_count"):
        assert callable(getattr(Engine, name)), name


def test_go_binding_defines_the_set_delta():
    src = ""
    for p in sorted(glob.glob(os.path.join(ROOT, "go", "crdt", "*.go"))):
        with open(p) as f:
            src += f.read()
    for fn in ("SetDelta", "SetDeltaCount"):
        assert re.search(r"^func " + fn + r"\(", src, flags=re.M), fn
    assert "C.crdt_set_delta(" in src
