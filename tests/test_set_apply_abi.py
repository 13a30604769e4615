"""CPU: the OR-Set mutator call (crdt_set_apply) is declared in
include/crdt_amd.h, carried by crdt_amd._lib.SIGNATURES with the matching
argument count, surfaced by the Engine (set_apply, set_apply_count, map_apply)
and bound by the Go files (SetApply, SetApplyCount).  Symbol export and the
NULL-context rejection are test_capi.py's, over every SIGNATURES entry."""
import glob
import os
import re

from crdt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, ARGS = "crdt_set_apply", 15


def _header(strip=True):
    with open(os.path.join(ROOT, "include", "crdt_amd.h")) as f:
        hdr = f.read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S) if strip else hdr


def test_header_declares_the_apply():
    hdr = _header()
    m = re.search(r"^int\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.M | re.S)
    assert m, NAME
    assert len(m.group(1).split(",")) == ARGS
    assert re.search(r"^#define\s+CRDT_APPLY_TOMBSTONE\s+0\s*$", hdr, flags=re.M)
    assert re.search(r"^#define\s+CRDT_APPLY_CAUSAL\s+1\s*$", hdr, flags=re.M)


def test_header_no_longer_leaves_local_writes_to_the_host():
    assert "Local adds and removes are the host's" not in _header(strip=False)


def test_signatures_carry_the_apply():
    assert NAME in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NAME][1]) == ARGS


def test_python_surface():
    from crdt_amd.engine import Engine
    for name in ("set_apply", "set_apply_count", "map_apply"):
        assert callable(getattr(Engine, name)), name


def test_go_binding_defines_the_calls():
    src = ""
    for p in sorted(glob.glob(os.path.join(ROOT, "go", "crdt", "*.go"))):
        with open(p) as f:
            src += f.read()
    for fn in ("SetApply", "SetApplyCount"):
        assert re.search(r"^func " + fn + r"\(", src, flags=re.M), fn
    assert "C." + NAME + "(" in src
