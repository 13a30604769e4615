"""CPU: the causal OR-Set merge (crdt_orset_merge_causal) is declared in
include/crdt_amd.h, carried by crdt_amd._lib.SIGNATURES with the matching
argument count, surfaced by the Engine (causal_merge, causal_merge_count,
causal_map_merge) and bound by the Go files (OrsetMergeCausal,
OrsetMergeCausalCount).  Symbol export and the NULL-context rejection are
test_capi.py's, over every SIGNATURES entry."""
import glob
import os
import re

from crdt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, ARGS = "crdt_orset_merge_causal", 15


def test_header_declares_the_causal_merge():
    with open(os.path.join(ROOT, "include", "crdt_amd.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"^int\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.M | re.S)
    assert m, NAME
    assert len(m.group(1).split(",")) == ARGS


def test_signatures_carry_the_causal_merge():
    assert NAME in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NAME][1]) == ARGS


def test_python_surface():
    from crdt_amd.engine import Engine
    for name in ("causal_merge", "causal_merge_count", "causal_map_merge"):
        assert callable(getattr(Engine, name)), name


def test_go_binding_defines_the_calls():
    src = ""
    for p in sorted(glob.glob(os.path.join(ROOT, "go", "crdt", "*.go"))):
        with open(p) as f:
            src += f.read()
    for fn in ("OrsetMergeCausal", "OrsetMergeCausalCount"):
        assert re.search(r"^func " + fn + r"\(", src, flags=re.M), fn
    assert "C." + NAME + "(" in src
