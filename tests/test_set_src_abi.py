"""CPU: the payload-carrying set merges (crdt_lww_merge_src,
crdt_orset_merge_src) and the gather by their source indices
(crdt_src_gather) are declared in include/crdt_amd.h, carried by
crdt_amd._lib.SIGNATURES with matching argument counts, surfaced by the Engine
(lww_merge_src, orset_merge_src, gather_src, lww_map_merge, orset_map_merge)
and bound by the Go files (LWWMergeSrc, ORSetMergeSrc, GatherSrc).  Symbol
export and the NULL-context rejection are test_capi.py's, over every
SIGNATURES entry."""
import glob
import os
import re

import pytest

from crdt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARGS = {"crdt_lww_merge_src": 8, "crdt_orset_merge_src": 8, "crdt_src_gather": 10}


@pytest.mark.parametrize("fn", sorted(ARGS))
def test_header_declares_the_src_calls(fn):
    with open(os.path.join(ROOT, "include", "crdt_amd.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"^int\s+" + fn + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.M | re.S)
    assert m, fn
    assert len(m.group(1).split(",")) == ARGS[fn]


@pytest.mark.parametrize("fn", sorted(ARGS))
def test_signatures_carry_the_src_calls(fn):
    assert fn in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[fn][1]) == ARGS[fn]


def test_python_surface():
    from crdt_amd.engine import Engine
    for name in ("lww_merge_src", "orset_merge_src", "gather_src", "lww_map_merge", "orset_map_merge"):
        assert callable(getattr(Engine, name)), name


def test_go_binding_defines_the_src_calls():
    src = ""
    for p in sorted(glob.glob(os.path.join(ROOT, "go", "crdt", "*.go"))):
        with open(p) as f:
            src += f.read()
    for fn in ("LWWMergeSrc", "ORSetMergeSrc", "GatherSrc"):
        assert re.search(r"^func " + fn + r"\(", src, flags=re.M), fn
    for c in ARGS:
        assert "C." + c + "(" in src, c
