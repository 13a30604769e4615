"""CPU: the range-restricted causal merge (crdt_orset_merge_causal_ranges) is
declared in include/crdt_amd.h, carried by crdt_amd._lib.SIGNATURES with the
matching argument count, surfaced by the Engine (causal_merge_ranges,
causal_merge_ranges_count, causal_map_merge_ranges) and crdt_amd.reconcile
(causal_round), bound by the Go files (OrsetMergeCausalRanges,
OrsetMergeCausalRangesCount) and named in INTEGRATION.md and the README.  Symbol
export and the NULL-context rejection are test_capi.py's, over every SIGNATURES
entry."""
import glob
import inspect
import os
import re

from crdt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, ARGS = "crdt_orset_merge_causal_ranges", 18


def test_header_declares_the_ranged_merge():
    with open(os.path.join(ROOT, "include", "crdt_amd.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"^int\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.M | re.S)
    assert m, NAME
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == ARGS
    names = [re.split(r"[\s*]+", a)[-1] for a in args]
    assert names[11:14] == ["splitters_dev", "m", "flags_dev"]
    assert names[14:] == ["out", "src_out_dev", "ctx_out_dev", "count_dev"]


def test_signatures_carry_the_ranged_merge():
    assert NAME in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NAME][1]) == ARGS
    plain = _lib.SIGNATURES["crdt_orset_merge_causal"][1]
    assert _lib.SIGNATURES[NAME][1][:11] == plain[:11] and _lib.SIGNATURES[NAME][1][14:] == plain[11:]


def test_python_surface():
    from crdt_amd import reconcile
    from crdt_amd.engine import Engine
    for name in ("causal_merge_ranges", "causal_merge_ranges_count", "causal_map_merge_ranges"):
        assert callable(getattr(Engine, name)), name
    p = list(inspect.signature(Engine.causal_merge_ranges).parameters)
    assert p[1:7] == ["a", "ctx_a", "b", "ctx_b", "splitters", "flags"]
    assert p[7:] == ["n_a_dev", "n_b_dev", "out", "src", "ctx_out", "count", "with_src", "trim"]
    p = list(inspect.signature(Engine.causal_map_merge_ranges).parameters)
    assert p[1:] == ["a", "a_val", "ctx_a", "b", "b_val", "ctx_b", "splitters", "flags", "n_b_dev"]
    assert list(inspect.signature(reconcile.causal_round).parameters) == ["eng", "A", "ctx_a", "B", "ctx_b", "splitters"]


def test_go_binding_defines_the_calls():
    src = ""
    for p in sorted(glob.glob(os.path.join(ROOT, "go", "crdt", "*.go"))):
        with open(p) as f:
            src += f.read()
    for fn in ("OrsetMergeCausalRanges", "OrsetMergeCausalRangesCount"):
        assert re.search(r"^func " + fn + r"\(", src, flags=re.M), fn
    assert "C." + NAME + "(" in src


def test_documents_name_the_call():
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        with open(os.path.join(ROOT, doc)) as f:
            assert NAME in f.read(), doc
