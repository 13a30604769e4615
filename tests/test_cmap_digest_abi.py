"""CPU: the counter map's range-digest calls (crdt_cmap_digest /
crdt_cmap_select) are declared in include/crdt_amd.h, carried by
crdt_amd._lib.SIGNATURES with the matching argument counts, exported by both
libraries, surfaced by the Engine and crdt_amd.reconcile, and bound by the Go
files."""
import ctypes as C
import glob
import inspect
import os
import re

import pytest

from crdt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (ctx, t, n_max, n_dev, splitters, m, hash, count) and (ctx, t, n_max, n_dev, splitters, m, flags, out, count)
CALLS = {"crdt_cmap_digest": 8, "crdt_cmap_select": 9}


def _header():
    with open(os.path.join(ROOT, "include", "crdt_amd.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_header_declares_the_call(name):
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), flags=re.M | re.S)
    assert m, name
    args = m.group(1).split(",")
    assert len(args) == CALLS[name]
    assert re.match(r"\s*crdt_ctx\s*\*\s*ctx\s*$", args[0])
    assert re.match(r"\s*const\s+crdt_cmap\s*\*\s*t\s*$", args[1])


def test_header_declares_them_beside_the_family():
    h = _header()
    at = [h.index("int " + n + "(") for n in ("crdt_cmap_delta", "crdt_cmap_digest", "crdt_cmap_select", "crdt_stream_copy")]
    assert at == sorted(at)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_signatures_carry_the_call(name):
    assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == CALLS[name]
    assert args[1] is C.POINTER(_lib.crdt_cmap)
    assert args[2] is C.c_size_t and args[5] is C.c_size_t
    if name == "crdt_cmap_select":
        assert args[7] is C.POINTER(_lib.crdt_cmap)


@pytest.mark.parametrize("diag", [False, True], ids=["product", "diag"])
def test_libraries_export_the_calls(diag):
    lib = C.CDLL(os.path.join(ROOT, "crdt_amd", "libcrdt_amd_diag.so"), mode=C.RTLD_LOCAL) if diag else _lib.lib()
    for name in CALLS:
        assert hasattr(lib, name), name


def test_python_surface():
    from crdt_amd import engine, reconcile
    for name in ("cmap_digest", "cmap_select", "cmap_select_count", "digest_diff"):
        assert callable(getattr(engine.Engine, name)), name
    assert list(inspect.signature(engine.Engine.cmap_digest).parameters) == [
        "self", "t", "splitters", "n_dev", "hash_out", "count_out"]
    assert list(inspect.signature(engine.Engine.cmap_select).parameters) == [
        "self", "t", "splitters", "flags", "n_dev", "out", "count", "trim"]
    assert list(inspect.signature(engine.Engine.cmap_select_count).parameters) == [
        "self", "t", "splitters", "flags", "n_dev", "count"]
    assert list(inspect.signature(reconcile.cmap_round).parameters) == ["eng", "A", "B", "splitters"]
    assert "cmap_digest" in engine.Engine.digest_diff.__doc__
    assert "CounterMap" in str(inspect.signature(reconcile.key_splitters)) and "counter map" in reconcile.key_splitters.__doc__


def test_key_splitters_takes_a_counter_map():
    import numpy as np
    from crdt_amd.engine import CounterMap, as_u64
    from crdt_amd.reconcile import key_splitters
    import cmap_digest_util as du
    import cmap_util as cu
    t = cu.random_state(np.random.default_rng(3), 700, 90)
    T = CounterMap.from_numpy(*t, "cpu")
    for m in (0, 1, 63, 127, 900):
        assert np.array_equal(as_u64(key_splitters(T, m)), du.quantile_splitters(t, m))
    assert key_splitters(CounterMap.empty(0, "cpu"), 5).tolist() == [0] * 5


def test_go_binding_defines_the_calls():
    src = ""
    for p in sorted(glob.glob(os.path.join(ROOT, "go", "crdt", "*.go"))):
        with open(p) as f:
            src += f.read()
    for fn in ("CMapDigest", "CMapSelect"):
        assert re.search(r"^func " + fn + r"\(", src, flags=re.M), fn
    for name in CALLS:
        assert "C." + name + "(" in src
