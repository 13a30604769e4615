"""CPU: crdt_cmap_combine / crdt_cmap_add / crdt_cmap_from_ops are declared in
include/crdt_amd.h with the agreed parameter lists, carried by
crdt_amd._lib.SIGNATURES with matching argument types, exported by both
libraries, surfaced by the Engine and bound by the Go files."""
import ctypes as C
import glob
import inspect
import os
import re

import pytest

from crdt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "crdt_cmap_combine": ["crdt_ctx *ctx", "const crdt_cmap *in", "size_t n_max", "const uint64_t *n_dev",
                          "const uint32_t *idx_dev", "size_t n_src", "const crdt_cmap *out", "uint64_t *count_dev"],
    "crdt_cmap_add": ["crdt_ctx *ctx", "const crdt_cmap *t", "size_t nt_max", "const uint64_t *nt_dev",
                      "const crdt_cmap *d", "size_t nd_max", "const uint64_t *nd_dev", "const crdt_cmap *out",
                      "uint64_t *count_dev"],
    "crdt_cmap_from_ops": ["crdt_ctx *ctx", "const uint64_t *op_key_dev", "const uint32_t *op_rep_dev",
                           "const uint64_t *op_dp_dev", "const uint64_t *op_dn_dev", "size_t m",
                           "const crdt_cmap *out", "uint64_t *count_dev"],
}
_M = C.POINTER(_lib.crdt_cmap)
_P, _SZ = C.c_void_p, C.c_size_t
ARGTYPES = {
    "crdt_cmap_combine": [_P, _M, _SZ, _P, _P, _SZ, _M, _P],
    "crdt_cmap_add": [_P, _M, _SZ, _P, _M, _SZ, _P, _M, _P],
    "crdt_cmap_from_ops": [_P, _P, _P, _P, _P, _SZ, _M, _P],
}


def _header(comments=False):
    with open(os.path.join(ROOT, "include", "crdt_amd.h")) as f:
        h = f.read()
    return h if comments else re.sub(r"/\*.*?\*/", "", h, flags=re.S)


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_header_declares_the_call(name):
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), flags=re.M | re.S)
    assert m, name
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == PROTOS[name]


def test_header_declares_them_beside_the_family_and_spells_the_contract_out():
    h = _header()
    at = [h.index("int " + n + "(") for n in ("crdt_cmap_select", "crdt_cmap_combine", "crdt_cmap_add",
                                               "crdt_cmap_from_ops", "crdt_stream_copy")]
    assert at == sorted(at)
    doc = " ".join(_header(comments=True).split())
    for phrase in ("NOT strictly", "contributes 0 and raises CRDT_DEV_RANGE", "NOT idempotent", "exactly once",
                   "SYNCHRONISES ONCE", "m >= 2^32", "capturable after crdt_ctx_reserve"):
        assert phrase in doc, phrase


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_signatures_carry_the_call(name):
    assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and list(args) == ARGTYPES[name]


@pytest.mark.parametrize("diag", [False, True], ids=["product", "diag"])
def test_libraries_export_the_calls(diag):
    lib = C.CDLL(os.path.join(ROOT, "crdt_amd", "libcrdt_amd_diag.so"), mode=C.RTLD_LOCAL) if diag else _lib.lib()
    for name in PROTOS:
        assert hasattr(lib, name), name


def test_python_surface():
    from crdt_amd import engine
    E = engine.Engine
    params = lambda f: list(inspect.signature(f).parameters)   # noqa: E731
    assert params(E.cmap_combine)[:5] == ["self", "t", "n_dev", "idx", "out"]
    assert params(E.cmap_combine_count)[:3] == ["self", "t", "n_dev"]
    assert params(E.cmap_add)[:6] == ["self", "t", "d", "n_t_dev", "n_d_dev", "out"]
    assert params(E.cmap_add_count)[:5] == ["self", "t", "d", "n_t_dev", "n_d_dev"]
    assert params(E.cmap_from_ops)[:6] == ["self", "op_keys", "op_reps", "op_dp", "op_dn", "out"]
    assert params(E.cmap_ingest)[:7] == ["self", "t", "op_keys", "op_reps", "op_dp", "op_dn", "n_t_dev"]
    for f in (E.cmap_combine, E.cmap_add, E.cmap_from_ops, E.cmap_ingest):
        assert f.__doc__
    assert "once" in E.cmap_add.__doc__ and "Synchronises once" in E.cmap_from_ops.__doc__


def test_go_binding_defines_the_calls():
    src = ""
    for p in sorted(glob.glob(os.path.join(ROOT, "go", "crdt", "*.go"))):
        with open(p) as f:
            src += f.read()
    for fn in ("CMapCombine", "CMapAdd", "CMapFromOps"):
        assert re.search(r"^func " + fn + r"\(", src, flags=re.M), fn
    for name in PROTOS:
        assert "C." + name + "(" in src
