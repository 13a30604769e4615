"""CPU: the map-read entry points (crdt_map_read, crdt_map_lookup) are declared
in include/crdt_amd.h, carried by crdt_amd._lib.SIGNATURES with matching
argument counts, surfaced by the Engine and bound by the Go files (MapRead,
MapLookup).  Symbol export and the NULL-context rejection are test_capi.py's,
over every SIGNATURES entry."""
import glob
import os
import re

from crdt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"crdt_map_read": 9, "crdt_map_lookup": 9}


def _header():
    with open(os.path.join(ROOT, "include", "crdt_amd.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_header_declares_the_map_reads():
    hdr = _header()
    for name, nargs in ARGS.items():
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.M | re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
    m = re.search(r"^int\s+crdt_map_read\s*\(([^;]*?)\)\s*;", hdr, flags=re.M | re.S)
    assert re.search(r"int64_t\s*\*\s*win_out_dev", m.group(1)) and re.search(r"uint32_t\s*\*\s*nsib_out_dev", m.group(1))


def test_signatures_carry_the_map_reads():
    for name, nargs in ARGS.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name


def test_python_surface():
    from crdt_amd.engine import Engine
    for name in ("map_read", "map_values", "map_lookup", "map_get"):
        assert callable(getattr(Engine, name)), name


def test_go_binding_defines_the_map_reads():
    src = ""
    for p in sorted(glob.glob(os.path.join(ROOT, "go", "crdt", "*.go"))):
        with open(p) as f:
            src += f.read()
    for fn in ("MapRead", "MapLookup"):
        assert re.search(r"^func " + fn + r"\(", src, flags=re.M), fn
    assert "C.crdt_map_read(" in src and "C.crdt_map_lookup(" in src
