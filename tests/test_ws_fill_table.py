"""CPU: tests/ws_fill_table.py covers every kernel file that carves the
context's workspace.  A new .hip / .hpp / .inc file under crdt_amd/csrc that
uses ``ctx->ws``, ``ws_reserve(`` or ``TileWs`` and is named by no row of the
table fails here, so its scratch cannot stay out of tests/test_gpu_ws_fill.py
silently."""
import os
import re

from ws_fill_table import NOT_KERNELS, ROWS, SEQUENCES

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "crdt_amd", "csrc")
USES_WS = re.compile(r"ctx->ws\b|ws_reserve\(|\bTileWs\b")


def _files_using_the_workspace():
    out = []
    for name in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, name)
        if os.path.isfile(path) and name.endswith((".hip", ".hpp", ".inc", ".h")):
            with open(path, encoding="utf-8", errors="replace") as f:
                if USES_WS.search(f.read()):
                    out.append(name)
    return out


def test_every_workspace_user_is_named_by_a_row():
    users = _files_using_the_workspace()
    assert len(users) >= 15 and "settile.hpp" in users and "sort.hip" in users     # the grep itself works
    named = {f for _, files, _ in ROWS for f in files}
    missing = [f for f in users if f not in named and f not in NOT_KERNELS]
    assert not missing, f"no row of tests/ws_fill_table.py names {missing}"
    assert "shard.hip" in named                                   # the members' second arena (scratch_reserve)


def test_rows_name_real_files_and_carry_a_shape():
    ids = [r[0] for r in ROWS]
    assert len(set(ids)) == len(ids)
    for rid, files, shape in ROWS:
        assert files and shape, rid
        for f in files:
            assert os.path.isfile(os.path.join(CSRC, f)), (rid, f)
    for f in NOT_KERNELS:
        assert os.path.isfile(os.path.join(CSRC, f)), f


def test_sequences_pair_different_families():
    assert len(SEQUENCES) >= 12
    ids = {r[0] for r in ROWS}
    for first, other in SEQUENCES:
        assert first != other and first in ids and other in ids
