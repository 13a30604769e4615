"""Test helpers for the device gossip decode (crdt_amd.codec): binary SoA
bodies served by the host mirror or built by hand, their upload, one
crdt_gossip_decode call over them, and the collider fixture of the string
tables (tests/golden/strtab_colliders.json) with a restatement of their hash."""
import json
import os
import struct

import numpy as np
import torch

from crdt_amd import codec
from crdt_amd.server import Server


def fnv1a(s: bytes) -> int:
    """32-bit FNV-1a, restated (the string tables' hash32, csrc/codec.hip)."""
    h = 2166136261
    for b in s:
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


def load_colliders():
    """tests/golden/strtab_colliders.json (make_strtab_colliders.py) as bytes:
    cluster [s], cluster_hash, pairs [(a, b)], last [s], first [s],
    extreme {hash32: [s]}."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "strtab_colliders.json")) as f:
        doc = json.load(f)
    B = bytes.fromhex
    return {"hash": doc["hash"],
            "cluster": [B(s) for s in doc["cluster"]["strings"]],
            "cluster_hash": int(doc["cluster"]["hash32"], 16),
            "pairs": [(B(a), B(b)) for a, b in doc["pairs"]],
            "last": [B(s) for s in doc["last"]],
            "first": [B(s) for s in doc["first"]],
            "extreme": {int(t, 16): [B(s) for s in ss] for t, ss in doc["extreme"].items()}}


def _serve(diff) -> bytes:
    """The binary gossip body of a Diff (host-only Server: main.go:153-170)."""
    s = Server(None, 8080)
    for ts, v in diff.items():
        s.Diff.Put(ts, v)
    st, body = s.GossipBinary()
    s.close()
    assert st == 200
    return body


def _raw_body(entries):
    """Hand-built binary body: entries = [(ts, [(k, v), ...] or None)] in the
    given order (None: a nil map)."""
    ts, pairs, kl, vl, by = [], [], [], [], []
    for t, kv in entries:
        ts.append(t)
        pairs.append(0xFFFFFFFF if kv is None else len(kv))
        for k, v in kv or []:
            kl.append(len(k))
            vl.append(len(v))
            by += [k, v]
    n = len(kl)
    by = b"".join(by)
    return (b"CRDTSOA1" + struct.pack("<QQQ", len(ts), n, len(by)) + struct.pack(f"<{len(ts)}q", *ts) +
            struct.pack(f"<{len(ts)}I", *pairs) + struct.pack(f"<{n}I", *kl) + struct.pack(f"<{n}I", *vl) + by)


def _upload(eng, bodies):
    off = np.zeros(len(bodies) + 1, np.int64)
    off[1:] = np.cumsum([len(b) for b in bodies])
    blob = b"".join(bodies) or b"\0"
    return torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(eng.device), off.tolist()


def _decode(eng, bodies, keys, vals, key_cap=1 << 20, kv_base=3):
    data, off = _upload(eng, bodies)
    ne = sum(codec.body_counts(b)[0] for b in bodies)
    npairs = sum(codec.body_counts(b)[1] for b in bodies)
    kk = torch.full((kv_base + npairs + 1,), -1, dtype=torch.int32, device=eng.device)
    kv = torch.full_like(kk, -1)
    dec, st = codec.decode(eng, data, off, [1000 * i for i in range(len(bodies))], key_cap, keys, vals, kv_base,
                           kk, kv, ne)
    return dec, st, kk.cpu().numpy(), kv.cpu().numpy()
