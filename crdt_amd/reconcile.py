"""Range-based reconciliation of two replicas of a keyed state type
(sets: DESIGN.md §5.16; counter maps: §5.24).

Two replicas that do not share a memory learn where they differ from small
per-range fingerprints instead of each other's state: both cut the key space
with the same splitters, digest their state per bucket
(:meth:`Engine.set_digest`, 16 bytes a bucket), exchange the digests, flag the
buckets that differ (:meth:`Engine.digest_diff`) and ship only those
(:meth:`Engine.set_select`).  The reference's gossip pull ships the entire
Diff every round (main.go:153-170, :245-256).  :func:`causal_round` is the
same round for the tombstone-free OR-Set, whose merge is not monotone and
needs the buckets along (:meth:`Engine.causal_merge_ranges`).
:func:`cmap_round` is the round for the keyed PN-Counter map
(:meth:`Engine.cmap_digest`, :meth:`Engine.cmap_select`), whose merge is
monotone and takes the selection as it is.

Everything here runs in the library's HIP kernels; torch allocates, indexes
the splitter keys and fills buffers.
"""
from __future__ import annotations

import torch

from .engine import CounterMap, Engine, TupleSet


def key_splitters(t: TupleSet | CounterMap, m: int) -> torch.Tensor:
    """``m`` splitters for about equally filled buckets of the sorted state
    ``t`` (a set state or a counter map: anything with ``.key`` and a
    length): every ceil(n / (m + 1))-th key, t.key[step], t.key[2 step], ...
    (indices past the end take the last key; duplicates are allowed and give
    empty buckets).  A counter map repeats a key once per replica cell, so a
    key with many cells is drawn more than once and some buckets come out
    empty.  An int64-storage device tensor, ascending as unsigned because t is
    sorted.  An empty ``t`` gives all-zero splitters."""
    if m < 0:
        raise ValueError("key_splitters: m must be >= 0")
    n = len(t)
    if n == 0 or m == 0:
        return torch.zeros(m, dtype=torch.int64, device=t.key.device)
    step = -(-n // (m + 1))
    idx = torch.arange(1, m + 1, dtype=torch.int64, device=t.key.device) * step
    return t.key[idx.clamp_(max=n - 1)].contiguous()


def _ship_and_merge(eng: Engine, dst: TupleSet, src: TupleSet, lww: bool, splitters, flags):
    """merge(dst, sel(src)) with no read-back of the selection's length.

    The merges take their sides' lengths from the host, the selection's is on
    the device.  So the selection buffer is first filled with copies of src's
    last tuple and merged at its whole capacity: the copies sort at or after
    every selected tuple, and they change nothing -- the tuple's bucket is
    either flagged (its tag is then in the selection, canonical copy first) or
    it is not (dst then holds the same canonical tuple there, and dst, the
    left operand, wins ties; an OR-Set tomb is OR-ed with one it already
    includes).  Between real replicas the receiver knows the length from the
    transfer and merges the shipped prefix alone."""
    cap = len(src)
    sel = TupleSet.empty(max(cap, 1), eng.device)
    if cap:
        for f, s in ((sel.key, src.key), (sel.ts, src.ts), (sel.rep, src.rep), (sel.tomb, src.tomb)):
            f.copy_(s[cap - 1:cap].expand(f.shape[0]))
    _, shipped = eng.set_select(src, lww, splitters, flags, out=sel)
    merge = eng.lww_merge if lww else eng.orset_merge
    merged, count = merge(dst, sel.slice(cap), trim=False)
    return merged, count, shipped


def reconcile_round(eng: Engine, A: TupleSet, B: TupleSet, lww: bool, splitters: torch.Tensor | None):
    """One reconciliation round between the sorted set states ``A`` and
    ``B``, both on ``eng``'s device, standing in for two replicas: each side's
    digest over ``splitters``, the diff of the two, each side's selection of
    the flagged buckets, and merge(A, sel(B)) / merge(B, sel(A)).  Everything
    is enqueued on the stream with no synchronisation and no read-back.

    Returns ``((MA, ca), (MB, cb), flags, (ship_a, ship_b))``: the merged
    states (TupleSets of capacity len(A) + len(B), their first ``ca`` /
    ``cb`` tuples valid, int64[1] device counts), the uint8 flags of the
    buckets that differed, and the numbers of tuples A and B had to ship
    (int64[1] on the device).  MA equals merge(A, B) and MB merge(B, A) with
    probability about 1 - 2^-64 per differing bucket; the digest is a
    checksum, not a defence against an adversary.

    What crosses the wire between real replicas is the digests (16 bytes a
    bucket) and the selections.  A host that wants to ship less recurses
    before it selects: finer splitters inside the flagged ranges only ::

        sp = key_splitters(A, 255)
        flags, n_diff = eng.digest_diff(eng.set_digest(A, lww, sp), eng.set_digest(B, lww, sp))
        if int(n_diff.item()):
            # bucket b covers keys [sp[b - 1], sp[b]); cut each flagged one finer
            a_part, _ = eng.set_select(A, lww, sp, flags, trim=True)   # or the peer's digest of
            fine = key_splitters(a_part, 4095)                         # its own flagged ranges
            fine = torch.cat([sp, fine]).sort().values                 # (keys >= 2^63: sort as unsigned)
            (MA, ca), (MB, cb), flags2, shipped = reconcile_round(eng, A, B, lww, fine)

    Unflagged coarse buckets stay unflagged under the finer cut (their
    sub-buckets agree too), so only the differing sub-ranges ship.
    """
    da = eng.set_digest(A, lww, splitters)
    db = eng.set_digest(B, lww, splitters)
    flags, _ = eng.digest_diff(da, db)
    ma, ca, ship_b = _ship_and_merge(eng, A, B, lww, splitters, flags)
    mb, cb, ship_a = _ship_and_merge(eng, B, A, lww, splitters, flags)
    return (ma, ca), (mb, cb), flags, (ship_a, ship_b)


def causal_round(eng: Engine, A: TupleSet, ctx_a: torch.Tensor | None, B: TupleSet, ctx_b: torch.Tensor | None,
                 splitters: torch.Tensor | None):
    """One reconciliation round between the causal OR-Set states ``(A,
    ctx_a)`` and ``(B, ctx_b)``, both on ``eng``'s device,
    standing in for two replicas: each side's OR-Set-mode digest over
    ``splitters``, the diff of the two, each side's selection of the flagged
    buckets, and :meth:`Engine.causal_merge_ranges` of each whole state with
    the other side's selection under the other side's whole context.  The
    selection's device count goes straight in as the merge's ``n_b_dev``.
    Everything is enqueued on the stream with no synchronisation and no
    read-back.

    The plain causal merge cannot take a selection: it is not monotone, and a
    tag the receiver holds that the peer's context covers is dropped unless
    the peer's copy is in the operand.  The ranged merge decides an unflagged
    bucket by the receiver's state alone.

    Returns ``((MA, ca, ctx), (MB, cb, ctx), flags, (ship_a, ship_b))``: the
    merged states (TupleSets of capacity len(A) + len(B), their first ``ca``
    / ``cb`` tuples valid, int64[1] device counts) each with its merged
    context, the uint8 flags of the buckets that differed, and the numbers of
    tuples A and B had to ship (int64[1] on the device).  MA and MB both equal
    ``causal_merge(A, B)``, tuple for tuple, and both contexts its merged
    context, with probability about 1 - 2^-64 per differing bucket.

    What crosses the wire between real replicas is the digests (16 bytes a
    bucket), the two contexts (8 bytes a replica) and the selections.
    Recursion with finer splitters inside the flagged ranges works as for
    :func:`reconcile_round`: unflagged coarse buckets stay unflagged under the
    finer cut, so only the differing sub-ranges ship.
    """
    da = eng.set_digest(A, False, splitters)
    db = eng.set_digest(B, False, splitters)
    flags, _ = eng.digest_diff(da, db)
    sel_a, ship_a = eng.set_select(A, False, splitters, flags)
    sel_b, ship_b = eng.set_select(B, False, splitters, flags)
    sel_a, sel_b = sel_a.slice(len(A)), sel_b.slice(len(B))      # (an empty state's buffer holds one slot)
    ma, ctx_ma, ca = eng.causal_merge_ranges(A, ctx_a, sel_b, ctx_b, splitters, flags, n_b_dev=ship_b)
    mb, ctx_mb, cb = eng.causal_merge_ranges(B, ctx_b, sel_a, ctx_a, splitters, flags, n_b_dev=ship_a)
    return (ma, ca, ctx_ma), (mb, cb, ctx_mb), flags, (ship_a, ship_b)


def cmap_round(eng: Engine, A: CounterMap, B: CounterMap, splitters: torch.Tensor | None):
    """One reconciliation round between the counter maps ``A`` and ``B``
    (DESIGN.md §5.24), both on ``eng``'s device, standing in for two replicas:
    each side's :meth:`Engine.cmap_digest` over ``splitters``, the diff of the
    two, each side's :meth:`Engine.cmap_select` of the flagged buckets, and
    ``cmap_merge(A, sel(B))`` / ``cmap_merge(B, sel(A))``.  The merge is
    monotone and takes its sides' lengths from the device, so each selection
    goes in as it is with its device count as ``n_b_dev``.  Everything is
    enqueued on the stream with no synchronisation and no read-back.

    Returns ``((MA, ca), (MB, cb), flags, (ship_a, ship_b))``: the merged
    maps (CounterMaps of capacity len(A) + len(B), their first ``ca`` /
    ``cb`` cells valid, int64[1] device counts), the uint8 flags of the
    buckets that differed, and the numbers of cells A and B had to ship
    (int64[1] on the device).  MA and MB both equal ``cmap_merge(A, B)`` with
    probability about 1 - 2^-64 per differing bucket; the digest is a
    checksum, not a defence against an adversary.

    What crosses the wire between real replicas is the digests (16 bytes a
    bucket) and the selections (28 bytes a cell).  Recursion with finer
    splitters inside the flagged ranges works as for :func:`reconcile_round`.
    """
    da = eng.cmap_digest(A, splitters)
    db = eng.cmap_digest(B, splitters)
    flags, _ = eng.digest_diff(da, db)
    sel_a, ship_a = eng.cmap_select(A, splitters, flags)
    sel_b, ship_b = eng.cmap_select(B, splitters, flags)
    sel_a, sel_b = sel_a.slice(len(A)), sel_b.slice(len(B))      # (an empty map's buffer holds one slot)
    ma, ca = eng.cmap_merge(A, sel_b, n_b_dev=ship_b)
    mb, cb = eng.cmap_merge(B, sel_a, n_b_dev=ship_a)
    return (ma, ca), (mb, cb), flags, (ship_a, ship_b)
