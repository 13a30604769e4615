"""Device-level host API over the C-ABI (include/crdt_amd.h).

PyTorch is plumbing here: it owns device memory (tensors in HBM) and the
stream; every merge/compare computation runs in libcrdt_amd.so's gfx950 HIP
kernels.  uint64 state is carried in int64 tensors (same bits); use
:func:`as_u64` to view a host copy as numpy uint64.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import (call, crdt_cmap, crdt_local_in, crdt_local_out, crdt_refmerge_acc, crdt_refmerge_in,
                   crdt_refmerge_kv_out, crdt_refmerge_out, crdt_refmerge_pull, crdt_replay_state, crdt_tuples)

VC_EQUAL, VC_BEFORE, VC_AFTER, VC_CONCURRENT = 0, 1, 2, 3


def as_u64(t: torch.Tensor) -> np.ndarray:
    """Host numpy uint64 view of an 8-byte integer tensor (any device)."""
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


def u64_tensor(a, device) -> torch.Tensor:
    """numpy uint64 (or int64) array -> int64 tensor with the same bits."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.int64:
        a = a.view(np.int64) if a.dtype.itemsize == 8 else a.astype(np.int64)
    return torch.from_numpy(a.copy()).to(device)


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _ref(s: "TupleSet | None"):
    """The by-reference crdt_tuples argument naming ``s``; None (an absent optional output) stays None."""
    return None if s is None else C.byref(s.c())


@dataclass
class TupleSet:
    """SoA (key u64, ts u64, rep u32, tomb u8) tuples, sorted by (key, ts, rep)."""

    key: torch.Tensor   # int64 storage of uint64 keys
    ts: torch.Tensor    # int64 storage of uint64 timestamps
    rep: torch.Tensor   # int32 storage of uint32 replica ids
    tomb: torch.Tensor  # uint8 0/1

    def __len__(self) -> int:
        return int(self.key.numel())

    @staticmethod
    def empty(n: int, device) -> "TupleSet":
        return TupleSet(torch.empty(n, dtype=torch.int64, device=device),
                        torch.empty(n, dtype=torch.int64, device=device),
                        torch.empty(n, dtype=torch.int32, device=device),
                        torch.empty(n, dtype=torch.uint8, device=device))

    def c(self) -> crdt_tuples:
        return crdt_tuples(self.key.data_ptr(), self.ts.data_ptr(), self.rep.data_ptr(), self.tomb.data_ptr())

    def slice(self, n: int) -> "TupleSet":
        return TupleSet(self.key[:n], self.ts[:n], self.rep[:n], self.tomb[:n])

    def to_numpy(self):
        return (as_u64(self.key), as_u64(self.ts), self.rep.cpu().numpy().view(np.uint32),
                self.tomb.cpu().numpy())

    @staticmethod
    def from_numpy(key, ts, rep, tomb, device) -> "TupleSet":
        return TupleSet(u64_tensor(key, device), u64_tensor(ts, device),
                        torch.from_numpy(np.ascontiguousarray(rep).view(np.int32).copy()).to(device),
                        torch.from_numpy(np.ascontiguousarray(tomb).astype(np.uint8)).to(device))


@dataclass
class CounterMap:
    """SoA (key u64, rep u32, p u64, n u64) cells of a keyed PN-Counter map,
    strictly ascending by (key, rep): replica rep's increments / decrements of key."""

    key: torch.Tensor   # int64 storage of uint64 keys
    rep: torch.Tensor   # int32 storage of uint32 replica ids
    p: torch.Tensor     # int64 storage of uint64 increments
    n: torch.Tensor     # int64 storage of uint64 decrements

    def __len__(self) -> int:
        return int(self.key.numel())

    @staticmethod
    def empty(n: int, device) -> "CounterMap":
        return CounterMap(torch.empty(n, dtype=torch.int64, device=device),
                          torch.empty(n, dtype=torch.int32, device=device),
                          torch.empty(n, dtype=torch.int64, device=device),
                          torch.empty(n, dtype=torch.int64, device=device))

    def c(self) -> crdt_cmap:
        return crdt_cmap(self.key.data_ptr(), self.rep.data_ptr(), self.p.data_ptr(), self.n.data_ptr())

    def slice(self, n: int) -> "CounterMap":
        return CounterMap(self.key[:n], self.rep[:n], self.p[:n], self.n[:n])

    def to_numpy(self):
        return (as_u64(self.key), self.rep.cpu().numpy().view(np.uint32), as_u64(self.p), as_u64(self.n))

    @staticmethod
    def from_numpy(key, rep, p, n, device) -> "CounterMap":
        return CounterMap(u64_tensor(key, device),
                          torch.from_numpy(np.ascontiguousarray(rep).view(np.int32).copy()).to(device),
                          u64_tensor(p, device), u64_tensor(n, device))


class Engine:
    """One crdt_ctx bound to one GPU and to torch's current stream."""

    def __init__(self, device: int | torch.device = 0):
        if not torch.cuda.is_available():
            raise _lib.CrdtLibraryError("no GPU visible: the crdt_amd engine has no CPU path")
        self.device = torch.device("cuda", device if isinstance(device, int) else device.index or 0)
        lib = _lib.lib()
        self._stream = torch.cuda.current_stream(self.device).cuda_stream
        ctx = C.c_void_p()
        call("crdt_ctx_create", self.device.index, self._stream, C.byref(ctx))
        self.ctx = ctx
        self._lib = lib
        self._dependents = []              # weakrefs to objects borrowing ctx (shard.Comm)

    def _depend(self, obj) -> None:
        import weakref
        self._dependents.append(weakref.ref(obj))

    def close(self) -> None:
        for r in getattr(self, "_dependents", []):   # borrowers first: they use ctx in their teardown
            o = r()
            if o is not None:
                o.close()
        self._dependents = []
        if getattr(self, "ctx", None):
            self._lib.crdt_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _bind(self) -> None:
        s = torch.cuda.current_stream(self.device).cuda_stream
        if s != self._stream:
            call("crdt_ctx_set_stream", self.ctx, s, ctx=self.ctx)
            self._stream = s

    def _call(self, fn: str, *args) -> None:
        self._bind()
        call(fn, self.ctx, *args, ctx=self.ctx)

    def _check(self, *ts: torch.Tensor | None, itemsize: int | None = None) -> None:
        """Refuse a tensor the library cannot take; None, an absent optional, passes."""
        for t in ts:
            if t is None:
                continue
            if t.device != self.device:
                raise ValueError(f"tensor on {t.device}, engine on {self.device}")
            if not t.is_contiguous():
                raise ValueError("tensors must be contiguous")
            if itemsize is not None and t.element_size() != itemsize:
                raise ValueError(f"expected {itemsize}-byte elements, got {t.dtype}")

    def _check_tuples(self, *sets: TupleSet | None) -> None:
        dev = self.device
        for s in sets:
            if s is None:
                continue
            key, ts, rep, tomb = s.key, s.ts, s.rep, s.tomb
            # one pass accepts well-formed fields; anything else gets _check's refusal, in field order
            if not (key.device == dev and key.is_contiguous() and key.element_size() == 8
                    and ts.device == dev and ts.is_contiguous() and ts.element_size() == 8
                    and rep.device == dev and rep.is_contiguous() and rep.element_size() == 4
                    and tomb.device == dev and tomb.is_contiguous() and tomb.element_size() == 1):
                self._check(s.key, s.ts, itemsize=8)
                self._check(s.rep, itemsize=4)
                self._check(s.tomb, itemsize=1)

    # -- what the set-state wrappers share: the buffers a call writes, allocated
    #    where not given and checked where given, and what it hands back
    def _count(self, count: torch.Tensor | None) -> torch.Tensor:
        return torch.empty(1, dtype=torch.int64, device=self.device) if count is None else count

    def _out_tuples(self, out: TupleSet | None, n: int, short: str) -> TupleSet:
        out = TupleSet.empty(max(n, 1), self.device) if out is None else out
        if len(out) < n:
            raise ValueError(short)
        return out

    def _out_src(self, src: torch.Tensor | None, with_src: bool, n: int, bad: str) -> torch.Tensor | None:
        if src is None and with_src:
            src = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        if src is not None:
            self._check(src, itemsize=8)
            if src.dtype != torch.int64 or src.numel() < n:
                raise ValueError(bad)
        return src

    def _trimmed(self, count: torch.Tensor) -> int:
        """The count read back, once the device status is checked: ``trim``'s one synchronisation."""
        self.check_device()
        return int(count.item())

    def _result(self, trim: bool, count: torch.Tensor, out: TupleSet, src: torch.Tensor | None, *extras):
        """(out[, src], *extras, count), out / src cut to the count with ``trim``."""
        if trim:
            k = self._trimmed(count)
            out, src = out.slice(k), None if src is None else src[:k]
        return (out, *extras, count) if src is None else (out, src, *extras, count)

    def sync(self) -> None:
        self._call("crdt_ctx_sync")

    def device_status(self, clear: bool = True) -> int:
        """Kernel-raised failure flags (CRDT_DEV_*) since the last clear; syncs."""
        v = C.c_uint32()
        self._call("crdt_ctx_device_status", C.byref(v), 1 if clear else 0)
        return v.value

    def check_device(self) -> None:
        """Raise if a kernel reported a device-side failure (its output is invalid)."""
        flags = self.device_status(clear=True)
        if flags:
            raise _lib.CrdtLibraryError(f"device-side failure flags 0x{flags:x} (CRDT_DEV_*): output invalid")

    def reserve(self, nbytes: int) -> None:
        self._call("crdt_ctx_reserve", nbytes)

    # ------------------------------------------------------------ counters (a6)
    def gcounter_join(self, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """out = max(a, b) elementwise (uint64); a, b: [rows, nodes]."""
        if a.shape != b.shape or a.dim() != 2:
            raise ValueError("a and b must be [rows, nodes] of equal shape")
        out = torch.empty_like(a) if out is None else out
        self._check(a, b, out, itemsize=8)
        if out.shape != a.shape:
            raise ValueError("out shape mismatch")
        self._call("crdt_gcounter_join", a.data_ptr(), b.data_ptr(), out.data_ptr(), a.shape[0], a.shape[1])
        return out

    vclock_join = gcounter_join

    def gcounter_fold(self, a: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """out[n] = max over rows of a[:, n]."""
        rows, nodes = a.shape
        out = torch.empty(nodes, dtype=torch.int64, device=self.device) if out is None else out
        self._check(a, out, itemsize=8)
        self._call("crdt_gcounter_fold", a.data_ptr(), rows, nodes, out.data_ptr())
        return out

    def stream_copy(self, src: torch.Tensor, dst: torch.Tensor, unroll: int = 4, blocks_per_cu: int = 2) -> None:
        """dst = src with the library's streaming copy kernel (peak measurement)."""
        self._check(src, dst)
        n = min(src.numel() * src.element_size(), dst.numel() * dst.element_size())
        self._call("crdt_stream_copy", src.data_ptr(), dst.data_ptr(), n & ~15, unroll, blocks_per_cu)

    def stream_read(self, src: torch.Tensor, sink: torch.Tensor, unroll: int = 4, blocks_per_cu: int = 2) -> None:
        """Read all of src (one word per workgroup to sink): read-only streaming peak."""
        self._check(src)
        self._check(sink, itemsize=8)
        n = src.numel() * src.element_size()
        self._call("crdt_stream_read", src.data_ptr(), n & ~15, sink.data_ptr(), sink.numel(), unroll, blocks_per_cu)

    def gcounter_value(self, a: torch.Tensor) -> torch.Tensor:
        rows, nodes = a.shape
        out = torch.empty(rows, dtype=torch.int64, device=self.device)
        self._check(a, out, itemsize=8)
        self._call("crdt_gcounter_value", a.data_ptr(), rows, nodes, out.data_ptr())
        return out

    def pncounter_join(self, pa, na, pb, nb, pout=None, nout=None):
        pout = torch.empty_like(pa) if pout is None else pout
        nout = torch.empty_like(na) if nout is None else nout
        for t in (na, pb, nb, pout, nout):
            if t.shape != pa.shape:
                raise ValueError("PN-Counter operands must share one [rows, nodes] shape")
        self._check(pa, na, pb, nb, pout, nout, itemsize=8)
        rows, nodes = pa.shape
        self._call("crdt_pncounter_join", pa.data_ptr(), na.data_ptr(), pb.data_ptr(), nb.data_ptr(),
                   pout.data_ptr(), nout.data_ptr(), rows, nodes)
        return pout, nout

    def pncounter_value(self, p: torch.Tensor, n: torch.Tensor) -> torch.Tensor:
        if p.shape != n.shape:
            raise ValueError("P and N must share one shape")
        rows, nodes = p.shape
        out = torch.empty(rows, dtype=torch.int64, device=self.device)
        self._check(p, n, out, itemsize=8)
        self._call("crdt_pncounter_value", p.data_ptr(), n.data_ptr(), out.data_ptr(), rows, nodes)
        return out

    # ------------------------------------------------------------ vector clocks (a7)
    def vclock_classify(self, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        if a.shape != b.shape or a.dim() != 2:
            raise ValueError("a and b must be [pairs, nodes] of equal shape")
        pairs, nodes = a.shape
        out = torch.empty(pairs, dtype=torch.uint8, device=self.device) if out is None else out
        self._check(a, b, itemsize=8)
        self._check(out, itemsize=1)
        self._call("crdt_vclock_classify", a.data_ptr(), b.data_ptr(), out.data_ptr(), pairs, nodes)
        return out

    # ------------------------------------------------------------ sets (a8)
    def _set_merge(self, fn: str, a: TupleSet, b: TupleSet, out: TupleSet | None,
                   count: torch.Tensor | None, trim: bool):
        na, nb = len(a), len(b)
        out = TupleSet.empty(max(na + nb, 1), self.device) if out is None else out
        count = self._count(count)
        self._check_tuples(a, b, out)
        self._call(fn, _ref(a), na, _ref(b), nb, _ref(out), count.data_ptr())
        # trim synchronises anyway: check the look-back's flag too
        return out.slice(self._trimmed(count)) if trim else (out, count)

    def lww_merge(self, a: TupleSet, b: TupleSet, out: TupleSet | None = None,
                  count: torch.Tensor | None = None, trim: bool = True):
        """LWW-Element-Set merge; a is the local (tie-winning) operand."""
        return self._set_merge("crdt_lww_merge", a, b, out, count, trim)

    def orset_merge(self, a: TupleSet, b: TupleSet, out: TupleSet | None = None,
                    count: torch.Tensor | None = None, trim: bool = True):
        """OR-Set merge: union of tags, tombstones OR-ed."""
        return self._set_merge("crdt_orset_merge", a, b, out, count, trim)

    # -- merges that carry a payload: every output's source index, and the
    #    gather of value columns by it (crdt_*_merge_src / crdt_src_gather)
    def _set_merge_src(self, fn: str, a: TupleSet, b: TupleSet, out: TupleSet | None, src: torch.Tensor | None):
        na, nb = len(a), len(b)
        short = "merge_src: out and src (int64) must hold len(a) + len(b) entries"
        out = TupleSet.empty(max(na + nb, 1), self.device) if out is None else out
        self._check_tuples(a, b, out)
        src = self._out_src(src, True, na + nb, short)
        if len(out) < na + nb:
            raise ValueError(short)
        count = self._count(None)
        self._call(fn, _ref(a), na, _ref(b), nb, _ref(out), src.data_ptr(), count.data_ptr())
        return out, count, src

    def lww_merge_src(self, a: TupleSet, b: TupleSet, out: TupleSet | None = None, src: torch.Tensor | None = None):
        """:meth:`lww_merge` that also says where every output tuple came
        from: returns (out, count, src), device-resident, no synchronisation
        -- out / src of capacity len(a) + len(b), their first ``count``
        entries valid.  src[i] >= 0: out[i] is a[src[i]]; src[i] < 0: it is
        b[-(src[i] + 1)] -- the first copy, in merged order, of the key's
        maximal (ts, rep) tag."""
        return self._set_merge_src("crdt_lww_merge_src", a, b, out, src)

    def orset_merge_src(self, a: TupleSet, b: TupleSet, out: TupleSet | None = None, src: torch.Tensor | None = None):
        """:meth:`orset_merge` with every output's source index (see
        :meth:`lww_merge_src`): the first copy of the tag in merged order;
        out.tomb stays the OR over all copies."""
        return self._set_merge_src("crdt_orset_merge_src", a, b, out, src)

    def gather_src(self, src: torch.Tensor, a_col: torch.Tensor, b_col: torch.Tensor,
                   n_dev: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
        """out[i] = a_col[src[i]] if src[i] >= 0 else b_col[-(src[i] + 1)]
        for the first ``n_dev`` (int64[1] on the device, e.g. the merge's
        count; default: all) entries of ``src``: one payload column moved by
        a merge's source indices, no synchronisation.  The columns share one
        dtype; an element is one entry of a 1-D column, or one row of a
        contiguous 2-D column whose rows are 1, 2, 4, 8 or 16 bytes.  An
        index outside its side leaves its output element alone and raises
        CRDT_DEV_RANGE in :meth:`device_status`, as does n_dev > len(src)."""
        if a_col.dtype != b_col.dtype or a_col.dim() != b_col.dim() or a_col.dim() not in (1, 2):
            raise ValueError("gather_src: a_col and b_col must share one dtype and be 1-D (or [n, w] rows)")
        if a_col.dim() == 2 and a_col.shape[1] != b_col.shape[1]:
            raise ValueError("gather_src: a_col and b_col rows differ in width")
        row = tuple(a_col.shape[1:])
        es = a_col.element_size() * (row[0] if row else 1)
        if es not in (1, 2, 4, 8, 16):
            raise ValueError(f"gather_src: {es}-byte elements (1, 2, 4, 8 or 16)")
        n = src.numel()
        out = torch.empty((max(n, 1),) + row, dtype=a_col.dtype, device=self.device) if out is None else out
        self._check(src, itemsize=8)
        self._check(a_col, b_col, out)
        if src.dtype != torch.int64 or src.dim() != 1:
            raise ValueError("gather_src: src must be a 1-D int64 tensor")
        if out.dtype != a_col.dtype or tuple(out.shape[1:]) != row or out.shape[0] < n:
            raise ValueError("gather_src: out must hold len(src) elements of the columns' dtype")
        self._check(n_dev, itemsize=8)
        self._call("crdt_src_gather", _ptr(src), n, _ptr(n_dev), _ptr(a_col), a_col.shape[0], _ptr(b_col),
                   b_col.shape[0], _ptr(out), es)
        return out

    def _map_merge(self, merge, a: TupleSet, a_val: torch.Tensor, b: TupleSet, b_val: torch.Tensor):
        if a_val.shape[0] != len(a) or b_val.shape[0] != len(b):
            raise ValueError("map_merge: one value per tuple on each side")
        out, count, src = merge(a, b)
        return out, self.gather_src(src, a_val, b_val, n_dev=count), count

    def lww_map_merge(self, a: TupleSet, a_val: torch.Tensor, b: TupleSet, b_val: torch.Tensor):
        """LWW-Map merge: the tuples of :meth:`lww_merge` and, beside each,
        the value its winning input tuple carried (a_val[i] belongs to a's
        tuple i).  Returns (out, out_val, count), device-resident: the merge,
        then one gather chained off its device count -- no read-back."""
        return self._map_merge(self.lww_merge_src, a, a_val, b, b_val)

    def orset_map_merge(self, a: TupleSet, a_val: torch.Tensor, b: TupleSet, b_val: torch.Tensor):
        """OR-Map merge: :meth:`orset_merge` with the payload of each tag's
        first copy in merged order (see :meth:`lww_map_merge`)."""
        return self._map_merge(self.orset_merge_src, a, a_val, b, b_val)

    def lww_merge_unsorted(self, a: TupleSet, b: TupleSet, out: TupleSet | None = None,
                           count: torch.Tensor | None = None, trim: bool = True):
        """LWW merge of UNSORTED sides (D2): one fused device sort + dedup;
        equal to sort_tuples of each side followed by lww_merge."""
        return self._set_merge("crdt_lww_merge_unsorted", a, b, out, count, trim)

    def orset_merge_unsorted(self, a: TupleSet, b: TupleSet, out: TupleSet | None = None,
                             count: torch.Tensor | None = None, trim: bool = True):
        """OR-Set merge of UNSORTED sides (D2): one fused device sort + dedup."""
        return self._set_merge("crdt_orset_merge_unsorted", a, b, out, count, trim)

    def set_merge_plan(self, lww: bool, a: TupleSet, b: TupleSet, widen: bool = False):
        """crdt_set_merge_plan: the exact plan of a D2 merge of this shape
        (one synchronisation); reserves the workspace its planned calls use."""
        from ._lib import crdt_set_plan
        plan = crdt_set_plan()
        self._call("crdt_set_merge_plan", 0 if lww else 1, _ref(a), len(a), _ref(b), len(b), 1 if widen else 0,
                   C.byref(plan))
        return plan

    def merge_unsorted_planned(self, lww: bool, plan, a: TupleSet, b: TupleSet, out: TupleSet,
                               count: torch.Tensor) -> None:
        """crdt_{lww,orset}_merge_unsorted_planned: the D2 merge enqueued with
        no host synchronisation (graph-capturable); *count = 2^64 - 1 and the
        CRDT_DEV_PLAN flag when the inputs left the plan."""
        self._check_tuples(a, b, out)
        fn = "crdt_lww_merge_unsorted_planned" if lww else "crdt_orset_merge_unsorted_planned"
        self._call(fn, C.byref(plan), _ref(a), len(a), _ref(b), len(b), _ref(out), count.data_ptr())

    def sort_tuples(self, t: TupleSet, out: TupleSet | None = None) -> TupleSet:
        """Device sort into ascending (key, ts, rep, tomb) order (config D2)."""
        n = len(t)
        out = TupleSet.empty(n, self.device) if out is None else out
        self._check_tuples(t, out)
        self._call("crdt_tuples_sort", _ref(t), n, _ref(out))
        return out

    def lower_bound_u64(self, sorted_u64: torch.Tensor, probes: torch.Tensor) -> torch.Tensor:
        """lower_bound of every probe in an ascending uint64 (int64-stored)
        device array, unsigned order (crdt_u64_lower_bound)."""
        self._check(sorted_u64, probes, itemsize=8)
        out = torch.empty(probes.numel(), dtype=torch.int64, device=self.device)
        self._call("crdt_u64_lower_bound", sorted_u64.data_ptr(), sorted_u64.numel(), probes.data_ptr(),
                   probes.numel(), out.data_ptr())
        return out

    # -- set reads: which keys are in a merged state (crdt_set_elements / crdt_u64_contains)
    def set_elements(self, t: TupleSet, lww: bool, n_dev: torch.Tensor | None = None,
                     out: torch.Tensor | None = None, count: torch.Tensor | None = None):
        """Live keys of the sorted set state ``t`` (ascending, each once):
        returns (keys, count), device tensors, no synchronisation -- keys is
        int64 storage of capacity len(t), its first ``count`` entries valid.
        ``n_dev`` (int64[1] on the device, e.g. a merge's count): only the
        first n_dev tuples of t are read; a value over len(t) leaves count =
        2^64 - 1 and raises CRDT_DEV_RANGE in :meth:`device_status`."""
        n = len(t)
        out = torch.empty(max(n, 1), dtype=torch.int64, device=self.device) if out is None else out
        self._check(out, itemsize=8)
        if out.numel() < n:
            raise ValueError("set_elements: out holds fewer keys than t has tuples")
        return out, self._set_read(t, lww, n_dev, out, count)

    def set_cardinality(self, t: TupleSet, lww: bool, n_dev: torch.Tensor | None = None,
                        count: torch.Tensor | None = None) -> torch.Tensor:
        """Number of live keys of ``t`` (int64[1] on the device, no
        synchronisation): one pass over the tuples, nothing else written."""
        return self._set_read(t, lww, n_dev, None, count)

    def _set_read(self, t: TupleSet, lww: bool, n_dev, out, count) -> torch.Tensor:
        count = self._count(count)
        self._check_tuples(t)
        self._check(count, n_dev, itemsize=8)
        self._call("crdt_set_elements", 0 if lww else 1, _ref(t), len(t), _ptr(n_dev), _ptr(out), count.data_ptr())
        return count

    def keys_contain(self, sorted_keys: torch.Tensor, probes: torch.Tensor,
                     n_dev: torch.Tensor | None = None) -> torch.Tensor:
        """uint8[i] = 1 iff probes[i] is among the first n_dev (default: all)
        of the ascending uint64 ``sorted_keys`` (crdt_u64_contains)."""
        self._check(sorted_keys, probes, n_dev, itemsize=8)
        res = torch.empty(probes.numel(), dtype=torch.uint8, device=self.device)
        self._call("crdt_u64_contains", _ptr(sorted_keys), sorted_keys.numel(), _ptr(n_dev), _ptr(probes),
                   probes.numel(), _ptr(res))
        return res

    # -- set deltas: the tuples of src that dst lacks (crdt_set_delta)
    def set_delta(self, src: TupleSet, dst: TupleSet, lww: bool, n_src_dev: torch.Tensor | None = None,
                  n_dst_dev: torch.Tensor | None = None, out: TupleSet | None = None,
                  count: torch.Tensor | None = None, trim: bool = False):
        """The smallest D with merge(dst, D) == merge(dst, src), dst the left
        (tie-winning) operand, in ascending tuple order: returns (D, count),
        device-resident, no synchronisation -- D of capacity len(src), its
        first ``count`` tuples valid.  ``n_src_dev`` / ``n_dst_dev`` (int64[1]
        on the device, e.g. a merge's count): only so many leading tuples of
        that side are read; a value over the side's length leaves count =
        2^64 - 1 and raises CRDT_DEV_RANGE in :meth:`device_status`.  With
        ``trim`` the device status is checked and the sliced D returned."""
        out = self._out_tuples(out, len(src), "set_delta: out holds fewer tuples than src")
        count = self._set_delta(src, dst, lww, n_src_dev, n_dst_dev, out, count)
        return out.slice(self._trimmed(count)) if trim else (out, count)

    def set_delta_count(self, src: TupleSet, dst: TupleSet, lww: bool, n_src_dev: torch.Tensor | None = None,
                        n_dst_dev: torch.Tensor | None = None, count: torch.Tensor | None = None) -> torch.Tensor:
        """len(delta(src, dst)) alone (int64[1] on the device, no
        synchronisation); 0 iff dst already holds all of src -- the in-sync
        test.  Nothing is written but the count."""
        return self._set_delta(src, dst, lww, n_src_dev, n_dst_dev, None, count)

    def _set_delta(self, src: TupleSet, dst: TupleSet, lww: bool, n_src_dev, n_dst_dev, out, count) -> torch.Tensor:
        count = self._count(count)
        self._check(count, itemsize=8)
        self._check_tuples(src, dst, out)
        self._check(n_src_dev, n_dst_dev, itemsize=8)
        self._call("crdt_set_delta", 0 if lww else 1, _ref(src), len(src), _ptr(n_src_dev), _ref(dst), len(dst),
                   _ptr(n_dst_dev), _ref(out), count.data_ptr())
        return count

    # -- tombstone compaction under a causal-stability cut (crdt_set_compact)
    def set_compact(self, t: TupleSet, lww: bool, cut: torch.Tensor | None, n_dev: torch.Tensor | None = None,
                    out: TupleSet | None = None, src: torch.Tensor | None = None, count: torch.Tensor | None = None,
                    with_src: bool = False, trim: bool = False):
        """merge(t, {}) of the sorted set state ``t`` without its stable dead
        tuples: a tag (key, ts, rep) is stable iff rep < len(cut) and ts <=
        cut[rep] (``cut``: int64 storage of uint64 on the device, e.g.
        :meth:`vclock_stable_cut`; None: no cut, nothing is dropped).  OR-Set
        drops a stable tag whose copies' tomb-OR is 1, LWW a key whose winner
        is a stable tombstone.  The caller vouches that every replica holds
        the tombstones the cut makes stable.  Returns (out, count), or (out,
        src, count) with ``with_src`` (or a ``src`` tensor): device-resident,
        no synchronisation -- out / src of capacity len(t), their first
        ``count`` entries valid, src[i] the index in t of out[i]'s tuple (the
        first copy of its tag), for :meth:`gather_src`.  ``n_dev`` as in
        :meth:`set_elements`; with ``trim`` the device status is checked and
        the sliced results returned."""
        n = len(t)
        out = self._out_tuples(out, n, "set_compact: out holds fewer tuples than t")
        src = self._out_src(src, with_src, n, "set_compact: src must be int64 and hold len(t) entries")
        count = self._set_compact(t, lww, cut, n_dev, out, src, count)
        return self._result(trim, count, out, src)

    def set_compact_count(self, t: TupleSet, lww: bool, cut: torch.Tensor | None, n_dev: torch.Tensor | None = None,
                          count: torch.Tensor | None = None) -> torch.Tensor:
        """len(compact(t, cut)) alone (int64[1] on the device, no
        synchronisation): one pass over the tuples, nothing else written."""
        return self._set_compact(t, lww, cut, n_dev, None, None, count)

    def _set_compact(self, t: TupleSet, lww: bool, cut, n_dev, out, src, count) -> torch.Tensor:
        count = self._count(count)
        self._check(count, itemsize=8)
        self._check_tuples(t, out)
        self._check(cut, n_dev, itemsize=8)
        self._call("crdt_set_compact", 0 if lww else 1, _ref(t), len(t), _ptr(n_dev), _ptr(cut),
                   0 if cut is None else cut.numel(), _ref(out), _ptr(src), count.data_ptr())
        return count

    def map_compact(self, t: TupleSet, val: torch.Tensor, lww: bool, cut: torch.Tensor | None):
        """:meth:`set_compact` of a state that keeps a value beside each
        tuple (val[i] belongs to t's tuple i): returns (out, out_val, count),
        device-resident -- the compaction, then one :meth:`gather_src` of
        ``val`` chained off its device count, no read-back."""
        if val.shape[0] != len(t):
            raise ValueError("map_compact: one value per tuple")
        out, src, count = self.set_compact(t, lww, cut, with_src=True)
        return out, self.gather_src(src, val, val[:0], n_dev=count), count

    # -- map reads: each member key's winning tuple, sibling count, point lookup (crdt_map_read / crdt_map_lookup)
    def map_read(self, t: TupleSet, lww: bool, n_dev: torch.Tensor | None = None, with_keys: bool = True,
                 with_nsib: bool = False, keys: torch.Tensor | None = None, win: torch.Tensor | None = None,
                 nsib: torch.Tensor | None = None, count: torch.Tensor | None = None):
        """One row per member key of the sorted set state ``t`` (the keys of
        :meth:`set_elements`, ascending): returns (keys, win, nsib, count),
        device tensors of capacity len(t) whose first ``count`` rows are
        valid, no synchronisation.  win[i] (int64) is the index in t of the
        first copy of key i's winner tag -- LWW: the key's maximal tag;
        OR-Set (also a causal-form state): the greatest live tag -- for
        :meth:`gather_src`; nsib[i] (int32 storage of uint32) the number of
        distinct live tags of the key (LWW: 1), > 1 where concurrent puts left
        the key multi-valued.  keys / nsib are None unless asked for
        (``with_keys`` / ``with_nsib``, or a tensor to write into).  ``n_dev``
        as in :meth:`set_elements`."""
        n = len(t)
        dev = self.device
        if keys is None and with_keys:
            keys = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        if nsib is None and with_nsib:
            nsib = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        win = torch.empty(max(n, 1), dtype=torch.int64, device=dev) if win is None else win
        count = self._count(count)
        self._check_tuples(t)
        self._check(win, count, itemsize=8)
        if win.dtype != torch.int64 or win.numel() < n:
            raise ValueError("map_read: win must be int64 and hold len(t) rows")
        self._check(keys, itemsize=8)
        self._check(nsib, itemsize=4)
        if (keys is not None and keys.numel() < n) or (nsib is not None and nsib.numel() < n):
            raise ValueError("map_read: keys / nsib hold fewer rows than t has tuples")
        self._check(n_dev, itemsize=8)
        self._call("crdt_map_read", 0 if lww else 1, _ref(t), n, _ptr(n_dev), _ptr(keys), _ptr(win), _ptr(nsib),
                   count.data_ptr())
        return keys, win, nsib, count

    def map_values(self, t: TupleSet, val: torch.Tensor, lww: bool, n_dev: torch.Tensor | None = None):
        """The map a state holds beside its value column (val[i] belongs to
        t's tuple i): returns (keys, values, count), device-resident -- the
        member keys ascending and each key's winning value: the read, then
        one :meth:`gather_src` chained off its device count, no read-back."""
        if val.shape[0] != len(t):
            raise ValueError("map_values: one value per tuple")
        keys, win, _, count = self.map_read(t, lww, n_dev=n_dev)
        return keys, self.gather_src(win, val, val[:0], n_dev=count), count

    def map_lookup(self, t: TupleSet, probes: torch.Tensor, lww: bool, n_dev: torch.Tensor | None = None,
                   with_nsib: bool = False, win: torch.Tensor | None = None, nsib: torch.Tensor | None = None):
        """:meth:`map_read`'s row of each probe key (uint64 in int64 storage,
        any order, duplicates allowed): returns (win, nsib), device tensors
        of len(probes), no synchronisation -- win[i] = -1 and nsib[i] = 0 for
        a key that is not a member; nsib is None unless asked for."""
        m = probes.numel()
        win = torch.empty(max(m, 1), dtype=torch.int64, device=self.device)[:m] if win is None else win
        if nsib is None and with_nsib:
            nsib = torch.empty(max(m, 1), dtype=torch.int32, device=self.device)[:m]
        self._check_tuples(t)
        self._check(probes, win, itemsize=8)
        if win.dtype != torch.int64 or win.numel() < m:
            raise ValueError("map_lookup: win must be int64 and hold one entry per probe")
        self._check(nsib, itemsize=4)
        if nsib is not None and nsib.numel() < m:
            raise ValueError("map_lookup: nsib holds fewer entries than there are probes")
        self._check(n_dev, itemsize=8)
        self._call("crdt_map_lookup", 0 if lww else 1, _ref(t), len(t), _ptr(n_dev), _ptr(probes), m, _ptr(win),
                   _ptr(nsib))
        return win, nsib

    def map_get(self, t: TupleSet, val: torch.Tensor, probes: torch.Tensor, default, lww: bool,
                n_dev: torch.Tensor | None = None) -> torch.Tensor:
        """The value of each probe key, ``default`` where the key is not a
        member: the lookup, then one :meth:`gather_src` whose b side is the
        one-element default column (a lookup's -1 names its element 0), no
        synchronisation.  ``default``: a scalar, or a tensor of one element /
        row of val's dtype."""
        if val.shape[0] != len(t):
            raise ValueError("map_get: one value per tuple")
        if torch.is_tensor(default):
            dflt = default.to(device=self.device, dtype=val.dtype).reshape((1,) + tuple(val.shape[1:])).contiguous()
        else:
            dflt = torch.full((1,) + tuple(val.shape[1:]), default, dtype=val.dtype, device=self.device)
        win, _ = self.map_lookup(t, probes, lww, n_dev=n_dev)
        out = self.gather_src(win, val, dflt)
        return out[:probes.numel()]

    # -- the tombstone-free OR-Set: causal merge under version vectors (crdt_orset_merge_causal)
    def causal_merge(self, a: TupleSet, ctx_a: torch.Tensor | None, b: TupleSet, ctx_b: torch.Tensor | None,
                     n_a_dev: torch.Tensor | None = None, n_b_dev: torch.Tensor | None = None,
                     out: TupleSet | None = None, src: torch.Tensor | None = None,
                     ctx_out: torch.Tensor | None = None, count: torch.Tensor | None = None,
                     with_src: bool = False, trim: bool = False):
        """Merge of two causal OR-Set states (tuples, context): a tag (key,
        ts, rep) survives iff it is present in both, or present in one side
        and not covered by the other side's context.  Present: the side holds
        a copy and none of its copies is tombstoned; covered by ``ctx``: rep <
        len(ctx) and ts <= ctx[rep], unsigned (``ctx_a`` / ``ctx_b``: int64
        storage of uint64 on the device; None: the empty context, which
        covers nothing).  The caller vouches that each state's context covers
        its own present tags and is contiguous.  Returns (out, ctx_out,
        count), or (out, src, ctx_out, count) with ``with_src`` (or a ``src``
        tensor): device-resident, no synchronisation -- out / src of capacity
        len(a) + len(b), their first ``count`` entries valid, every out.tomb
        0; src[i] >= 0: out[i] is a[src[i]], src[i] < 0: it is b[-(src[i] +
        1)] -- the first copy of the tag on a side that holds it present, a
        before b -- for :meth:`gather_src`; ctx_out the element-wise maximum
        of the contexts (the shorter one padded with zeros), written even when
        a length is out of range.  ``n_a_dev`` / ``n_b_dev`` as in
        :meth:`set_delta`; with ``trim`` the device status is checked and the
        sliced results returned."""
        out, src, ctx_out = self._causal_outputs("causal_merge", a, ctx_a, b, ctx_b, out, src, ctx_out, with_src)
        count = self._causal_merge(a, ctx_a, b, ctx_b, n_a_dev, n_b_dev, out, src, ctx_out, count)
        return self._result(trim, count, out, src, ctx_out)

    def _causal_outputs(self, who: str, a: TupleSet, ctx_a, b: TupleSet, ctx_b, out, src, ctx_out, with_src: bool):
        """The output buffers of a causal merge, allocated where not given and checked where given."""
        n = len(a) + len(b)
        out = self._out_tuples(out, n, f"{who}: out holds fewer tuples than len(a) + len(b)")
        src = self._out_src(src, with_src, n, f"{who}: src must be int64 and hold len(a) + len(b) entries")
        nc = max(0 if ctx_a is None else ctx_a.numel(), 0 if ctx_b is None else ctx_b.numel())
        ctx_out = torch.empty(nc, dtype=torch.int64, device=self.device) if ctx_out is None else ctx_out
        self._check(ctx_out, itemsize=8)
        if ctx_out.numel() < nc:
            raise ValueError(f"{who}: ctx_out holds fewer entries than the longer context")
        return out, src, ctx_out

    def causal_merge_count(self, a: TupleSet, ctx_a: torch.Tensor | None, b: TupleSet, ctx_b: torch.Tensor | None,
                           n_a_dev: torch.Tensor | None = None, n_b_dev: torch.Tensor | None = None,
                           count: torch.Tensor | None = None) -> torch.Tensor:
        """len(causal_merge(a, b)) alone (int64[1] on the device, no
        synchronisation): nothing is written but the count."""
        return self._causal_merge(a, ctx_a, b, ctx_b, n_a_dev, n_b_dev, None, None, None, count)

    def _causal_merge(self, a: TupleSet, ctx_a, b: TupleSet, ctx_b, n_a_dev, n_b_dev, out, src, ctx_out, count,
                      ranges=None) -> torch.Tensor:
        """crdt_orset_merge_causal, or with ranges = (splitters, flags) crdt_orset_merge_causal_ranges."""
        count = self._count(count)
        self._check(count, itemsize=8)
        self._check_tuples(a, b, out)
        self._check(ctx_a, ctx_b, n_a_dev, n_b_dev, itemsize=8)
        fn, mid = "crdt_orset_merge_causal", ()
        if ranges is not None:
            splitters, flags = ranges
            m = 0 if splitters is None else splitters.numel()
            self._check(flags, itemsize=1)
            if flags.numel() < m + 1:
                raise ValueError("causal_merge_ranges: flags must hold len(splitters) + 1 entries")
            self._check(splitters, itemsize=8)
            fn, mid = "crdt_orset_merge_causal_ranges", (_ptr(splitters) if m else None, m, _ptr(flags))
        self._call(fn, _ref(a), len(a), _ptr(n_a_dev), _ptr(ctx_a), 0 if ctx_a is None else ctx_a.numel(),
                   _ref(b), len(b), _ptr(n_b_dev), _ptr(ctx_b), 0 if ctx_b is None else ctx_b.numel(), *mid,
                   _ref(out), _ptr(src), _ptr(ctx_out), count.data_ptr())
        return count

    def causal_map_merge(self, a: TupleSet, a_val: torch.Tensor, ctx_a: torch.Tensor | None, b: TupleSet,
                         b_val: torch.Tensor, ctx_b: torch.Tensor | None):
        """:meth:`causal_merge` of states that keep a value beside each tuple
        (a_val[i] belongs to a's tuple i): returns (out, out_val, ctx_out,
        count), device-resident -- the merge, then one :meth:`gather_src`
        chained off its device count, no read-back."""
        if a_val.shape[0] != len(a) or b_val.shape[0] != len(b):
            raise ValueError("causal_map_merge: one value per tuple on each side")
        out, src, ctx_out, count = self.causal_merge(a, ctx_a, b, ctx_b, with_src=True)
        return out, self.gather_src(src, a_val, b_val, n_dev=count), ctx_out, count

    # -- the OR-Set mutators: a batch of local adds and removes (crdt_set_apply)
    def set_apply(self, t: TupleSet, clock: torch.Tensor, rep: int, op_keys: torch.Tensor, op_kinds: torch.Tensor,
                  causal: bool, n_dev: torch.Tensor | None = None, out: TupleSet | None = None,
                  src: torch.Tensor | None = None, clock_out: torch.Tensor | None = None,
                  count: torch.Tensor | None = None, trim: bool = True, with_src: bool = False):
        """A batch of local operations of replica ``rep`` applied to its
        sorted OR-Set state ``t``: ``op_keys`` (int64 storage of uint64,
        non-decreasing) and ``op_kinds`` (uint8: 0 add, else remove) on the
        device, ``clock`` the replica's clock row / causal context (int64
        storage of uint64).  Operation i is rep's event clock[rep] + 1 + i,
        add and remove alike; the result is the batch applied one operation
        at a time: an add inserts (key, event, rep), a remove tombstones
        (``causal`` False) or deletes (``causal`` True) every tag of its key
        held at that point.  Each tag is written once in ascending order,
        tombstone form with the tomb-OR of its copies then the removes,
        causal form without the tombstoned tags and with every tomb 0.
        Returns (out, clock_out, count), or (out, src, clock_out, count) with
        ``with_src`` (or a ``src`` tensor): out / src of capacity len(t) +
        len(op_keys), src[i] >= 0 the index in t of the tag's first copy,
        src[i] < 0 the add at batch index -(src[i] + 1), for
        :meth:`gather_src`; clock_out = clock with [rep] advanced by the
        batch's length.  ``n_dev`` as in :meth:`set_elements`; a length out
        of range, or events that would wrap past 2^64, write nothing but
        count = ~0 and raise CRDT_DEV_RANGE.  The caller vouches that every
        tag of rep in t has ts <= clock[rep].  With ``trim`` (the default)
        the device status is checked and the sliced results returned; without
        it everything stays on the device, no synchronisation."""
        n = len(t) + op_keys.numel()
        out = self._out_tuples(out, n, "set_apply: out holds fewer tuples than len(t) + len(op_keys)")
        src = self._out_src(src, with_src, n, "set_apply: src must be int64 and hold len(t) + len(op_keys) entries")
        clock_out = torch.empty(clock.numel(), dtype=torch.int64, device=self.device) if clock_out is None else clock_out
        count = self._set_apply(t, clock, rep, op_keys, op_kinds, causal, n_dev, out, src, clock_out, count)
        return self._result(trim, count, out, src, clock_out)

    def set_apply_count(self, t: TupleSet, clock: torch.Tensor, rep: int, op_keys: torch.Tensor,
                        op_kinds: torch.Tensor, causal: bool, n_dev: torch.Tensor | None = None,
                        clock_out: torch.Tensor | None = None, count: torch.Tensor | None = None) -> torch.Tensor:
        """len(set_apply(...)) alone (int64[1] on the device, no
        synchronisation): nothing is written but the count and, when given,
        ``clock_out``."""
        return self._set_apply(t, clock, rep, op_keys, op_kinds, causal, n_dev, None, None, clock_out, count)

    def _set_apply(self, t: TupleSet, clock, rep: int, op_keys, op_kinds, causal: bool, n_dev, out, src, clock_out,
                   count) -> torch.Tensor:
        count = self._count(count)
        self._check(count, clock, op_keys, itemsize=8)
        self._check(op_kinds, itemsize=1)
        m = op_keys.numel()
        if op_kinds.numel() != m:
            raise ValueError("set_apply: one kind per operation key")
        if not 0 <= rep < 2 ** 32:
            raise ValueError("set_apply: rep is a uint32")
        self._check_tuples(t, out)
        self._check(n_dev, clock_out, itemsize=8)
        if clock_out is not None and clock_out.numel() < clock.numel():
            raise ValueError("set_apply: clock_out holds fewer entries than clock")
        self._call("crdt_set_apply", 1 if causal else 0, _ref(t), len(t), _ptr(n_dev), _ptr(clock), clock.numel(),
                   rep, _ptr(op_keys) if m else None, _ptr(op_kinds) if m else None, m, _ref(out), _ptr(src),
                   _ptr(clock_out), count.data_ptr())
        return count

    def map_apply(self, t: TupleSet, val: torch.Tensor, clock: torch.Tensor, rep: int, op_keys: torch.Tensor,
                  op_kinds: torch.Tensor, op_vals: torch.Tensor, causal: bool):
        """:meth:`set_apply` of a state that keeps a value beside each tuple
        (val[i] belongs to t's tuple i, op_vals[i] to operation i; a remove's
        value is never read): an OR-Map put / delete.  Returns (out, out_val,
        clock_out, count), device-resident -- the apply, then one
        :meth:`gather_src` chained off its device count, no read-back."""
        if val.shape[0] != len(t) or op_vals.shape[0] != op_keys.numel():
            raise ValueError("map_apply: one value per tuple and per operation")
        out, src, clock_out, count = self.set_apply(t, clock, rep, op_keys, op_kinds, causal, with_src=True, trim=False)
        return out, self.gather_src(src, val, op_vals, n_dev=count), clock_out, count

    # -- the keyed PN-Counter map: merge, increments, reads and deltas (crdt_cmap_*)
    def _check_cmap(self, *maps: CounterMap | None) -> None:
        for s in maps:
            if s is not None:
                self._check(s.key, s.p, s.n, itemsize=8)
                self._check(s.rep, itemsize=4)

    def _out_cmap(self, out: CounterMap | None, n: int, short: str) -> CounterMap:
        out = CounterMap.empty(max(n, 1), self.device) if out is None else out
        if len(out) < n:
            raise ValueError(short)
        return out

    def cmap_merge(self, a: CounterMap, b: CounterMap, n_a_dev: torch.Tensor | None = None,
                   n_b_dev: torch.Tensor | None = None, out: CounterMap | None = None,
                   count: torch.Tensor | None = None, trim: bool = False):
        """The join of two counter maps: the union of their cells, a cell held
        by both with p = max(p_a, p_b), n = max(n_a, n_b), unsigned.  Returns
        (out, count), device-resident, no synchronisation -- out of capacity
        len(a) + len(b), its first ``count`` cells valid.  ``n_a_dev`` /
        ``n_b_dev`` (int64[1] on the device, e.g. another call's count): only
        so many leading cells of that side are read; a value over the side's
        length leaves count = 2^64 - 1 and raises CRDT_DEV_RANGE in
        :meth:`device_status`.  With ``trim`` the device status is checked and
        out is cut to the count."""
        out = self._out_cmap(out, len(a) + len(b), "cmap_merge: out holds fewer cells than len(a) + len(b)")
        count = self._cmap_merge(a, b, n_a_dev, n_b_dev, out, count)
        return self._result(trim, count, out, None)

    def cmap_merge_count(self, a: CounterMap, b: CounterMap, n_a_dev: torch.Tensor | None = None,
                         n_b_dev: torch.Tensor | None = None, count: torch.Tensor | None = None) -> torch.Tensor:
        """len(cmap_merge(a, b)) alone (int64[1] on the device, no
        synchronisation): nothing is written but the count."""
        return self._cmap_merge(a, b, n_a_dev, n_b_dev, None, count)

    def _cmap_merge(self, a: CounterMap, b: CounterMap, n_a_dev, n_b_dev, out, count) -> torch.Tensor:
        count = self._count(count)
        self._check(count, n_a_dev, n_b_dev, itemsize=8)
        self._check_cmap(a, b, out)
        self._call("crdt_cmap_merge", _ref(a), len(a), _ptr(n_a_dev), _ref(b), len(b), _ptr(n_b_dev), _ref(out),
                   count.data_ptr())
        return count

    def cmap_apply(self, t: CounterMap, rep: int, op_keys: torch.Tensor, op_dp: torch.Tensor, op_dn: torch.Tensor,
                   n_dev: torch.Tensor | None = None, out: CounterMap | None = None,
                   count: torch.Tensor | None = None, trim: bool = False):
        """Replica ``rep``'s batch of increments applied to the counter map
        ``t``: ``op_keys`` (int64 storage of uint64, strictly ascending),
        ``op_dp`` / ``op_dn`` (int64 storage of uint64) on the device.  Cell
        (op_keys[i], rep) becomes (p + op_dp[i], n + op_dn[i]) mod 2^64; an
        absent cell is created from (0, 0).  Returns (out, count) as
        :meth:`cmap_merge` does, out of capacity len(t) + len(op_keys)."""
        m = op_keys.numel()
        out = self._out_cmap(out, len(t) + m, "cmap_apply: out holds fewer cells than len(t) + len(op_keys)")
        count = self._count(count)
        self._check(count, op_keys, op_dp, op_dn, n_dev, itemsize=8)
        if op_dp.numel() != m or op_dn.numel() != m:
            raise ValueError("cmap_apply: one dp and one dn per operation key")
        if not 0 <= rep < 2 ** 32:
            raise ValueError("cmap_apply: rep is a uint32")
        self._check_cmap(t, out)
        self._call("crdt_cmap_apply", _ref(t), len(t), _ptr(n_dev), rep, _ptr(op_keys) if m else None,
                   _ptr(op_dp) if m else None, _ptr(op_dn) if m else None, m, _ref(out), count.data_ptr())
        return self._result(trim, count, out, None)

    def cmap_values(self, t: CounterMap, n_dev: torch.Tensor | None = None, keys: torch.Tensor | None = None,
                    p: torch.Tensor | None = None, n: torch.Tensor | None = None, value: torch.Tensor | None = None,
                    count: torch.Tensor | None = None, trim: bool = False):
        """One row per distinct key of ``t``, in key order: returns (keys, P,
        N, value, count), device tensors (int64 storage) of capacity len(t)
        whose first ``count`` rows are valid, no synchronisation -- P / N the
        sums of the key's p / n cells mod 2^64, value = (int64)(P - N).
        ``n_dev`` as in :meth:`cmap_merge`; with ``trim`` the device status is
        checked and the rows are cut to the count."""
        rows = len(t)
        cols = []
        for c in (keys, p, n, value):
            c = torch.empty(max(rows, 1), dtype=torch.int64, device=self.device) if c is None else c
            self._check(c, itemsize=8)
            if c.numel() < rows:
                raise ValueError("cmap_values: an output holds fewer rows than t has cells")
            cols.append(c)
        count = self._count(count)
        self._check(count, n_dev, itemsize=8)
        self._check_cmap(t)
        self._call("crdt_cmap_values", _ref(t), rows, _ptr(n_dev), *(c.data_ptr() for c in cols), count.data_ptr())
        if trim:
            k = self._trimmed(count)
            cols = [c[:k] for c in cols]
        return (*cols, count)

    def cmap_count_keys(self, t: CounterMap, n_dev: torch.Tensor | None = None,
                        count: torch.Tensor | None = None) -> torch.Tensor:
        """The number of distinct keys of ``t`` alone (int64[1] on the device,
        no synchronisation): :meth:`cmap_values` with no output."""
        count = self._count(count)
        self._check(count, n_dev, itemsize=8)
        self._check_cmap(t)
        self._call("crdt_cmap_values", _ref(t), len(t), _ptr(n_dev), None, None, None, None, count.data_ptr())
        return count

    def cmap_get(self, t: CounterMap, probes: torch.Tensor, n_dev: torch.Tensor | None = None,
                 value: torch.Tensor | None = None, found: torch.Tensor | None = None, with_found: bool = True):
        """The counter of each probe key (uint64 in int64 storage, any order,
        repeats allowed): returns (value, found), device tensors of
        len(probes), no synchronisation -- value[i] (int64) is 0 and found[i]
        (uint8) is 0 where the key is absent; found is None unless asked for.
        A device length over len(t) gives zeros and raises CRDT_DEV_RANGE."""
        m = probes.numel()
        value = torch.empty(max(m, 1), dtype=torch.int64, device=self.device)[:m] if value is None else value
        if found is None and with_found:
            found = torch.empty(max(m, 1), dtype=torch.uint8, device=self.device)[:m]
        self._check_cmap(t)
        self._check(probes, value, n_dev, itemsize=8)
        self._check(found, itemsize=1)
        if value.dtype != torch.int64 or value.numel() < m or (found is not None and found.numel() < m):
            raise ValueError("cmap_get: value (int64) and found must hold one entry per probe")
        self._call("crdt_cmap_lookup", _ref(t), len(t), _ptr(n_dev), _ptr(probes), m, _ptr(value), _ptr(found))
        return value, found

    def cmap_delta(self, src: CounterMap, dst: CounterMap, n_src_dev: torch.Tensor | None = None,
                   n_dst_dev: torch.Tensor | None = None, out: CounterMap | None = None,
                   count: torch.Tensor | None = None, trim: bool = False):
        """The smallest D with merge(dst, D) == merge(dst, src): the cells of
        src that dst lacks or holds with a smaller p or n, with src's own p
        and n.  Returns (D, count) as :meth:`cmap_merge` does, D of capacity
        len(src)."""
        out = self._out_cmap(out, len(src), "cmap_delta: out holds fewer cells than src")
        count = self._cmap_delta(src, dst, n_src_dev, n_dst_dev, out, count)
        return self._result(trim, count, out, None)

    def cmap_delta_count(self, src: CounterMap, dst: CounterMap, n_src_dev: torch.Tensor | None = None,
                         n_dst_dev: torch.Tensor | None = None, count: torch.Tensor | None = None) -> torch.Tensor:
        """len(cmap_delta(src, dst)) alone (int64[1] on the device, no
        synchronisation); 0 iff dst already holds all of src."""
        return self._cmap_delta(src, dst, n_src_dev, n_dst_dev, None, count)

    def _cmap_delta(self, src: CounterMap, dst: CounterMap, n_src_dev, n_dst_dev, out, count) -> torch.Tensor:
        count = self._count(count)
        self._check(count, n_src_dev, n_dst_dev, itemsize=8)
        self._check_cmap(src, dst, out)
        self._call("crdt_cmap_delta", _ref(src), len(src), _ptr(n_src_dev), _ref(dst), len(dst), _ptr(n_dst_dev),
                   _ref(out), count.data_ptr())
        return count

    # -- range digests of a counter map: where two replicas that share no memory
    #    differ (crdt_cmap_digest / crdt_cmap_select; the diff is digest_diff)
    def cmap_digest(self, t: CounterMap, splitters: torch.Tensor | None, n_dev: torch.Tensor | None = None,
                    hash_out: torch.Tensor | None = None, count_out: torch.Tensor | None = None):
        """One order-independent fingerprint per key range of the counter map
        ``t``: returns (hash, count), int64 storage of uint64 on the device,
        len(splitters) + 1 entries each, no synchronisation.  The buckets are
        :meth:`set_digest`'s (``splitters`` ascending uint64 in int64 storage
        on the device; None or empty: one bucket; all cells of a key share a
        bucket); hash[b] is the wrapping sum over the cells in b of
        sm(sm(sm(sm(key) ^ rep) ^ p) ^ n), sm =
        :func:`crdt_amd.synth.splitmix64`, count[b] their number.  ``n_dev``
        as in :meth:`cmap_merge`; a value over len(t) leaves every entry
        2^64 - 1 and raises CRDT_DEV_RANGE."""
        m = 0 if splitters is None else splitters.numel()
        hash_out = torch.empty(m + 1, dtype=torch.int64, device=self.device) if hash_out is None else hash_out
        count_out = torch.empty(m + 1, dtype=torch.int64, device=self.device) if count_out is None else count_out
        self._check_cmap(t)
        self._check(hash_out, count_out, itemsize=8)
        if hash_out.numel() < m + 1 or count_out.numel() < m + 1:
            raise ValueError("cmap_digest: the outputs must hold len(splitters) + 1 entries")
        self._check(splitters, n_dev, itemsize=8)
        self._call("crdt_cmap_digest", _ref(t), len(t), _ptr(n_dev), _ptr(splitters) if m else None, m,
                   hash_out.data_ptr(), count_out.data_ptr())
        return hash_out, count_out

    def cmap_select(self, t: CounterMap, splitters: torch.Tensor | None, flags: torch.Tensor,
                    n_dev: torch.Tensor | None = None, out: CounterMap | None = None,
                    count: torch.Tensor | None = None, trim: bool = False):
        """The cells of ``t`` whose key falls into a bucket with ``flags[b] !=
        0`` (uint8[len(splitters) + 1], e.g. :meth:`digest_diff`'s), in order
        and unchanged: what a replica ships for the differing ranges.  The
        merge is monotone, so the receiver's side is ``cmap_merge(dst, out,
        n_b_dev=count)``.  Returns (out, count) as :meth:`cmap_delta` does,
        out of capacity len(t)."""
        out = self._out_cmap(out, len(t), "cmap_select: out holds fewer cells than t")
        count = self._cmap_select(t, splitters, flags, n_dev, out, count)
        return self._result(trim, count, out, None)

    def cmap_select_count(self, t: CounterMap, splitters: torch.Tensor | None, flags: torch.Tensor,
                          n_dev: torch.Tensor | None = None, count: torch.Tensor | None = None) -> torch.Tensor:
        """len(:meth:`cmap_select`) alone (int64[1] on the device, no
        synchronisation): how much the flagged ranges would ship."""
        return self._cmap_select(t, splitters, flags, n_dev, None, count)

    def _cmap_select(self, t: CounterMap, splitters, flags, n_dev, out, count) -> torch.Tensor:
        count = self._count(count)
        m = 0 if splitters is None else splitters.numel()
        self._check(count, itemsize=8)
        self._check(flags, itemsize=1)
        if flags.numel() < m + 1:
            raise ValueError("cmap_select: flags must hold len(splitters) + 1 entries")
        self._check_cmap(t, out)
        self._check(splitters, n_dev, itemsize=8)
        self._call("crdt_cmap_select", _ref(t), len(t), _ptr(n_dev), _ptr(splitters) if m else None, m, _ptr(flags),
                   _ref(out), count.data_ptr())
        return count

    # -- counter-map state from unsorted increment logs: combine, add, ingest
    #    (crdt_cmap_combine / crdt_cmap_add / crdt_cmap_from_ops)
    def cmap_combine(self, t: CounterMap, n_dev: torch.Tensor | None = None, idx: torch.Tensor | None = None,
                     out: CounterMap | None = None, count: torch.Tensor | None = None, trim: bool = False):
        """Sorted cells with repeats to a state: ``t.key`` / ``t.rep``
        ascending by (key, rep) but not strictly; out holds one cell per
        distinct (key, rep) with p / n summed over the run mod 2^64 (a run
        summing to 0 keeps its cell).  With ``idx`` (int32 storage of uint32,
        one per cell of ``t.key``) cell i contributes ``t.p[idx[i]]``,
        ``t.n[idx[i]]`` -- ``t.p`` / ``t.n`` are then columns of any length,
        every index checked against it; one out of range contributes 0 and
        raises CRDT_DEV_RANGE.  Returns (out, count) as :meth:`cmap_merge`
        does, out of capacity len(t); ``n_dev`` as there.  No
        synchronisation."""
        out = self._out_cmap(out, len(t), "cmap_combine: out holds fewer cells than t")
        count = self._cmap_combine(t, n_dev, idx, out, count)
        return self._result(trim, count, out, None)

    def cmap_combine_count(self, t: CounterMap, n_dev: torch.Tensor | None = None,
                           count: torch.Tensor | None = None) -> torch.Tensor:
        """len(cmap_combine(t)) alone (int64[1] on the device, no
        synchronisation): the number of distinct (key, rep)."""
        return self._cmap_combine(t, n_dev, None, None, count)

    def _cmap_combine(self, t: CounterMap, n_dev, idx, out, count) -> torch.Tensor:
        count = self._count(count)
        self._check(count, n_dev, itemsize=8)
        self._check(idx, itemsize=4)
        n = len(t)
        if t.rep.numel() != n or t.p.numel() != t.n.numel():
            raise ValueError("cmap_combine: one rep per key, and p and n of one length")
        if idx is None and out is not None and t.p.numel() != n:   # (the count alone reads neither)
            raise ValueError("cmap_combine: without idx, one p and one n per key")
        if idx is not None and idx.numel() != n:
            raise ValueError("cmap_combine: one index per cell")
        self._check_cmap(t, out)
        self._call("crdt_cmap_combine", _ref(t), n, _ptr(n_dev), _ptr(idx), t.p.numel() if idx is not None else 0,
                   _ref(out), count.data_ptr())
        return count

    def cmap_add(self, t: CounterMap, d: CounterMap, n_t_dev: torch.Tensor | None = None,
                 n_d_dev: torch.Tensor | None = None, out: CounterMap | None = None,
                 count: torch.Tensor | None = None, trim: bool = False):
        """The additive join of the state ``t`` and the batch ``d`` (both
        strictly ascending): the union of the cells, a cell held by both with
        (p_t + p_d, n_t + n_d) mod 2^64, a cell of ``d`` alone created with
        d's values.  ``cmap_apply`` with many replicas in one pass.  NOT
        idempotent: each batch is delivered once, which is the caller's to
        ensure.  Returns (out, count) as :meth:`cmap_merge` does, out of
        capacity len(t) + len(d); ``n_t_dev`` / ``n_d_dev`` as its lengths."""
        out = self._out_cmap(out, len(t) + len(d), "cmap_add: out holds fewer cells than len(t) + len(d)")
        count = self._cmap_add(t, d, n_t_dev, n_d_dev, out, count)
        return self._result(trim, count, out, None)

    def cmap_add_count(self, t: CounterMap, d: CounterMap, n_t_dev: torch.Tensor | None = None,
                       n_d_dev: torch.Tensor | None = None, count: torch.Tensor | None = None) -> torch.Tensor:
        """len(cmap_add(t, d)) alone (int64[1] on the device, no
        synchronisation): nothing is written but the count."""
        return self._cmap_add(t, d, n_t_dev, n_d_dev, None, count)

    def _cmap_add(self, t: CounterMap, d: CounterMap, n_t_dev, n_d_dev, out, count) -> torch.Tensor:
        count = self._count(count)
        self._check(count, n_t_dev, n_d_dev, itemsize=8)
        self._check_cmap(t, d, out)
        self._call("crdt_cmap_add", _ref(t), len(t), _ptr(n_t_dev), _ref(d), len(d), _ptr(n_d_dev), _ref(out),
                   count.data_ptr())
        return count

    def cmap_from_ops(self, op_keys: torch.Tensor, op_reps: torch.Tensor, op_dp: torch.Tensor, op_dn: torch.Tensor,
                      out: CounterMap | None = None, count: torch.Tensor | None = None, trim: bool = False):
        """An increment log to a state: operations (op_keys[i], op_reps[i],
        +op_dp[i], -op_dn[i]) in any order, repeats and any mix of replicas
        (int64 storage of uint64; ``op_reps`` int32 storage of uint32).  Cell
        (k, r) of the result holds the sums mod 2^64 over the operations of
        that key and replica; the operations' order does not matter.  Returns
        (out, count) as :meth:`cmap_merge` does, out of capacity
        len(op_keys) < 2^32.  Synchronises once (the device sort's plan)."""
        m = op_keys.numel()
        out = self._out_cmap(out, m, "cmap_from_ops: out holds fewer cells than there are operations")
        count = self._count(count)
        self._check(count, op_keys, op_dp, op_dn, itemsize=8)
        self._check(op_reps, itemsize=4)
        if op_reps.numel() != m or op_dp.numel() != m or op_dn.numel() != m:
            raise ValueError("cmap_from_ops: one rep, one dp and one dn per operation key")
        self._check_cmap(out)
        self._call("crdt_cmap_from_ops", _ptr(op_keys) if m else None, _ptr(op_reps) if m else None,
                   _ptr(op_dp) if m else None, _ptr(op_dn) if m else None, m, _ref(out), count.data_ptr())
        return self._result(trim, count, out, None)

    def cmap_ingest(self, t: CounterMap, op_keys: torch.Tensor, op_reps: torch.Tensor, op_dp: torch.Tensor,
                    op_dn: torch.Tensor, n_t_dev: torch.Tensor | None = None, out: CounterMap | None = None,
                    count: torch.Tensor | None = None, trim: bool = False):
        """The log applied to the state ``t``: :meth:`cmap_from_ops`, then
        :meth:`cmap_add` chained off its device count with no further
        read-back.  Returns (out, count), out of capacity len(t) +
        len(op_keys).  Each log is ingested once (see :meth:`cmap_add`)."""
        batch, nb = self.cmap_from_ops(op_keys, op_reps, op_dp, op_dn)
        return self.cmap_add(t, batch.slice(op_keys.numel()), n_t_dev=n_t_dev, n_d_dev=nb, out=out, count=count,
                             trim=trim)

    # -- the causal merge restricted to the key ranges whose digests differ
    #    (crdt_orset_merge_causal_ranges)
    def causal_merge_ranges(self, a: TupleSet, ctx_a: torch.Tensor | None, b: TupleSet, ctx_b: torch.Tensor | None,
                            splitters: torch.Tensor | None, flags: torch.Tensor,
                            n_a_dev: torch.Tensor | None = None, n_b_dev: torch.Tensor | None = None,
                            out: TupleSet | None = None, src: torch.Tensor | None = None,
                            ctx_out: torch.Tensor | None = None, count: torch.Tensor | None = None,
                            with_src: bool = False, trim: bool = False):
        """:meth:`causal_merge` of the receiver's whole causal state ``a``
        with what a peer shipped for the buckets whose digests differ: ``b``
        is normally ``set_select(B, False, splitters, flags)`` with its device
        count as ``n_b_dev``, ``ctx_b`` the peer's whole context.  The causal
        merge is not monotone -- a tag a holds and ctx_b covers is dropped
        unless b's copy is in the operand -- so the buckets come along
        (:meth:`set_digest`'s: ``splitters``, None or empty for one bucket;
        ``flags`` uint8[len(splitters) + 1], e.g. :meth:`digest_diff`'s).  In
        a flagged bucket the rule of :meth:`causal_merge` applies unchanged;
        in an unflagged one b is taken to hold what a holds: a tag survives
        iff a holds it present, b's copies there are ignored entirely (never
        emitted, never named by src, no revival of a tag tombstoned on a) and
        neither context is read.  Every flag set equals :meth:`causal_merge`
        bit for bit; no flag set gives a's present tags and the merged
        context.  The caller vouches that the replicas' canonical tuples are
        equal in every unflagged bucket.  Arguments and results otherwise as
        :meth:`causal_merge`."""
        out, src, ctx_out = self._causal_outputs("causal_merge_ranges", a, ctx_a, b, ctx_b, out, src, ctx_out, with_src)
        count = self._causal_merge(a, ctx_a, b, ctx_b, n_a_dev, n_b_dev, out, src, ctx_out, count,
                                   ranges=(splitters, flags))
        return self._result(trim, count, out, src, ctx_out)

    def causal_merge_ranges_count(self, a: TupleSet, ctx_a: torch.Tensor | None, b: TupleSet,
                                  ctx_b: torch.Tensor | None, splitters: torch.Tensor | None, flags: torch.Tensor,
                                  n_a_dev: torch.Tensor | None = None, n_b_dev: torch.Tensor | None = None,
                                  count: torch.Tensor | None = None) -> torch.Tensor:
        """len(causal_merge_ranges(...)) alone (int64[1] on the device, no
        synchronisation): nothing is written but the count."""
        return self._causal_merge(a, ctx_a, b, ctx_b, n_a_dev, n_b_dev, None, None, None, count,
                                  ranges=(splitters, flags))

    def causal_map_merge_ranges(self, a: TupleSet, a_val: torch.Tensor, ctx_a: torch.Tensor | None, b: TupleSet,
                                b_val: torch.Tensor, ctx_b: torch.Tensor | None, splitters: torch.Tensor | None,
                                flags: torch.Tensor, n_b_dev: torch.Tensor | None = None):
        """:meth:`causal_merge_ranges` of states that keep a value beside each
        tuple (a_val[i] belongs to a's tuple i; ``b``, ``b_val`` and
        ``n_b_dev`` are :meth:`map_select`'s tuples, column and count):
        returns (out, out_val, ctx_out, count), device-resident -- the merge,
        then one :meth:`gather_src` chained off its device count, no
        read-back."""
        if a_val.shape[0] != len(a) or b_val.shape[0] != len(b):
            raise ValueError("causal_map_merge_ranges: one value per tuple on each side")
        out, src, ctx_out, count = self.causal_merge_ranges(a, ctx_a, b, ctx_b, splitters, flags, n_b_dev=n_b_dev,
                                                            with_src=True)
        return out, self.gather_src(src, a_val, b_val, n_dev=count), ctx_out, count

    # -- range digests: where two states differ, without shipping either
    #    (crdt_set_digest / crdt_set_digest_diff / crdt_set_select)
    def set_digest(self, t: TupleSet, lww: bool, splitters: torch.Tensor | None, n_dev: torch.Tensor | None = None,
                   hash_out: torch.Tensor | None = None, count_out: torch.Tensor | None = None):
        """One order-independent fingerprint per key range of the sorted set
        state ``t``: returns (hash, count), int64 storage of uint64 on the
        device, len(splitters) + 1 entries each, no synchronisation.
        ``splitters`` (ascending uint64 in int64 storage on the device; None
        or empty: one bucket) put a key into bucket #{j : splitters[j] <=
        key}; hash[b] is the wrapping sum over the tuples of merge(t, {}) in b
        of sm(sm(sm(key) ^ ts) ^ (rep << 1 | tomb)), sm =
        :func:`crdt_amd.synth.splitmix64`, count[b] their number.  Equal
        canonical tuples in a bucket give equal entries, whatever the copies
        and their order.  ``n_dev`` as in :meth:`set_elements`; a value over
        len(t) leaves every entry 2^64 - 1 and raises CRDT_DEV_RANGE."""
        m = 0 if splitters is None else splitters.numel()
        hash_out = torch.empty(m + 1, dtype=torch.int64, device=self.device) if hash_out is None else hash_out
        count_out = torch.empty(m + 1, dtype=torch.int64, device=self.device) if count_out is None else count_out
        self._check_tuples(t)
        self._check(hash_out, count_out, itemsize=8)
        if hash_out.numel() < m + 1 or count_out.numel() < m + 1:
            raise ValueError("set_digest: the outputs must hold len(splitters) + 1 entries")
        self._check(splitters, n_dev, itemsize=8)
        self._call("crdt_set_digest", 0 if lww else 1, _ref(t), len(t), _ptr(n_dev),
                   _ptr(splitters) if m else None, m, hash_out.data_ptr(), count_out.data_ptr())
        return hash_out, count_out

    def digest_diff(self, da, db, flags: torch.Tensor | None = None, n_diff: torch.Tensor | None = None):
        """Which buckets of two :meth:`set_digest` -- or two
        :meth:`cmap_digest` -- results (hash, count) differ: returns (flags,
        n_diff) -- uint8[buckets], 1 where the hashes or the counts differ or
        either digest is poisoned, and their number (int64[1]), on the device,
        no synchronisation.  It compares plain arrays, so it serves both
        digests.  The digests may come from another replica; both must be of
        one state type and over the same splitters."""
        (ha, ca), (hb, cb) = da, db
        nb = ha.numel()
        if not (ca.numel() == hb.numel() == cb.numel() == nb):
            raise ValueError("digest_diff: the four arrays differ in length")
        flags = torch.empty(max(nb, 1), dtype=torch.uint8, device=self.device) if flags is None else flags
        n_diff = self._count(n_diff)
        self._check(ha, ca, hb, cb, n_diff, itemsize=8)
        self._check(flags, itemsize=1)
        if flags.numel() < nb:
            raise ValueError("digest_diff: flags holds fewer entries than the digests have buckets")
        self._call("crdt_set_digest_diff", _ptr(ha), _ptr(ca), _ptr(hb), _ptr(cb), nb, _ptr(flags), _ptr(n_diff))
        return flags[:nb], n_diff

    def set_select(self, t: TupleSet, lww: bool, splitters: torch.Tensor | None, flags: torch.Tensor,
                   n_dev: torch.Tensor | None = None, out: TupleSet | None = None, src: torch.Tensor | None = None,
                   count: torch.Tensor | None = None, with_src: bool = False, trim: bool = False):
        """The tuples of merge(t, {}) whose key falls into a bucket with
        ``flags[b] != 0`` (uint8[len(splitters) + 1], e.g.
        :meth:`digest_diff`'s), ascending: what a replica ships for the
        differing ranges.  Returns (out, count), or (out, src, count) with
        ``with_src`` (or a ``src`` tensor), as :meth:`set_compact` does."""
        n = len(t)
        out = self._out_tuples(out, n, "set_select: out holds fewer tuples than t")
        src = self._out_src(src, with_src, n, "set_select: src must be int64 and hold len(t) entries")
        count = self._set_select(t, lww, splitters, flags, n_dev, out, src, count)
        return self._result(trim, count, out, src)

    def set_select_count(self, t: TupleSet, lww: bool, splitters: torch.Tensor | None, flags: torch.Tensor,
                         n_dev: torch.Tensor | None = None, count: torch.Tensor | None = None) -> torch.Tensor:
        """len(:meth:`set_select`) alone (int64[1] on the device, no
        synchronisation): how much the flagged ranges would ship."""
        return self._set_select(t, lww, splitters, flags, n_dev, None, None, count)

    def _set_select(self, t: TupleSet, lww: bool, splitters, flags, n_dev, out, src, count) -> torch.Tensor:
        count = self._count(count)
        m = 0 if splitters is None else splitters.numel()
        self._check(count, itemsize=8)
        self._check(flags, itemsize=1)
        if flags.numel() < m + 1:
            raise ValueError("set_select: flags must hold len(splitters) + 1 entries")
        self._check_tuples(t, out)
        self._check(splitters, n_dev, itemsize=8)
        self._call("crdt_set_select", 0 if lww else 1, _ref(t), len(t), _ptr(n_dev), _ptr(splitters) if m else None,
                   m, _ptr(flags), _ref(out), _ptr(src), count.data_ptr())
        return count

    def map_select(self, t: TupleSet, val: torch.Tensor, lww: bool, splitters: torch.Tensor | None,
                   flags: torch.Tensor):
        """:meth:`set_select` of a state that keeps a value beside each tuple
        (val[i] belongs to t's tuple i): returns (out, out_val, count),
        device-resident -- the selection, then one :meth:`gather_src` of
        ``val`` chained off its device count, no read-back."""
        if val.shape[0] != len(t):
            raise ValueError("map_select: one value per tuple")
        out, src, count = self.set_select(t, lww, splitters, flags, with_src=True)
        return out, self.gather_src(src, val, val[:0], n_dev=count), count

    def vclock_stable_cut(self, clocks: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """out[c] = min over rows of clocks[:, c] (unsigned): the
        causal-stability cut of a [replicas, nodes] clock population -- what
        :meth:`set_compact` takes as ``cut``.  No replicas is an error (the
        minimum over none would make every tombstone droppable)."""
        rows, nodes = clocks.shape
        out = torch.empty(nodes, dtype=torch.int64, device=self.device) if out is None else out
        self._check(clocks, out, itemsize=8)
        if out.numel() < nodes:
            raise ValueError("vclock_stable_cut: out holds fewer entries than the clocks have nodes")
        self._call("crdt_vclock_stable_cut", clocks.data_ptr(), rows, nodes, out.data_ptr())
        return out

    def tuples_merge(self, a: TupleSet, b: TupleSet, out: TupleSet | None = None) -> TupleSet:
        """Stable merge of two sorted tuple arrays, every tuple kept (a's
        copies first on an equal tag): crdt_tuples_merge."""
        out = TupleSet.empty(max(len(a) + len(b), 1), self.device) if out is None else out
        self._check_tuples(a, b, out)
        self._call("crdt_tuples_merge", _ref(a), len(a), _ref(b), len(b), _ref(out))
        return out.slice(len(a) + len(b))

    def count_unsorted(self, t: TupleSet) -> int:
        bad = self._count(None)
        self._call("crdt_tuples_count_unsorted", _ref(t), len(t), bad.data_ptr())
        return int(bad.item())

    # ------------------------------------------------------------ RefMerge (a1-a3)
    def _refmerge_in(self, d: dict) -> crdt_refmerge_in:
        return crdt_refmerge_in(
            d["replicas"], int(d["n_slots"]), d["l_ts"].numel(), int(d.get("n_r", d["r_ts"].numel())),
            d["kv_key"].numel(),
            d["str_off"].numel() - 1,
            _ptr(d["l_off"]), _ptr(d["l_ts"]), _ptr(d["l_origin"]), _ptr(d["l_kv"]),
            _ptr(d["r_off"]), _ptr(d["r_ts"]), _ptr(d["r_kv"]),
            _ptr(d["kv_key"]), _ptr(d["kv_val"]), _ptr(d["str_bytes"]), _ptr(d["str_off"]))

    def refmerge_batch(self, packed: dict, maxl: torch.Tensor | None = None,
                       acc: dict | None = None, _delta: dict | None = None, kv: dict | None = None,
                       pull: dict | None = None) -> dict:
        """Run the batched bit-exact reference merge on a packed batch.

        ``packed`` holds device tensors produced by
        :func:`crdt_amd.refmerge.pack_batch`; returns device output tensors.
        ``maxl`` / ``acc``: the ts-range-sharded form (crdt_refmerge_batch_ex;
        see :func:`crdt_amd.shard.sharded_refmerge`).
        ``kv`` = {"off": int64 [n_l + n_r + 1], "key", "val": int32 [cap]}:
        also the new Diff's kv pairs (crdt_refmerge_batch_kv): entry i owns
        key/val[off[i] .. off[i+1]), off[out["off"][-1]] = the total.
        ``pull`` = {"r_end": int64 [replicas], "r_slot_delta": int32
        [replicas] or None}: in-place pulls (crdt_refmerge_batch_pull) --
        replica p's R is r_ts[r_off[p] .. r_end[p]) (may alias L), and
        ``packed["n_r"]`` the total of the R ranges.
        """
        d = packed
        n_l, n_r = d["l_ts"].numel(), int(d.get("n_r", d["r_ts"].numel()))
        n_slots = int(d["n_slots"])
        dev = self.device
        out = {
            "off": torch.empty(d["replicas"] + 1, dtype=torch.int64, device=dev),
            "ts": torch.empty(max(n_l + n_r, 1), dtype=torch.int64, device=dev),
            "origin": torch.empty(max(n_l + n_r, 1), dtype=torch.uint8, device=dev),
            "src": torch.empty(max(n_l + n_r, 1), dtype=torch.int64, device=dev),
            "st_kind": torch.empty(max(n_slots, 1), dtype=torch.uint8, device=dev),
            "st_str": torch.empty(max(n_slots, 1), dtype=torch.int32, device=dev),
            "st_sum": torch.empty(max(n_slots, 1), dtype=torch.int64, device=dev),
        }
        cin = self._refmerge_in(d)
        cout = crdt_refmerge_out(*(out[k].data_ptr() for k in
                                   ("off", "ts", "origin", "src", "st_kind", "st_str", "st_sum")))
        if kv is not None:
            if _delta is not None or maxl is not None or acc is not None:
                raise ValueError("refmerge_batch: kv output only with the plain batch merge")
            self._check(kv["off"], itemsize=8)
            self._check(kv["key"], kv["val"], itemsize=4)
            if kv["off"].numel() < n_l + n_r + 1 or kv["val"].numel() < kv["key"].numel():
                raise ValueError("refmerge_batch: kv output too small")
            ckv = crdt_refmerge_kv_out(kv["off"].data_ptr(), kv["key"].data_ptr(), kv["val"].data_ptr(),
                                       kv["key"].numel())
        if pull is not None:
            if _delta is not None or maxl is not None or acc is not None:
                raise ValueError("refmerge_batch: in-place pulls only with the plain batch merge")
            self._check(pull["r_end"], itemsize=8)
            sd = pull.get("r_slot_delta")
            if sd is not None:
                self._check(sd, itemsize=4)
            cp = crdt_refmerge_pull(pull["r_end"].data_ptr(), sd.data_ptr() if sd is not None else None)
            self._call("crdt_refmerge_batch_pull", C.byref(cin), C.byref(cout), C.byref(cp),
                       C.byref(ckv) if kv is not None else None)
        elif kv is not None:
            self._call("crdt_refmerge_batch_kv", C.byref(cin), C.byref(cout), C.byref(ckv))
        elif _delta is not None:
            cs = self._rstate(_delta)
            self._call("crdt_refmerge_delta", C.byref(cin), C.byref(cout), C.byref(cs))
        elif maxl is None and acc is None:
            self._call("crdt_refmerge_batch", C.byref(cin), C.byref(cout))
        else:
            if maxl is not None:
                self._check(maxl, itemsize=8)
            cacc = self._acc(acc) if acc is not None else None
            self._call("crdt_refmerge_batch_ex", C.byref(cin), C.byref(cout),
                       maxl.data_ptr() if maxl is not None else None, C.byref(cacc) if cacc is not None else None)
        return out

    # -- incremental replay
    def replay_state_new(self, n_slots: int) -> dict:
        n = max(n_slots, 1)
        z = lambda dt: torch.zeros(n, dtype=dt, device=self.device)
        return {"best_key": z(torch.int64), "best_str": z(torch.int32), "sum": z(torch.int64),
                "npar": z(torch.int32), "nhold": z(torch.int32)}

    @staticmethod
    def _rstate(st: dict) -> crdt_replay_state:
        return crdt_replay_state(*(st[k].data_ptr() for k in ("best_key", "best_str", "sum", "npar", "nhold")))

    def replay_state_init(self, packed: dict, st: dict | None = None) -> dict:
        """Replay state of the batch's L logs (crdt_replay_state_init)."""
        st = self.replay_state_new(int(packed["n_slots"])) if st is None else st
        cin, cs = self._refmerge_in(packed), self._rstate(st)
        self._call("crdt_replay_state_init", C.byref(cin), C.byref(cs))
        return st

    def refmerge_delta(self, packed: dict, st: dict) -> dict:
        """crdt_refmerge_batch with the replay folded incrementally into
        ``st`` (the state of ``packed``'s L logs; updated in place)."""
        out = self.refmerge_batch(packed, _delta=st)
        return out

    # -- ts-range-sharded RefMerge steps
    def refmerge_acc_new(self, n_slots: int) -> dict:
        n = max(n_slots, 1)
        return {"best": torch.zeros(n, dtype=torch.int64, device=self.device),
                "sum": torch.zeros(n, dtype=torch.int64, device=self.device),
                "npar": torch.zeros(n, dtype=torch.int32, device=self.device)}

    @staticmethod
    def _acc(acc: dict) -> crdt_refmerge_acc:
        return crdt_refmerge_acc(acc["best"].data_ptr(), acc["sum"].data_ptr(), acc["npar"].data_ptr())

    def refmerge_local_maxl(self, packed: dict) -> torch.Tensor:
        out = torch.empty(max(packed["replicas"], 1), dtype=torch.int64, device=self.device)
        cin = self._refmerge_in(packed)
        self._call("crdt_refmerge_local_maxl", C.byref(cin), out.data_ptr())
        return out

    def refmerge_acc_rank(self, acc: dict, n_slots: int, shard: int) -> torch.Tensor:
        c = torch.empty(max(n_slots, 1), dtype=torch.int64, device=self.device)
        ca = self._acc(acc)
        self._call("crdt_refmerge_acc_rank", C.byref(ca), n_slots, shard, c.data_ptr())
        return c

    def refmerge_acc_owner_str(self, acc: dict, n_slots: int, c: torch.Tensor, cmax: torch.Tensor) -> torch.Tensor:
        v = torch.empty(max(n_slots, 1), dtype=torch.int64, device=self.device)
        ca = self._acc(acc)
        self._call("crdt_refmerge_acc_owner_str", C.byref(ca), n_slots, c.data_ptr(), cmax.data_ptr(), v.data_ptr())
        return v

    def refmerge_acc_set_best(self, acc: dict, n_slots: int, cmax: torch.Tensor, v: torch.Tensor) -> None:
        ca = self._acc(acc)
        self._call("crdt_refmerge_acc_set_best", C.byref(ca), n_slots, cmax.data_ptr(), v.data_ptr())

    def refmerge_finalize(self, packed: dict, acc: dict, out: dict) -> dict:
        ca = self._acc(acc)
        cout = crdt_refmerge_out(*(out[k].data_ptr() for k in
                                   ("off", "ts", "origin", "src", "st_kind", "st_str", "st_sum")))
        self._call("crdt_refmerge_finalize", C.byref(ca), int(packed["n_slots"]), _ptr(packed["str_bytes"]),
                   _ptr(packed["str_off"]), packed["str_off"].numel() - 1, C.byref(cout))
        return out

    # -- batched local apply
    def local_apply(self, diff: dict, cmds: dict, state: dict, str_bytes: torch.Tensor,
                    str_off: torch.Tensor, n_slots: int) -> dict:
        """AddCommand (main.go:173-215) for every replica at once
        (crdt_local_apply).  diff = {off, ts, origin} (device), cmds = {off,
        ts, kv_off, kv_key, kv_val} (device; arrival order per replica),
        state = {st_kind, st_str, st_sum} updated in place.  Returns the new
        Diff {off, ts, origin, src} (src < 0: command -(src+1)) and the
        per-command HTTP status."""
        dev = self.device
        n_l, n_c = diff["ts"].numel(), cmds["ts"].numel()
        P = diff["off"].numel() - 1
        out = {"off": torch.empty(P + 1, dtype=torch.int64, device=dev),
               "ts": torch.empty(max(n_l + n_c, 1), dtype=torch.int64, device=dev),
               "origin": torch.empty(max(n_l + n_c, 1), dtype=torch.uint8, device=dev),
               "src": torch.empty(max(n_l + n_c, 1), dtype=torch.int64, device=dev),
               "status": torch.empty(max(n_c, 1), dtype=torch.int16, device=dev)}
        cin = crdt_local_in(P, n_slots, n_l, n_c, cmds["kv_key"].numel(), str_off.numel() - 1,
                            _ptr(diff["off"]), _ptr(diff["ts"]), _ptr(diff["origin"]),
                            _ptr(cmds["off"]), _ptr(cmds["ts"]), _ptr(cmds["kv_off"]),
                            _ptr(cmds["kv_key"]), _ptr(cmds["kv_val"]), _ptr(str_bytes), _ptr(str_off))
        cout = crdt_local_out(*(out[k].data_ptr() for k in ("off", "ts", "origin", "src", "status")),
                              *(state[k].data_ptr() for k in ("st_kind", "st_str", "st_sum")))
        self._call("crdt_local_apply", C.byref(cin), C.byref(cout))
        return out

    def atoi_batch(self, str_bytes: torch.Tensor, str_off: torch.Tensor):
        n = str_off.numel() - 1
        ok = torch.empty(max(n, 1), dtype=torch.uint8, device=self.device)
        val = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        self._call("crdt_atoi_batch", str_bytes.data_ptr(), str_off.data_ptr(), n, ok.data_ptr(), val.data_ptr())
        return ok[:n], val[:n]

    # ------------------------------------------------------------ sharding helpers (a9)
    def u64_to_ordered_i64(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        out = torch.empty_like(x) if out is None else out
        self._call("crdt_u64_to_ordered_i64", x.data_ptr(), out.data_ptr(), x.numel())
        return out

    def ordered_i64_to_u64(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        out = torch.empty_like(x) if out is None else out
        self._call("crdt_ordered_i64_to_u64", x.data_ptr(), out.data_ptr(), x.numel())
        return out

    # ------------------------------------------------------------ synthetic state
    def synth_counters(self, seed: int, stream: int, rows: int, nodes: int, row_base: int = 0,
                       out: torch.Tensor | None = None) -> torch.Tensor:
        out = torch.empty(rows, nodes, dtype=torch.int64, device=self.device) if out is None else out
        self._call("crdt_synth_counters", seed, stream, out.data_ptr(), rows * nodes, row_base * nodes)
        return out

    def synth_vclock_pairs(self, seed: int, pairs: int, nodes: int, pair_base: int = 0):
        a = torch.empty(pairs, nodes, dtype=torch.int64, device=self.device)
        b = torch.empty(pairs, nodes, dtype=torch.int64, device=self.device)
        self._call("crdt_synth_vclock_pairs", seed, a.data_ptr(), b.data_ptr(), pairs, nodes, pair_base)
        return a, b

    def synth_set_tuples(self, seed: int, side: int, n: int, key_space: int, sort: bool = True) -> TupleSet:
        t = TupleSet.empty(n, self.device)
        ct = t.c()
        self._call("crdt_synth_set_tuples", seed, side, C.byref(ct), n, key_space)
        if sort:                                          # D1 inputs: the device tuple sort
            t = self.sort_tuples(t)
        return t
