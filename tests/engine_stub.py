"""A stub Engine for tests of the Python wrapper layer (crdt_amd/engine.py):
no GPU and no library.  The engine lives on the CPU device and its ``_call``
is a recorder, so a test sees which C function a wrapper would call, with
which pointers and lengths, and what it hands back -- no kernel runs."""
import ctypes as C

import torch

from crdt_amd import _lib
from crdt_amd.engine import Engine, TupleSet

STATUS = "crdt_ctx_device_status"
# the C calls whose last argument is the int64[1] count they write
COUNTED = {
    "crdt_lww_merge", "crdt_orset_merge", "crdt_lww_merge_unsorted", "crdt_orset_merge_unsorted",
    "crdt_lww_merge_src", "crdt_orset_merge_src", "crdt_set_elements", "crdt_set_delta", "crdt_set_compact",
    "crdt_map_read", "crdt_orset_merge_causal", "crdt_orset_merge_causal_ranges", "crdt_set_apply",
    "crdt_set_select", "crdt_set_digest_diff", "crdt_tuples_count_unsorted",
}


class Recorder:
    """Engine._call's stand-in: keeps (fn, args), writes ``k`` through a
    count pointer (host memory here) and ``status`` into the flag word of a
    device-status read."""

    def __init__(self, k: int = 0, status: int = 0):
        self.k, self.status, self.calls = k, status, []

    def __call__(self, fn, *args):
        self.calls.append((fn, args))
        if fn == STATUS:
            args[0]._obj.value = self.status
        elif fn in COUNTED:
            C.c_int64.from_address(args[-1]).value = self.k

    def status_reads(self):
        return [c for c in self.calls if c[0] == STATUS]

    def c_calls(self):
        """The recorded calls but the status reads, by-reference arguments resolved (see :func:`arg`)."""
        return [(fn, tuple(arg(a) for a in args)) for fn, args in self.calls if fn != STATUS]


def arg(a):
    """A recorded argument in comparable form: a by-reference crdt_tuples
    as :func:`T` gives it, another by-reference struct as the object itself."""
    if type(a).__name__ == "CArgObject":
        a = a._obj
        if isinstance(a, _lib.crdt_tuples):
            return ("tuples", a.key, a.ts, a.rep, a.tomb)
    return a


def T(s: TupleSet):
    """What :func:`arg` makes of a by-reference crdt_tuples naming ``s``.
    ctypes reads a null c_void_p field back as None."""
    return ("tuples",) + tuple(p or None for p in (s.key.data_ptr(), s.ts.data_ptr(), s.rep.data_ptr(),
                                                   s.tomb.data_ptr()))


def P(t):
    return None if t is None else t.data_ptr()


def stub(k: int = 0, status: int = 0):
    """(engine, recorder): an Engine on the CPU device whose C calls are recorded."""
    e = Engine.__new__(Engine)
    e.device, e._dependents, e.ctx = torch.device("cpu"), [], None
    e._call = rec = Recorder(k, status)
    return e, rec


def tuples(n: int, base: int = 0) -> TupleSet:
    return TupleSet(torch.arange(base, base + n, dtype=torch.int64), torch.arange(n, dtype=torch.int64) + 7,
                    torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.uint8))


def i64(n: int) -> torch.Tensor:
    return torch.zeros(n, dtype=torch.int64)


def u8(n: int) -> torch.Tensor:
    return torch.zeros(n, dtype=torch.uint8)


def i32(n: int) -> torch.Tensor:
    return torch.zeros(n, dtype=torch.int32)


def cap(t: torch.Tensor) -> int:
    """Elements in the allocation behind ``t`` (a slice keeps its buffer's)."""
    return t.untyped_storage().nbytes() // t.element_size()


def tuples_cap(s: TupleSet):
    return cap(s.key), cap(s.ts), cap(s.rep), cap(s.tomb)


def is_tuples(s: TupleSet, n: int):
    """s is a TupleSet of the four field dtypes and n tuples."""
    return (isinstance(s, TupleSet) and (s.key.dtype, s.ts.dtype, s.rep.dtype, s.tomb.dtype)
            == (torch.int64, torch.int64, torch.int32, torch.uint8)
            and (s.key.numel(), s.ts.numel(), s.rep.numel(), s.tomb.numel()) == (n,) * 4)


def same(x, y) -> bool:
    """x names the storage of y from its start (a tensor or a TupleSet; a leading slice counts)."""
    if isinstance(y, TupleSet):
        return all(same(p, q) for p, q in ((x.key, y.key), (x.ts, y.ts), (x.rep, y.rep), (x.tomb, y.tomb)))
    return x.dtype == y.dtype and base(x) == base(y) and x.storage_offset() == y.storage_offset() == 0


def base(t: torch.Tensor) -> int:
    """The address of t's allocation: what data_ptr() gives for a view from its
    start, also where the view is empty (data_ptr() is 0 then)."""
    return t.untyped_storage().data_ptr()


def Tb(s: TupleSet):
    """:func:`T` by the fields' allocations: also right for an empty leading slice."""
    return ("tuples",) + tuple(base(t) or None for t in (s.key, s.ts, s.rep, s.tomb))
