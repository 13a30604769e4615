"""GPU: combine, add, from_ops and ingest of the counter map do not depend on
what the scratch held before the call -- tests/test_gpu_ws_fill.py's mechanism
through tests/test_gpu_cmap_digest_ws_fill.py's fixtures.  crdt_cmap_from_ops
is the call this is for: it keeps the view's and the sorted columns in the
workspace across the device sort, which reserves and carves the same arena.

1. Under the diagnostic build's ``ctx.ws_fill`` at 0x00, 0xFF and 0xA5 (and
   once with the fill off): ``Filling`` reserves 64 MiB in front of EVERY
   engine call, which sets the whole workspace.  The four calls run at three
   full tiles plus 17 cells, with the full length and with a device count
   below the buffer.
2. One shrink-and-swap sequence on one engine with no reserve in between (any
   build): five tiles, two and 9 cells, none, one cell, an OR-Set merge whose
   carve lays other arrays over the columns, then five tiles again.
3. from_ops and ingest on a fresh engine at growing sizes (any build): the
   arena has to grow, and so move, inside the call.

Every result is compared bit for bit with tests/cmap_ingest_util.py and the
device status stays 0."""
import numpy as np
import pytest

import cmap_ingest_util as iu
import cmap_util as cu
import test_gpu_cmap as t_cmap
import test_gpu_cmap_digest_ws_fill as dwf
import test_gpu_cmap_ingest as t_ing
import test_gpu_ws_fill as wf

pytestmark = pytest.mark.gpu

T = t_cmap.T
N = 3 * T + 17                 # cells / operations under the fill
N_DEV = 2 * T + 5              # a device count below the buffer: the last tile is never read
U64 = np.uint64

_fill_off_after_the_module = dwf._fill_off_after_the_module
filling = dwf.filling


def fam_cmap_ingest(e, n, seed, n_dev=None):
    """The four calls at n operations; n_dev: the state's / the sorted log's device length."""
    rng = np.random.default_rng(seed)
    ops = iu.random_log(rng, n, max(1, n // 12), reps=4, big=True)
    srt = iu.sorted_log(ops)
    t = cu.random_state(rng, min(n, 4 * max(1, n // 12)), max(1, n // 12), reps=4)
    t = (t[0] * U64(7) + U64(3), t[1], t[2], t[3])       # the log's key space
    st = iu.from_ops_np(ops)
    nd = None if n_dev is None else min(n_dev, len(t[0]))
    t_ing.check_combine(e, srt if n_dev is None else t_cmap._poisoned(srt, n_dev), n=n_dev, what=f"combine n={n}")
    order = np.lexsort((ops[1], ops[0])).astype(np.uint32)
    t_ing.check_combine(e, srt if n_dev is None else t_cmap._poisoned(srt, n_dev), n=n_dev, idx=order,
                        src=(ops[2], ops[3]), what=f"combine idx n={n}")
    t_ing.check_add(e, t if nd is None else t_cmap._poisoned(t, nd), st, nt=nd, what=f"add n={n}")
    t_ing.check_from_ops(e, ops, what=f"from_ops n={n}")
    Tt = t_cmap._up(e, t if nd is None else t_cmap._poisoned(t, nd))
    out, cnt = e.cmap_ingest(Tt, *t_ing._ops(e, ops), n_t_dev=None if nd is None else t_cmap._dev(e, nd))
    t_cmap._eq(t_cmap._take(out, cnt), iu.add_np(t if nd is None else t_cmap._cut(t, nd), st), f"ingest n={n}")


@pytest.mark.diag
@pytest.mark.parametrize("fill", wf.FILLS, ids=lambda f: "off" if f < 0 else f"0x{f:02X}")   # (0x00 first)
def test_cmap_ingest_under_fill(filling, fill):
    fam_cmap_ingest(filling, N, 81)
    fam_cmap_ingest(filling, N, 82, n_dev=N_DEV)
    fam_cmap_ingest(filling, 1, 83)
    assert filling.fills > 0
    assert filling.device_status() == 0


def test_cmap_ingest_shrink_and_swap(eng):
    """One engine, no reserve in between: what each call finds in its carve is
    what the call before it left there."""
    fam_cmap_ingest(eng, 5 * T, 91)
    fam_cmap_ingest(eng, 2 * T + 9, 92)
    fam_cmap_ingest(eng, 0, 93)
    fam_cmap_ingest(eng, 1, 94)
    wf.fam_merge(eng, 2 * T + 9, seed=95)
    fam_cmap_ingest(eng, 5 * T, 96)
    assert eng.device_status() == 0


def test_from_ops_grows_the_workspace_inside_the_call():
    """A fresh engine, so that the arena is as small as the calls before left it:
    each from_ops below needs more than the one before and has to grow (and so
    move) the workspace itself -- once, up front, before it carves the columns
    that must outlive the sort's own reserve and carve."""
    from crdt_amd.engine import Engine
    e = Engine(0)
    try:
        rng = np.random.default_rng(97)
        for m in (100, 300_000, 5, 700_000):
            ops = iu.random_log(rng, m, max(1, m // 20), reps=4, big=True)
            exp = iu.from_ops_np(ops)
            out, cnt = e.cmap_from_ops(*t_ing._ops(e, ops))
            t_cmap._eq(t_cmap._take(out, cnt), exp, f"from_ops m={m} on a growing arena")
            t = t_cmap._cut(exp, len(exp[0]) // 2)
            out, cnt = e.cmap_ingest(t_cmap._up(e, t), *t_ing._ops(e, ops))
            t_cmap._eq(t_cmap._take(out, cnt), iu.add_np(t, exp), f"ingest m={m} on a growing arena")
        assert e.device_status() == 0
    finally:
        e.close()
