"""GPU: the counter map's selection (crdt_cmap_select, the one range-digest
call that carves the workspace) and the whole reconciliation round do not
depend on what the scratch held before the call -- tests/test_gpu_ws_fill.py's
mechanism through tests/test_gpu_cmap_ws_fill.py's fixtures.

1. Under the diagnostic build's ``ctx.ws_fill`` at 0x00, 0xFF and 0xA5 (and
   once with the fill off): ``Filling`` reserves 64 MiB in front of EVERY
   engine call, which sets the whole workspace.  Select, digest and the round
   run at three full tiles plus 17 cells, with the full length and with a
   device count below the buffer.
2. One shrink-and-swap sequence on one engine with no reserve in between (any
   build): five tiles, two and 9 cells, none, one cell, an OR-Set merge whose
   carve lays other arrays over the selection's, then five tiles again.

Every result is compared bit for bit with tests/cmap_digest_util.py and
tests/cmap_util.py and the device status stays 0."""
import numpy as np
import pytest

import cmap_digest_util as du
import cmap_util as cu
import test_gpu_cmap as t_cmap
import test_gpu_cmap_digest as t_dig
import test_gpu_cmap_ws_fill as cwf
import test_gpu_ws_fill as wf

pytestmark = pytest.mark.gpu

T = t_cmap.T
N = 3 * T + 17                 # cells under the fill
N_DEV = 2 * T + 5              # a device count below the buffer: the last tile is never written

_fill_off_after_the_module = cwf._fill_off_after_the_module
filling = cwf.filling


def fam_cmap_digest(e, n, seed, n_dev=None):
    """Digest, the selections and the round at n cells a side."""
    a, b = du.drifted_pair(n, raised=min(5, n // 2), dropped=min(3, n // 4), seed=seed)
    for m in (0, 63):
        sp = du.quantile_splitters(a, m)
        t = a if n_dev is None else t_cmap._poisoned(a, n_dev)
        t_dig.check_digest(e, t, sp, n=n_dev, what=f"digest n={n} m={m}")
        for flags in ((np.ones(m + 1, np.uint8), t_dig._alternating(m)) if m else ([1], [0])):
            t_dig.check_select(e, t, sp, flags, n=n_dev, what=f"select n={n} m={m}")
    t_dig._round(e, a, b, m=63)
    t_dig._round(e, a, a, m=63)


@pytest.mark.diag
@pytest.mark.parametrize("fill", wf.FILLS, ids=lambda f: "off" if f < 0 else f"0x{f:02X}")   # (0x00 first)
def test_cmap_digest_under_fill(filling, fill):
    fam_cmap_digest(filling, N, 81)
    fam_cmap_digest(filling, N, 82, n_dev=N_DEV)
    fam_cmap_digest(filling, 1, 83)
    assert filling.fills > 0
    assert filling.device_status() == 0


def test_cmap_digest_shrink_and_swap(eng):
    """One engine, no reserve in between: what each call finds in its carve is
    what the call before it left there."""
    fam_cmap_digest(eng, 5 * T, 91)
    fam_cmap_digest(eng, 2 * T + 9, 92)
    fam_cmap_digest(eng, 0, 93)
    fam_cmap_digest(eng, 1, 94)
    wf.fam_merge(eng, 2 * T + 9, seed=95)
    fam_cmap_digest(eng, 5 * T, 96)
    assert eng.device_status() == 0
