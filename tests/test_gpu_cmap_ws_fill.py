"""GPU: no kernel of the keyed PN-Counter map (crdt_cmap_*) depends on what its
scratch held before the call -- the counter map's share of
tests/test_gpu_ws_fill.py, with that module's mechanism.

1. Under the diagnostic build's ``ctx.ws_fill`` at 0x00, 0xFF and 0xA5 (and
   once with the fill off): ``Filling`` reserves 64 MiB in front of EVERY
   engine call, which sets the whole workspace, and holds ``ctx.ws_filled_mb``
   to have advanced.  The five ops run at three full tiles plus 17 cells a
   side, with device counts below the buffers and with the full lengths.
2. One shrink-and-swap sequence on one engine with no reserve in between (any
   build): five tiles, two and a partial, none, one cell, an OR-Set merge whose
   carve lays other arrays over the counter map's, then the first shape again.

Every result is compared bit for bit with tests/cmap_util.py and the device
status stays 0."""
import numpy as np
import pytest

import cmap_util as cu
import test_gpu_cmap as t_cmap
import test_gpu_ws_fill as wf
from crdt_amd import _lib
from knobs import set_knob

pytestmark = pytest.mark.gpu

T = t_cmap.T
N = 3 * T + 17                 # cells a side under the fill
N_DEV = (4101, 4001)           # device counts below the buffers


@pytest.fixture(scope="module", autouse=True)
def _fill_off_after_the_module():
    yield
    if _lib.is_diag():
        _lib.set_option(b"ctx.ws_fill", -1)


@pytest.fixture
def filling(eng, fill):
    set_knob(b"ctx.ws_fill", fill)       # the product build: -1 is a plain parity run, the others skip
    try:
        yield wf.Filling(eng, fill)
    finally:
        if _lib.is_diag():
            _lib.set_option(b"ctx.ws_fill", -1)


def _sides(na, nb, seed):
    rng = np.random.default_rng(seed)
    ks = max(1, (na + nb) // 4)                          # 8 replicas a key: about half of each side is shared
    return cu.random_state(rng, na, ks), cu.random_state(rng, nb, ks)


def fam_cmap(e, a, b, na=None, nb=None):
    """The five ops on (a, b); with na / nb as device counts below the buffers."""
    ea = a if na is None else t_cmap._cut(a, na)
    t_cmap.check_merge(e, a, b, na=na, nb=nb)
    t_cmap.check_delta(e, a, b, ns=na, nd=nb)
    t_cmap.check_delta(e, b, a, ns=nb, nd=na)
    t_cmap.check_values(e, a, n=na)
    probes = np.concatenate([ea[0][::7], ea[0][::7] + np.uint64(1)]) if len(ea[0]) else []
    t_cmap.check_lookup(e, a, probes, n=na)
    keys = np.unique(b[0])
    t_cmap.check_apply(e, a, 3, keys, keys * np.uint64(3) + np.uint64(1), keys % np.uint64(5), n=na)


@pytest.mark.diag
@pytest.mark.parametrize("fill", wf.FILLS, ids=lambda f: "off" if f < 0 else f"0x{f:02X}")   # (0x00 first)
def test_cmap_under_fill(filling, fill):
    a, b = _sides(N, N, 62)                              # (a seed under which both assertions below hold)
    t_cmap._assert_not_vacuous(a, b)
    t_cmap._assert_not_vacuous(t_cmap._cut(a, N_DEV[0]), t_cmap._cut(b, N_DEV[1]))
    fam_cmap(filling, a, b)
    fam_cmap(filling, t_cmap._poisoned(a, N_DEV[0]), t_cmap._poisoned(b, N_DEV[1]), *N_DEV)
    fam_cmap(filling, *_sides(1, 0, 63))
    assert filling.fills > 0
    assert filling.device_status() == 0


def test_cmap_shrink_and_swap(eng):
    """One engine, no reserve in between: what each call finds in its carve is
    what the call before it left there."""
    def at(size, seed):
        fam_cmap(eng, *_sides(size - size // 3, size // 3, seed))

    at(5 * T, 51)
    at(2 * T + 9, 52)
    at(0, 53)
    at(1, 54)
    wf.fam_merge(eng, 2 * T + 9, seed=55)
    at(5 * T, 56)
    assert eng.device_status() == 0
