"""The identity the history-from-Montgomery form of the fused u+v sweep rests on, on the CPU.

update_u / update_v store one new level of the Montgomery-gradient history per step, dmd4 = (mont(b) - mont) * (1/dl) * grav *
mask with b = W, mask = mk_u for u and b = S, mask = mk_v for v (private_mod.f95:1422-1591).  A stored level is therefore a
function of that step's Montgomery potential alone, and the engine may keep three levels of `mont` instead of reading six
history arrays and writing two.  Here the oracle is stepped one step at a time over every golden fixture without a lid
(periodic seams, land, open boundaries, outcropping, restarts, private_mod3d, 2-16 layers), the potential of every step is
kept, and after every step all three levels of dmdx and dmdy at the cells 1..ndeg are compared with the expression formed
left to right from the kept potentials: bit for bit, the sign of zero included."""
import numpy as np
import pytest

import oracle_lib
from helpers import Golden, golden_names, same_bits

NSTEPS = 12
NAMES = [n for n in golden_names() if float(Golden(n).p.rgld) < 0.5]


def test_fixtures_without_a_lid_present():
    assert len(NAMES) >= 10


def _from_mont(mont, nb, i_dl, grav, mask):
    """(mont(b) - mont) * i_dl * grav * mask at the cells 1..ndeg of every layer, the products formed left to right."""
    return (mont[:, nb[1:]] - mont[:, 1:]) * i_dl * grav * mask[None, 1:]


@pytest.mark.parametrize("name", NAMES)
def test_stored_history_is_a_function_of_the_kept_montgomery_levels(name):
    g = Golden(name)
    f = g.fields()
    f.invf = float(g.static("invf"))
    o = oracle_lib.Oracle(f, variant=g.variant)
    i_dl, grav = 1.0 / float(g.p.dl), float(g.p.grav)
    west, south = np.asarray(f.neig)[:, 4], np.asarray(f.neig)[:, 6]
    mk_u, mk_v = np.asarray(f.mk_u, dtype=np.float64), np.asarray(f.mk_v, dtype=np.float64)
    kept = {}                                          # step -> mont(nlay, 0:ndeg) of that step
    compared = 0
    for t in range(1, NSTEPS + 1):
        o.step(t, 1)
        kept[t] = np.array(o.scratch()["mont"], copy=True)
        assert not kept[t][:, 0].any() and not np.signbit(kept[t][:, 0]).any(), (name, t, "mont(0) is +0")
        st = o.state()
        for lev in range(3):                           # level 3 of the reference = this step's, level 1 = two steps back
            src = t - (2 - lev)
            if src < 1:
                continue                               # (a level older than the first step: the start state's)
            for key, nb, mask in (("dmdx", west, mk_u), ("dmdy", south, mk_v)):
                want = _from_mont(kept[src], nb, i_dl, grav, mask)
                assert same_bits(st[key][:, 1:, lev], want), (name, t, key, lev)
                compared += want.size
    assert compared == 6 * (NSTEPS - 1) * g.p.nlay * g.p.ndeg
