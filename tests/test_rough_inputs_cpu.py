"""The rough inputs of rough_inputs.py, judged on the CPU before the GPU tests rely on them: on the inputs and on the
oracle's result only, never on a handle's.

Rough: every roughened array differs from its copy shifted by one cell in x, one cell in y, one layer and one level at 80 %
or more of the places.  Straddling: with ocrp = 1, at least 10 % of the wet cell-layers lie below 2 hsal and at least 10 %
above, in every layer.  Bounded: after step plan A (steps 1-5) and B (steps 7-12) the oracle's fields are finite, wet
thicknesses positive and max |u|, |v| <= 20 U, so that no blow-up swamps the small terms.  Liveness: re-seeding one input
alone changes the oracle's state after plan B, unless the configuration's parameters switch that term off
(rough_inputs.switched_off says which, and the test holds it to that list in both directions)."""
import numpy as np
import pytest

import oracle_lib
import rough_inputs as RI
import tracers_ref as T
from helpers import same, same_bits

PLANS = {"A": (1, 5), "B": (7, 6)}
MUST_BE_LIVE = ("h_to", "taus:0", "taus:1", "bodf", "rs_h:0", "rs_h:1", "dmdx:0", "dmdx:1", "dmdx:2", "dmdy:0", "dmdy:1", "dmdy:2",
                "v_cc", "v_ll", "tt3d", "tb3d", "tu3d", "hdot", "tide", "nudg", "fnud", "fcor", "h_th", "hlay", "u", "v", "h_u", "h_v")
_DEAD = {}


def _oracle_after(g, plan):
    o = oracle_lib.Oracle(g)
    o.step(*PLANS[plan])
    return o.state()


@pytest.mark.parametrize("frame", ["130x18", "321x50"])
@pytest.mark.parametrize("config", list(RI.CONFIGS))
def test_rough_straddling_bounded(config, frame):
    f = RI.base_fields(config, frame)
    before = {k: np.array(getattr(f, k), copy=True) for k in RI.AXES}
    g = RI.rough_fields(f, 1)
    for k in RI.AXES:
        assert same_bits(getattr(f, k), before[k]), (k, "the shared object was written")
    for k in g.rough_support:
        for shift, frac in RI.shifted_fractions(g, k).items():
            assert frac >= 0.8, (config, frame, k, shift, frac)
    for k in ("hlay", "u", "v", "h_u", "h_v", "rs_h", "dmdx", "dmdy", "fcor", "h_to", "h_th"):
        fr = RI.shifted_fractions(g, k)
        assert "x" in fr and "y" in fr, (config, k, fr)
        assert ("layer" in fr) == (RI.AXES[k][1] is not None and f.p.nlay > 1) and ("level" in fr) == (RI.AXES[k][2] is not None), (config, k, fr)
    assert len(set(g.bodf.ravel())) == g.bodf.size and np.all(g.bodf != 0.0)
    wet = g.mk_n > 0.5
    assert np.all(g.h_to[wet] != 0.0)
    open_u = np.broadcast_to((g.mk_u > 0.5)[None], g.u.shape)
    zero = g.u[open_u] == 0.0
    neg = zero & np.signbit(g.u[open_u])
    assert 0.03 <= neg.mean() <= 0.07 and 0.03 <= (zero & ~neg).mean() <= 0.07, (neg.mean(), zero.mean())
    assert np.array_equal(g.nudg == 0.0, f.nudg == 0.0)                  # exact 0 outside the sponge: the ng == 0 shortcuts
    if float(f.p.ocrp) > 0.5:
        for k, (below, above) in enumerate(RI.straddling(g)):
            assert below >= 0.10 and above >= 0.10, (config, frame, k, below, above)
    for plan in PLANS:
        growth = RI.bounded(g, _oracle_after(g, plan))
        print("%s %s plan %s: growth %.2f" % (config, frame, plan, growth))


@pytest.mark.parametrize("config", list(RI.CONFIGS))
def test_liveness(config):
    f = RI.base_fields(config, "130x18")
    ref = {k: v.copy() for k, v in _oracle_after(RI.rough_fields(f, 1), "B").items()}
    dead = set()
    for x in RI.INPUTS:
        st = _oracle_after(RI.rough_fields(f, 1, reseed=(x,)), "B")
        if all(same_bits(st[k], ref[k]) for k in ("hlay", "u", "v", "h_u", "h_v")):
            dead.add(x)
    _DEAD[config] = dead
    assert dead == RI.switched_off(f.p, f), (config, sorted(dead), sorted(RI.switched_off(f.p, f)))


def test_every_term_is_live_somewhere():
    for config in RI.CONFIGS:
        if config not in _DEAD:
            test_liveness(config)
    for x in MUST_BE_LIVE:
        assert any(x not in _DEAD[c] for c in RI.CONFIGS), (x, "dead in every configuration")


def test_reseeding_changes_one_input_alone():
    f = RI.base_fields("closed_dt3d_forced_3l", "130x18")
    a, b = RI.rough_fields(f, 1), RI.rough_fields(f, 1, reseed=("dmdx:1",))
    for k in RI.AXES:
        if k != "dmdx":
            assert same_bits(getattr(a, k), getattr(b, k)), k
    assert same_bits(a.dmdx[:, :, 0], b.dmdx[:, :, 0]) and same_bits(a.dmdx[:, :, 2], b.dmdx[:, :, 2])
    assert not same(a.dmdx[:, :, 1], b.dmdx[:, :, 1])
    assert same_bits(a.bodf, b.bodf)


@pytest.mark.parametrize("frame", ["130x18", "4200x9"])
def test_tracer_of_concentration_one_is_the_thickness_with_dry_cells(frame):
    """Empty cells away from coasts, with transports beside them: tracers_ref.update on a tracer of concentration 1 and
    relaxation concentration 1 equals the oracle's update_h, three sweeps in a row (the no-gradient rule at an empty upwind
    cell takes the other side's concentration: 1)."""
    config = "closed_leith_3l" if frame == "130x18" else "zero_visc_2l"
    f = RI.base_fields(config, frame)
    g = RI.dry_cell_state(f, 3)
    wet = g.mk_n > 0.5
    share = g.dry[:, wet].mean()
    assert 0.08 <= share <= 0.12 and np.all(g.hlay[g.dry] == 0.0) and not np.signbit(g.hlay[g.dry]).any(), share
    W, S = g.neig[:, 4], g.neig[:, 6]
    interior = g.dry & (g.mk_u > 0.5)[None] & (g.mk_v > 0.5)[None] & (g.mk_u[g.neig[:, 0]] > 0.5)[None] & (g.mk_v[g.neig[:, 2]] > 0.5)[None]
    assert interior.sum() > 0.05 * wet.sum() * f.p.nlay                 # away from coasts
    assert np.all(g.h_u[interior] != 0.0) and np.all(g.h_v[interior] != 0.0)
    assert not (g.dry & g.dry[:, W]).any() and not (g.dry & g.dry[:, S]).any()
    o = oracle_lib.Oracle(g)
    q = np.array(g.hlay, copy=True)[None]
    rq = np.array(g.rs_h, copy=True)[None]
    ctrg = np.ones_like(q)
    for tstp in (7, 8, 9):
        gene, ramp, ctim = T.step_scalars(f.p, tstp)
        h = o.a["hlay"].copy()
        q, rq = T.update(g, h, g.h_u, g.h_v, q, rq, ctrg, gene, ramp, ctim)
        o.update_h(gene, ramp, ctim)
        assert np.isfinite(q).all()
        assert same(q[0], o.a["hlay"]), (frame, tstp, float(np.max(np.abs(q[0] - o.a["hlay"]))))
        assert same(rq[0], o.a["rs_h"]), (frame, tstp)
    assert not same(o.a["hlay"], g.hlay)
