"""The flux-limited tracer scheme on the device (beom_set_tracer_scheme, scheme 2) against its numpy restatement
(tracers_limited_ref, pinned to the reference by test_tracers_limited_cpu) fed with the thicknesses and transports downloaded
from the same handle, step by step, on an input that reaches every outcome of the limiter (wavy; its mix is asserted by the CPU
test); the same bits from every handle kind (dense or embedded, table path, 2 and 3 bands); the default, switching between the
schemes, continuation; the per-sweep entry; and a handle without tracers, which the choice of scheme must leave alone.
Comparisons are helpers.same (every value equal, +-0 alike, all finite) unless stated; the one fixture with a tidal constituent
is held to the project's 1e-12 relative for its cos term.

These are smooth flows from rest with two tracers: no cell-layer inside an interior tile is dry, so the staged body's wet mask
is 0x1FF throughout.  Rough states with dry cells inside interior tiles, 1, 3 and 8 tracers, 12 layers, hdot and a band's
edge tiles meet scheme 2 in test_gpu_tracers_limited_rough (inputs held to that by test_tracers_limited_rough_cpu)."""
import os

import numpy as np
import pytest

import tracers_limited_ref as TL
import tracers_ref as T
from beom_amd import capi, inputs as I
from helpers import STATE, Golden, maxrel, same, same_bits, tile_geometry
from test_gpu_biharm_tiled import CASES
from test_gpu_parity import COS_TOL, _fields, _live
from test_gpu_tracers import GOLDENS, MODES, NSTEPS, _big_case, _finite_same, _refused, _run, _tracers

pytestmark = pytest.mark.gpu
assert NSTEPS == 12 and len(GOLDENS) == 10 and sorted(MODES) == ["dense_64x4", "dense_64x8", "table"]


@pytest.fixture(autouse=True)
def _no_geometry_leak():
    before = os.environ.get("BEOM_TILE4")
    yield
    assert os.environ.get("BEOM_TILE4") == before


def _wavy_tracers(f):
    """Two tracers: concentration 1 everywhere with relaxation concentration 1, and the wavy one with the relaxation
    concentration of test_gpu_tracers that varies from cell to cell and layer to layer."""
    q, rq, ctrg = _tracers(f)
    q[1] = TL.wavy(f) * np.asarray(f.hlay, dtype=np.float64)
    return np.ascontiguousarray(q), rq, ctrg


def _engine(f, dense_hint=1, scheme=2, tracers=True):
    e = capi.Engine(f, dense_hint=dense_hint)
    if scheme is not None:
        e.set_tracer_scheme(scheme)
    if tracers:
        q, rq, ctrg = _wavy_tracers(f)
        e.set_tracers(2)
        e.upload_tracers(q=q, rq=rq, ctrg=ctrg)
    return e


def _follow(e, f, q, rq, ctrg, steps, scheme, exact, what, also=None):
    """The handle's steps one by one against the restatement fed with the handle's own hlay, h_u, h_v.  also = [q, rq]: the
    restatement of scheme 1 carried along on the same inputs.  Returns (q, rq) of the restatement after the last step."""
    tres = float(getattr(f, "tres", 0.0))
    for t in steps:
        if t <= 3:
            e.rebuild_fluxes()              # what the step is about to do itself: the same values
        st = e.download(("hlay", "h_u", "h_v"))
        gene, ramp, ctim = T.step_scalars(f.p, t, tres)
        q, rq = TL.update(f, st["hlay"], st["h_u"], st["h_v"], q, rq, ctrg, gene, ramp, ctim, scheme=scheme)
        if also is not None:
            also[0], also[1] = T.update(f, st["hlay"], st["h_u"], st["h_v"], also[0], also[1], ctrg, gene, ramp, ctim)
        e.step(t, 1)
        got = e.download_tracers()
        if exact:
            assert _finite_same(got["q"], q), (what, t, "q", maxrel(got["q"], q))
            assert _finite_same(got["rq"], rq), (what, t, "rq", maxrel(got["rq"], rq))
            h = e.download(("hlay",))["hlay"]
            assert _finite_same(got["q"][0][:, 1:], h[:, 1:]), (what, t, "q of the uniform tracer vs hlay")
        else:
            assert np.isfinite(got["q"]).all() and np.isfinite(got["rq"]).all()
            print("%s step %d: maxrel q %.3g rq %.3g" % (what, t, maxrel(got["q"], q), maxrel(got["rq"], rq)))
            assert maxrel(got["q"], q) <= COS_TOL, (what, t, "q", maxrel(got["q"], q))
            assert maxrel(got["rq"], rq) <= COS_TOL, (what, t, "rq", maxrel(got["rq"], rq))
            q, rq = got["q"], got["rq"]     # (the next step is judged on its own)
    return q, rq


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", GOLDENS)
def test_every_step_equals_the_restatement(name, mode):
    g = Golden(name)
    f = _fields(g)
    dense_hint, rows = MODES[mode]
    with tile_geometry(rows):
        e = _engine(f, dense_hint)
    assert dense_hint or not e.is_dense, (name, mode)
    assert e.info("tracer_scheme") == 2 and e.info("tracers") == 2
    q, rq, ctrg = _wavy_tracers(f)
    upstream = [q, rq]
    _follow(e, f, q, rq, ctrg, range(1, NSTEPS + 1), 2, not g.uses_cos(), (name, mode), also=upstream)
    got = e.download_tracers()
    assert not same(got["q"][1], upstream[0][1]), (name, "the wavy tracer is where scheme 1 puts it: nothing tested")
    e.close()


# ---- handle kinds on frames of several tiles and chunks -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["closed_3l", "island_ragged_3l", "sill_sponges", "wide_67_chunks", "jet_xyper_2l"])
def test_handle_kinds_give_the_same_bits(name):
    f = _big_case(name)
    q, rq, ctrg = _wavy_tracers(f)
    e, tab = _engine(f), _engine(f, dense_hint=0)
    assert e.is_dense and not tab.is_dense
    if name in CASES:
        assert e.is_embedded == CASES[name][1]
    a, b = _run(e), _run(tab)
    assert np.isfinite(a["q"]).all() and np.isfinite(a["rq"]).all()
    assert same_bits(a["q"], b["q"]) and same_bits(a["rq"], b["rq"]), (name, "dense vs table path")
    assert same(a["q"][0][:, 1:], e.download(("hlay",))["hlay"][:, 1:]), (name, "uniform tracer vs hlay")
    assert not same(a["q"][1], q[1]), (name, "the wavy tracer did not move: nothing tested")
    bands = () if name in ("wide_67_chunks", "jet_xyper_2l") else (2, 3)       # (10 rows are too few; a ring is refused)
    for nb in bands:
        many = capi.MultiEngine(f, devices=[0] * nb)
        assert many.count == nb
        many.set_tracer_scheme("limited")
        many.set_tracers(2)
        many.upload_tracers(q=q, rq=rq, ctrg=ctrg)
        c = _run(many)
        assert same_bits(a["q"], c["q"]) and same_bits(a["rq"], c["rq"]), (name, nb, "bands vs the single handle")
        if name == "closed_3l":
            s = many.stats()
            assert s["split"] >= nb * (NSTEPS - 3), (name, nb, s, "the bands' steps were not cut")
        many.close()
    if name == "closed_3l":                 # the schemes differ on the device too
        one = _run(_engine(f, scheme=1))
        assert not same(a["q"][1], one["q"][1])
    e.close(); tab.close()


_TABLE = {}


def _table_path(name):
    """12 steps of the table path, once per frame."""
    if name not in _TABLE:
        tab = _engine(_big_case(name), dense_hint=0)
        _TABLE[name] = _run(tab)
        tab.close()
    return _TABLE[name]


@pytest.mark.parametrize("rows", [4, 8])
@pytest.mark.parametrize("name", ["closed_3l", "sill_sponges"])
def test_interior_tiles_of_both_geometries(name, rows):
    """The goldens are smaller than a tile, and frames of this size pick 64 x 4 by themselves: here the staged form of 64 x 8
    runs too, with and without relaxation (sill_sponges), on frames that have interior tiles in either geometry."""
    f = _big_case(name)
    # the tile at (65, rows + 1) and its ring of two lie in 2..L-2 x 2..M-2
    assert 65 + 64 + 1 <= f.p.lm + 1 - 2 and (rows + 1) + rows + 1 <= f.p.mm + 1 - 2
    with tile_geometry(rows):
        e = _engine(f)
    assert e.is_dense and e.info("tile_rows") == rows
    assert not e.is_embedded, "a frame with land may send every tile to the by-links form: the staged body would not run"
    a, b = _run(e), _table_path(name)
    assert np.isfinite(a["q"]).all() and np.isfinite(a["rq"]).all()
    assert same_bits(a["q"], b["q"]) and same_bits(a["rq"], b["rq"]), (name, rows, "tiled vs table path")
    e.close()


# ---- the default, switching, continuation---------------------------------------------------------------------------------------
def test_default_is_scheme_1():
    f = _big_case("closed_3l")
    fresh, one = _engine(f, scheme=None), _engine(f, scheme="upstream")
    assert fresh.info("tracer_scheme") == 1 and one.info("tracer_scheme") == 1
    a, b = _run(fresh), _run(one)
    assert same_bits(a["q"], b["q"]) and same_bits(a["rq"], b["rq"])
    fresh.set_tracers(0)
    fresh.set_tracer_scheme(2)
    fresh.set_tracers(1)
    assert fresh.info("tracer_scheme") == 2, "beom_set_tracers reset the scheme"
    with pytest.raises(capi.BeomError):
        fresh.set_tracer_scheme(3)
    with pytest.raises(capi.BeomError):
        fresh.set_tracer_scheme("central")
    assert fresh.info("tracer_scheme") == 2
    fresh.close(); one.close()


@pytest.mark.parametrize("mode", ["dense_64x8", "table"])
def test_schemes_switched_between_steps(mode):
    f = _fields(Golden("island_3l_forced"))
    dense_hint, rows = MODES[mode]
    with tile_geometry(rows):
        e = _engine(f, dense_hint)
    q, rq, ctrg = _wavy_tracers(f)
    for scheme, steps in ((2, range(1, 5)), (1, range(5, 9)), (2, range(9, 13))):
        e.set_tracer_scheme(scheme)
        assert e.info("tracer_scheme") == scheme
        q, rq = _follow(e, f, q, rq, ctrg, steps, scheme, True, ("island_3l_forced", mode, scheme))
    e.close()


def test_continuation_from_downloaded_tracers():
    f = _big_case("closed_3l")
    q, rq, ctrg = _wavy_tracers(f)
    whole = _run(_engine(f))
    first = _engine(f)
    first.step(1, 7)
    st, tr = first.download(), first.download_tracers()
    first.close()
    second = capi.Engine(f)
    second.upload(**st)
    second.set_tracers(2)
    second.set_tracer_scheme(2)
    second.upload_tracers(q=tr["q"], rq=tr["rq"], ctrg=ctrg)
    second.step(8, 5)
    got = second.download_tracers()
    assert same_bits(got["q"], whole["q"]) and same_bits(got["rq"], whole["rq"])
    second.close()


def test_per_sweep_entry_is_the_steps_sweep():
    """beom_update_tracers in front of beom_update_h with the step's scalars = what beom_step does for q and hlay, scheme 2."""
    f = _big_case("closed_3l")
    a, b = _engine(f), _engine(f)
    a.step(1, 5)
    b.step(1, 4)
    gene, ramp, ctim = T.step_scalars(f.p, 5, float(getattr(f, "tres", 0.0)))
    b.update_tracers(gene, ramp, ctim)
    b.update_h(gene, ramp, ctim)
    ta, tb = a.download_tracers(), b.download_tracers()
    assert same_bits(ta["q"], tb["q"]) and same_bits(ta["rq"], tb["rq"])
    assert same_bits(a.download(("hlay",))["hlay"], b.download(("hlay",))["hlay"])
    one = _engine(f, scheme=1)
    one.step(1, 5)
    assert not same(ta["q"][1], one.download_tracers()["q"][1]), "scheme 2 was not what ran"
    a.close(); b.close(); one.close()


# ---- off means off ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["closed_3l", "sill_sponges"])
def test_scheme_without_tracers_leaves_the_step_as_it_was(name):
    f = _big_case(name)
    plain, off = capi.Engine(f), _engine(f, tracers=False)
    assert off.info("tracer_scheme") == 2 and off.info("tracers") == 0
    plain.step(1, NSTEPS); off.step(1, NSTEPS)
    a, b = plain.download(), off.download()
    for k in _live(plain, STATE):
        assert same_bits(a[k], b[k]), (name, k)
    plain.close(); off.close()


def test_refusals_are_unchanged_under_scheme_2():
    ring = capi.MultiEngine(_big_case("jet_xyper_2l"), devices=(0, 0))
    assert ring.describe()["ring"] == 1
    ring.set_tracer_scheme(2)
    _refused(lambda: ring.set_tracers(1), "bands of a frame periodic in y")
    ring.close()
    from beom_amd import slab
    recipe = I.recipe_headline(150, 131, 3)
    fw, _, orphan = slab.build_band(recipe, 1, 0)
    band = capi.BandEngine(fw, recipe.p, 1, 0, device=0, rccl_id=None, orphan=orphan)
    band.set_tracer_scheme(2)
    _refused(lambda: band.set_tracers(1), "a handle that holds one band's window")
    band.close()
