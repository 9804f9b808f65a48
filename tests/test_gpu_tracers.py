"""Passive tracers on the device (beom_set_tracers ..., include/beom_hip.h) against the numpy restatement of the scheme
(tracers_ref, pinned to the reference by test_tracers_cpu) fed with the thicknesses and transports downloaded from the same
handle, step by step; the identity "a tracer of concentration 1 is the layer thickness" on the handle's own hlay; the same
bits from every handle kind (dense or embedded, table path, 2 and 3 bands); continuation; refusals; tracers switched off.
Comparisons are helpers.same (every value equal, +-0 alike, all finite) unless stated; the one fixture with a tidal
constituent is held to the project's 1e-12 relative for its cos term."""
import os

import numpy as np
import pytest

import tracers_ref as T
from beom_amd import capi, inputs as I
from beom_amd.grid import read_input_data
from helpers import STATE, Golden, maxrel, same, same_bits, tile_geometry
from test_gpu_biharm_tiled import CASES
from test_gpu_parity import COS_TOL, _fields, _live

pytestmark = pytest.mark.gpu
NSTEPS = 12
GOLDENS = ("stommel_24x16", "soliton_31x15_xper", "jet_2l_xyper", "island_3l_forced", "random_coast_2l_xper", "sill_4l_ocrp",
           "tc_wave_sponge", "obc_mcbc0_2l", "biharm_island_2l", "tide_sponge")
MODES = {"dense_64x4": (1, 4), "dense_64x8": (1, 8), "table": (0, 8)}      # name: (dense_hint, tile rows)


@pytest.fixture(autouse=True)
def _no_geometry_leak():
    before = os.environ.get("BEOM_TILE4")
    yield
    assert os.environ.get("BEOM_TILE4") == before


def _finite_same(a, b):
    return bool(np.isfinite(a).all()) and same(a, b)


def _tracers(f):
    """Two tracers: concentration 1 everywhere with relaxation concentration 1 (its content is the layer thickness), and a
    patchy one with a relaxation concentration that varies from cell to cell and layer to layer."""
    p = f.p
    i, j = f.subc[0].astype(np.float64), f.subc[1].astype(np.float64)
    c = np.stack([np.ones((p.nlay, p.ndeg + 1)), T.patchy(f)])
    ctrg = np.ones_like(c)
    for l in range(p.nlay):
        ctrg[1, l] = 0.4 + 0.3 * np.sin(0.37 * i + 0.1 * l) * np.cos(0.23 * j)
    q = c * np.asarray(f.hlay, dtype=np.float64)[None]
    rq = np.zeros(q.shape + (2,))
    rq[0] = f.rs_h
    return np.ascontiguousarray(q), rq, np.ascontiguousarray(ctrg)


def _engine(f, dense_hint=1, variant=0, tracers=True):
    e = capi.Engine(f, variant=variant, dense_hint=dense_hint)
    if tracers:
        q, rq, ctrg = _tracers(f)
        e.set_tracers(2)
        assert e.info("tracers") == 2
        e.upload_tracers(q=q, rq=rq, ctrg=ctrg)
    return e


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", GOLDENS)
def test_every_step_equals_the_restatement(name, mode):
    g = Golden(name)
    f = _fields(g)
    exact = not g.uses_cos()
    dense_hint, rows = MODES[mode]
    with tile_geometry(rows):
        e = _engine(f, dense_hint)
    assert dense_hint or not e.is_dense, (name, mode)
    q, rq, ctrg = _tracers(f)
    up = e.download_tracers()
    assert same_bits(up["q"], q) and same_bits(up["rq"], rq), (name, "upload / download round trip")
    tres = float(getattr(f, "tres", 0.0))
    for t in range(1, NSTEPS + 1):
        if t <= 3:
            e.rebuild_fluxes()              # what the step is about to do itself: the same values
        st = e.download(("hlay", "h_u", "h_v"))
        gene, ramp, ctim = T.step_scalars(f.p, t, tres)
        q, rq = T.update(f, st["hlay"], st["h_u"], st["h_v"], q, rq, ctrg, gene, ramp, ctim)
        e.step(t, 1)
        got = e.download_tracers()
        if exact:
            assert _finite_same(got["q"], q), (name, mode, t, "q", maxrel(got["q"], q))
            assert _finite_same(got["rq"], rq), (name, mode, t, "rq", maxrel(got["rq"], rq))
            # the identity on the device: the uniform tracer's content is the handle's own layer thickness
            h = e.download(("hlay",))["hlay"]
            assert _finite_same(got["q"][0][:, 1:], h[:, 1:]), (name, mode, t, "q of the uniform tracer vs hlay")
        else:
            assert np.isfinite(got["q"]).all() and np.isfinite(got["rq"]).all()
            print("%s %s step %d: maxrel q %.3g rq %.3g" % (name, mode, t, maxrel(got["q"], q), maxrel(got["rq"], rq)))
            assert maxrel(got["q"], q) <= COS_TOL, (name, mode, t, "q", maxrel(got["q"], q))
            assert maxrel(got["rq"], rq) <= COS_TOL, (name, mode, t, "rq", maxrel(got["rq"], rq))
            q, rq = got["q"], got["rq"]     # (the next step is judged on its own)
    assert not same(got["q"][1], _tracers(f)[0][1]), (name, "the patchy tracer did not move: nothing tested")
    e.close()


# ---- handle kinds on frames of several tiles and chunks -----------------------------------------------------------------------
def _big_case(name):
    if name == "closed_3l":
        p, files = I.case_headline(150, 131, 3)
    elif name == "wide_67_chunks":
        p, files = I.case_headline(4200, 9, 2)
    elif name == "sill_sponges":
        p, files = I.case_sill_exchange3d(lm=133, mm=199, nlay=4, dt_s=0.01, npts=5, sill_halfwidth=20.0)
    else:
        p, files = CASES[name][0]()
    return read_input_data(p.replace(svis="0."), files=files)


def _run(x, calls=(5, 7)):
    t = 1
    for n in calls:
        x.step(t, n)
        t += n
    assert t - 1 == NSTEPS
    return x.download_tracers()


@pytest.mark.parametrize("name", ["closed_3l", "island_ragged_3l", "sill_sponges", "wide_67_chunks", "jet_xyper_2l"])
def test_handle_kinds_give_the_same_bits(name):
    f = _big_case(name)
    q, rq, ctrg = _tracers(f)
    e, tab = _engine(f), _engine(f, dense_hint=0)
    assert e.is_dense and not tab.is_dense
    if name in CASES:
        assert e.is_embedded == CASES[name][1]
    if name == "sill_sponges":
        assert np.any(f.nudg[0] != 0.0)
    a, b = _run(e), _run(tab)
    assert np.isfinite(a["q"]).all() and np.isfinite(a["rq"]).all()
    assert same_bits(a["q"], b["q"]) and same_bits(a["rq"], b["rq"]), (name, "dense vs table path")
    assert same(a["q"][0][:, 1:], e.download(("hlay",))["hlay"][:, 1:]), (name, "uniform tracer vs hlay")
    assert not same(a["q"][1], q[1]), (name, "the patchy tracer did not move: nothing tested")
    bands = () if name in ("wide_67_chunks", "jet_xyper_2l") else (2, 3)       # (10 rows are too few; a ring is refused)
    for nb in bands:
        many = capi.MultiEngine(f, devices=[0] * nb)
        assert many.count == nb
        many.set_tracers(2)
        many.upload_tracers(q=q, rq=rq, ctrg=ctrg)
        c = _run(many)
        assert same_bits(a["q"], c["q"]) and same_bits(a["rq"], c["rq"]), (name, nb, "bands vs the single handle")
        if name == "closed_3l":
            s = many.stats()
            assert s["split"] >= nb * (NSTEPS - 3), (name, nb, s, "the bands' steps were not cut")
        many.close()
    e.close(); tab.close()


def test_continuation_from_downloaded_tracers():
    f = _big_case("closed_3l")
    q, rq, ctrg = _tracers(f)
    whole = _run(_engine(f))
    first = _engine(f)
    first.step(1, 7)
    st, tr = first.download(), first.download_tracers()
    first.close()
    second = capi.Engine(f)
    second.upload(**st)
    second.set_tracers(2)
    second.upload_tracers(q=tr["q"], rq=tr["rq"], ctrg=ctrg)
    second.step(8, 5)
    got = second.download_tracers()
    assert same_bits(got["q"], whole["q"]) and same_bits(got["rq"], whole["rq"])
    second.close()


def test_set_concentration_multiplies_by_the_handles_thickness():
    f = _big_case("closed_3l")
    e = capi.Engine(f)
    e.step(1, 4)
    e.set_tracers(1)
    h = e.download(("hlay",))["hlay"]
    e.set_concentration(0.5)
    assert same_bits(e.download_tracers()["q"][0], 0.5 * h)
    e.close()


def test_per_sweep_entry_is_the_steps_sweep():
    """beom_update_tracers in front of beom_update_h with the step's scalars = what beom_step does for q and hlay."""
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
    a.close(); b.close()


# ---- refusals, and tracers switched off again ---------------------------------------------------------------------------------
def _refused(call, what):
    with pytest.raises(capi.BeomError) as ei:
        call()
    msg = str(ei.value)
    assert "error -6:" in msg and len(msg.split("error -6:")[1].strip()) > 20, (what, msg)


def test_refused_configurations():
    g = Golden("variant3d_3l")
    assert g.variant == 1
    e = capi.Engine(_fields(g), variant=1)
    _refused(lambda: e.set_tracers(1), "variant 1")
    assert e.info("tracers") == 0
    e.close()
    g = Golden("rigid_lid_sill_2l")
    e = capi.Engine(_fields(g), variant=g.variant)
    _refused(lambda: e.set_tracers(1), "rgld = 1")
    e.close()
    ring = capi.MultiEngine(_big_case("jet_xyper_2l"), devices=(0, 0))
    assert ring.describe()["ring"] == 1
    _refused(lambda: ring.set_tracers(1), "bands of a frame periodic in y")
    ring.close()
    from beom_amd import slab
    recipe = I.recipe_headline(150, 131, 3)
    fw, _, orphan = slab.build_band(recipe, 1, 0)
    band = capi.BandEngine(fw, recipe.p, 1, 0, device=0, rccl_id=None, orphan=orphan)
    _refused(lambda: band.set_tracers(1), "a handle that holds one band's window")
    band.close()
    e = capi.Engine(_big_case("closed_3l"))
    with pytest.raises(capi.BeomError):
        e.set_tracers(capi.BEOM_MAX_TRACERS + 1)
    e.set_tracers(capi.BEOM_MAX_TRACERS)
    assert e.info("tracers") == capi.BEOM_MAX_TRACERS
    e.close()


@pytest.mark.parametrize("name", ["closed_3l", "sill_sponges"])
def test_tracers_switched_off_leave_the_step_as_it_was(name):
    f = _big_case(name)
    plain, off = capi.Engine(f), _engine(f)
    off.step(1, 2)
    plain.step(1, 2)
    off.set_tracers(0)
    assert off.info("tracers") == 0
    with pytest.raises(capi.BeomError):
        off.download_tracers()
    plain.step(3, 10); off.step(3, 10)
    a, b = plain.download(), off.download()
    for k in _live(plain, STATE):
        assert same_bits(a[k], b[k]), (name, k)
    plain.close(); off.close()
