"""Tracer mixing on the device (beom_set_tracer_mixing, include/beom_hip.h): lateral diffusion, decay and sources in a launch
of their own in front of the tracer sweep, against the numpy restatement (tracer_mix_ref, held by test_tracer_mix_cpu)
followed by the restated sweep of either scheme, fed with the thicknesses and transports downloaded from the same handle,
step by step; the identity "a tracer of concentration 1 is the layer thickness" with diffusion at its cap; the same bits
from every handle kind (dense or embedded, table path, 2 and 3 bands); a rough ocrp = 1 state; the per-sweep entry;
continuation; the refusals; mixing switched off again.  Frames and step counts are test_gpu_tracers'.  Comparisons are
helpers.same (every value equal, +-0 alike, all finite) unless stated; the one fixture with a tidal constituent is held to
the project's 1e-12 relative for its cos term."""
import os

import numpy as np
import pytest

import rough_inputs as RI
import tracer_mix_ref as TM
import tracers_limited_ref as TL
import tracers_ref as T
from addons_kit import mix_coefficients
from beom_amd import capi, inputs as I
from helpers import STATE, Golden, maxrel, same, same_bits, tile_geometry
from test_gpu_biharm_tiled import CASES
from test_gpu_parity import COS_TOL, _fields, _live
from test_gpu_tracers import GOLDENS, MODES, NSTEPS, _big_case, _finite_same, _run, _tracers

pytestmark = pytest.mark.gpu
assert NSTEPS == 12 and len(GOLDENS) == 10 and sorted(MODES) == ["dense_64x4", "dense_64x8", "table"]
NTRC = 3


@pytest.fixture(autouse=True)
def _no_geometry_leak():
    before = os.environ.get("BEOM_TILE4")
    yield
    assert os.environ.get("BEOM_TILE4") == before


def _tracers3(f):
    """Three tracers: concentration 1 everywhere with relaxation concentration 1, the patchy one of test_gpu_tracers, and a
    second patchy one with other values and the mirrored relaxation concentration."""
    q, rq, ctrg = _tracers(f)
    q = np.concatenate([q, (T.patchy(f, low=0.1, high=2.0) * np.asarray(f.hlay, dtype=np.float64))[None]])
    rq = np.concatenate([rq, np.zeros_like(rq[:1])])
    ctrg = np.concatenate([ctrg, 1.1 - ctrg[1:2]])
    return np.ascontiguousarray(q), np.ascontiguousarray(rq), np.ascontiguousarray(ctrg)


def _coefficients(p):
    """kappa, decay, source [3, nlay] (addons_kit.mix_coefficients, which the kit of every add-on shares): the uniform tracer
    diffuses at the cap; the patchy one with another kappa in every layer, a decay in layer 1 and a source in the others; the
    third with decay and source alone."""
    return mix_coefficients(p, NTRC)


def _engine(f, dense_hint=1, scheme=1, mixing=True):
    e = capi.Engine(f, dense_hint=dense_hint)
    e.set_tracer_scheme(scheme)
    q, rq, ctrg = _tracers3(f)
    e.set_tracers(NTRC)
    e.upload_tracers(q=q, rq=rq, ctrg=ctrg)
    assert e.info("tracer_mixing") == 0 and e.info("tracer_mix_launches") == 0
    if mixing:
        kappa, decay, source = _coefficients(f.p)
        e.set_tracer_mixing(kappa=kappa, decay=decay, source=source)
        assert e.info("tracer_mixing") == 1
    return e


def _sweep(scheme, f, st, q, rq, ctrg, scalars):
    if scheme == 1:
        return T.update(f, st["hlay"], st["h_u"], st["h_v"], q, rq, ctrg, *scalars)
    return TL.update(f, st["hlay"], st["h_u"], st["h_v"], q, rq, ctrg, *scalars, scheme=2)


def _follow(e, f, steps, scheme, exact, what, ntrc=NTRC, start=None, coefficients=None):
    """The handle's steps one by one against mix + sweep of the restatement fed with the handle's own hlay, h_u, h_v; the
    sweep alone is carried along on the same inputs.  Returns the handle's tracers and the unmixed q."""
    q, rq, ctrg = start if start is not None else _tracers3(f)
    kappa, decay, source = coefficients if coefficients is not None else _coefficients(f.p)
    plain = [q, rq]
    tres = float(getattr(f, "tres", 0.0))
    launches = e.info("tracer_mix_launches")
    got = None
    for t in steps:
        if t <= 3:
            e.rebuild_fluxes()              # what the step is about to do itself: the same values
        st = e.download(("hlay", "h_u", "h_v"))
        sc = T.step_scalars(f.p, t, tres)
        q, rq = _sweep(scheme, f, st, TM.mix(f, st["hlay"], q, kappa, decay, source), rq, ctrg, sc)
        plain = list(_sweep(scheme, f, st, plain[0], plain[1], ctrg, sc))
        e.step(t, 1)
        launches += 1
        assert e.info("tracer_mix_launches") == launches
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
    for k in range(1, ntrc):
        assert not same(got["q"][k], plain[0][k]), (what, k, "the tracer is where a run without mixing puts it: nothing tested")
    return got, plain[0]


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", GOLDENS)
def test_every_step_equals_the_restatement(name, mode, scheme):
    g = Golden(name)
    f = _fields(g)
    dense_hint, rows = MODES[mode]
    with tile_geometry(rows):
        e = _engine(f, dense_hint, scheme)
    assert dense_hint or not e.is_dense, (name, mode)
    assert e.info("tracer_scheme") == scheme and e.info("tracers") == NTRC
    _follow(e, f, range(1, NSTEPS + 1), scheme, not g.uses_cos(), (name, mode, scheme))
    e.close()


# ---- handle kinds on frames of several tiles and chunks -----------------------------------------------------------------------
def _many(f, nb, scheme, mixing=True):
    many = capi.MultiEngine(f, devices=[0] * nb)
    assert many.count == nb
    many.set_tracer_scheme(scheme)
    q, rq, ctrg = _tracers3(f)
    many.set_tracers(NTRC)
    many.upload_tracers(q=q, rq=rq, ctrg=ctrg)
    if mixing:
        kappa, decay, source = _coefficients(f.p)
        many.set_tracer_mixing(kappa=kappa, decay=decay, source=source)
        assert many.info("tracer_mixing") == 1
    return many


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("name", ["closed_3l", "island_ragged_3l", "sill_sponges", "wide_67_chunks", "jet_xyper_2l"])
def test_handle_kinds_give_the_same_bits(name, scheme):
    f = _big_case(name)
    q = _tracers3(f)[0]
    e, tab, off = _engine(f, scheme=scheme), _engine(f, dense_hint=0, scheme=scheme), _engine(f, scheme=scheme, mixing=False)
    assert e.is_dense and not tab.is_dense
    if name in CASES:
        assert e.is_embedded == CASES[name][1]
    a, b, c = _run(e), _run(tab), _run(off)
    assert e.info("tracer_mix_launches") == NSTEPS and tab.info("tracer_mix_launches") == NSTEPS and off.info("tracer_mix_launches") == 0
    assert np.isfinite(a["q"]).all() and np.isfinite(a["rq"]).all()
    assert same_bits(a["q"], b["q"]) and same_bits(a["rq"], b["rq"]), (name, "dense vs table path")
    assert same(a["q"][0][:, 1:], e.download(("hlay",))["hlay"][:, 1:]), (name, "uniform tracer vs hlay")
    assert same_bits(a["q"][0], c["q"][0]), (name, "the uniform tracer with and without mixing")
    for k in (1, 2):
        assert not same(a["q"][k], c["q"][k]), (name, k, "the tracer is where a run without mixing puts it: nothing tested")
    bands = () if name in ("wide_67_chunks", "jet_xyper_2l") else (2, 3)       # (10 rows are too few; a ring is refused)
    for nb in bands:
        many = _many(f, nb, scheme)
        m = _run(many)
        assert same_bits(a["q"], m["q"]) and same_bits(a["rq"], m["rq"]), (name, nb, "bands vs the single handle")
        assert many.info("tracer_mix_launches") == NSTEPS
        if name == "closed_3l":
            s = many.stats()
            assert s["split"] >= nb * (NSTEPS - 3), (name, nb, s, "the bands' steps were not cut")
        many.close()
    e.close(); tab.close(); off.close()


def test_rough_state_with_thin_cells_next_to_thick_ones():
    """A rough ocrp = 1 state (rough_inputs: a share of the cell-layers at 1-3 hsal among layers of the case's own thickness),
    rough tracers, dense, steps 7-12 against the restatement."""
    config = "sill_ocrp_sponge_3l"
    g = RI.rough_fields(RI.base_fields(config, "130x18"), 1)
    assert float(g.p.ocrp) > 0.5
    E = g.neig[:, 0].astype(np.int64)
    both = (g.hlay > 0) & (g.hlay[:, E] > 0)
    ratio = np.where(both, g.hlay / np.where(both, g.hlay[:, E], 1.0), 1.0)
    print("thickness ratio between E neighbours: %.3g .. %.3g" % (ratio.min(), ratio.max()))
    assert ratio.max() >= 20.0 and ratio.min() <= 0.05
    e = capi.Engine(g, dense_hint=1)
    assert e.is_dense
    start = RI.rough_tracers(g, g.hlay, NTRC, 7)
    e.set_tracers(NTRC)
    e.upload_tracers(q=start[0], rq=start[1], ctrg=start[2])
    co = _coefficients(g.p)
    e.set_tracer_mixing(*co)
    _follow(e, g, range(7, 13), 1, True, config, start=start, coefficients=co)
    e.close()


def test_per_sweep_entry_is_the_steps_launch():
    """beom_update_tracer_mixing + beom_update_tracers + beom_update_h with the step's scalars = what beom_step does."""
    f = _big_case("closed_3l")
    a, b = _engine(f), _engine(f)
    a.step(1, 5)
    b.step(1, 4)
    gene, ramp, ctim = T.step_scalars(f.p, 5, float(getattr(f, "tres", 0.0)))
    b.update_tracer_mixing()
    b.update_tracers(gene, ramp, ctim)
    b.update_h(gene, ramp, ctim)
    assert a.info("tracer_mix_launches") == 5 and b.info("tracer_mix_launches") == 5
    ta, tb = a.download_tracers(), b.download_tracers()
    assert same_bits(ta["q"], tb["q"]) and same_bits(ta["rq"], tb["rq"])
    assert same_bits(a.download(("hlay",))["hlay"], b.download(("hlay",))["hlay"])
    # beom_update_tracers alone stays the advective sweep: no mixing launch
    b.update_tracers(gene, ramp, ctim)
    assert b.info("tracer_mix_launches") == 5
    a.close(); b.close()


def test_continuation_from_downloaded_tracers():
    f = _big_case("closed_3l")
    ctrg = _tracers3(f)[2]
    whole = _run(_engine(f))
    first = _engine(f)
    first.step(1, 7)
    st, tr = first.download(), first.download_tracers()
    first.close()
    second = capi.Engine(f)
    second.upload(**st)
    second.set_tracers(NTRC)
    second.upload_tracers(q=tr["q"], rq=tr["rq"], ctrg=ctrg)
    second.set_tracer_mixing(*_coefficients(f.p))
    second.step(8, 5)
    got = second.download_tracers()
    assert same_bits(got["q"], whole["q"]) and same_bits(got["rq"], whole["rq"])
    second.close()


# ---- the interface: broadcasting, refusals, switched off ----------------------------------------------------------------------
def test_scalars_and_per_tracer_values_broadcast():
    f = _big_case("closed_3l")
    cap = TM.kappa_cap(f.p)
    dec = np.array([0.0, 0.02, 0.04]) / float(f.p.dt)
    a, b = _engine(f, mixing=False), _engine(f, mixing=False)
    a.set_tracer_mixing(kappa=0.5 * cap, decay=dec)
    b.set_tracer_mixing(kappa=np.full((NTRC, f.p.nlay), 0.5 * cap), decay=np.repeat(dec[:, None], f.p.nlay, axis=1), source=np.zeros(NTRC))
    a.step(1, 4); b.step(1, 4)
    assert same_bits(a.download_tracers()["q"], b.download_tracers()["q"])
    with pytest.raises(capi.BeomError):
        a.set_tracer_mixing(kappa=np.zeros(NTRC + 1))
    a.close(); b.close()


def _refused(call, code, what):
    with pytest.raises(capi.BeomError) as ei:
        call()
    msg = str(ei.value)
    tag = "error %d:" % code
    assert tag in msg and len(msg.split(tag)[1].strip()) > 20, (what, msg)


def test_refused_arguments_leave_the_handle_as_it_was():
    f = _big_case("closed_3l")
    cap, dt = TM.kappa_cap(f.p), float(f.p.dt)
    bare = capi.Engine(f)
    _refused(lambda: bare.set_tracer_mixing(kappa=1.0), -3, "no tracers")
    with pytest.raises(capi.BeomError):
        bare.update_tracer_mixing()
    bare.close()
    for mixing in (False, True):
        e = _engine(f, mixing=mixing)
        before = e.download_tracers()
        for what, kw in (("nan", dict(kappa=np.nan)), ("inf", dict(source=np.inf)), ("-inf", dict(decay=-np.inf)),
                         ("kappa < 0", dict(kappa=-1.0e-9 * cap)), ("kappa above the cap", dict(kappa=1.001 * cap)),
                         ("decay < 0", dict(decay=-1.0e-9 / dt)), ("decay dt > 1", dict(decay=1.001 / dt)),
                         ("one bad layer", dict(kappa=np.array([[0.0] * f.p.nlay, [0.0] * (f.p.nlay - 1) + [1.001 * cap], [0.0] * f.p.nlay])))):
            _refused(lambda: e.set_tracer_mixing(**kw), -3, what)
            assert e.info("tracer_mixing") == int(mixing), what
        # nothing was touched: the handle steps as one that was never asked
        twin = _engine(f, mixing=mixing)
        e.step(1, 3); twin.step(1, 3)
        assert same_bits(before["q"], _tracers3(f)[0])
        assert same_bits(e.download_tracers()["q"], twin.download_tracers()["q"])
        # the caps themselves pass; another count drops the mixing, the same count keeps it
        e.set_tracer_mixing(kappa=cap, decay=1.0 / dt)
        assert e.info("tracer_mixing") == 1
        e.set_tracers(NTRC)
        assert e.info("tracer_mixing") == 1
        e.set_tracers(NTRC - 1)
        assert e.info("tracer_mixing") == 0
        e.close(); twin.close()


def test_rings_and_rank_local_handles_are_refused():
    ring = capi.MultiEngine(_big_case("jet_xyper_2l"), devices=(0, 0))
    assert ring.describe()["ring"] == 1
    _refused(lambda: ring.set_tracer_mixing(kappa=1.0), -6, "bands of a frame periodic in y")
    ring.close()
    from beom_amd import slab
    recipe = I.recipe_headline(150, 131, 3)
    fw, _, orphan = slab.build_band(recipe, 1, 0)
    band = capi.BandEngine(fw, recipe.p, 1, 0, device=0, rccl_id=None, orphan=orphan)
    _refused(lambda: band.set_tracer_mixing(kappa=1.0), -6, "a handle that holds one band's window")
    band.close()
    many = _many(_big_case("closed_3l"), 2, 1, mixing=False)
    _refused(lambda: many.set_tracer_mixing(kappa=-1.0), -3, "bands: kappa < 0")
    assert many.info("tracer_mixing") == 0
    many.close()


@pytest.mark.parametrize("name", ["closed_3l", "sill_sponges"])
def test_mixing_switched_off_leaves_the_step_as_it_was(name):
    f = _big_case(name)
    never, off = _engine(f, mixing=False), _engine(f)
    assert never.info("tracer_mix_launches") == 0
    off.step(1, 2)
    assert off.info("tracer_mix_launches") == 2
    off.set_tracer_mixing(kappa=0.0, decay=None, source=np.zeros(NTRC))        # all zero: off
    assert off.info("tracer_mixing") == 0
    with pytest.raises(capi.BeomError):
        off.update_tracer_mixing()
    # the twin makes the same two steps (tracers are passive: the same state), takes over the mixed tracers, and never sets
    # the mixing
    never.step(1, 2)
    tr = off.download_tracers()
    never.upload_tracers(q=tr["q"], rq=tr["rq"])
    never.step(3, 10); off.step(3, 10)
    assert off.info("tracer_mix_launches") == 2 and never.info("tracer_mix_launches") == 0
    a, b = never.download(), off.download()
    for k in _live(never, STATE):
        assert same_bits(a[k], b[k]), (name, k)
    ta, tb = never.download_tracers(), off.download_tracers()
    assert same_bits(ta["q"], tb["q"]) and same_bits(ta["rq"], tb["rq"]), name
    never.close(); off.close()
