"""Vertical tracer mixing on the device (beom_set_tracer_vmixing, include/beom_hip.h): the column solve in a launch of its own
between the lateral mixing and the tracer sweep, against the numpy restatement (tracer_vmix_ref, held by
test_tracer_vmix_cpu).  Every layer count 2..16 in every cell context on thicknesses over four decades with dry layers;
the handle's steps one by one against lateral mix + vertical mix + the restated sweep of either scheme, fed with the
thicknesses and transports downloaded from the same handle; the identity "a tracer of concentration 1 is the layer
thickness"; the same bits from every handle kind (dense or embedded, table path, 2 and 3 bands); a rough ocrp = 1 state;
continuation; the refusals; switched off again; dropped with the tracers.  Frames, step counts and helpers are
test_gpu_tracers' and test_gpu_tracer_mix's.  Comparisons are helpers.same (every value equal, +-0 alike, all finite) unless
stated; the one fixture with a tidal constituent is held to the project's 1e-12 relative for its cos term."""
import os

import numpy as np
import pytest

import rough_inputs as RI
import tracer_mix_ref as TM
import tracer_vmix_ref as TV
import tracers_ref as T
from addons_kit import kappa_v_table
from beom_amd import capi, inputs as I
from beom_amd.grid import read_input_data
from helpers import STATE, Golden, maxrel, same, same_bits, tile_geometry
from test_gpu_biharm_tiled import CASES
from test_gpu_parity import COS_TOL, _fields, _live
from test_gpu_tracer_mix import NTRC, _coefficients, _refused, _sweep, _tracers3
from test_gpu_tracers import GOLDENS, MODES, NSTEPS, _big_case, _finite_same, _run

pytestmark = pytest.mark.gpu
assert NSTEPS == 12 and NTRC == 3 and sorted(MODES) == ["dense_64x4", "dense_64x8", "table"]
LAYERED = tuple(n for n in GOLDENS if Golden(n).fields().p.nlay >= 2)
assert len(LAYERED) >= 6 and "tide_sponge" in GOLDENS, LAYERED


@pytest.fixture(autouse=True)
def _no_geometry_leak():
    before = os.environ.get("BEOM_TILE4")
    yield
    assert os.environ.get("BEOM_TILE4") == before


def _kappa_v(p, ntrc=NTRC):
    """[ntrc, nlay-1] in m2/s (addons_kit.kappa_v_table, which the kit of every add-on shares): another value for every
    tracer and interface, from 1e-5 (explicit would do) to dt kappa_v / hbar^2 far beyond any explicit limit; tracer 0 (the
    uniform one) gets the largest; the last tracer's row has a zero."""
    return kappa_v_table(p, ntrc)


def _moved(kv, got, plain, what):
    """Every tracer but the uniform one is elsewhere than without vertical mixing; one whose interfaces are all closed (the
    last tracer of a two-layer frame) is where it was, bit for bit."""
    for k in range(1, kv.shape[0]):
        if np.any(kv[k] > 0):
            assert not same(got[k], plain[k]), (what, k, "the tracer is where it is without vertical mixing: nothing tested")
        else:
            assert same_bits(got[k], plain[k]), (what, k, "a tracer with every interface closed moved")


# ---- every NL in every context -------------------------------------------------------------------------------------------------
def _reseeded(f, seed):
    """Thicknesses 10^uniform(-2, 2) with about 15 % of the cell-layers dry, and three tracers of other concentrations."""
    r = np.random.default_rng(seed)
    shape = (f.p.nlay, f.p.ndeg + 1)
    h = 10.0 ** r.uniform(-2.0, 2.0, shape)
    h[r.uniform(0, 1, shape) < 0.15] = 0.0
    h[:, 0] = np.asarray(f.hlay, dtype=np.float64)[:, 0]
    c = r.uniform(0.25, 1.0, (NTRC,) + shape)
    c[0] = 1.0
    q = np.ascontiguousarray(c * h[None])
    q[:, :, 0] = 0.0
    return h, q


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("nlay", range(2, 17))
def test_every_layer_count_in_every_context(nlay, mode):
    p, files = I.case_headline(70, 9, nlay)
    f = read_input_data(p, files=files)
    assert f.p.nlay == nlay and f.p.lm + 1 > 64 and f.p.mm + 1 > 8
    dense_hint, rows = MODES[mode]
    with tile_geometry(rows):
        e = capi.Engine(f, dense_hint=dense_hint)
    assert dense_hint or not e.is_dense, (nlay, mode)
    h, q = _reseeded(f, 100 + nlay)
    e.upload(hlay=h)
    e.set_tracers(NTRC)
    e.upload_tracers(q=q)
    kv = _kappa_v(f.p)
    assert np.any(kv == 0.0) and len(np.unique(kv)) >= min(kv.size - 1, 6)
    assert e.info("tracer_vmixing") == 0 and e.info("tracer_vmix_launches") == 0
    e.set_tracer_vertical_mixing(kv)
    assert e.info("tracer_vmixing") == 1
    hd = e.download(("hlay",))["hlay"]
    assert same_bits(hd[:, 1:], h[:, 1:])
    want, G = TV.vmix(f, hd, q, kv)
    e.update_tracer_vertical_mixing()
    assert e.info("tracer_vmix_launches") == 1
    got = e.download_tracers()["q"]
    assert np.isfinite(got).all()
    assert same(got, want), (nlay, mode, maxrel(got, want))
    assert same(got[0], q[0]), "the uniform tracer moved"
    _moved(kv, got, q, (nlay, mode))
    e.update_tracer_vertical_mixing()
    assert e.info("tracer_vmix_launches") == 2
    assert same(e.download_tracers()["q"], TV.vmix(f, hd, want, kv)[0])
    e.close()


# ---- step by step --------------------------------------------------------------------------------------------------------------
def _engine(f, dense_hint=1, scheme=1, lateral=True, vertical=True):
    e = capi.Engine(f, dense_hint=dense_hint)
    e.set_tracer_scheme(scheme)
    q, rq, ctrg = _tracers3(f)
    e.set_tracers(NTRC)
    e.upload_tracers(q=q, rq=rq, ctrg=ctrg)
    assert e.info("tracer_vmixing") == 0 and e.info("tracer_vmix_launches") == 0
    if lateral:
        e.set_tracer_mixing(*_coefficients(f.p))
    if vertical:
        e.set_tracer_vertical_mixing(_kappa_v(f.p))
        assert e.info("tracer_vmixing") == 1
    return e


def _follow(e, f, steps, scheme, exact, what, start=None):
    """The handle's steps one by one against lateral mix + vertical mix + sweep of the restatement fed with the handle's own
    hlay, h_u, h_v; the same without the vertical mix is carried along on the same inputs."""
    q, rq, ctrg = start if start is not None else _tracers3(f)
    co, kv = _coefficients(f.p), _kappa_v(f.p)
    plain = [q, rq]
    tres = float(getattr(f, "tres", 0.0))
    launches = e.info("tracer_vmix_launches")
    lateral = e.info("tracer_mix_launches")
    got = None
    for t in steps:
        if t <= 3:
            e.rebuild_fluxes()              # what the step is about to do itself: the same values
        st = e.download(("hlay", "h_u", "h_v"))
        sc = T.step_scalars(f.p, t, tres)
        mixed = TV.vmix(f, st["hlay"], TM.mix(f, st["hlay"], q, *co), kv)[0]
        q, rq = _sweep(scheme, f, st, mixed, rq, ctrg, sc)
        plain = list(_sweep(scheme, f, st, TM.mix(f, st["hlay"], plain[0], *co), plain[1], ctrg, sc))
        e.step(t, 1)
        launches += 1
        lateral += 1
        assert e.info("tracer_vmix_launches") == launches and e.info("tracer_mix_launches") == lateral
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
    _moved(kv, got["q"], plain[0], what)
    return got


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", LAYERED)
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


def test_rough_state_with_thin_salmon_layers_next_to_thick_ones():
    """A rough ocrp = 1 state (rough_inputs: a share of the cell-layers at 1-3 hsal among layers of the case's own thickness),
    rough tracers, dense, steps 7-12 against the restatement."""
    config = "sill_ocrp_sponge_3l"
    g = RI.rough_fields(RI.base_fields(config, "130x18"), 1)
    assert float(g.p.ocrp) > 0.5 and g.p.nlay >= 3
    both = (g.hlay[:-1] > 0) & (g.hlay[1:] > 0)
    ratio = np.where(both, g.hlay[:-1] / np.where(both, g.hlay[1:], 1.0), 1.0)
    print("thickness ratio between vertical neighbours: %.3g .. %.3g" % (ratio.min(), ratio.max()))
    assert ratio.max() >= 20.0 and ratio.min() <= 0.05
    e = capi.Engine(g, dense_hint=1)
    assert e.is_dense
    start = RI.rough_tracers(g, g.hlay, NTRC, 7)
    e.set_tracers(NTRC)
    e.upload_tracers(q=start[0], rq=start[1], ctrg=start[2])
    e.set_tracer_mixing(*_coefficients(g.p))
    e.set_tracer_vertical_mixing(_kappa_v(g.p))
    # (rough tracers: no uniform one, so the comparison with hlay is left to the other tests)
    q, rq, ctrg = start
    co, kv = _coefficients(g.p), _kappa_v(g.p)
    tres = float(getattr(g, "tres", 0.0))
    for t in range(7, 13):
        st = e.download(("hlay", "h_u", "h_v"))
        mixed, G = TV.vmix(g, st["hlay"], TM.mix(g, st["hlay"], q, *co), kv)
        assert np.any(G[1:])
        q, rq = _sweep(1, g, st, mixed, rq, ctrg, T.step_scalars(g.p, t, tres))
        e.step(t, 1)
        got = e.download_tracers()
        assert _finite_same(got["q"], q), (config, t, "q", maxrel(got["q"], q))
        assert _finite_same(got["rq"], rq), (config, t, "rq", maxrel(got["rq"], rq))
    assert e.info("tracer_vmix_launches") == 6
    e.close()


# ---- handle kinds on frames of several tiles and chunks -----------------------------------------------------------------------
def _many(f, nb, scheme, vertical=True):
    many = capi.MultiEngine(f, devices=[0] * nb)
    assert many.count == nb
    many.set_tracer_scheme(scheme)
    q, rq, ctrg = _tracers3(f)
    many.set_tracers(NTRC)
    many.upload_tracers(q=q, rq=rq, ctrg=ctrg)
    many.set_tracer_mixing(*_coefficients(f.p))
    if vertical:
        many.set_tracer_vertical_mixing(_kappa_v(f.p))
        assert many.info("tracer_vmixing") == 1
    return many


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("name", ["closed_3l", "island_ragged_3l", "sill_sponges", "wide_67_chunks", "jet_xyper_2l"])
def test_handle_kinds_give_the_same_bits(name, scheme):
    f = _big_case(name)
    e, tab, off = _engine(f, scheme=scheme), _engine(f, dense_hint=0, scheme=scheme), _engine(f, scheme=scheme, vertical=False)
    assert e.is_dense and not tab.is_dense
    if name in CASES:
        assert e.is_embedded == CASES[name][1]
    a, b, c = _run(e), _run(tab), _run(off)
    assert e.info("tracer_vmix_launches") == NSTEPS and tab.info("tracer_vmix_launches") == NSTEPS and off.info("tracer_vmix_launches") == 0
    assert np.isfinite(a["q"]).all() and np.isfinite(a["rq"]).all()
    assert same_bits(a["q"], b["q"]) and same_bits(a["rq"], b["rq"]), (name, "dense vs table path")
    assert same(a["q"][0][:, 1:], e.download(("hlay",))["hlay"][:, 1:]), (name, "uniform tracer vs hlay")
    assert same_bits(a["q"][0], c["q"][0]), (name, "the uniform tracer with and without vertical mixing")
    _moved(_kappa_v(f.p), a["q"], c["q"], name)
    bands = () if name in ("wide_67_chunks", "jet_xyper_2l") else (2, 3)       # (10 rows are too few; a ring is refused)
    for nb in bands:
        many = _many(f, nb, scheme)
        m = _run(many)
        assert same_bits(a["q"], m["q"]) and same_bits(a["rq"], m["rq"]), (name, nb, "bands vs the single handle")
        assert many.info("tracer_vmix_launches") == NSTEPS
        if name == "closed_3l":
            s = many.stats()
            assert s["split"] >= nb * (NSTEPS - 3), (name, nb, s, "the bands' steps were not cut")
        many.close()
    e.close(); tab.close(); off.close()


def test_per_sweep_entry_is_the_steps_launch():
    """beom_update_tracer_mixing + beom_update_tracer_vmixing + beom_update_tracers + beom_update_h with the step's scalars =
    what beom_step does."""
    f = _big_case("closed_3l")
    a, b = _engine(f), _engine(f)
    a.step(1, 5)
    b.step(1, 4)
    gene, ramp, ctim = T.step_scalars(f.p, 5, float(getattr(f, "tres", 0.0)))
    b.update_tracer_mixing()
    b.update_tracer_vertical_mixing()
    b.update_tracers(gene, ramp, ctim)
    b.update_h(gene, ramp, ctim)
    assert a.info("tracer_vmix_launches") == 5 and b.info("tracer_vmix_launches") == 5
    ta, tb = a.download_tracers(), b.download_tracers()
    assert same_bits(ta["q"], tb["q"]) and same_bits(ta["rq"], tb["rq"])
    # beom_update_tracers alone stays the advective sweep: no mixing launch of either kind
    b.update_tracers(gene, ramp, ctim)
    assert b.info("tracer_vmix_launches") == 5 and b.info("tracer_mix_launches") == 5
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
    second.set_tracer_vertical_mixing(_kappa_v(f.p))
    second.step(8, 5)
    got = second.download_tracers()
    assert same_bits(got["q"], whole["q"]) and same_bits(got["rq"], whole["rq"])
    second.close()


# ---- the interface: broadcasting, refusals, switched off, dropped --------------------------------------------------------------
def test_scalars_and_per_interface_values_broadcast():
    f = _big_case("closed_3l")
    nk = f.p.nlay - 1
    per = np.array([0.5, 2.0e-3])[:nk]
    a, b, c = (_engine(f, lateral=False, vertical=False) for _ in range(3))
    a.set_tracer_vertical_mixing(per)
    b.set_tracer_vertical_mixing(np.repeat(per[None], NTRC, axis=0))
    c.set_tracer_vertical_mixing(0.5)
    for x in (a, b, c):
        x.step(1, 4)
    qa, qb, qc = (x.download_tracers()["q"] for x in (a, b, c))
    assert same_bits(qa, qb) and not same_bits(qa, qc)
    with pytest.raises(capi.BeomError):
        a.set_tracer_vertical_mixing(np.zeros(nk + 1))
    with pytest.raises(capi.BeomError):
        a.set_tracer_vertical_mixing(np.zeros((NTRC + 1, nk)))
    for x in (a, b, c):
        x.close()


def test_refused_arguments_leave_the_handle_as_it_was():
    f = _big_case("closed_3l")
    dt, nk = float(f.p.dt), f.p.nlay - 1
    bare = capi.Engine(f)
    _refused(lambda: bare.set_tracer_vertical_mixing(1.0), -3, "no tracers")
    with pytest.raises(capi.BeomError):
        bare.update_tracer_vertical_mixing()
    bare.close()
    assert np.isinf(dt * 1.0e308) and 1.0 / (dt * 1.0e-320) == np.inf
    one_bad = np.full((NTRC, nk), 1.0e-3); one_bad[NTRC - 1, nk - 1] = -1.0e-3
    for vertical in (False, True):
        e = _engine(f, vertical=vertical)
        for what, kv in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf), ("negative", -1.0e-9), ("one bad interface", one_bad),
                         ("dt kappa_v overflows", 1.0e308), ("1 / (dt kappa_v) overflows", 1.0e-320)):
            _refused(lambda: e.set_tracer_vertical_mixing(kv), -3, what)
            assert e.info("tracer_vmixing") == int(vertical), what
        if not vertical:
            with pytest.raises(capi.BeomError):
                e.update_tracer_vertical_mixing()
        # nothing was touched: the handle steps as one that was never asked
        twin = _engine(f, vertical=vertical)
        e.step(1, 3); twin.step(1, 3)
        assert same_bits(e.download_tracers()["q"], twin.download_tracers()["q"])
        assert e.info("tracer_vmix_launches") == (3 if vertical else 0)
        # a huge kappa_v passes: there is no cap
        e.set_tracer_vertical_mixing(1.0e12)
        assert e.info("tracer_vmixing") == 1
        e.step(4, 2)
        assert np.isfinite(e.download_tracers()["q"]).all()
        e.close(); twin.close()
    g = Golden("stommel_24x16")
    one = capi.Engine(_fields(g))
    assert one.p.nlay == 1
    one.set_tracers(1)
    _refused(lambda: one.set_tracer_vertical_mixing(1.0), -3, "nlay = 1")
    one.set_tracer_vertical_mixing(None)                       # (switching off what is off is allowed on any handle with tracers)
    assert one.info("tracer_vmixing") == 0
    one.close()


def test_rings_and_rank_local_handles_are_refused():
    ring = capi.MultiEngine(_big_case("jet_xyper_2l"), devices=(0, 0))
    assert ring.describe()["ring"] == 1
    _refused(lambda: ring.set_tracer_vertical_mixing(1.0), -6, "bands of a frame periodic in y")
    ring.close()
    from beom_amd import slab
    recipe = I.recipe_headline(150, 131, 3)
    fw, _, orphan = slab.build_band(recipe, 1, 0)
    band = capi.BandEngine(fw, recipe.p, 1, 0, device=0, rccl_id=None, orphan=orphan)
    _refused(lambda: band.set_tracer_vertical_mixing(1.0), -6, "a handle that holds one band's window")
    band.close()
    many = _many(_big_case("closed_3l"), 2, 1, vertical=False)
    _refused(lambda: many.set_tracer_vertical_mixing(-1.0), -3, "bands: kappa_v < 0")
    assert many.info("tracer_vmixing") == 0
    many.close()


@pytest.mark.parametrize("name", ["closed_3l", "sill_sponges"])
def test_switched_off_leaves_the_step_as_it_was(name):
    f = _big_case(name)
    never, off = _engine(f, vertical=False), _engine(f)
    off.step(1, 2)
    assert off.info("tracer_vmix_launches") == 2
    off.set_tracer_vertical_mixing(None)
    assert off.info("tracer_vmixing") == 0
    with pytest.raises(capi.BeomError):
        off.update_tracer_vertical_mixing()
    off.set_tracer_vertical_mixing(_kappa_v(f.p))
    off.set_tracer_vertical_mixing(np.zeros((NTRC, f.p.nlay - 1)))          # all zero: off as well
    assert off.info("tracer_vmixing") == 0
    # the twin makes the same two steps (tracers are passive: the same state), takes over the mixed tracers, and never sets
    # the vertical mixing
    never.step(1, 2)
    tr = off.download_tracers()
    never.upload_tracers(q=tr["q"], rq=tr["rq"])
    never.step(3, 10); off.step(3, 10)
    assert off.info("tracer_vmix_launches") == 2 and never.info("tracer_vmix_launches") == 0
    a, b = never.download(), off.download()
    for k in _live(never, STATE):
        assert same_bits(a[k], b[k]), (name, k)
    ta, tb = never.download_tracers(), off.download_tracers()
    assert same_bits(ta["q"], tb["q"]) and same_bits(ta["rq"], tb["rq"]), name
    never.close(); off.close()


def test_another_tracer_count_drops_it_and_the_same_count_keeps_it():
    f = _big_case("closed_3l")
    e = _engine(f)
    q, rq, ctrg = _tracers3(f)
    e.upload_tracers(q=q, rq=rq, ctrg=ctrg)                    # uploads leave it alone
    assert e.info("tracer_vmixing") == 1
    e.set_tracers(NTRC)
    assert e.info("tracer_vmixing") == 1 and e.info("tracer_mixing") == 1
    e.set_tracers(NTRC - 1)
    assert e.info("tracer_vmixing") == 0 and e.info("tracer_mixing") == 0
    e.set_concentration(0.5)
    e.step(1, 2)
    assert e.info("tracer_vmix_launches") == 0
    e.set_tracer_vertical_mixing(_kappa_v(f.p, NTRC - 1))
    e.step(3, 2)
    assert e.info("tracer_vmixing") == 1 and e.info("tracer_vmix_launches") == 2
    e.close()
