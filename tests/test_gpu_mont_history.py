"""The history-from-Montgomery form of the fused u+v sweep (option "mont_history", default on) against the
same handle with the option off and against the oracle: bit for bit over helpers.STATE minus what the fused sweeps do not
keep (v_cc, v_ll; the stress arrays when the stress folds), the sign of zero included.

From step 4 on a dense single-frame handle re-forms the Adams-Bashforth history dmdx / dmdy inside k_uv_fused from three kept
levels of `mont` and leaves the six arrays alone; a download, an upload, a sweep called on its own or a step of another form
first brings the arrays up to date (k_hist_from_mont).  Every case runs 13 steps in uneven calls with downloads in between,
so the arrays are rebuilt several times in mid-run and both u/v orders follow every rebuild."""
import os

import numpy as np
import pytest

import oracle_lib
from beom_amd import capi, inputs as I
from beom_amd.grid import read_input_data
from helpers import STATE, Golden, golden_names, land_mask, same_bits, tile_geometry

pytestmark = pytest.mark.gpu
KEPT = tuple(k for k in STATE if k not in ("v_cc", "v_ll"))       # (the fused Montgomery sweep forms only their products)
CALLS = (3, 1, 2, 1, 4, 2)                                        # 13 steps; a download after every call


@pytest.fixture(autouse=True)
def _no_geometry_leak():
    before = os.environ.get("BEOM_TILE4")
    yield
    assert os.environ.get("BEOM_TILE4") == before


def _with_land(pf):
    p, files = pf
    files = {k: np.array(v, dtype=np.float64) for k, v in files.items()}
    if "h_bo" not in files:
        files["h_bo"] = np.zeros((p.lm + 2, p.mm + 2))
        files["h_bo"][1:-1, 1:-1] = float(p.cext) ** 2 / float(p.grav)
    land = land_mask(p, True)
    files["h_bo"][land] = 0.0
    if "init" in files:
        files["init"][land] = 0.0
    return p.replace(ndeg=I.get_nbr_deg_freedom(files["h_bo"])), files


# name: (lm, mm) -> (params, files); options set on the handle; embedded?
CONFIGS = {
    "closed_leith_3l": (lambda lm, mm: I.case_headline(lm, mm, 3), {}, False),
    "soliton_xper": (lambda lm, mm: I.case_soliton(lm=lm, mm=mm, dt_s=5.0), {}, False),
    "jet_xyper": (lambda lm, mm: I.case_unstable_jet(lm=lm, mm=mm, nlay=2, dt_s=1.5), {}, False),
    "sill_ocrp_nudged": (lambda lm, mm: I.case_sill_exchange3d(lm=lm, mm=mm, nlay=3, dt_s=0.01, npts=5,
                                                               sill_halfwidth=max(3.0, mm / 6.0)), {}, False),
    "beach_zero_visc": (lambda lm, mm: I.case_carrier_beach(lm=lm, mm=mm, nlay=2, dt_s=0.08), {}, False),
    # wind-driven: k_uv_fused_sf stays on the arrays, so the form under test is the one with the stress launched
    "stommel_wind_drag": (lambda lm, mm: I.case_stommel(lm=lm, mm=mm, dl=50.0e3, dt_s=0.2), {"fold_stress": 0}, False),
    "island_ragged_coast": (lambda lm, mm: _with_land(I.case_headline(lm, mm, 3)), {}, True),
}
# 321 x 50: interior, deep and edge tiles in the 64 x 8 geometry (L = 322 >= 259, M = 51 >= 35); 130 x 18: one interior tile row
FRAMES = {"321x50": (321, 50), "130x18": (130, 18)}


def _fields(config, frame):
    make, opts, embedded = CONFIGS[config]
    p, files = make(*FRAMES[frame])
    if float(p.g_fb) == 0.0:
        p = p.replace(g_fb="1.")           # the multistep term is what the form is about
    return read_input_data(p, files=files), opts, embedded


def _engine(f, opts, rows=None, mont_history=1, **kw):
    if rows is None:
        e = capi.Engine(f, **kw)
    else:
        with tile_geometry(rows):
            e = capi.Engine(f, **kw)
        assert e.info("tile_rows") == rows
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_option("mont_history", mont_history)
    return e


def _keys(e):
    return [k for k in KEPT if not (k in ("tt3d", "tb3d", "tu3d") and e.info("stress_folded"))]


def _assert_state(st, ref, keys, what):
    for k in keys:
        assert same_bits(st[k], ref[k]), what + (k, float(np.max(np.abs(st[k] - ref[k]))))


@pytest.mark.parametrize("rows", [4, 8])
@pytest.mark.parametrize("config,frame", [(c, "321x50") for c in CONFIGS] + [("closed_leith_3l", "130x18"), ("jet_xyper", "130x18")])
def test_on_against_off_and_oracle(config, frame, rows):
    f, opts, embedded = _fields(config, frame)
    on, off = _engine(f, opts, rows, 1), _engine(f, opts, rows, 0)
    assert on.is_dense and on.is_embedded == embedded
    o = oracle_lib.Oracle(f)
    t = 0
    for n in CALLS:
        for e in (on, off):
            e.step(t + 1, n)
        o.step(t + 1, n)
        t += n
        assert on.info("uv_fused") == 1
        assert on.info("mont_history") == (1 if t >= 4 else 0), (config, frame, rows, t)
        assert off.info("mont_history") == 0
        a, b = on.download(), off.download()
        _assert_state(a, b, _keys(on), (config, frame, rows, t, "on vs off"))
        _assert_state(a, o.state(), _keys(on), (config, frame, rows, t, "on vs oracle"))
        sa = on.download_scratch()
        assert same_bits(sa["mont"][f.p.nlay - 1], o.a["mont"]), (config, frame, rows, t, "mont")
    assert np.isfinite(a["hlay"]).all()
    on.close(); off.close()


def test_every_step_from_the_fourth_reports_the_form():
    f, opts, _ = _fields("closed_leith_3l", "321x50")
    e = _engine(f, opts)
    for t in range(1, 10):
        e.step(t, 1)
        assert e.info("mont_history") == (1 if t >= 4 else 0), t
    e.close()


def test_not_taken_by_band_lid_unfused_or_without_multistep():
    f, opts, _ = _fields("closed_leith_3l", "321x50")
    many = capi.MultiEngine(f, devices=[0, 0])
    many.step(1, 6)
    assert many.info("mont_history") == 0
    many.close()
    e = _engine(f, opts)
    e.set_option("fuse_uv", 0)
    e.step(1, 6)
    assert e.info("mont_history") == 0
    e.close()
    p, files = CONFIGS["closed_leith_3l"][0](*FRAMES["321x50"])
    e = capi.Engine(read_input_data(p.replace(g_fb="0."), files=files))
    e.step(1, 6)
    assert e.info("mont_history") == 0
    e.close()
    lid = [n for n in golden_names() if float(Golden(n).p.rgld) > 0.5]
    assert lid
    g = Golden(lid[0])
    e = capi.Engine(g.fields())
    e.step(1, 6)
    assert e.info("mont_history") == 0
    e.close()


@pytest.mark.parametrize("config", ["closed_leith_3l", "jet_xyper", "island_ragged_coast"])
def test_upload_in_mid_run(config):
    """An upload breaks the sequence of kept levels: the steps after it run on the uploaded arrays until three new levels
    are there."""
    f, opts, _ = _fields(config, "321x50")
    e, o = _engine(f, opts), oracle_lib.Oracle(f)
    e.step(1, 7); o.step(1, 7)
    assert e.info("mont_history") == 1
    st = e.download()
    _assert_state(st, o.state(), _keys(e), (config, 7, "before the upload"))
    e.upload(**st)                                      # (v_cc, v_ll as the handle holds them)
    seen = []
    for t in range(8, 14):
        e.step(t, 1); o.step(t, 1)
        seen.append(e.info("mont_history"))
    assert seen[:2] == [0, 0] and seen[-1] == 1, seen
    _assert_state(e.download(), o.state(), _keys(e), (config, 13, "after the upload"))
    # a partial upload (one field) keeps the rest of the state, the history arrays included
    e.upload(hlay=np.ascontiguousarray(o.state()["hlay"]))
    e.step(14, 2); o.step(14, 2)
    _assert_state(e.download(), o.state(), _keys(e), (config, 15, "after a partial upload"))
    e.close()


@pytest.mark.parametrize("config", ["closed_leith_3l", "soliton_xper"])
def test_sweeps_called_on_their_own_after_steps_of_the_form(config):
    """beom_update_u / beom_update_v read and shift the history arrays: after steps of the form they must find them up to
    date.  Steps 7 and 8 (both u/v orders) run as the reference's sequence of sweeps, one layer at a time
    (private_mod.f95:2259-2290) — update_u / update_v need the Montgomery and viscosity sweeps of their own step in front of
    them: the fused steps before keep neither v_cc, v_ll nor rvor, dive."""
    f, opts, _ = _fields(config, "321x50")
    e, o = _engine(f, opts), oracle_lib.Oracle(f)
    e.step(1, 6); o.step(1, 6)
    assert e.info("mont_history") == 1
    p = f.p
    gene = float(p.g_fb)
    for tstp in (7, 8):
        ctim = float(getattr(f, "tres", 0.0)) + float(p.dtd8) * tstp
        ramp = ctim / float(p.dt_r) if (float(p.rsta) < 0.5 and ctim < float(p.dt_r)) else 1.0
        upst = tstp % p.n_3d == 0
        for x in (e, o):
            if upst:
                x.distribute_stress()
            x.update_h(gene, ramp, ctim)
        for il in range(1, p.nlay + 1):
            for x in (e, o):
                x.update_mont(il)
                if float(p.dvis) > 1e-3 and upst:
                    x.update_viscosity(il)
            for w in (("u", "v") if tstp % 2 == 0 else ("v", "u")):
                for x in (e, o):
                    getattr(x, "update_" + w)(il, gene, ramp, ctim)
        e.sync()
        _assert_state(e.download(), o.state(), KEPT, (config, tstp, "after the sweeps of a step"))
    e.step(9, 5); o.step(9, 5)                          # three steps on the arrays, then the form again
    assert e.info("mont_history") == 1
    _assert_state(e.download(), o.state(), _keys(e), (config, 13, "steps after the sweeps"))
    e.close()


@pytest.mark.parametrize("rows", [4, 8])
def test_option_toggled_in_mid_run(rows):
    f, opts, _ = _fields("closed_leith_3l", "321x50")
    e, o = _engine(f, opts, rows), oracle_lib.Oracle(f)
    t = 0
    for n, flag in ((5, 1), (2, 0), (1, 1), (3, 0), (2, 1)):
        e.set_option("mont_history", flag)
        e.step(t + 1, n); o.step(t + 1, n)
        t += n
        assert e.info("mont_history") == flag, (t, flag)       # (the levels are kept either way)
    _assert_state(e.download(), o.state(), _keys(e), (rows, t, "toggled"))
    e.set_option("fuse", 0)                                     # the other paths read the arrays
    e.step(t + 1, 2); o.step(t + 1, 2)
    assert e.info("mont_history") == 0
    _assert_state(e.download(), o.state(), KEPT, (rows, t + 2, "unfused after the form"))
    e.close()
