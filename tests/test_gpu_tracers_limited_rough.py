"""The flux-limited tracer scheme (scheme 2) on the device, on rough states: the first frames that have both interior tiles
(the staged body of k_tracers_lim: two LDS images with a ring of two, a nine-bit wet mask per cell, a loop over tracers with
barriers between them) and inputs on which that body's branches differ — dry cells inside the tiles and in their rings,
transports of either sign at every face, 1, 3 and 8 tracers, 12 layers, hdot, nudging, the tide, a band's edge tiles.
test_tracers_limited_rough_cpu holds the inputs to that (every outer-ring read in every layer, with a non-zero limiter and
with the ring cell the only dry one) and the restatement to a scalar form written on its own.

a. the sweep on its own with dry cells (beom_update_tracers in front of beom_update_h, no dynamics), every handle kind;
b. plan B (steps 7-12, one at a time) on rough states without dry cells — the dynamics divide by the thickness;
c. 2 and 3 bands against the single handle.
Every step is compared with tracers_limited_ref.update fed with the handle's own hlay, h_u, h_v of that step: helpers.same
on finite values (and same_bits between handle kinds); the one tidal configuration to the project's COS_TOL."""
import hashlib
import os

import numpy as np
import pytest

import rough_inputs as RI
import tracers_limited_ref as TL
import tracers_ref as T
from beom_amd import capi
from helpers import maxrel, same, same_bits, tile_geometry
from test_gpu_parity import COS_TOL
from test_gpu_rough_inputs import CALLS_B, _engine as _rough_engine, _exact, _finite_same, _keys, _rough
from test_tracers_limited_rough_cpu import SEED_STATE, SEED_TRACERS, interior_tiles, nudged_inside, regular_tiles

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_geometry_leak():
    before = os.environ.get("BEOM_TILE4")
    yield
    assert os.environ.get("BEOM_TILE4") == before


# ---- the restatement, once per input ------------------------------------------------------------------------------------------
_MEMO = {}


def _restated(key, g, st, q, rq, ctrg, scalars, scheme):
    """TL.update(scheme) of these very inputs: handle kinds and tile geometries that reach the same state share the result.
    key names g and ctrg; the arrays that change from step to step are told apart by their bytes."""
    h = hashlib.sha1()
    for a in (st["hlay"], st["h_u"], st["h_v"], q, rq):
        h.update(np.ascontiguousarray(a, dtype=np.float64).data)
    k = (key, scheme, scalars, h.hexdigest())
    if k not in _MEMO:
        while len(_MEMO) >= 14:
            _MEMO.pop(next(iter(_MEMO)))
        _MEMO[k] = TL.update(g, st["hlay"], st["h_u"], st["h_v"], q, rq, ctrg, *scalars, scheme=scheme)
    return _MEMO[k]


def _tiles(g, e, rows):
    """The interior tiles of a single dense or embedded handle on the whole frame, by the restated condition."""
    reg = regular_tiles(g) if e.is_embedded else None
    return interior_tiles(g.p.lm + 1, g.p.mm + 1, rows, regular=reg)


# ---- a. the sweep on its own, with dry cells -------------------------------------------------------------------------------------
_STATES, _SWEPT = {}, {}


def _dry_case(config, frame, pick):
    key = (config, frame, pick)
    if key not in _STATES:
        g = RI.dry_cell_state(RI.base_fields(config, frame), SEED_STATE)
        q, rq, ctrg = RI.rough_tracers(g, g.hlay, 8, SEED_TRACERS)
        if pick == "one":                                  # a single rough tracer: the one the CPU conditions are stated on
            q, rq, ctrg = (np.ascontiguousarray(a[1:2]) for a in (q, rq, ctrg))
        _STATES[key] = (g, q, rq, ctrg)
    return _STATES[key]


def _swept(config, frame, kind, rows, pick="eight"):
    """Three sweeps (steps 7, 8, 9) of one handle against the restatement; (q, rq) after the last, kept per handle."""
    key = (config, frame, kind, rows, pick)
    if key in _SWEPT:
        return _SWEPT[key]
    what = key
    g, q, rq, ctrg = _dry_case(config, frame, pick)
    q0 = q
    ntrc = q.shape[0]
    if kind == "table":
        e = capi.Engine(g, dense_hint=0)
        assert not e.is_dense
    else:
        with tile_geometry(rows):
            e = capi.Engine(g, dense_hint=1)
        assert e.is_dense and bool(e.is_embedded) == (kind == "embedded") and e.info("tile_rows") == rows, what
        ntiles = len(_tiles(g, e, rows))
        if frame == "321x50":
            assert ntiles >= 1, what + ("no interior tile: the staged body would not run",)
        else:
            assert ntiles == 0, what + ("meant to be all edge tiles",)
    e.set_tracer_scheme(2)
    e.set_tracers(ntrc)
    assert e.info("tracer_scheme") == 2 and e.info("tracers") == ntrc
    e.upload_tracers(q=q, rq=rq, ctrg=ctrg)
    q1, rq1 = q, rq                                          # scheme 1 on the same inputs, restated
    withdrawn = g.dry & (g.hdot < 0.0) if g.has.get("hdot", False) else np.zeros(g.dry.shape, bool)
    for tstp in (7, 8, 9):
        scalars = T.step_scalars(g.p, tstp)
        st = e.download(("hlay", "h_u", "h_v"))
        assert same_bits(st["h_u"], g.h_u) and same_bits(st["h_v"], g.h_v)
        q, rq = _restated((config, frame, pick), g, st, q, rq, ctrg, scalars, 2)
        q1, rq1 = _restated((config, frame, pick), g, st, q1, rq1, ctrg, scalars, 1)
        e.update_tracers(*scalars)
        e.update_h(*scalars)
        e.sync()
        got = e.download_tracers()
        assert _finite_same(got["q"], q), what + (tstp, "q", maxrel(got["q"], q))
        assert _finite_same(got["rq"], rq), what + (tstp, "rq", maxrel(got["rq"], rq))
        if pick == "eight" and not withdrawn.any():
            h = e.download(("hlay",))["hlay"]
            assert _finite_same(got["q"][0][:, 1:], h[:, 1:]), what + (tstp, "q of the uniform tracer vs hlay")
        elif pick == "eight" and tstp == 7:
            # hdot < 0 in an empty cell takes thickness but, by the contract, content at the local concentration +0: the
            # identity holds everywhere else after the first sweep, and spreads from those cells afterwards
            h = e.download(("hlay",))["hlay"]
            assert not same(got["q"][0][withdrawn], h[withdrawn]), what
            keep = ~withdrawn[:, 1:]
            assert _finite_same(got["q"][0][:, 1:][keep], h[:, 1:][keep]), what + (tstp, "q of the uniform tracer vs hlay")
    for t in range(0 if pick == "one" else 1, ntrc):
        assert not same(got["q"][t], q0[t]), what + (t, "the tracer did not move")
        assert not same(got["q"][t], q1[t]), what + (t, "scheme 2 gave what scheme 1 gives: nothing tested")
    e.close()
    _SWEPT[key] = (got["q"], got["rq"])
    return _SWEPT[key]


def _dense_config(frame):
    return "zero_visc_2l" if frame == "4200x9" else "closed_leith_3l"


SWEEP_FRAMES = ("321x50", "130x18", "4200x9")
SWEEPS = [(cfg, frame, kind, rows) for frame in SWEEP_FRAMES
          for cfg, kinds in ((_dense_config(frame), ("dense", "table")), ("island_ragged_3l", ("embedded", "table")))
          for kind in kinds for rows in ((0,) if kind == "table" else (4, 8))]


@pytest.mark.parametrize("config,frame,kind,rows", SWEEPS)
def test_sweep_on_its_own_with_dry_cells(config, frame, kind, rows):
    """test_gpu_rough_inputs.test_tracer_sweep_on_its_own_with_dry_cells under scheme 2: 8 tracers on a state with empty
    cells away from coasts and transports of either sign beside them.  130 x 18 and 4200 x 9 (66 tile columns) are all edge
    tiles; 321 x 50 has interior tiles, with dry cells inside them and in their rings."""
    if frame == "4200x9":
        assert (RI.FRAMES[frame][0] + 1 + 63) // 64 == 66
    _swept(config, frame, kind, rows)


@pytest.mark.parametrize("config,frame", sorted({(c, f) for c, f, _, _ in SWEEPS}))
def test_handle_kinds_give_the_same_bits_on_dry_cell_states(config, frame):
    """The tiled handle of both geometries (dense, or embedded where the frame has land) and the table path, the sign of
    zero included."""
    tiled = "embedded" if config == "island_ragged_3l" else "dense"
    a = _swept(config, frame, "table", 0)
    for rows in (4, 8):
        b = _swept(config, frame, tiled, rows)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), (config, frame, tiled, rows, "vs the table path")


@pytest.mark.parametrize("rows", [4, 8])
def test_single_tracer_with_dry_cells(rows):
    """ntrc = 1: the staged loop over tracers runs once, without its barrier in front of the re-staging."""
    _swept("closed_leith_3l", "321x50", "dense", rows, pick="one")


@pytest.mark.parametrize("rows", [4, 8])
def test_twelve_layers_hdot_and_eight_tracers_with_dry_cells(rows):
    """closed_12l_hdot: the hdot source (ctrg where hdot > 0, the local concentration elsewhere: want_ctrg without nudging),
    12 layers in the launch's y dimension, 8 tracers through the staged loop."""
    g = _dry_case("closed_12l_hdot", "321x50", "eight")[0]
    assert g.p.nlay == 12 and np.any(g.hdot > 0.0) and np.any(g.hdot < 0.0) and not np.any(g.nudg != 0.0)
    _swept("closed_12l_hdot", "321x50", "dense", rows)


# ---- b. plan B steps on rough states -----------------------------------------------------------------------------------------
# 321 x 51: the sill's northern sponge lies inside an interior 64 x 8 tile (on 321 x 50 only the 64 x 4 tiles reach a sponge)
PLAN_B = [("sill_ocrp_sponge_3l", 1, "321x50"), ("sill_ocrp_sponge_3l", 1, "321x51"), ("jet_xyper_2l", 3, "321x50"),
          ("closed_12l_hdot", 8, "321x50"), ("tide_sponge_2l", 2, "321x50")]


def _plan_b_tracers(g, ntrc):
    """ntrc tracers; a single one is a rough one (the uniform tracer never reaches the limiter), otherwise tracer 0 is uniform."""
    if ntrc == 1:
        return tuple(np.ascontiguousarray(a[1:2]) for a in RI.rough_tracers(g, g.hlay, 2, 7))
    return RI.rough_tracers(g, g.hlay, ntrc, 7)


def _plain_state(config, frame, rows):
    """The state of a handle without tracers after steps 7-12 taken one at a time."""
    e = _rough_engine(_rough(config, frame), config, rows)
    for tstp in range(7, 13):
        e.step(tstp, 1)
    st = e.download()
    e.close()
    return st


@pytest.mark.parametrize("rows", [4, 8])
@pytest.mark.parametrize("config,ntrc,frame", PLAN_B)
def test_plan_b_steps_on_rough_states(config, ntrc, frame, rows):
    g = _rough(config, frame)
    exact = _exact(g)
    assert exact == (config != "tide_sponge_2l")
    what = (config, ntrc, frame, rows)
    e = _rough_engine(g, config, rows)
    assert e.is_dense and not e.is_embedded
    assert len(_tiles(g, e, rows)) == {("321x50", 4): 30, ("321x50", 8): 12, ("321x51", 4): 33, ("321x51", 8): 15}[(frame, rows)]
    if config == "sill_ocrp_sponge_3l" and (frame, rows) != ("321x50", 8):
        nudged, cells = nudged_inside(g, rows)
        assert 1 <= nudged < cells, what + ("no nudged cell inside an interior tile",)
    e.set_tracer_scheme(2)
    q, rq, ctrg = _plan_b_tracers(g, ntrc)
    q0 = q
    e.set_tracers(ntrc)
    assert e.info("tracers") == ntrc and e.info("tracer_scheme") == 2
    e.upload_tracers(q=q, rq=rq, ctrg=ctrg)
    q1, rq1 = q, rq
    for tstp in range(7, 13):
        st = e.download(("hlay", "h_u", "h_v"))
        scalars = T.step_scalars(g.p, tstp)
        q, rq = _restated((config, frame, ntrc, "rough"), g, st, q, rq, ctrg, scalars, 2)
        if exact:
            q1, rq1 = _restated((config, frame, ntrc, "rough"), g, st, q1, rq1, ctrg, scalars, 1)
        e.step(tstp, 1)
        got = e.download_tracers()
        if exact:
            assert _finite_same(got["q"], q), what + (tstp, "q", maxrel(got["q"], q))
            assert _finite_same(got["rq"], rq), what + (tstp, "rq", maxrel(got["rq"], rq))
        else:
            assert np.isfinite(got["q"]).all() and np.isfinite(got["rq"]).all()
            print("%s step %d: maxrel q %.3g rq %.3g" % (what, tstp, maxrel(got["q"], q), maxrel(got["rq"], rq)))
            assert maxrel(got["q"], q) <= COS_TOL, what + (tstp, "q", maxrel(got["q"], q))
            assert maxrel(got["rq"], rq) <= COS_TOL, what + (tstp, "rq", maxrel(got["rq"], rq))
            q, rq = got["q"], got["rq"]                      # (the next step is judged on its own)
    for t in range(0 if ntrc == 1 else 1, ntrc):
        assert not same(got["q"][t], q0[t]), what + (t, "the tracer did not move")
        if exact:
            assert not same(got["q"][t], q1[t]), what + (t, "scheme 2 gave what scheme 1 gives: nothing tested")
    st, plain = e.download(), _plain_state(config, frame, rows)
    for k in _keys(e, g.p):
        assert same_bits(st[k], plain[k]), what + (k, "the tracers changed the state")
    e.close()


# ---- c. bands ------------------------------------------------------------------------------------------------------------------
def _plan_b_calls(x):
    t = 7
    for n in CALLS_B:
        x.step(t, n)
        t += n
    return x.download_tracers()


@pytest.mark.parametrize("rows", [4, 8])
@pytest.mark.parametrize("config,frame", [("closed_leith_3l", "321x50"), ("closed_leith_3l", "321x83"), ("island_ragged_3l", "321x83")])
def test_bands_give_the_single_handles_bits(config, frame, rows):
    """2 and 3 bands under scheme 2 with 8 tracers on a rough state, every band's window with an interior tile of its own
    beside its edge tiles, whose ring of two reaches into the ghost rows.  A band's step is cut around the exchange only in a
    window of at least 32 rows (beom_step_phase): on 321 x 50 no window has them and every step runs whole, on 321 x 83
    steps are cut; and the island's ragged corner leaves band 0 of 3 without an interior tile on 321 x 50."""
    g = _rough(config, frame)
    p = g.p
    q, rq, ctrg = RI.rough_tracers(g, g.hlay, 8, 9)
    with tile_geometry(rows):
        one = capi.Engine(g)
    assert one.is_dense and bool(one.is_embedded) == (config == "island_ragged_3l") and one.info("tile_rows") == rows
    one.set_tracer_scheme(2)
    one.set_tracers(8)
    one.upload_tracers(q=q, rq=rq, ctrg=ctrg)
    a = _plan_b_calls(one)
    one.close()
    assert np.isfinite(a["q"]).all() and np.isfinite(a["rq"]).all() and not same(a["q"][1:], q[1:])
    for nb in (2, 3):
        with tile_geometry(rows):
            many = capi.MultiEngine(g, devices=[0] * nb)
        assert many.count == nb and many.info("tile_rows") == rows
        cut = False
        for k in range(nb):
            b = many.band(k)
            hk = many.band_engine_handle(k)
            assert many.lib.beom_info(hk, b"tile_rows") == rows
            win = (b["win0"], b["win1"])
            assert 1 <= win[0] <= b["own0"] <= b["own1"] <= win[1] <= p.mm + 1, b
            cut = cut or win[1] - win[0] + 1 >= 32
            reg = regular_tiles(g, win) if many.lib.beom_is_dense(hk) == 2 else None
            tiles = interior_tiles(p.lm + 1, win[1] - win[0] + 1, rows, joff=win[0] - 1, Mg=p.mm + 1, regular=reg)
            assert len(tiles) >= 1, (config, frame, rows, nb, k, b, "no interior tile in this band's window")
        many.set_tracer_scheme(2)
        many.set_tracers(8)
        assert many.info("tracer_scheme") == 2
        many.upload_tracers(q=q, rq=rq, ctrg=ctrg)
        c = _plan_b_calls(many)
        assert same_bits(a["q"], c["q"]) and same_bits(a["rq"], c["rq"]), (config, frame, rows, nb, "bands vs the single handle")
        assert cut == (frame == "321x83"), (config, frame, nb, "windows of 32 rows or more")
        assert (many.stats()["split"] > 0) == cut, (config, frame, nb, many.stats(), "cut steps, against the windows' rows")
        many.close()
