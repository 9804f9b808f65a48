"""The two tile geometries of the tiled sweeps (k_mont_visc, k_uv_fused, k_uv_fused_sf) against the oracle, and columns of
more than 8 layers.

beom_engine.hip instantiates both sweeps for 64 x 8 tiles (two rows per thread, Q = 2) and for 64 x 4 tiles (one row per
thread, Q = 1) and picks 64 x 4 for every frame of at most 5000 tiles of 64 x 8, so that small frames would otherwise only
ever meet one of them.  Here BEOM_TILE4 (read when a handle is created) forces each geometry in turn on frames around the
tile thresholds of both, with every boundary configuration, with every layer count of the fused Montgomery sweep, in every
scheduling regime of TileMap (beom_dev.h), and at the README's land figure, where the engine picks 64 x 8 on its own.
Above 8 layers the engine runs per-layer Montgomery and viscosity launches next to the fused u+v sweep.

"vs oracle": after the steps, the state equals oracle_lib.Oracle on the same inputs (numeric equality; a tidal term calls
the device cos(): COS_TOL there), so do mont and pvor of the last layer, and the 64 x 4 and 64 x 8 runs of a case equal each
other bit for bit, the sign of zero included.  Twelve steps cover the rebuild of steps 1-3, both u/v orders and, where
dt3d > 0, a refresh of the viscosity."""
import importlib.util
import os

import numpy as np
import pytest

import oracle_lib
from beom_amd import capi, inputs as I
from beom_amd.grid import read_input_data
from helpers import STATE, land_mask, maxrel, same, same_bits, tile_geometry
from test_gpu_parity import COS_TOL, PROGNOSTIC, _fuses, _live

pytestmark = pytest.mark.gpu
PROG8 = ("hlay", "u", "v", "h_u", "h_v", "rs_h", "dmdx", "dmdy")


def _make_golden():
    spec = importlib.util.spec_from_file_location(
        "make_golden", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(autouse=True)
def _no_geometry_leak():
    before = os.environ.get("BEOM_TILE4")
    yield
    assert os.environ.get("BEOM_TILE4") == before


def _with_land(pf, ragged=True):
    p, files = pf
    files = {k: np.array(v, dtype=np.float64) for k, v in files.items()}
    if "h_bo" not in files:                                  # the default flat depth (:121), as a file
        files["h_bo"] = np.zeros((p.lm + 2, p.mm + 2))
        files["h_bo"][1:-1, 1:-1] = float(p.cext) ** 2 / float(p.grav)
    land = land_mask(p, ragged)
    files["h_bo"][land] = 0.0
    if "init" in files:
        files["init"][land] = 0.0
    return p.replace(ndeg=I.get_nbr_deg_freedom(files["h_bo"])), files


def _sponge(lm, mm, npts=6):
    """wave_sponge.m's recipe (inputs.case_wave_sponge) on a frame of exactly lm x mm cells, open boundaries with the
    original treatment (mcbc = 0, no_gradient_obc): flat two-layer basin, a Gaussian mound, relaxation sponges all round."""
    dl, hfla = 10.0e3, 200.0
    cext = np.sqrt(I.GRAV * hfla)
    dt = 0.5 * dl / cext
    h_bo = np.zeros((lm + 2, mm + 2)); h_bo[1:-1, 1:-1] = hfla
    xx = ((np.arange(lm + 2) - 0.5 * (lm + 1)) * dl)[:, None] * np.ones((1, mm + 2))
    yy = np.ones((lm + 2, 1)) * ((np.arange(mm + 2) - 0.5 * (mm + 1)) * dl)[None, :]
    init = np.zeros((lm + 2, mm + 2, 2, 3))
    init[:, :, 0, 0] = np.exp(-(xx ** 2 + yy ** 2) / (5.0 * dl) ** 2)
    one = np.ones((lm + 2, mm + 2))
    ce = I._frs_coefficients(lm, lm, npts, dt, cext, dl, True)[:, None] * one
    cw = I._frs_coefficients(lm, lm, npts, dt, cext, dl, False)[:, None] * one
    cn = I._frs_coefficients(mm, mm, npts, dt, cext, dl, True)[None, :] * one
    cs = I._frs_coefficients(mm, mm, npts, dt, cext, dl, False)[None, :] * one
    nudg = np.stack([np.maximum.reduce([ce, cw, cn, cs]), np.maximum(ce, cw), np.maximum(cn, cs)], axis=2)
    p = I.make_params(lm, mm, 2, I.get_nbr_deg_freedom(h_bo), dl, cext, 1.0e-4, [1000.0, 1030.0], [0.0, 0.5],
                      12.2 * dt / 86400.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 10.0, 10.0, 1.0, 1.0,
                      0.0, 0.0, 0.0, 0.0, 0.0, 0.0, desc="wave sponge, mcbc = 0", mcbc="0.")
    return p, {"h_bo": h_bo, "init": init, "nudg": nudg}


CONFIGS = {       # name: (lm, mm) -> (params, files, variant)
    "closed_leith": lambda lm, mm: I.case_headline(lm, mm, 2) + (0,),
    "beach_zero_visc_ocrp": lambda lm, mm: I.case_carrier_beach(lm=lm, mm=mm, nlay=2, dt_s=0.08) + (0,),
    "soliton_xper": lambda lm, mm: I.case_soliton(lm=lm, mm=mm, dt_s=5.0) + (0,),
    "jet_xyper": lambda lm, mm: I.case_unstable_jet(lm=lm, mm=mm, nlay=2, dt_s=1.5) + (0,),
    "sill_ocrp_nudged": lambda lm, mm: I.case_sill_exchange3d(lm=lm, mm=mm, nlay=3, dt_s=0.01, npts=5,
                                                              sill_halfwidth=max(3.0, mm / 6.0)) + (0,),
    "stommel_wind_drag": lambda lm, mm: I.case_stommel(lm=lm, mm=mm, dl=50.0e3, dt_s=0.2) + (0,),
    "island_ragged_coast": lambda lm, mm: _with_land(I.case_headline(lm, mm, 3)) + (0,),
    "sponge_mcbc0": lambda lm, mm: _sponge(lm, mm) + (0,),
    "tide_sponge": lambda lm, mm: _make_golden().case_tide(lm, mm) + (0,),
    "variant3d_3l": lambda lm, mm: _make_golden().case_3d_variant(lm, mm) + (1,),
}


def _run_both(p, files, nsteps, variant=0, dense_hint=1, per_layer_scratch=True, embedded=None):
    """Both geometries vs oracle and vs each other; returns the 64 x 8 handle's state."""
    f = read_input_data(p, files=files)
    exact = "tide" not in files
    o = oracle_lib.Oracle(f, variant=variant, per_layer_scratch=per_layer_scratch)
    o.step(1, nsteps)
    ost = o.state()
    runs = {}
    for rows in (4, 8):
        with tile_geometry(rows):
            e = capi.Engine(f, variant=variant, dense_hint=dense_hint)
        assert e.info("tile_rows") == (rows if e.is_dense else 0)
        assert e.is_dense == (dense_hint == 1)
        if embedded is not None:
            assert e.is_embedded == embedded
        e.step(1, nsteps)
        st = e.download()
        keys = _live(e, PROGNOSTIC if (e.is_dense and _fuses(p)) else STATE)
        for k in keys:
            if exact:
                assert same(st[k], ost[k]), (rows, k, maxrel(st[k], ost[k]))
            else:
                assert maxrel(st[k], ost[k]) <= COS_TOL, (rows, k, maxrel(st[k], ost[k]))
        sc = e.download_scratch()
        for k in ("mont", "pvor"):
            if exact:
                assert same(sc[k][p.nlay - 1], o.a[k]), (rows, k)
            else:
                assert maxrel(sc[k][p.nlay - 1], o.a[k]) <= COS_TOL, (rows, k)
        runs[rows] = {k: st[k] for k in PROG8}
        e.close()
    for k in PROG8:
        assert same_bits(runs[4][k], runs[8][k]), ("64 x 4 vs 64 x 8", k)
    assert np.isfinite(runs[8]["hlay"]).all()
    return runs[8]


# (lm, mm); L = lm + 1, M = mm + 1.  A tile is interior for L >= 131, M >= 2 TY + 3, deep for L >= 259 and M >= 35 (64 x 8)
# or M >= 19 (64 x 4).
FRAMES = {
    "129x17": (129, 17),      # 64 x 8: no interior tile
    "130x18": (130, 18),      # 64 x 8: exactly one interior tile row
    "257x33": (257, 33),      # 64 x 8: no deep tile
    "258x34": (258, 34),      # 64 x 8: the first deep tile
    "191x24": (191, 24),      # L % 64 == 0, M % 8 == 1: the last tile row holds one row
    "192x30": (192, 30),      # L % 64 == 1 (a pitch padding of 15), M % 8 == 7
    "63x7": (63, 7),          # one tile
}
CASES_3A = ([("closed_leith", fr) for fr in FRAMES]
            + [(c, fr) for c in CONFIGS if c != "closed_leith" for fr in ("130x18", "258x34", "191x24")])


@pytest.mark.parametrize("config,frame", CASES_3A)
def test_frames_at_the_tile_thresholds(config, frame):
    lm, mm = FRAMES[frame]
    p, files, variant = CONFIGS[config](lm, mm)
    assert (p.lm, p.mm) == (lm, mm)
    _run_both(p, files, 12, variant=variant, embedded=(config == "island_ragged_coast"))


@pytest.mark.parametrize("leith", [True, False], ids=["leith", "standing_visc"])
@pytest.mark.parametrize("nlay", range(1, 9))
def test_every_mont_visc_instantiation(nlay, leith):
    """k_mont_visc<Q, NL, LEITH> for NL = 1..8 in both geometries on a frame with deep tiles and a ragged M in both (M = 41:
    M % 8 == 1, M % 4 == 1).  Without Leith (dvis = 0) v_cc, v_ll stand at bvis after step 3."""
    p, files = I.case_headline(258, 40, nlay, dvis=0.2 if leith else 0.0)
    if not leith:
        p = p.replace(bvis="5.")
    assert (float(p.dvis) > 1e-3) == leith
    _run_both(p, files, 12)


def _tilemap_regime(L, M, TY, TX=64):
    """TileMap's choice (beom_dev.h) for a whole frame: "rim_first", "by_tiles" or "rows"."""
    gx, total = (L + TX - 1) // TX, (M + TY - 1) // TY
    nt, rpx = total * gx, (total + 7) // 8
    if nt <= 4096:
        return "rim_first"
    return "by_tiles" if (rpx * 8 - total) * 100 > 3 * total else "rows"


@pytest.mark.parametrize("lm,mm,regimes", [(8191, 263, ("by_tiles", "by_tiles")), (4095, 263, ("by_tiles", "rim_first")),
                                           (2999, 700, ("rows", "rows"))])
def test_scheduling_regimes(lm, mm, regimes):
    """Each TileMap regime in each geometry: (regime of 64 x 4, regime of 64 x 8)."""
    assert (_tilemap_regime(lm + 1, mm + 1, 4), _tilemap_regime(lm + 1, mm + 1, 8)) == regimes
    p, files = I.case_headline(lm, mm, 2)
    _run_both(p, files, 4, per_layer_scratch=False)


def test_headline_with_land_picks_64x8_and_matches_oracle():
    """The README's land figure (the headline recipe with an island and a ragged coast: the embedded path) at 2047^2 x 2,
    in the geometry the engine picks on its own."""
    assert "BEOM_TILE4" not in os.environ
    p, files = _with_land(I.case_headline(2047, 2047, 2))
    assert p.ndeg <= 0.95 * (p.lm + 1) * (p.mm + 1)
    f = read_input_data(p, files=files)
    del files
    e = capi.Engine(f)
    assert e.is_embedded and e.info("tile_rows") == 8
    o = oracle_lib.Oracle(f, per_layer_scratch=False)
    e.step(1, 6); o.step(1, 6)
    st = e.download(PROG8)
    for k in PROG8:
        assert same(st[k], o.state()[k]), (k, maxrel(st[k], o.state()[k]))
    for k in ("hlay", "u", "v", "h_u", "h_v"):
        assert same_bits(st[k], o.state()[k]), (k, "sign of zero")
    sc = e.download_scratch()
    for k in ("mont", "pvor"):
        assert same(sc[k][p.nlay - 1], o.a[k]), k
    e.close()


@pytest.mark.parametrize("nlay", [9, 12, 16])
def test_deep_columns_dense_table_and_embedded(nlay):
    """More than 8 layers (up to BEOM_MAX_LAYERS): per-layer Montgomery and viscosity launches next to the fused u+v sweep,
    on a ragged dense frame (M = 31: M % 8 == 7, M % 4 == 3) in both geometries, on the table path, and with land."""
    p, files = I.case_headline(191, 30, nlay)
    dense = _run_both(p, files, 12)
    f = read_input_data(p, files=files)
    tab, o = capi.Engine(f, dense_hint=0), oracle_lib.Oracle(f)
    assert not tab.is_dense
    tab.step(1, 12); o.step(1, 12)
    st = tab.download()
    for k in STATE:
        assert same(st[k], o.state()[k]), ("table path", k)
        if k in PROG8:
            assert same(st[k], dense[k]), ("table path vs dense", k)
    tab.close()
    pl, fl = _with_land((p, files))
    _run_both(pl, fl, 12, embedded=True)


@pytest.mark.parametrize("nband", [2, 3])
def test_deep_column_bands_match_single_handle(nband):
    p, files = I.case_headline(150, 131, 12)
    f = read_input_data(p, files=files)
    one, many = capi.Engine(f), capi.MultiEngine(f, devices=[0] * nband)
    assert many.count == nband
    one.step(1, 12); many.step(1, 12)
    a, b = one.download(), many.download()
    for k in PROG8:
        assert same_bits(a[k], b[k]), (nband, k)
    one.close(); many.close()
