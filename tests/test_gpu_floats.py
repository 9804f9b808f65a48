"""Lagrangian floats on the device (beom_set_floats ..., include/beom_hip.h) against the numpy restatement of the scheme
(floats_ref, held to its own conditions by test_floats_cpu): the per-sweep entry on rough velocities and the real steps fed
with the velocities downloaded from the same handle, bit for bit after every step; one call of K steps against K calls; the
track recorder; a handle with floats steps as one without; refusals; the same bits from every handle kind.
Comparisons are helpers.same_bits on x and y and equality of the int32 `rejected`."""
import ctypes as C
import os
import uuid

import numpy as np
import pytest

import floats_ref as R
from beom_amd import capi, inputs as I
from beom_amd.grid import read_input_data
from helpers import STATE, Golden, same_bits, tile_geometry
from test_floats_cpu import CDT, FIXTURES, LAND, NSTEPS, SEED
from test_gpu_biharm_tiled import CASES
from test_gpu_parity import _fields, _live

pytestmark = pytest.mark.gpu
MODES = {"dense_64x4": (1, 4), "dense_64x8": (1, 8), "table": (0, 8)}      # name: (dense_hint, tile rows)
COUNTS = (3, 1000, 4096)                  # fewer than a wave, not a multiple of the block, several blocks
REAL = ("jet_2l_xyper", "island_3l_forced", "sill_4l_ocrp", "variant3d_3l", "rigid_lid_sill_2l")


@pytest.fixture(autouse=True)
def _no_geometry_leak():
    before = os.environ.get("BEOM_TILE4")
    yield
    assert os.environ.get("BEOM_TILE4") == before


# random_coast_2l_xper wraps in x row by row, only where both ends of a row are wet (private_mod.f95:614-640): no offset
# rule on the rectangle gives its links, so the engine keeps it on the table path whatever the hint.  Its "dense" cases run
# all the same (the geometry then changes nothing); island_3l_forced is the land fixture that runs embedded.
NEVER_DENSE = ("random_coast_2l_xper",)


def _engine(g, mode="dense_64x4"):
    dense_hint, rows = MODES[mode]
    with tile_geometry(rows):
        e = capi.Engine(_fields(g), variant=g.variant, dense_hint=dense_hint)
    assert e.is_dense == (bool(dense_hint) and g.name not in NEVER_DENSE), (g.name, mode)
    return e


def _cdt(e):
    """dt * i_dl as the engine forms it: i_dl = 1.0 / dl first."""
    return float(e.prm.dt) * (1.0 / float(e.prm.dl))


def _same_floats(got, x, y, rejected, what):
    assert same_bits(got["x"], x), (what, "x", float(np.max(np.abs(got["x"] - x))))
    assert same_bits(got["y"], y), (what, "y", float(np.max(np.abs(got["y"] - y))))
    assert np.array_equal(got["rejected"], rejected), (what, "rejected")


# ---- the per-sweep entry on rough velocities ----------------------------------------------------------------------------------
_ROUGH = {}


def _rough_reference(name, f, n, cdt):
    """The restatement's run on the rough inputs of test_floats_cpu, once per (fixture, count): the engine's own cdt is a
    property of the fixture, so the velocities are scaled to make cdt x max|u| the 0.9 of the CPU conditions."""
    key = (name, n, cdt)
    if key not in _ROUGH:
        fr = R.Frame(f)
        amp = CDT / cdt
        x, y, layer = R.seed_floats(f, n, SEED)
        steps, rej = [], np.zeros(n, dtype=np.int32)
        x0, y0 = x, y
        for t in range(1, NSTEPS + 1):
            before, after = R.rough_velocities(f, SEED, 2 * t - 1, amp), R.rough_velocities(f, SEED, 2 * t, amp)
            x, y, branch = R.step(fr, before, after, x, y, layer, cdt)
            rej = rej + (branch != 0).astype(np.int32)
            steps.append((before, after, x, y, rej))
        _ROUGH[key] = (x0, y0, layer, steps)
    return _ROUGH[key]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", FIXTURES)
def test_per_sweep_entry_equals_the_restatement(name, mode):
    g = Golden(name)
    e = _engine(g, mode)
    if mode != "table":
        assert e.is_embedded == (name in LAND and name not in NEVER_DENSE), (name, mode)
    f = e.f
    cdt = _cdt(e)
    for n in COUNTS:
        x0, y0, layer, steps = _rough_reference(name, f, n, cdt)
        e.set_floats(x0, y0, layer)
        assert e.info("floats") == n
        got = e.download_floats()
        assert same_bits(got["x"], x0) and same_bits(got["y"], y0) and np.array_equal(got["layer"], layer)
        assert not got["rejected"].any()
        for t, (before, after, x, y, rej) in enumerate(steps, 1):
            e.upload(u=before[0], v=before[1])
            e.update_floats(1)
            e.upload(u=after[0], v=after[1])
            e.update_floats(2)
            _same_floats(e.download_floats(), x, y, rej, (name, mode, n, t))
        if n == COUNTS[-1]:
            assert not same_bits(x, x0)
            if name in LAND:
                assert rej.sum() >= 20, (name, int(rej.sum()))
    e.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_every_landing_branch_on_the_device(mode):
    """The hand-placed floats of floats_ref.corner_floats: each takes another candidate of the landing rule."""
    g = Golden("random_coast_2l_xper")
    e = _engine(g, mode)
    x, y, layer, (u, v), cdt_ref, want = R.corner_floats(e.f)
    cdt = _cdt(e)
    u, v = u * (cdt_ref / cdt), v * (cdt_ref / cdt)
    xn, yn, branch = R.step(R.Frame(e.f), (u, v), (u, v), x, y, layer, cdt)
    assert branch.tolist() == want.tolist()
    e.set_floats(x, y, layer)
    e.upload(u=u, v=v)
    e.update_floats(1)
    e.update_floats(2)
    _same_floats(e.download_floats(), xn, yn, (branch != 0).astype(np.int32), mode)
    e.close()


# ---- real steps -------------------------------------------------------------------------------------------------------------
def _calls(e, calls):
    t = 1
    for k in calls:
        e.step(t, k)
        t += k
    assert t - 1 == NSTEPS


@pytest.mark.parametrize("mode", ["dense_64x4", "table"])
@pytest.mark.parametrize("name", REAL)
def test_real_steps_equal_the_restatement(name, mode):
    """12 steps one at a time with u, v downloaded around each: the restatement fed those velocities equals the device's floats
    after every step; calls of (5, 7) steps give the same bits with 6 + 8 launches instead of 24."""
    g = Golden(name)
    e = _engine(g, mode)
    fr, cdt = R.Frame(e.f), _cdt(e)
    x, y, layer = R.seed_floats(e.f, 1000, SEED)
    x0, y0 = x, y
    rej = np.zeros(x.size, dtype=np.int32)
    e.set_floats(x, y, layer)
    for t in range(1, NSTEPS + 1):
        b = e.download(("u", "v"))
        e.step(t, 1)
        a = e.download(("u", "v"))
        x, y, branch = R.step(fr, (b["u"], b["v"]), (a["u"], a["v"]), x, y, layer, cdt)
        rej = rej + (branch != 0).astype(np.int32)
        _same_floats(e.download_floats(), x, y, rej, (name, mode, t))
    assert np.isfinite(x).all() and np.isfinite(y).all() and fr.wet(x, y).all()
    assert not same_bits(x, x0) and not same_bits(y, y0), (name, "the floats did not move: nothing tested")
    assert e.info("float_launches") == 2 * NSTEPS
    st = e.download()
    e.close()
    k = _engine(g, mode)
    k.set_floats(x0, y0, layer)
    _calls(k, (5, 7))
    _same_floats(k.download_floats(), x, y, rej, (name, mode, "calls of 5 and 7 steps"))
    assert k.info("float_launches") == (5 + 1) + (7 + 1)
    sk = k.download()
    for key in _live(k, STATE):
        assert same_bits(st[key], sk[key]), (name, mode, key)
    k.close()


# ---- the track recorder -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dense_64x4", "table"])
def test_recorder(mode):
    g = Golden("island_3l_forced")
    one = _engine(g, mode)
    fr = R.Frame(one.f)
    x0, y0, layer = R.seed_floats(one.f, 1000, SEED)
    one.set_floats(x0, y0, layer)
    want = {}
    for t in range(1, NSTEPS + 1):
        one.step(t, 1)
        if t % 3 == 0:
            fl = one.download_floats()
            h = one.download(("hlay",))["hlay"]
            want[t] = (fl["x"], fl["y"], h[layer.astype(np.int64) - 1, fr.cell(fl["x"], fl["y"])])
    one.close()
    e = _engine(g, mode)
    e.set_floats(x0, y0, layer, records=4, stride=3)
    assert e.info("float_records") == 0
    e.step(1, NSTEPS)
    assert e.info("float_records") == 4
    # a call that would overflow: refused before anything is launched
    state, floats, launches = e.download(), e.download_floats(), e.info("float_launches")
    with pytest.raises(capi.BeomError) as ei:
        e.step(NSTEPS + 1, 3)
    msg = str(ei.value)
    assert "error -3:" in msg and "beom_download_float_track" in msg, msg
    after, fl = e.download(), e.download_floats()
    for key in STATE:
        assert same_bits(state[key], after[key]), key
    _same_floats(fl, floats["x"], floats["y"], floats["rejected"], "after the refused call")
    assert e.info("float_records") == 4 and e.info("float_launches") == launches
    e.step(NSTEPS + 1, 2)                                            # (steps 13, 14 write no record)
    assert e.info("float_records") == 4
    tr = e.download_float_track()
    assert tr["tstp"].tolist() == [3, 6, 9, 12]
    for k, t in enumerate((3, 6, 9, 12)):
        assert same_bits(tr["x"][k], want[t][0]) and same_bits(tr["y"][k], want[t][1]), (mode, t)
        assert same_bits(tr["h"][k], want[t][2]), (mode, t, "h")
        assert (tr["h"][k] > 0.0).all()
    assert e.info("float_records") == 0
    assert e.download_float_track()["tstp"].size == 0
    e.step(NSTEPS + 3, 1)                                            # step 15: room again
    assert e.download_float_track()["tstp"].tolist() == [15]
    e.close()


# ---- a handle with floats steps as one without ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["jet_2l_xyper", "island_3l_forced", "rigid_lid_sill_2l"])
def test_floats_leave_the_step_as_it_was(name):
    g = Golden(name)
    plain, fl = _engine(g), _engine(g)
    x, y, layer = R.seed_floats(fl.f, 1000, SEED)
    fl.set_floats(x, y, layer, records=2, stride=5)
    _calls(plain, (5, 7)); _calls(fl, (5, 7))
    for what in ("mont_history", "plain_sweeps", "uv_fused", "stress_folded"):
        assert plain.info(what) == fl.info(what), (name, what)
    a, b = plain.download(), fl.download()
    for key in _live(plain, STATE):
        assert same_bits(a[key], b[key]), (name, key)
    assert plain.info("float_launches") == 0 and plain.info("floats") == 0
    fl.set_floats([], [], [])                                        # freed: back to a handle without floats
    assert fl.info("floats") == 0
    plain.step(NSTEPS + 1, 2); fl.step(NSTEPS + 1, 2)
    a, b = plain.download(), fl.download()
    for key in _live(plain, STATE):
        assert same_bits(a[key], b[key]), (name, key, "after the floats were freed")
    plain.close(); fl.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _band_refuses(lib, h, what):
    err = C.create_string_buffer(capi.ERRLEN + 1)
    rc = lib.beom_set_floats(h, 10, 0, 1, err, capi.ERRLEN)
    assert rc == -6 and len(err.value.decode().strip()) > 20, (what, rc, err.value)
    assert lib.beom_info(h, b"floats") == 0


def test_bands_refuse_floats():
    p, files = I.case_headline(150, 131, 3)
    many = capi.MultiEngine(read_input_data(p, files=files), devices=(0, 0))
    assert many.count == 2
    for k in range(2):
        _band_refuses(many.lib, many.band_engine_handle(k), "band %d of a MultiEngine" % k)
    many.close()
    from beom_amd import slab
    recipe = I.recipe_headline(150, 131, 3)
    fw, _, orphan = slab.build_band(recipe, 2, 0)              # band 0 of 2, alone: its exchange looped back over shared memory
    band = capi.BandEngine(fw, recipe.p, 2, 0, device=0, orphan=orphan, loopback=True,
                           shm_name="/beom_floats_%d_%s" % (os.getpid(), uuid.uuid4().hex[:8]))
    _band_refuses(band.lib, band.band_engine_handle(0), "a BandEngine")
    band.close()


def test_bad_floats_are_refused():
    g = Golden("island_3l_forced")
    e = _engine(g)
    fr = R.Frame(e.f)
    x, y, layer = R.seed_floats(e.f, 100, SEED)
    dry = np.flatnonzero(~fr.wetc & (np.arange(fr.n1) > 0))[0]
    cases = {"a dry start": (37, float(fr.i[dry]) - 0.5, None), "outside the frame": (5, -0.5, None),
             "not finite": (7, float("nan"), None), "layer 0": (11, None, 0), "layer nlay + 1": (99, None, e.p.nlay + 1)}
    for what, (k, bad_x, bad_l) in cases.items():
        xb, yb, lb = x.copy(), y.copy(), layer.copy()
        if bad_x is not None:
            xb[k] = bad_x
            if what == "a dry start":
                yb[k] = float(fr.j[dry]) - 0.5
        else:
            lb[k] = bad_l
        with pytest.raises(capi.BeomError) as ei:
            e.set_floats(xb, yb, lb)
        msg = str(ei.value)
        assert "error -3:" in msg and ("float %d " % k) in msg and len(msg.split("error -3:")[1].strip()) > 20, (what, msg)
        assert e.info("floats") == 0
    # the C call leaves the floats the handle holds untouched
    e.set_floats(x, y, layer)
    xb = x.copy(); xb[3] = -1.0
    rc = e.lib.beom_upload_floats(e.h, capi._dp(xb), capi._dp(y), capi._ip(layer), e._err, capi.ERRLEN)
    assert rc == -3
    _same_floats(e.download_floats(), x, y, np.zeros(100, dtype=np.int32), "after a refused upload")
    with pytest.raises(capi.BeomError):
        e.update_floats(3)
    e.close()


# ---- handle kinds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["island_ragged_3l", "jet_xyper_2l"])
def test_handle_kinds_give_the_same_bits(name):
    """Frames of several tiles and blocks: 4096 floats after 12 real steps on the dense (embedded, where the frame has land)
    handle in both tile geometries and on the table path."""
    p, files = CASES[name][0]()
    f = read_input_data(p.replace(svis="0."), files=files)
    x, y, layer = R.seed_floats(f, 4096, SEED)
    got = {}
    for mode, (dense_hint, rows) in MODES.items():
        with tile_geometry(rows):
            e = capi.Engine(f, dense_hint=dense_hint)
        assert e.is_dense == bool(dense_hint) and (not dense_hint or e.is_embedded == CASES[name][1])
        e.set_floats(x, y, layer)
        _calls(e, (5, 7))
        got[mode] = e.download_floats()
        e.close()
    ref = got["table"]
    assert not same_bits(ref["x"], x) and not same_bits(ref["y"], y)
    for mode in ("dense_64x4", "dense_64x8"):
        _same_floats(got[mode], ref["x"], ref["y"], ref["rejected"], (name, mode))
