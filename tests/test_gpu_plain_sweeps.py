"""The plain forms of the fused momentum sweep and of the Montgomery sweep (option "plain_sweeps", default 1): instantiations of
k_uv_fused and k_mont_visc with the optional forcing compiled out (uv_core: nudging, tide, stress arrays, body force, lid;
body_mont_visc: outcropping, lid, h_to, keep_diag, keep_visc), picked per launch from the handle's flags of the moment.

info("plain_sweeps") is a bit mask of the last step: 1 = the u+v sweep ran plain, 2 = the Montgomery sweep did.  Only the
staged (PROD) momentum forms have a plain instantiation, so a handle whose viscosity is never refreshed (dvis <= 1e-3) reports
0 in steps 1-3, where update_viscosity runs on its own and neither sweep is the fused one.

Frames: the smallest with interior, deep and edge workgroups (test_gpu_tile_geometry: 258 x 34 has the first deep 64 x 8 tile,
130 x 18 one interior tile row), in both tile geometries, with 2 and 4 layers.  Inputs: the headline recipe as it is, and the
same frame with rough_inputs.rough_fields over it and everything that is a forcing put back to +0 (stress arrays, body force,
h_to), so that nothing else is constant, smooth or zero and the velocities carry exact +-0.  Steps 1-9 in calls of 2, 1, 3, 3:
steps 1-3 run the array forms with gene = 0, steps 4-9 the history-from-Montgomery form in both u/v orders ("mont_history" = 0:
the array forms throughout).  After every call the eight prognostic arrays equal oracle_lib.Oracle bit for bit, the sign of
zero included, and the handle with "plain_sweeps" = 0 (the general instantiations) holds the same bits."""
import copy
import os

import numpy as np
import pytest

import oracle_lib
import rough_inputs as RI
from beom_amd import capi, inputs as I
from beom_amd.grid import read_input_data
from helpers import land_mask, maxrel, same_bits, tile_geometry
from test_gpu_parity import COS_TOL

pytestmark = pytest.mark.gpu
PROG8 = ("hlay", "u", "v", "h_u", "h_v", "rs_h", "dmdx", "dmdy")
CALLS = (2, 1, 3, 3)
UV, MONT = 1, 2                       # the bits of info("plain_sweeps")
FRAMES = {"258x34": (258, 34), "130x18": (130, 18)}
# form: (dvis, bvis, v_cc / v_ll of the rough state)
FORMS = {
    "leith": (0.2, None, "rough"),            # k_mont_visc<.., LEITH = true>, products staged in every step
    "zero_visc": (0.0, None, "zero"),         # dvis = bvis = 0 and v_cc = v_ll = +0: the ZV forms from step 4 on
    "standing_visc": (0.0, "5.", "rough"),    # dvis <= 1e-3: LEITH = false, v_cc = v_ll = bvis stand after step 3
}
_FIELDS, _ORACLE = {}, {}


@pytest.fixture(autouse=True)
def _no_geometry_leak():
    before = os.environ.get("BEOM_TILE4")
    yield
    assert os.environ.get("BEOM_TILE4") == before


def _params_files(lm, mm, nlay, form):
    dvis, bvis, _ = FORMS[form]
    p, files = I.recipe_headline(lm, mm, nlay, dvis=dvis).whole()
    if bvis is not None:
        p = p.replace(bvis=bvis)
    return p, files


def _unforced(g):
    """A rough Fields object without forcing: body force and h_to back to +0 (the stress arrays: rough_fields(zero=...))."""
    g = copy.copy(g)
    g.bodf = np.zeros_like(g.bodf)
    g.h_to = np.zeros_like(g.h_to)
    return g


def _read(lm, mm, nlay, form):
    p, files = _params_files(lm, mm, nlay, form)
    return read_input_data(p, files=files)


def _fields(inputs, frame, nlay, form):
    key = (inputs, frame, nlay, form)
    if key not in _FIELDS:
        f = _read(*FRAMES[frame], nlay, form)
        if inputs == "rough":
            f = _unforced(RI.rough_fields(f, 1, visc=FORMS[form][2], zero=("tt3d", "tb3d", "tu3d")))
        _FIELDS[key] = f
    return _FIELDS[key]


def _snap(o):
    return {k: np.array(o.state()[k], copy=True) for k in PROG8}


def _oracle(inputs, frame, nlay, form):
    """The oracle's state after each call of CALLS, computed once and shared by the geometries and the options."""
    key = (inputs, frame, nlay, form)
    if key not in _ORACLE:
        o = oracle_lib.Oracle(_fields(*key))
        t, res = 1, []
        for n in CALLS:
            o.step(t, n)
            t += n
            res.append(_snap(o))
        assert all(np.isfinite(a).all() for a in res[-1].values())
        _ORACLE[key] = res
    return _ORACLE[key]


def _expect_bits(form, last_step):
    return UV | MONT if (form == "leith" or last_step >= 4) else 0


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("nlay", [2, 4])
@pytest.mark.parametrize("rows", [4, 8])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_plain_runs_against_the_oracle(frame, rows, nlay, form):
    for inputs in ("headline", "rough"):
        f = _fields(inputs, frame, nlay, form)
        ref = _oracle(inputs, frame, nlay, form)
        for mont_history in (1, 0):
            eng = {}
            for plain in (1, 0):
                with tile_geometry(rows):
                    eng[plain] = capi.Engine(f)
                assert eng[plain].info("tile_rows") == rows
                eng[plain].set_option("mont_history", mont_history)
                eng[plain].set_option("plain_sweeps", plain)
            t = 1
            for n, want in zip(CALLS, ref):
                what = (inputs, frame, rows, nlay, form, mont_history, t + n - 1)
                st = {}
                for plain in (1, 0):
                    eng[plain].step(t, n)
                    assert eng[plain].info("plain_sweeps") == (_expect_bits(form, t + n - 1) if plain else 0), what
                    if not mont_history or t + n - 1 < 4:
                        assert eng[plain].info("mont_history") == 0, what
                    elif t + n - 1 == 9:          # steps 7-9: both u/v orders in the history-from-Montgomery form
                        assert eng[plain].info("mont_history") == 1, what
                    st[plain] = eng[plain].download(PROG8)
                t += n
                for k in PROG8:
                    assert same_bits(st[1][k], want[k]), what + (k, "plain vs oracle", maxrel(st[1][k], want[k]))
                    assert same_bits(st[0][k], st[1][k]), what + (k, "plain_sweeps = 0 vs 1")
            for e in eng.values():
                e.close()


# ---- bands and an embedded frame ----------------------------------------------------------------------------------------------
def _table_run(g):
    tab = capi.Engine(g, dense_hint=0)
    assert not tab.is_dense
    out, t = [], 1
    for n in CALLS:
        tab.step(t, n)
        t += n
        out.append(tab.download(PROG8))
    tab.close()
    return out


@pytest.mark.parametrize("nband", [2, 3])
def test_plain_forms_on_bands_match_the_table_path(nband):
    f = _read(130, 99, 2, "leith")
    g = _unforced(RI.rough_fields(f, 1, zero=("tt3d", "tb3d", "tu3d")))
    want = _table_run(g)
    many = capi.MultiEngine(g, devices=[0] * nband)
    assert many.count == nband
    t = 1
    for n, w in zip(CALLS, want):
        many.step(t, n)
        t += n
        assert many.info("plain_sweeps") == UV | MONT, (nband, t - 1)
        st = many.download()
        for k in PROG8:
            assert same_bits(st[k], w[k]), (nband, t - 1, k)
    assert np.isfinite(st["hlay"]).all()
    many.close()


@pytest.mark.parametrize("rows", [4, 8])
def test_plain_forms_on_an_embedded_frame_match_the_table_path(rows):
    p, files = _params_files(258, 34, 2, "leith")
    files = {k: np.array(v, dtype=np.float64) for k, v in files.items()}
    land = land_mask(p, True)
    files["h_bo"][land] = 0.0
    if "init" in files:
        files["init"][land] = 0.0
    f = read_input_data(p.replace(ndeg=I.get_nbr_deg_freedom(files["h_bo"])), files=files)
    g = _unforced(RI.rough_fields(f, 1, zero=("tt3d", "tb3d", "tu3d")))
    want = _table_run(g)
    with tile_geometry(rows):
        e = capi.Engine(g)
    assert e.is_embedded and e.info("tile_rows") == rows
    t = 1
    for n, w in zip(CALLS, want):
        e.step(t, n)
        t += n
        assert e.info("plain_sweeps") == UV | MONT, (rows, t - 1)
        st = e.download(PROG8)
        for k in PROG8:
            assert same_bits(st[k], w[k]), (rows, t - 1, k)
    assert np.isfinite(st["hlay"]).all()
    e.close()


# ---- gating -------------------------------------------------------------------------------------------------------------------
def _rough_headline(nlay=2, **kw):
    f = _read(130, 18, nlay, "leith")
    return RI.rough_fields(f, 1, **dict({"zero": ("tt3d", "tb3d", "tu3d")}, **kw))


def _sponged(tide):
    if tide:
        p, files = RI._tide_sponge(130, 18)
    else:
        p, files = I.case_headline(130, 18, 2)
        files = dict(files, nudg=RI._sponges(p))
    return _unforced(RI.rough_fields(read_input_data(p, files=files), 1, zero=("tt3d", "tb3d", "tu3d")))


def _with_param(**kw):
    p, files = _params_files(130, 18, 2, "leith")
    return read_input_data(p.replace(**kw), files=files)


def _keep(g, name):
    """The unforced rough state with the one forcing `name` left rough."""
    h = _unforced(g)
    setattr(h, name, getattr(g, name))
    return h


GATES = {     # name: (fields, options, bits that must be off, bits that must be on, exact?)
    "sponge": (lambda: _sponged(False), {}, UV, MONT, True),
    "tide": (lambda: _sponged(True), {}, UV, MONT, False),
    "uploaded_stress_unfolded": (lambda: _unforced(_rough_headline(zero=())), {"fold_stress": 0}, UV, MONT, True),
    "body_force": (lambda: _keep(_rough_headline(), "bodf"), {}, UV, MONT, True),
    "svis": (lambda: _with_param(svis="1.e9"), {}, UV, 0, True),
    "ocrp": (lambda: _with_param(ocrp="1."), {}, MONT, UV, True),
    "h_to": (lambda: _keep(_rough_headline(), "h_to"), {}, MONT, UV, True),
    "keep_diag": (lambda: _unforced(_rough_headline()), {"keep_diag": 1}, MONT, UV, True),
}


@pytest.mark.parametrize("gate", list(GATES))
def test_a_forcing_or_a_diagnostic_switches_its_plain_form_off(gate):
    make, opts, off, on, exact = GATES[gate]
    g = make()
    e, o = capi.Engine(g), oracle_lib.Oracle(g)
    for k, v in opts.items():
        e.set_option(k, v)
    for t, n in ((1, 3), (4, 3)):
        e.step(t, n); o.step(t, n)
        bits = e.info("plain_sweeps")
        assert bits & off == 0 and bits & on == on, (gate, t + n - 1, bits)
        assert e.info("stress_folded") == 0, gate
        st = e.download(PROG8)
        for k in PROG8:
            if exact:
                assert same_bits(st[k], o.state()[k]), (gate, t + n - 1, k, maxrel(st[k], o.state()[k]))
            else:
                assert maxrel(st[k], o.state()[k]) <= COS_TOL, (gate, t + n - 1, k, maxrel(st[k], o.state()[k]))
    assert np.isfinite(st["hlay"]).all()
    e.close()


def test_keep_diag_between_two_calls_flips_the_montgomery_bit():
    g = _unforced(_rough_headline())
    e, o = capi.Engine(g), oracle_lib.Oracle(g)
    t = 1
    for n, keep, bits in ((4, 0, UV | MONT), (2, 1, UV), (2, 0, UV | MONT)):
        e.set_option("keep_diag", keep)
        e.step(t, n); o.step(t, n)
        t += n
        assert e.info("plain_sweeps") == bits, (t - 1, keep)
        st = e.download(PROG8)
        for k in PROG8:
            assert same_bits(st[k], o.state()[k]), (t - 1, keep, k)
    e.close()
