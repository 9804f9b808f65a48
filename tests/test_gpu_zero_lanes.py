"""Lanes of the momentum sweeps whose new velocity is an exact zero, on handles whose velocity targets are all +0
(info("vel_targets_zero") = 1): uv_core then takes the target as the literal +0 instead of fetching fnud(:, :, ix_u | ix_v).

Frames: the smallest with interior, deep and edge workgroups (test_gpu_plain_sweeps: 258 x 34, 130 x 18), in both tile
geometries, with 2 and 4 layers.  Input: the headline recipe with the mound narrowed to radius lm / 40, so that most of the
frame is exactly at rest — measured with the oracle, 72-74 % of the cell-layers hold u = v = 0 after step 2 and 60-70 % after
step 9, whole interior and edge tiles of both kinds among them.  The oracle's fraction must lie in [0.5, 0.8] after every
call: a test that has lost its zero lanes fails.  Steps 1-9 in calls of 2, 1, 3, 3 with the forms leith and zero_visc and
"plain_sweeps" 1 and 0; after every call the eight prognostic arrays equal oracle_lib.Oracle bit for bit.  The same runs
with u, v uploaded as -0.0 (the oracle holds +0 in every zero from step 1 on).  A flag that must be cleared (-0.0 targets,
-1.0 in half the frame, one non-zero target in the last slot) reports 0 and the bits still equal the oracle's.  Three bands
of the 258 x 34 frame hold the single handle's bits."""
import copy
import os

import numpy as np
import pytest

import oracle_lib
from beom_amd import capi, inputs as I
from beom_amd.grid import IX_U, IX_V, read_input_data
from helpers import maxrel, same_bits, tile_geometry

pytestmark = pytest.mark.gpu
PROG8 = ("hlay", "u", "v", "h_u", "h_v", "rs_h", "dmdx", "dmdy")
CALLS = (2, 1, 3, 3)
FRAMES = {"258x34": (258, 34), "130x18": (130, 18)}
FORMS = {"leith": 0.2, "zero_visc": 0.0}          # dvis (test_gpu_plain_sweeps.FORMS)
_FIELDS, _ORACLE = {}, {}


@pytest.fixture(autouse=True)
def _no_geometry_leak():
    before = os.environ.get("BEOM_TILE4")
    yield
    assert os.environ.get("BEOM_TILE4") == before


def _narrow_headline(lm, mm, nlay, dvis):
    """recipe_headline with its mound (radius lm / 12) narrowed to lm / 40, through the files dict."""
    p, files = I.recipe_headline(lm, mm, nlay, dvis=dvis).whole()
    x = (np.arange(lm + 2, dtype=np.float64) - 0.5 * (lm + 1))[:, None]
    y = (np.arange(mm + 2, dtype=np.float64) - 0.5 * (mm + 1))[None, :]
    mound = np.exp(-(x * x + y * y) / (lm / 40.0) ** 2).astype(np.float32)
    init = np.zeros_like(files["init"])
    for k in range(nlay):
        init[:, :, k, 0] = mound * np.float32(1.0 - k / nlay)
    return p, dict(files, init=init)


def _fields(frame, nlay, form, start="+0"):
    key = (frame, nlay, form, start)
    if key not in _FIELDS:
        if start == "+0":
            p, files = _narrow_headline(*FRAMES[frame], nlay, FORMS[form])
            f = read_input_data(p, files=files)
            assert not f.fnud[[IX_U, IX_V]].view(np.uint64).any()      # the targets are +0 bit for bit
        else:                                     # the same frame, every cell's velocity a negative zero
            f = copy.copy(_fields(frame, nlay, form))
            f.u, f.v = f.u.copy(), f.v.copy()
            f.u[:, 1:] = -0.0
            f.v[:, 1:] = -0.0
            assert np.signbit(f.u[:, 1:]).all() and np.signbit(f.v[:, 1:]).all()
        _FIELDS[key] = f
    return _FIELDS[key]


def _with_targets(f, change):
    g = copy.copy(f)
    g.fnud = f.fnud.copy()
    change(g.fnud)
    return g


def _snap(o):
    return {k: np.array(o.state()[k], copy=True) for k in PROG8}


def _census(st):
    return float(((st["u"][:, 1:] == 0.0) & (st["v"][:, 1:] == 0.0)).mean())


def _oracle_run(f, census=True):
    o = oracle_lib.Oracle(f)
    t, res = 1, []
    for n in CALLS:
        o.step(t, n)
        t += n
        res.append(_snap(o))
        if census:
            frac = _census(res[-1])
            print("zero lanes after step %d: %.3f" % (t - 1, frac))
            assert 0.5 <= frac <= 0.8, (t - 1, frac)
    assert all(np.isfinite(a).all() for a in res[-1].values())
    return res


def _oracle(*key):
    """The oracle's state after each call of CALLS, computed once and shared by the geometries and the options."""
    if key not in _ORACLE:
        _ORACLE[key] = _oracle_run(_fields(*key))
    return _ORACLE[key]


def _check_against(f, ref, rows, what, flag):
    eng = {}
    for plain in (1, 0):
        with tile_geometry(rows):
            eng[plain] = capi.Engine(f)
        assert eng[plain].info("tile_rows") == rows
        eng[plain].set_option("plain_sweeps", plain)
    t = 1
    for n, want in zip(CALLS, ref):
        for plain in (1, 0):
            eng[plain].step(t, n)
            assert eng[plain].info("vel_targets_zero") == flag, what
            if not plain:
                assert eng[plain].info("plain_sweeps") == 0, what
            st = eng[plain].download(PROG8)
            for k in PROG8:
                assert same_bits(st[k], want[k]), what + (t + n - 1, plain, k, maxrel(st[k], want[k]))
        t += n
    for e in eng.values():
        e.close()


@pytest.mark.parametrize("start", ["+0", "-0"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("nlay", [2, 4])
@pytest.mark.parametrize("rows", [4, 8])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_zero_lanes_against_the_oracle(frame, rows, nlay, form, start):
    ref = _oracle(frame, nlay, form, start)
    if start == "-0":                             # no zero of the oracle keeps the sign it was given
        for st in ref:
            assert not (np.signbit(st["u"]) & (st["u"] == 0.0)).any() and not (np.signbit(st["v"]) & (st["v"] == 0.0)).any()
    _check_against(_fields(frame, nlay, form, start), ref, rows, (frame, rows, nlay, form, start), 1)


def _minus_zero(fnud):
    fnud[[IX_U, IX_V]] = -0.0


def _minus_one_in_half(fnud):
    fnud[[IX_U, IX_V], :, fnud.shape[2] // 2:] = -1.0


def _one_in_the_last_slot(fnud):
    fnud[IX_V, -1, -1] = 1.0


CLEARED = {"minus_zero": _minus_zero, "minus_one_in_half": _minus_one_in_half, "one_in_the_last_slot": _one_in_the_last_slot}


@pytest.mark.parametrize("targets", list(CLEARED))
def test_targets_that_are_not_plus_zero_clear_the_flag(targets):
    f = _with_targets(_fields("258x34", 2, "leith"), CLEARED[targets])
    _check_against(f, _oracle_run(f, census=False), 8, (targets,), 0)


def test_three_bands_hold_the_single_handles_bits():
    f = _fields("258x34", 2, "leith")
    ref = _oracle("258x34", 2, "leith", "+0")
    one = capi.Engine(f)
    many = capi.MultiEngine(f, devices=[0] * 3)
    assert many.count == 3 and many.info("vel_targets_zero") == 1
    t = 1
    for n, want in zip(CALLS, ref):
        one.step(t, n)
        many.step(t, n)
        t += n
        a, b = one.download(PROG8), many.download()
        for k in PROG8:
            assert same_bits(b[k], a[k]), (t - 1, k, "bands vs single handle")
            assert same_bits(a[k], want[k]), (t - 1, k, "single handle vs oracle")
    one.close()
    many.close()
