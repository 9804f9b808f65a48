"""Forcing in time without a GPU: the host function beom_forcing_weight against tests/forcing_ref.py bit for bit, the
refusals that need no handle, why the rule selects instead of forming (1-a)*A + a*B, and the conditions the GPU tests'
inputs are held to on the oracle, so that tests/test_gpu_forcing.py cannot pass vacuously."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np
import pytest

import forcing_cases as FC
import forcing_ref as FR
from beom_amd import capi
from helpers import Golden, same_bits


def _bits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def _same_weight(times, period, ctim):
    got, want = capi.forcing_weight(times, period, ctim), FR.weight(times, period, ctim)
    assert got[:2] == want[:2] and _bits(got[2]) == _bits(want[2]), (list(times), period, ctim, got, want)
    return want


# ---- the weight -----------------------------------------------------------------------------------------------------------------
TIMES = np.array([0.3125, 0.75, 1.15625, 2.0 + 1.0 / 3.0])


def test_weight_equals_the_reference_on_a_table_of_times():
    last = len(TIMES) - 1
    assert _same_weight(TIMES, 0.0, 0.1) == (0, 0, 0.0)                      # before the first frame
    assert _same_weight(TIMES, 0.0, -1.e9) == (0, 0, 0.0)
    for k, t in enumerate(TIMES):                                            # exactly at each frame
        assert _same_weight(TIMES, 0.0, t) == ((k, k + 1, 0.0) if k < last else (last, last, 0.0))
    for k in range(last):                                                    # between frames
        for x in (0.37, 0.5, 1.0 / 3.0, 0.999):
            k0, k1, a = _same_weight(TIMES, 0.0, TIMES[k] + x * (TIMES[k + 1] - TIMES[k]))
            assert (k0, k1) == (k, k + 1) and 0.0 < a < 1.0
    assert _same_weight(TIMES, 0.0, 7.0) == (last, last, 0.0)                 # after the last
    assert _same_weight(TIMES, 0.0, 1.e12) == (last, last, 0.0)
    rng = np.random.default_rng(3)
    for ctim in rng.uniform(-1.0, 4.0, 400):
        _same_weight(TIMES, 0.0, ctim)


def test_weight_of_one_frame_is_always_the_frame():
    for period in (0.0, 2.5):
        for ctim in (-3.0, 0.0, 1.0, 1.0e6):
            assert _same_weight([1.0], period, ctim) == (0, 0, 0.0)


def test_weight_of_a_cyclic_set():
    period = 2.75                                                            # > TIMES[-1] - TIMES[0] = 2.0208...
    last = len(TIMES) - 1
    seen_wrap = 0
    for n in (-7, -3, -1, 0, 1, 2, 5, 11):                                   # several periods ahead of and behind times[0]
        for x in (0.0, 0.01, 0.2, 0.5, 0.73, 0.74, 0.9, 0.999):
            k0, k1, a = _same_weight(TIMES, period, TIMES[0] + (n + x) * period)
            assert 0.0 <= a < 1.0
            if k1 == 0 and k0 == last:
                seen_wrap += 1
    assert seen_wrap >= 8, "the wrap interval was never met"
    k0, k1, a = _same_weight(TIMES, period, TIMES[last] + 0.25 * (TIMES[0] + period - TIMES[last]))      # inside the wrap interval
    assert (k0, k1) == (last, 0) and abs(a - 0.25) < 1.e-12
    rng = np.random.default_rng(4)
    for ctim in rng.uniform(-30.0, 30.0, 400):
        _same_weight(TIMES, period, ctim)


def test_weight_of_a_few_ulps():
    for period in (0.0, 2.75):
        t = float(TIMES[1])
        for _ in range(3):
            t = float(np.nextafter(t, np.inf))
            k0, k1, a = _same_weight(TIMES, period, t)
            assert (k0, k1) == (1, 2) and 0.0 < a < 1.e-14


# ---- refusals that need no handle -------------------------------------------------------------------------------------------------
def _set_rc(field, times, period, frames=None):
    lib = capi.load()
    err = C.create_string_buffer(capi.ERRLEN + 1)
    t = None if times is None else np.ascontiguousarray(times, dtype=np.float64)
    fr = np.zeros(8) if frames is None else frames
    n = 0 if t is None else t.size
    return lib.beom_set_forcing(None, field, n, capi._dp(t), float(period), capi._dp(fr), err, capi.ERRLEN), err.value.decode()


def test_malformed_sets_are_refused_before_the_handle_is_looked_at():
    nan, inf = float("nan"), float("inf")
    bad = [(0, [1.0, 2.0], 0.0), (3, [1.0, 2.0], 0.0),                      # an unknown field
           (1, [1.0, 1.0], 0.0), (1, [2.0, 1.0], 0.0), (2, [1.0, 2.0, 1.5], 0.0),      # times not strictly increasing
           (1, [1.0, nan], 0.0), (1, [-inf, 1.0], 0.0), (2, [inf], 0.0),            # times not finite
           (1, [1.0, 2.0], 1.0), (1, [1.0, 2.0], 0.5), (2, [1.0, 2.0], -1.0), (1, [1.0, 2.0], nan), (1, [1.0, 2.0], inf)]      # period
    for field, times, period in bad:
        rc, msg = _set_rc(field, times, period)
        assert rc == -3 and msg.startswith("beom_set_forcing:") and len(msg) > 30, (field, times, period, rc, msg)
    # well-formed arguments get as far as the handle
    for field, times, period in ((1, [1.0, 2.0], 0.0), (2, [1.0, 2.0], 1.0 + 1.e-9), (1, [5.0], 0.0), (2, None, 0.0)):
        rc, msg = _set_rc(field, times, period)
        assert rc == -1, (field, times, period, rc, msg)
    k0, k1, a = C.c_int(), C.c_int(), C.c_double()
    assert capi.load().beom_forcing_weight(0, capi._dp(TIMES), 0.0, 1.0, C.byref(k0), C.byref(k1), C.byref(a)) == -1


# ---- the select -------------------------------------------------------------------------------------------------------------------
def test_equal_frames_give_the_frames_bits_and_the_convex_form_does_not():
    rng = np.random.default_rng(11)
    A = rng.standard_normal(4096) * 10.0 ** rng.integers(-8, 3, 4096)
    A[::17] = -0.0
    A[5::17] = 0.0
    for a in (0.37, 1.0 / 3.0, 0.9999999):
        assert same_bits(FR.lerp(A, A.copy(), a), A), "the rule does not return equal frames bit for bit"
    assert np.signbit(FR.lerp(A, A.copy(), 0.37)[::17]).all()
    plain = FR.convex(A, A.copy(), 0.37)
    assert not same_bits(plain, A), "(1-a)*A + a*B returned equal frames bit for bit: the select would be needless"
    # and A + a*(B - A) without the select turns a -0 that both frames hold into +0
    unselected = A + np.float64(0.37) * (A.copy() - A)
    assert not np.signbit(unselected[::17]).any() and np.signbit(A[::17]).all()
    # a = 0 is the frame itself, whatever the other frame holds
    B = A + 1.0
    assert same_bits(FR.lerp(A, B, 0.0), A)
    # and between different values it is A + a*(B - A)
    assert same_bits(FR.lerp(A, B, 0.37)[1:5], (A + np.float64(0.37) * (B - A))[1:5])
    # a field of equal frames is the frame at every time
    fr = np.stack([A, A, A])
    for ctim in (0.0, 1.1, 1.7, 2.9, 9.0):
        assert same_bits(FR.field(fr, [1.0, 2.0, 3.0], 0.0, ctim), A)
        assert same_bits(FR.field(fr, [1.0, 2.0, 3.0], 2.5, ctim), A)


def test_special_entries_are_where_the_gpu_test_needs_them():
    f = Golden("island_3l_forced").fields()
    fr = FC.with_special_entries(FC.make_frames(f, "taus"))
    z = fr == 0.0
    assert (z & np.signbit(fr)).any() and (z & ~np.signbit(fr)).any(), "no exact +0 and -0 entries"
    eq = (fr[1:] == fr[:-1]) & (fr[1:] != 0.0)
    assert eq.any(axis=(0, 2)).all(), "no entries equal between consecutive frames in some slice"
    assert ((fr[1] == 0.0) & np.signbit(fr[1]) & (fr[0] != 0.0)).any(), "no -0 next to a value"


# ---- the GPU tests' inputs on the oracle --------------------------------------------------------------------------------------------
TAUS_CASES = ["stommel_24x16", "island_3l_forced", "random_coast_2l_xper", "island_10l_deep", "biharm_island_2l", "jet_2l_xyper"]
HDOT_CASES = ["island_3l_forced", "topdrag_topo_2l", "stommel_24x16"]


def _held_to_conditions(name, field):
    g = Golden(name)
    f = g.fields()
    f.invf = float(g.static("invf"))
    sets = {field: (FC.frame_times(f), FC.make_frames(f, field), 0.0)}
    seen = []
    o = FC.oracle_run(f, g.variant, sets, watch=lambda t, k, x: seen.append(float(np.max(np.abs(x)))))
    s = FC.steady_run(f, g.variant, sets)
    assert len(seen) == FC.NSTEPS
    if field == "taus":
        assert min(seen) > 1.e-7, (name, "a step's interpolated taus has nothing above 1e-7: the oracle would drop the wind", seen)
    else:
        assert min(seen) > 0.0, (name, seen)
    a, b = o.state(), s.state()
    for k in ("u", "v", "hlay"):
        frac = float(np.mean(a[k] != b[k]))
        print("%s %s frames: %.0f %% of %s differ from the steady run" % (name, field, 100.0 * frac, k))
        assert frac >= 0.5, (name, field, k, frac)
        assert np.all(np.isfinite(a[k])), (name, field, k)
    for k in ("u", "v"):
        assert float(np.max(np.abs(a[k]))) <= 2.0 * float(np.max(np.abs(b[k]))), (name, field, k)


@pytest.mark.parametrize("name", TAUS_CASES)
def test_taus_frames_change_the_run_and_keep_it_sane(name):
    _held_to_conditions(name, "taus")


@pytest.mark.parametrize("name", HDOT_CASES)
def test_hdot_frames_change_the_run_and_keep_it_sane(name):
    """island_3l_forced has an hdot of its own; stommel_24x16 and the others have none and gain it from the frames."""
    _held_to_conditions(name, "hdot")


def test_two_oracles_do_not_share_their_forcing():
    g = Golden("stommel_24x16")
    f = g.fields()
    a, b = FC.oracle_of(f, g.variant, ("taus",)), FC.oracle_of(f, g.variant, ("taus",))
    a.a["taus"][...] = 7.0
    assert not (b.a["taus"] == 7.0).any() and not (np.asarray(f.taus) == 7.0).any()
