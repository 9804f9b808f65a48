"""The inputs of addons_kit held to their conditions without a GPU, for every frame test_gpu_addons_together puts the kit on:
coefficients inside the documented caps, floats in wet cells, frame times and strides that meet every branch within the 12
steps, recorders that just hold the run, bands whose windows are tall enough, and restated tracer steps that stay finite: a
non-finite value on the device would be the device's doing."""
import numpy as np
import pytest

import addons_kit as K
import floats_ref as FR
import forcing_ref as FO
import rough_inputs as RI
import tracer_mix_ref as TM
import tracer_vmix_ref as TV
import tracers_limited_ref as TL
import tracers_ref as T
from beom_amd import capi

FRAMES = tuple(K.FRAMES)
DIVISIONS = ((12,), (5, 7), (1,) * 12, (5, 4, 3))
TINY = np.finfo(np.float64).tiny


def _kits(name):
    f = K.frame(name)
    return f, [K.Kit(f, seed=1, scheme=s, ntrc=n) for s in (1, 2) for n in (3, 2)]


@pytest.mark.parametrize("name", FRAMES)
def test_mixing_coefficients_pass_the_caps(name):
    f, kits = _kits(name)
    p = f.p
    dt, dl = float(p.dt), float(p.dl)
    for kit in kits:
        assert kit.kappa.shape == kit.decay.shape == kit.source.shape == (kit.ntrc, p.nlay)
        assert kit.kappa.any() and kit.decay.any() and kit.source.any(), "kappa, decay and source are all in play"
        assert np.all(kit.kappa >= 0.0) and np.all(kit.kappa * dt / (dl * dl) <= 0.25)
        assert np.all(kit.decay >= 0.0) and np.all(kit.decay * dt <= 1.0)
        assert np.isfinite(kit.source).all()
        assert not kit.decay[0].any() and not kit.source[0].any(), "the unit tracer must stay the thickness"
        assert kit.kappa[0].all() and kit.kappa_v[0].all(), "the unit tracer's own coefficients are in play"
        assert kit.kappa_v.shape == (kit.ntrc, p.nlay - 1) and np.all(kit.kappa_v > 0.0)
        rk = TV.rk(p, kit.kappa_v)
        assert np.all(rk >= TINY) and np.isfinite(rk).all(), "1 / (dt kappa_v) positive and normal"
        # tracer 0 is the unit tracer: content = thickness, relaxation concentration 1, the thickness' own history
        assert K.same_bits(kit.q[0][:, 1:], np.asarray(f.hlay, dtype=np.float64)[:, 1:]) and np.all(kit.ctrg[0] == 1.0)
        assert K.same_bits(kit.rq[0], f.rs_h)
        for t in range(1, kit.ntrc):
            wet = np.asarray(f.hlay)[:, 1:] > 0.0
            c = kit.q[t][:, 1:] / np.where(wet, np.asarray(f.hlay, dtype=np.float64)[:, 1:], 1.0)
            assert np.unique(c[wet]).size > 0.9 * wet.sum(), "a rough tracer"


@pytest.mark.parametrize("name", FRAMES)
def test_floats_start_in_wet_cells(name):
    f, kits = _kits(name)
    x, y, layer = kits[0].floats
    assert x.size == y.size == layer.size == K.NFLOATS
    assert FR.Frame(f).wet(x, y).all()
    assert sorted(set(layer.tolist())) == list(range(1, f.p.nlay + 1)), "floats over all layers"


@pytest.mark.parametrize("name", FRAMES)
def test_frame_times_meet_every_branch_within_the_steps(name):
    f, kits = _kits(name)
    kit = kits[0]
    d = float(f.p.dtd8)
    for times, frames, period in (kit.taus, kit.hdot):
        assert np.all(np.diff(times) > 0.0) and frames.shape[0] == times.size and np.isfinite(frames).all()
        assert period == 0.0 or period > times[-1] - times[0]
    assert kit.taus[1].shape == (3, 2, f.p.ndeg + 1) and kit.taus[2] == 7.0 * d
    assert kit.hdot[1].shape == (2, f.p.nlay, f.p.ndeg + 1) and kit.hdot[2] == 0.0
    assert not f.has.get("hdot", False), "the frame is created without hdot: the set brings it"
    fr = kit.taus[1]
    assert np.any((fr == 0.0) & ~np.signbit(fr)) and np.any((fr == 0.0) & np.signbit(fr)) and np.any(fr[1] == fr[0]), "special entries"
    times, _, period = kit.taus
    w = [FO.weight(times, period, kit.ctim(t)) for t in range(1, K.NSTEPS + 1)]
    last = times.size - 1
    assert any(a == 0.0 for _, _, a in w), w
    assert any(0.0 < a < 1.0 and k1 == k0 + 1 for k0, k1, a in w), w
    assert any(0.0 < a < 1.0 and (k0, k1) == (last, 0) for k0, k1, a in w), (w, "no step in the wrap interval")
    # without a period the same steps would read other frames: the period is in play
    assert w != [FO.weight(times, 0.0, kit.ctim(t)) for t in range(1, K.NSTEPS + 1)]
    wh = [FO.weight(kit.hdot[0], 0.0, kit.ctim(t)) for t in range(1, K.NSTEPS + 1)]
    assert any(0.0 < a < 1.0 for _, _, a in wh) and wh[0] == (0, 0, 0.0) and wh[-1] == (1, 1, 0.0), wh


def test_strides_and_recorders():
    f, kits = _kits("island_ragged_129x33_2l")
    kit = kits[0]
    for k, stride in K.STRIDES.items():
        s = K.samples(stride, 1, K.NSTEPS)
        assert len(s) >= 2 and s[-1] == K.NSTEPS, (k, s, "the last step carries a record of every recorder")
    for k in K.RECORDERS + ("float_track",):
        n = kit.records[k]
        assert n == len(K.samples(K.STRIDES[k], 1, K.NSTEPS)), (k, "the run just fits")
        for calls in DIVISIONS:                       # nothing is downloaded between the calls: what is held adds up
            held, t = 0, 1
            for c in calls:
                new = len(K.samples(K.STRIDES[k], t, t + c - 1))
                assert held + new <= n, (k, calls, t)
                held, t = held + new, t + c
            assert held == n and t - 1 == K.NSTEPS
    assert sorted(K.STRIDES.values()) == [1, 1, 2, 2, 2, 2, 3, 3, 3]
    for name in FRAMES:
        M = K.frame(name).p.mm + 1
        win = K.Kit(K.frame(name)).windows
        for jlo, jhi in win.values():
            assert 1 < jlo < jhi < M, (name, jlo, jhi, "a window strictly inside the frame")
        assert win["column_series"] != win["tracer_column_series"]


def test_what_each_handle_kind_keeps():
    kit = K.Kit(K.frame("island_ragged_129x33_2l"))
    assert kit.keeps("single") == K.EVERYTHING and len(K.EVERYTHING) == 12
    assert set(K.EVERYTHING) - set(kit.keeps("bands")) == {"column_series", "tracer_column_series", "maps", "float_track"}
    assert kit.keeps("ring") == ("forcing", "moments", "harmonics", "series", "floats")
    assert set(K.DIAGNOSTICS) | set(K.BASE) | {"float_track"} == set(K.EVERYTHING)


@pytest.mark.parametrize("nband", [2, 3])
@pytest.mark.parametrize("name", K.BANDED)
def test_band_windows_are_tall_enough_to_be_cut(name, nband):
    """beom_multi_window is a host function: the library loads without a device."""
    f = K.frame(name)
    yper = float(f.p.yper) > 0.5
    assert yper == ("ring" in K.FRAMES[name][1])
    own = []
    for band in range(nband):
        w = capi.multi_window(f.p, nband, band, yper)
        rows = (w["own1"] - w["own0"] + 1) + w["ghost_s"] + w["ghost_n"]
        assert rows >= 32, (name, nband, band, w)
        own.append((w["own0"], w["own1"]))
    assert own[0][0] == 1 and all(b[0] == a[1] + 1 for a, b in zip(own[:-1], own[1:]))
    assert own[-1][1] == (f.p.mm if yper else f.p.mm + 1), (name, own)


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("name", [n for n in FRAMES if "ring" not in K.FRAMES[n][1]])
def test_restated_tracer_steps_stay_finite(name, scheme):
    """Lateral mixing, vertical mixing and the sweep of either scheme, 12 times over a fixed rough state."""
    f = K.frame(name)
    g = RI.rough_fields(f, 1)
    st = {k: np.ascontiguousarray(getattr(g, k), dtype=np.float64) for k in ("hlay", "h_u", "h_v", "rs_h")}
    kit = K.Kit(f, seed=1, scheme=scheme, state=st)
    q, rq = kit.q.copy(), kit.rq.copy()
    update = T.update if scheme == 1 else TL.update
    for t in range(1, K.NSTEPS + 1):
        q = TM.mix(g, st["hlay"], q, kit.kappa, kit.decay, kit.source)
        q, _ = TV.vmix(g, st["hlay"], q, kit.kappa_v)
        q, rq = update(g, st["hlay"], st["h_u"], st["h_v"], q, rq, kit.ctrg, *T.step_scalars(f.p, t))
        assert np.isfinite(q).all() and np.isfinite(rq).all(), (name, scheme, t)
    assert not K.same_bits(q[1], kit.q[1]), "the tracers did not move: nothing tested"
