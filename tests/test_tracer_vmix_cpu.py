"""Vertical tracer mixing without a GPU: the numpy restatement of the scheme (tracer_vmix_ref) against the same statements
in longdouble (the error is rounding of the content), its maximum principle, column conservation, the limits kappa_v ->
infinity and two layers in closed form, columns that fall into independent pieces, the identity that pins the tracers to
the reference (a tracer of concentration 1 IS the oracle's layer thickness, bit for bit, behind lateral mixing at its cap
and vertical mixing, under either sweep), liveness, and the ctypes prototypes."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import oracle_lib
import tracer_mix_ref as TM
import tracer_vmix_ref as TV
import tracers_limited_ref as TL
import tracers_ref as T
from beom_amd import capi
from helpers import Golden, same_bits
from test_tracers_cpu import _CTYPE, NSTEPS, PIN, _fields, _prototypes

EPS = 2.0 ** -52
LD = np.longdouble
NCOL, NTRC, DT = 20000, 4, 300.0
assert np.finfo(LD).eps < 2.0 ** -60, "longdouble is no wider than double here: it measures nothing"


def _columns(nlay, seed=5, dry=0.15, ncol=NCOL, ntrc=NTRC, conc=(0.25, 1.0)):
    """ncol water columns as a packed cell vector (cell 0 is the sentinel): thicknesses 10^uniform(-3, 3.5) m with about
    15 % of the cell-layers dry, kappa_v = 10^uniform(-6, 0) per tracer and interface, dt = 300 s.  Concentrations
    uniform(0.25, 1), the range of the project's patchy tracers: the content metric scale_l = |q_l| + |G_{l-1}| + |G_l| is at
    least |c_l| h_l, while the difference c_k - c_{k+1} that drives a flux carries the rounding of q/h, 2^-53 max |c|, which
    reaches q'_l as that times h_l at the most (den >= b_l); in units of 2^-52 scale_l this is the ratio of the column's
    largest concentration to c_l, which this range holds at 4 and a range through zero does not bound at all.
    test_error_with_concentrations_of_both_signs takes such a range and the metric that goes with it."""
    r = np.random.default_rng(seed + nlay)
    h = 10.0 ** r.uniform(-3.0, 3.5, (nlay, ncol + 1))
    h[r.uniform(0, 1, h.shape) < dry] = 0.0
    h[:, 0] = 0.0
    c = r.uniform(conc[0], conc[1], (ntrc, nlay, ncol + 1))
    kv = 10.0 ** r.uniform(-6.0, 0.0, (ntrc, nlay - 1))
    mk_n = np.ones(ncol + 1); mk_n[0] = 0.0
    f = SimpleNamespace(p=SimpleNamespace(ndeg=ncol, nlay=nlay, dt=DT), mk_n=mk_n)
    return f, h, np.ascontiguousarray(c * h[None]), kv


# ---- accuracy: rounding of the content -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlay", [2, 3, 5, 16])
def test_error_is_rounding_of_the_content(nlay):
    """|q' - q'_longdouble| <= 32 * 2^-52 * scale_l, scale_l = |q_l| + |G_{l-1}| + |G_l| (measured here: 1.5, 2.0, 2.0, 3.6
    at 2, 3, 5, 16 layers)."""
    f, h, q, kv = _columns(nlay)
    got, G = TV.vmix(f, h, q, kv)
    ref, _ = TV.vmix(f, h, q, kv, dtype=LD)
    assert got.dtype == np.float64 and ref.dtype == LD
    sc = TV.scale(q, G)
    wet = np.broadcast_to(h > 0, q.shape)
    err = np.abs(got.astype(LD) - ref)
    assert not np.any(err[~wet]) and same_bits(got[~wet], q[~wet])
    worst = float(np.max(err[wet] / (EPS * sc[wet])))
    moved = float(np.mean(got[wet] != q[wet]))
    print("nlay %d: max |q' - q'_ld| / (2^-52 scale) = %.3g; %.0f %% of the wet cell-layers moved" % (nlay, worst, 100 * moved))
    assert moved > 0.5, "nothing mixed"
    assert worst <= 32.0, (nlay, worst)


@pytest.mark.parametrize("nlay", [2, 3, 5, 16])
def test_error_with_concentrations_of_both_signs(nlay):
    """Concentrations uniform(-1, 3): a layer whose own concentration is near zero still receives the rounding of its
    neighbours' q/h (see _columns), so the error is held to 32 * 2^-52 * (scale_l + h_l max_column |c|)."""
    f, h, q, kv = _columns(nlay, conc=(-1.0, 3.0))
    got, G = TV.vmix(f, h, q, kv)
    ref, _ = TV.vmix(f, h, q, kv, dtype=LD)
    wet = np.broadcast_to(h > 0, q.shape)
    cmax = np.max(np.abs(TM.concentration(h[None], q)), axis=1, keepdims=True)
    sc = TV.scale(q, G) + h[None] * cmax
    worst = float(np.max((np.abs(got.astype(LD) - ref))[wet] / (EPS * sc[wet])))
    plain = float(np.max((np.abs(got.astype(LD) - ref))[wet] / (EPS * TV.scale(q, G)[wet])))
    print("nlay %d: max |q' - q'_ld| / (2^-52 (scale + h max |c|)) = %.3g (in units of 2^-52 scale alone: %.3g)" % (nlay, worst, plain))
    assert worst <= 32.0, (nlay, worst)


@pytest.mark.parametrize("nlay", [2, 3, 5, 16])
def test_maximum_principle_over_100_applications(nlay):
    """The wet concentrations of a column stay within their initial [min, max], up to 4 tau, tau_l = 2^-52 scale_l / h_l
    (measured here: no overshoot at all), after every one of 100 applications."""
    f, h, q, kv = _columns(nlay)
    wet = h > 0
    hl = np.where(wet, h, 1.0).astype(LD)
    c0 = q.astype(LD) / hl
    lo = np.min(np.where(wet, c0, np.inf), axis=1, keepdims=True)
    hi = np.max(np.where(wet, c0, -np.inf), axis=1, keepdims=True)
    worst, spread0 = 0.0, None
    for n in range(100):
        new, G = TV.vmix(f, h, q, kv)
        tau = (EPS * TV.scale(q, G)).astype(LD) / hl
        c = new.astype(LD) / hl
        over = np.maximum(np.maximum(lo - c, c - hi), 0.0)
        w = np.broadcast_to(wet, over.shape) & (tau > 0)
        worst = max(worst, float(np.max(over[w] / tau[w])))
        assert not np.any(over[np.broadcast_to(wet, over.shape) & ~(tau > 0)])
        if spread0 is None:
            spread0 = float(np.std(c0[np.broadcast_to(wet, c0.shape)]))
        q = new
    spread = float(np.std(c[np.broadcast_to(wet, c.shape)]))
    print("nlay %d: worst overshoot %.3g tau over 100 applications; std of c %.3g -> %.3g" % (nlay, worst, spread0, spread))
    assert spread < spread0, "nothing mixed"
    assert worst <= 4.0, (nlay, worst)


@pytest.mark.parametrize("nlay", [2, 3, 5, 16])
def test_every_column_keeps_its_content(nlay):
    """A layer's new content (q + G_above) - G_below rounds twice, each time on a value no larger than scale_l, and every
    G_k enters two layers with opposite sign from the same bits: the exact sum of the increments is zero and the column sum
    changes by at most 2 * 2^-53 * sum_l scale_l = 2^-52 sum_l scale_l per application (sums formed in longdouble, whose
    own roundings and the second rounding's own growth are covered by a factor 1 + 2^-40)."""
    f, h, q, kv = _columns(nlay)
    new, G = TV.vmix(f, h, q, kv)
    drift = np.abs(np.sum(new.astype(LD), axis=1) - np.sum(q.astype(LD), axis=1))
    bound = EPS * (1 + LD(2.0) ** -40) * np.sum(TV.scale(q, G).astype(LD), axis=1)
    size = np.sum(np.abs(q).astype(LD), axis=1)
    ok = size > 0
    print("nlay %d: max drift / bound %.3g; max drift in ulp of sum |q| %.3g" % (nlay, float(np.max(drift[ok] / bound[ok])),
                                                                                 float(np.max(drift[ok] / (EPS * size[ok])))))
    assert np.all(drift <= bound)
    assert np.all(bound <= 8 * nlay * EPS * size)          # (the bound itself means something: a few ulp of the column's content)


# ---- limits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlay", [2, 5, 16])
def test_huge_kappa_gives_the_thickness_weighted_column_mean(nlay):
    """kappa_v = 1e12 on columns without dry layers.  The exact solution has c'_k - c'_{k+1} = G_k R_k (R_k = hbar / (dt
    kappa_v)) and its mean is the column's, so |c'_l - mean| <= sum_k |G_k| R_k; the computed content is within the 32 units
    of the accuracy test of it: |q'_l - h_l mean| <= h_l sum_k |G_k| R_k + 32 * 2^-52 scale_l.  There is no cap on kappa_v."""
    f, h, q, _ = _columns(nlay, dry=0.0, ncol=4000, ntrc=2)
    kv = 1.0e12
    new, G = TV.vmix(f, h, q, kv)
    assert np.isfinite(new).all()
    hl = h.astype(LD)
    mean = np.sum(q.astype(LD), axis=1, keepdims=True)[:, :, 1:] / np.sum(hl, axis=0)[None, None, 1:]
    R = (0.5 * (hl[:-1] + hl[1:])) / (LD(DT) * LD(kv))
    slack = np.sum(np.abs(G[:, 1:nlay]).astype(LD) * R[None], axis=1, keepdims=True)[:, :, 1:]
    dev = np.abs(new.astype(LD)[:, :, 1:] - hl[None, :, 1:] * mean)
    bound = hl[None, :, 1:] * slack + 32 * EPS * TV.scale(q, G)[:, :, 1:]
    c = new[:, :, 1:] / h[None, :, 1:]
    print("nlay %d: max dev / bound %.3g; max |c' - mean| %.3g; max sum |G| R %.3g" % (nlay, float(np.max(dev / bound)),
                                                                                      float(np.max(np.abs(c - mean))), float(np.max(slack))))
    assert np.all(dev <= bound)
    assert float(np.max(slack)) <= 1.0e-4                  # (of concentrations spread over [0.25, 1]: the mean is reached)


def test_two_layers_against_the_closed_form():
    """G = w dc / (1 + w (1/h1 + 1/h2)), w = dt kappa_v / hbar, in longdouble from dc = q1/h1 - q2/h2; compared in the content
    metric, 32 * 2^-52 * scale_l (dc itself carries the rounding of q/h, so G is not accurate relative to itself)."""
    f, h, q, kv = _columns(2)
    new, G = TV.vmix(f, h, q, kv)
    both = (h[0] > 0) & (h[1] > 0)
    both[0] = False
    hl = np.where(both, h, 1.0).astype(LD)
    ql = q.astype(LD)
    w = LD(DT) * kv.astype(LD)[:, 0, None] / (0.5 * (hl[0] + hl[1]))[None]
    Gc = np.where(both[None], w * (ql[:, 0] / hl[0] - ql[:, 1] / hl[1]) / (1 + w * (1 / hl[0] + 1 / hl[1])), 0)
    sc = TV.scale(q, G)
    e0 = np.abs(new[:, 0].astype(LD) - (ql[:, 0] - Gc))[:, both] / (EPS * sc[:, 0][:, both])
    e1 = np.abs(new[:, 1].astype(LD) - (ql[:, 1] + Gc))[:, both] / (EPS * sc[:, 1][:, both])
    worst = max(float(np.max(e0)), float(np.max(e1)))
    print("two layers: max |q' - closed form| / (2^-52 scale) = %.3g" % worst)
    assert worst <= 32.0
    assert same_bits(new[:, :, ~both], q[:, :, ~both])      # a dry partner: nothing moves


# ---- columns that fall into pieces ----------------------------------------------------------------------------------------------
def test_a_closed_interface_and_a_dry_layer_split_the_column():
    f, h, q, kv = _columns(5, dry=0.0, ncol=500, ntrc=2)
    # kappa_v = 0 at interface 2 (between layers 2 and 3) for tracer 0 only
    kv0 = kv.copy(); kv0[0, 1] = 0.0
    base, G = TV.vmix(f, h, q, kv0)
    assert not np.any(G[0, 2]) and np.any(G[1, 2]) and np.any(G[0, 1]) and np.any(G[0, 3])
    q2 = q.copy(); q2[:, 2:] *= 1.5                        # the lower piece changes
    other, _ = TV.vmix(f, h, q2, kv0)
    assert same_bits(other[0, :2], base[0, :2]), "the upper piece felt the lower one through a closed interface"
    assert not same_bits(other[0, 2:], base[0, 2:]) and not same_bits(other[1, :2], base[1, :2])
    q3 = q.copy(); q3[:, :2] += 0.25 * h[None, :2]         # the upper piece changes
    other, _ = TV.vmix(f, h, q3, kv0)
    assert same_bits(other[0, 2:], base[0, 2:]) and not same_bits(other[0, :2], base[0, :2])
    # a dry layer 3 in every second column: what is above it does not feel what is below it; the dry layer keeps its bits
    hd = h.copy(); hd[2, 1::2] = 0.0
    qd = q.copy(); qd[:, 2, 1::2] = 0.0
    base, G = TV.vmix(f, hd, qd, kv)
    assert not np.any(G[:, 2, 1::2]) and not np.any(G[:, 3, 1::2]) and np.any(G[:, 2, 2::2]) and np.any(G[:, 3, 2::2])
    qe = qd.copy(); qe[:, 3:] *= -2.0
    other, _ = TV.vmix(f, hd, qe, kv)
    assert same_bits(other[:, :3, 1::2], base[:, :3, 1::2])
    assert not same_bits(other[:, :2, 2::2], base[:, :2, 2::2])          # (the whole columns do feel it)
    assert same_bits(base[:, 2, 1::2], qd[:, 2, 1::2])
    # a thin wet layer conducts
    ht = h.copy(); ht[2, 1:] = 1.0e-3
    qt = q.copy(); qt[:, 2] = 0.5 * ht[2]
    base, _ = TV.vmix(f, ht, qt, 1.0e3)
    qe = qt.copy(); qe[:, 3:] *= -2.0
    other, _ = TV.vmix(f, ht, qe, 1.0e3)
    assert np.mean(other[:, 0, 1:] != base[:, 0, 1:]) > 0.9


def test_land_cells_and_the_sentinel_keep_their_values():
    f, h, q, kv = _columns(5, ncol=500, ntrc=2)
    f.mk_n[3::7] = 0.0
    q[:, :, 0] = 7.0
    h[:, 0] = 2.0                                          # (even a sentinel with thickness is not a cell)
    new, G = TV.vmix(f, h, q, kv)
    land = f.mk_n < 0.5
    assert land[0] and land.sum() > 50
    assert same_bits(new[:, :, land], q[:, :, land]) and not np.any(G[:, :, land])
    assert not same_bits(new[:, :, ~land], q[:, :, ~land])


# ---- the identity with the oracle's thickness, and liveness ----------------------------------------------------------------------
LAYERED = tuple(n for n in PIN if Golden(n).fields().p.nlay >= 2)
assert len(LAYERED) >= 8, LAYERED


def _sweep(scheme, f, st, q, rq, ctrg, scalars):
    if scheme == 1:
        return T.update(f, st["hlay"], st["h_u"], st["h_v"], q, rq, ctrg, *scalars)
    return TL.update(f, st["hlay"], st["h_u"], st["h_v"], q, rq, ctrg, *scalars, scheme=2)


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("name", LAYERED)
def test_uniform_tracer_is_the_oracles_layer_thickness_and_a_patchy_one_is_moved(name, scheme):
    """Tracer 0 (concentration 1): lateral mix at the cap, vertical mix with a large kappa_v, the restated sweep, 40 steps:
    the oracle's hlay bit for bit.  Tracer 1 (patchy) ends elsewhere than in a run without vertical mixing."""
    g = Golden(name)
    assert not g.uses_cos(), name
    f = _fields(g)
    o = oracle_lib.Oracle(f, variant=g.variant)
    h0 = np.array(f.hlay, dtype=np.float64)
    q = np.stack([h0, T.patchy(f) * h0])
    rq = np.stack([np.array(f.rs_h, dtype=np.float64), np.zeros(h0.shape + (2,))])
    ctrg = np.ones_like(q)
    plain = [q.copy(), rq.copy()]
    kappa, kappa_v = TM.kappa_cap(f.p), 50.0
    tres = float(getattr(f, "tres", 0.0))
    for t in range(1, NSTEPS + 1):
        if t <= 3:
            o.rebuild_fluxes()                      # what the step is about to do itself: the same values
        sc = T.step_scalars(f.p, t, tres)
        st = o.state()
        lat = TM.mix(f, st["hlay"], q, kappa=kappa)
        mixed, _ = TV.vmix(f, st["hlay"], lat, kappa_v)
        assert same_bits(mixed[0], q[0]), (name, t, "the mixing moved a tracer of concentration 1")
        q, rq = _sweep(scheme, f, st, mixed, rq, ctrg, sc)
        plain = list(_sweep(scheme, f, st, TM.mix(f, st["hlay"], plain[0], kappa=kappa), plain[1], ctrg, sc))
        o.step(t, 1)
        assert same_bits(q[0][:, 1:], o.state()["hlay"][:, 1:]), (name, scheme, t)
    assert same_bits(plain[0][0], q[0])
    assert not same_bits(plain[0][1], q[1]), (name, "the patchy tracer is where a run without vertical mixing puts it")


# ---- the host's reciprocal ----------------------------------------------------------------------------------------------------
def test_rk_is_product_then_reciprocal_and_zero_means_closed():
    p = SimpleNamespace(dt=0.1)
    kv = np.array([[0.0, 3.0, 1.0e-5, -0.0]])
    r = TV.rk(p, kv)
    assert same_bits(r, np.array([[0.0, 1.0 / (0.1 * 3.0), 1.0 / (0.1 * 1.0e-5), 0.0]]))
    assert r[0, 1] != (1.0 / 0.1) / 3.0                    # (the other order rounds elsewhere: the order is part of the contract)


# ---- the binding --------------------------------------------------------------------------------------------------------------
def test_exports_are_declared_and_prototypes_match_the_header():
    protos = _prototypes()
    lib = capi.load()
    assert set(capi.TRACER_VMIX_EXPORTS) == {"beom_set_tracer_vmixing", "beom_update_tracer_vmixing", "beom_multi_set_tracer_vmixing"}
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "beom_hip.h")).read()
    for name in capi.TRACER_VMIX_EXPORTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in protos and name in capi.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int, name
        assert list(fn.argtypes) == [_CTYPE[t] for t in protos[name]], (name, protos[name], fn.argtypes)
    for m in ("set_tracer_vertical_mixing", "update_tracer_vertical_mixing"):
        assert hasattr(capi.Engine, m), m
    assert hasattr(capi.MultiEngine, "set_tracer_vertical_mixing")


def test_null_handle_is_refused():
    lib = capi.load()
    err = C.create_string_buffer(200)
    assert lib.beom_set_tracer_vmixing(None, None, err, 199) == -1
    assert lib.beom_multi_set_tracer_vmixing(None, None, err, 199) == -1
    assert lib.beom_update_tracer_vmixing(None) == -1
