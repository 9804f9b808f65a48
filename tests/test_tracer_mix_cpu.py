"""Tracer mixing without a GPU: the numpy restatement of the scheme (tracer_mix_ref) in front of the restated sweeps keeps
the identity that pins the tracers to the reference (a tracer of concentration 1 IS the oracle's layer thickness, bit for
bit, with diffusion at its cap), its maximum principle on a frame with land, dry cells and thickness contrasts of four
decades, conservation, the decay / source recursion, liveness of each coefficient, and the ctypes prototypes."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import oracle_lib
import tracer_mix_ref as TM
import tracers_limited_ref as TL
import tracers_ref as T
from beom_amd import capi
from helpers import Golden, same_bits
from test_tracers_cpu import _CTYPE, NSTEPS, PIN, _fields, _prototypes


# ---- the identity with the oracle's thickness, diffusion on -------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("name", PIN)
def test_uniform_tracer_is_the_oracles_layer_thickness_with_diffusion_at_the_cap(name, scheme):
    g = Golden(name)
    assert not g.uses_cos(), name
    f = _fields(g)
    o = oracle_lib.Oracle(f, variant=g.variant)
    q = np.array(f.hlay, dtype=np.float64)[None].copy()
    rq = np.array(f.rs_h, dtype=np.float64)[None].copy()
    ctrg = np.ones_like(q)
    kappa = TM.kappa_cap(f.p)
    assert kappa > 0 and kappa * float(f.p.dt) / float(f.p.dl) ** 2 >= 0.25 * (1 - 1e-15)
    tres = float(getattr(f, "tres", 0.0))
    for t in range(1, NSTEPS + 1):
        if t <= 3:
            o.rebuild_fluxes()                      # what the step is about to do itself: the same values
        gene, ramp, ctim = T.step_scalars(f.p, t, tres)
        st = o.state()
        mixed = TM.mix(f, st["hlay"], q, kappa=kappa)
        assert same_bits(mixed, q), (name, t, "the mix moved a tracer of concentration 1")
        if scheme == 1:
            q, rq = T.update(f, st["hlay"], st["h_u"], st["h_v"], mixed, rq, ctrg, gene, ramp, ctim)
        else:
            q, rq = TL.update(f, st["hlay"], st["h_u"], st["h_v"], mixed, rq, ctrg, gene, ramp, ctim, scheme=2)
        o.step(t, 1)
        assert same_bits(q[0][:, 1:], o.state()["hlay"][:, 1:]), (name, scheme, t)


# ---- a frame built here: land, dry cells, thicknesses over four decades between neighbours ------------------------------------
def _frame(lm=37, mm=53, nlay=2, seed=11, land=0.06, dry=0.15):
    """A closed lm x mm frame with a packed cell vector as the engine's callers have it: land cells are no cells (links to
    them are 0, the sentinel), about 15 % of the cell-layers are dry (+0 thickness), the others are 10^uniform(-2, 2) m."""
    r = np.random.default_rng(seed)
    is_cell = r.uniform(0, 1, (mm, lm)) >= land
    idx = np.zeros((mm + 2, lm + 2), dtype=np.int64)           # a rim of sentinels around the frame
    ndeg = int(is_cell.sum())
    idx[1:-1, 1:-1][is_cell] = np.arange(1, ndeg + 1)
    neig = np.zeros((ndeg + 1, 8), dtype=np.int32)
    jj, ii = np.nonzero(idx)
    for k, (di, dj) in enumerate(((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))):
        neig[idx[jj, ii], k] = idx[jj + dj, ii + di]
    p = SimpleNamespace(ndeg=ndeg, nlay=nlay, dl=2000.0, dt=64.0)           # (0.25 dl^2 / dt = 15625 exactly)
    mk_n = np.ones(ndeg + 1); mk_n[0] = 0.0
    h = 10.0 ** r.uniform(-2.0, 2.0, (nlay, ndeg + 1))
    h[r.uniform(0, 1, h.shape) < dry] = 0.0
    h[:, 0] = 0.0
    # two water masses, -1 and 3, cell by cell, each jittered by a quarter: a thin cell of one mass among four thicker cells
    # of the other is what a step beyond the cap throws out of the bounds
    c = np.where(r.uniform(0, 1, (1, nlay, ndeg + 1)) < 0.5, -1.0, 3.0) + r.uniform(-0.25, 0.25, (1, nlay, ndeg + 1))
    c[:, :, 0] = 0.0
    f = SimpleNamespace(p=p, neig=neig, mk_n=mk_n)
    return f, h, np.ascontiguousarray(c * h[None])


def test_the_frame_is_rough_enough():
    f, h, q = _frame()
    assert f.p.nlay == 2 and 1700 < f.p.ndeg < 37 * 53
    wet = h[:, 1:] > 0
    assert 0.12 <= 1 - wet.mean() <= 0.18
    for k in (0, 2):                                # E and N neighbours: contrasts of three decades and more between wet pairs
        nb = f.neig[:, k].astype(np.int64)
        both = (h > 0) & (h[:, nb] > 0)
        ratio = np.where(both, h / np.where(both, h[:, nb], 1.0), 1.0)
        assert ratio.max() >= 1.0e3 and ratio.min() <= 1.0e-3
    assert np.any(f.neig[1:, [0, 2, 4, 6]] == 0)    # coasts and the frame's edge


def _bounds(h, q):
    wet = h > 0
    c = TM.concentration(h, q[0])
    return c, wet, float(c[wet].min()), float(c[wet].max())


def test_maximum_principle_at_the_cap_and_its_failure_above():
    """400 applications at kappa dt / dl^2 = 0.25: the wet concentrations stay within the initial [min, max] widened by
    8 ulp of max |c| (the roughly twelve roundings of a convex combination of five values).  The restatement called
    directly at 0.30 leaves the bounds: the bound can fail."""
    f, h, q0 = _frame()
    cap = TM.kappa_cap(f.p)
    assert cap * f.p.dt / f.p.dl ** 2 == 0.25
    c, wet, lo, hi = _bounds(h, q0)
    margin = 8 * np.spacing(max(abs(lo), abs(hi)))
    q = q0
    for _ in range(400):
        q = TM.mix(f, h, q, kappa=cap)
    c1, _, lo1, hi1 = _bounds(h, q)
    over = max(lo - lo1, hi1 - hi, 0.0)
    print("at the cap: [%r, %r] -> [%r, %r], overshoot %.3g (margin %.3g)" % (lo, hi, lo1, hi1, over, margin))
    assert lo1 >= lo - margin and hi1 <= hi + margin, (lo, hi, lo1, hi1)
    assert c1[wet].std() < 0.5 * c[wet].std(), "nothing mixed"
    assert same_bits(q[0][~wet], q0[0][~wet])       # dry cells and the sentinel keep what they held
    q = q0
    worst = 0.0
    for _ in range(400):
        q = TM.mix(f, h, q, kappa=cap * 1.2)        # 0.30
        _, _, lo2, hi2 = _bounds(h, q)
        worst = max(worst, lo - lo2, hi2 - hi)
    print("at 0.30: overshoot %.3g" % worst)
    assert worst > 1.0e-3, worst


def test_content_is_conserved_on_a_closed_frame():
    """decay = source = 0: sum(mk_n q) per layer changes by rounding only.  The bound, in longdouble from the absolute
    values of the terms: a cell's update q + dt*((Gu - GuE) + (Gv - GvN))*i_dl rounds at most 5 times on terms no larger
    than A = dt*i_dl*(|Gu| + |GuE| + |Gv| + |GvN|) and once on the sum, no larger than |q| + A; every G appears once with
    each sign, in two cells, evaluated from the same bits, so the exact sum of the increments is zero and what remains is
    u * sum(5 A + |q| + A) per application (the two sums that are compared are formed in longdouble, whose own roundings
    are 2^-11 of that)."""
    f, h, q = _frame()
    cap = TM.kappa_cap(f.p)
    E, N, W, S = (f.neig[:, k].astype(np.int64) for k in (0, 2, 4, 6))
    here = np.arange(f.p.ndeg + 1)
    u = np.longdouble(np.finfo(np.float64).eps) / 2
    napp = 400
    total0 = np.sum((f.mk_n * q[0]).astype(np.longdouble), axis=1)
    bound = np.zeros(f.p.nlay, dtype=np.longdouble)
    for _ in range(napp):
        for l in range(f.p.nlay):
            c = TM.concentration(h[l], q[0, l])
            kd = cap * (1.0 / f.p.dl)
            Gu = np.abs(TM._face(kd, c, h[l], W, here)).astype(np.longdouble)
            Gv = np.abs(TM._face(kd, c, h[l], S, here)).astype(np.longdouble)
            A = np.longdouble(f.p.dt / f.p.dl) * (Gu + Gu[E] + Gv + Gv[N])
            bound[l] += u * np.sum((6 * A + np.abs(q[0, l]).astype(np.longdouble))[1:])
        q = TM.mix(f, h, q, kappa=cap)
    total = np.sum((f.mk_n * q[0]).astype(np.longdouble), axis=1)
    scale = np.sum(np.abs(q[0]).astype(np.longdouble), axis=1)
    drift = np.abs(total - total0)
    print("drift %s, bound %s, relative drift %s" % (drift, bound, drift / scale))
    assert np.all(drift <= bound), (drift, bound)
    assert np.all(bound <= 1.0e-11 * scale), (bound, scale)         # (the bound itself is tight enough to mean something)


def test_decay_and_source_follow_their_recursion():
    """kappa = 0, a uniform concentration: c <- c (1 - decay dt) + source dt, up to the roundings of the content form, and
    it reaches source / decay."""
    f, h, _ = _frame()
    wet = h > 0
    dt = f.p.dt
    decay, source, c0 = 1.0e-3, 2.0, 5.0
    q = (c0 * h)[None].copy()
    c = c0
    for n in range(2000):
        q = TM.mix(f, h, q, decay=decay, source=source)
        c = c * (1.0 - decay * dt) + source * dt
        if n in (0, 9, 1999):
            got = TM.concentration(h, q[0])
            assert np.max(np.abs(got[wet] - c)) <= 1.0e-12 * abs(c), (n, c)
    got = TM.concentration(h, q[0])[wet]
    print("after 2000 applications: %r .. %r (source / decay = %r)" % (got.min(), got.max(), source / decay))
    assert np.max(np.abs(got - source / decay)) <= 1.0e-9 * source / decay
    assert same_bits(q[0][~wet], np.zeros((~wet).sum()))


def test_each_coefficient_is_live_and_all_zero_is_the_identity():
    f, h, q = _frame()
    q3 = np.ascontiguousarray(np.broadcast_to(q, (3,) + q.shape[1:]))
    cap = TM.kappa_cap(f.p)
    base = dict(kappa=0.5 * cap, decay=1.0e-4, source=1.0e-3)
    ref = TM.mix(f, h, q3, **base)
    for k in base:
        other = TM.mix(f, h, q3, **dict(base, **{k: base[k] * 0.5}))
        assert not same_bits(other, ref), k
        alone = TM.mix(f, h, q3, **{k: base[k]})
        assert not same_bits(alone, q3), (k, "alone")
    # per tracer and per layer: tracer 1 has all three zero and comes back bit for bit, the others move
    kap = np.array([[cap, 0.0], [0.0, 0.0], [0.0, 0.0]])
    dec = np.array([0.0, 0.0, 1.0e-4])
    out = TM.mix(f, h, q3, kappa=kap, decay=dec)
    assert same_bits(out[1], q3[1])
    assert not same_bits(out[0][0], q3[0][0]) and same_bits(out[0][1], q3[0][1])
    assert not same_bits(out[2], q3[2])
    assert same_bits(TM.mix(f, h, q3), q3)


# ---- the binding --------------------------------------------------------------------------------------------------------------
def test_ctypes_prototypes_match_the_header():
    protos = _prototypes()
    lib = capi.load()
    assert set(capi.TRACER_MIX_EXPORTS) == {"beom_set_tracer_mixing", "beom_update_tracer_mixing", "beom_multi_set_tracer_mixing"}
    for name in capi.TRACER_MIX_EXPORTS:
        assert name in protos and name in capi.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int, name
        assert list(fn.argtypes) == [_CTYPE[t] for t in protos[name]], (name, protos[name], fn.argtypes)


def test_null_handle_is_refused():
    lib = capi.load()
    err = C.create_string_buffer(200)
    assert lib.beom_set_tracer_mixing(None, None, None, None, err, 199) == -1
    assert lib.beom_multi_set_tracer_mixing(None, None, None, None, err, 199) == -1
    assert lib.beom_update_tracer_mixing(None) == -1
