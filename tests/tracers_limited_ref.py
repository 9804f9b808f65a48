"""The flux-limited tracer scheme of include/beom_hip.h (beom_set_tracer_scheme, scheme 2) restated in numpy: the yardstick of
the tests of that scheme.

Everything of tracers_ref.update stays except the face concentration: where the upwind cell U, the downwind cell D and the cell
UU behind the upwind one are all wet, the face takes Koren's limited third-order value c(U) + 0.5 * lim; everywhere else it
takes the scheme-1 face of tracers_ref.  FP64 throughout, every expression in the order the header writes it.  Imports nothing
from the code under test (f is the init mirror's Fields).  Shapes as in tracers_ref."""
import numpy as np

import tracers_ref as T

T3 = 1.0 / 3.0
OUTCOMES = ("fallback", "lim0", "two_du", "two_dd", "third")


def wavy(f):
    """[nlay, ndeg+1]: a concentration without flat stretches, so that every outcome of the limiter occurs; +0.0 at the
    sentinel."""
    i, j = f.subc[0].astype(np.float64), f.subc[1].astype(np.float64)
    c = np.empty((f.p.nlay, f.p.ndeg + 1))
    for l in range(f.p.nlay):
        c[l] = 0.6 + 0.3 * np.sin(0.9 * i + 0.4 * l) * np.cos(0.7 * j + 0.3 * l) + 0.05 * np.sin(2.3 * i * j + l)
    c[:, 0] = 0.0
    return c


def _stencil(flux, back, fwd, here):
    """(U, D, UU) of every face: upwind, downwind and the cell behind the upwind one."""
    pos = flux > 0
    U = np.where(pos, back, here)
    D = np.where(pos, here, back)
    UU = np.where(pos, back[back], fwd[here])
    return U, D, UU


def _limited(c, U, D, UU):
    """(lim, which): Koren's limited term and which of its branches gave it (1 lim = 0, 2 m = 2|du|, 3 m = 2|dd|, 4 third order)."""
    du = c[U] - c[UU]
    dd = c[D] - c[U]
    a, b, t = 2.0 * np.abs(du), 2.0 * np.abs(dd), np.abs((du + 2.0 * dd) * T3)
    m = np.minimum(np.minimum(a, b), t)
    steep = du * dd > 0.0
    lim = np.where(steep, np.copysign(m, dd), 0.0)
    which = np.where(steep, np.where(m == t, 4, np.where(m == b, 3, 2)), 1)
    return lim, which


def _face(flux, c, wet, back, fwd, here):
    """flux * cf over all cells 0..ndeg under scheme 2."""
    U, D, UU = _stencil(flux, back, fwd, here)
    lim, _ = _limited(c, U, D, UU)
    full = wet[U] & wet[D] & wet[UU]
    return np.where(full, flux * (c[U] + 0.5 * lim), T._face(flux, c, wet, back, here))


def outcomes(f, hlay, h_u, h_v, q):
    """Counts over the faces with mk_u (mk_v) > 0.5, all layers of one tracer q [nlay, ndeg+1]: {outcome: number}."""
    E, N, W, S = (f.neig[:, k].astype(np.int64) for k in (0, 2, 4, 6))
    here = np.arange(f.p.ndeg + 1)
    n = dict.fromkeys(OUTCOMES, 0)
    for l in range(f.p.nlay):
        c, wet = T.concentration(hlay[l], q[l])
        for flux, back, fwd, mask in ((h_u[l], W, E, f.mk_u), (h_v[l], S, N, f.mk_v)):
            U, D, UU = _stencil(flux, back, fwd, here)
            _, which = _limited(c, U, D, UU)
            which = np.where(wet[U] & wet[D] & wet[UU], which, 0)[mask > 0.5]
            for k, name in enumerate(OUTCOMES):
                n[name] += int(np.sum(which == k))
    return n


def update(f, hlay, h_u, h_v, q, rq, ctrg, gene, ramp, ctim, scheme=2):
    """Returns (q_new, rq_new); the arguments are left as they are.  ctrg = None: +0.0 everywhere.  scheme = 1: tracers_ref."""
    if scheme == 1:
        return T.update(f, hlay, h_u, h_v, q, rq, ctrg, gene, ramp, ctim)
    assert scheme == 2, scheme
    p = f.p
    E, N, W, S = (f.neig[:, k].astype(np.int64) for k in (0, 2, 4, 6))
    assert E[0] == 0 and N[0] == 0 and W[0] == 0 and S[0] == 0          # the links of the sentinel
    here = np.arange(p.ndeg + 1)
    i_dl = 1.0 / float(p.dl)
    dt, beta = float(p.dt), float(p.beta)
    has_hdot = bool(f.has.get("hdot", True)) and bool(np.any(f.hdot != 0.0))
    has_tide = bool(f.has.get("tide", True)) and bool(np.any(f.tide != 0.0))
    nudg = f.nudg[0]
    q = np.asarray(q, dtype=np.float64)
    rq = np.asarray(rq, dtype=np.float64)
    qn, rqn = q.copy(), rq.copy()
    for t in range(q.shape[0]):
        for l in range(p.nlay):
            h = hlay[l]
            ct = ctrg[t, l] if ctrg is not None else np.zeros(p.ndeg + 1)
            c, wet = T.concentration(h, q[t, l])
            Fu = _face(h_u[l], c, wet, W, E, here)
            Fv = _face(h_v[l], c, wet, S, N, here)
            src = f.hdot[l] * np.where(f.hdot[l] > 0, ct, c) if has_hdot else 0.0
            r3 = ((Fu - Fu[E]) * i_dl + (Fv - Fv[N]) * i_dl + src) * f.mk_n
            r1, r2 = rq[t, l, :, 0], rq[t, l, :, 1]
            rhsi = ((1.5 + beta) * r3 - (0.5 + 2.0 * beta) * r2 + beta * r1) * dt * gene + r3 * dt * (1.0 - gene)
            qh = q[t, l] + rhsi
            hfor = f.fnud[0, l]
            if has_tide:
                vecl = 1.0 if l == 0 else 0.0
                hfor = hfor + ramp * f.tide[0, :, 0, 0] * vecl * np.cos(f.tide[0, :, 0, 1] - float(f.w_ti[0]) * ctim)
            new = (ct * hfor) * nudg + (1.0 - nudg) * qh
            qn[t, l, 1:] = new[1:]
            rqn[t, l, 1:, 0] = r2[1:]
            rqn[t, l, 1:, 1] = r3[1:]
    return qn, rqn
