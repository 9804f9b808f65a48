"""The tracers' diffusion, decay and sources of include/beom_hip.h (beom_set_tracer_mixing) restated in numpy: the yardstick
of the tracer-mixing tests.

One forward-Euler application to every tracer from the thicknesses and contents of one time level: the flux form of
div(kappa h grad c) with the face as thick as the thinner of its two cells, a decay rate and a concentration source.  FP64
throughout, every expression in the order the header writes it.  Imports nothing from the code under test (f is the init
mirror's Fields, or anything with p.ndeg, p.nlay, p.dl, p.dt, neig [ndeg+1, 8] and mk_n [ndeg+1]).

Shapes as in tracers_ref: hlay [nlay, ndeg+1]; q [ntrc, nlay, ndeg+1]; kappa, decay, source broadcast to [ntrc, nlay]."""
import numpy as np


def coefficients(x, ntrc, nlay):
    """None, a scalar, [ntrc] or [ntrc, nlay] -> [ntrc, nlay]; None = +0.0."""
    if x is None:
        return np.zeros((ntrc, nlay))
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    return np.ascontiguousarray(np.broadcast_to(x, (ntrc, nlay)))


def kappa_cap(p):
    """The largest kappa with kappa * dt / dl^2 <= 0.25 (as the double nearest to 0.25 * dl * dl / dt)."""
    return 0.25 * float(p.dl) * float(p.dl) / float(p.dt)


def concentration(h, q):
    """c = q / hlay where hlay > 0, else +0.0."""
    wet = h > 0
    with np.errstate(all="ignore"):
        return np.where(wet, q / np.where(wet, h, 1.0), 0.0)


def _face(kd, c, h, back, here):
    """G(back, here) over all cells 0..ndeg: the diffusive flux of content into `here` through the face towards `back`."""
    hf = np.minimum(h[back], h[here])
    with np.errstate(all="ignore"):
        return np.where(hf > 0, (kd * hf) * (c[back] - c[here]), 0.0)


def mix(f, hlay, q, kappa=None, decay=None, source=None, dt=None):
    """Returns q_mix; the arguments are left as they are.  dt: the step of this application (the handle's p.dt)."""
    p = f.p
    E, N, W, S = (np.asarray(f.neig)[:, k].astype(np.int64) for k in (0, 2, 4, 6))
    here = np.arange(p.ndeg + 1)
    i_dl = 1.0 / float(p.dl)
    dt = float(p.dt) if dt is None else float(dt)
    q = np.asarray(q, dtype=np.float64)
    ntrc = q.shape[0]
    kappa, decay, source = (coefficients(x, ntrc, p.nlay) for x in (kappa, decay, source))
    mk_n = np.asarray(f.mk_n, dtype=np.float64)
    out = q.copy()
    for t in range(ntrc):
        for l in range(p.nlay):
            h = np.asarray(hlay[l], dtype=np.float64)
            c = concentration(h, q[t, l])
            kd = kappa[t, l] * i_dl
            Gu = _face(kd, c, h, W, here)             # Gu[E] is G(W(E), E) with E's own back link, Gu[0] = G(0, 0) = +0
            Gv = _face(kd, c, h, S, here)
            div = ((Gu - Gu[E]) + (Gv - Gv[N])) * i_dl
            r = ((div + source[t, l] * h) - decay[t, l] * q[t, l]) * mk_n
            new = np.where(h > 0, q[t, l] + dt * r, q[t, l])
            out[t, l, 1:] = new[1:]
    return out
