"""The passive-tracer update of include/beom_hip.h (beom_update_tracers) restated in numpy: the yardstick of the tracer tests.

One update of every tracer from the thicknesses and face transports update_h is about to read (DESIGN.md f-N6): first-order
upstream fluxes of the concentration c = q / hlay with the no-gradient rule at empty upwind cells, the source and relaxation
terms of update_h carrying the relaxation concentration ctrg, and update_h's own time scheme.  FP64 throughout, every
expression in the order the header writes it.  Imports nothing from the code under test (f is the init mirror's Fields).

Shapes: hlay, h_u, h_v [nlay, ndeg+1]; q, ctrg [ntrc, nlay, ndeg+1]; rq [ntrc, nlay, ndeg+1, 2] (as rs_h per tracer)."""
import numpy as np


def step_scalars(p, tstp, tres=0.0):
    """(gene, ramp, ctim) of time step tstp as integrate_time sets them (private_mod.f95:1858-1901; no rigid lid)."""
    dtd8, dt_r, rsta = float(p.dtd8), float(p.dt_r), float(p.rsta)
    ctim = tres + dtd8 * float(tstp)
    ramp = 1.0
    if tstp <= 3:
        c1 = tres + dtd8 * 1.0
        if rsta < 0.5 and c1 < dt_r:
            ramp = c1 / dt_r
    elif rsta < 0.5 and ctim < dt_r:
        ramp = ctim / dt_r
    gene = 0.0 if tstp <= 3 else float(p.g_fb)
    return gene, ramp, ctim


def patchy(f, low=0.25, high=1.0):
    """[nlay, ndeg+1]: a concentration in rectangular patches of 5 x 4 cells, shifted by one patch from layer to layer; +0.0
    at the sentinel."""
    i, j = f.subc[0].astype(np.int64), f.subc[1].astype(np.int64)
    c = np.empty((f.p.nlay, f.p.ndeg + 1))
    for l in range(f.p.nlay):
        c[l] = np.where((i // 5 + j // 4 + l) % 2 == 0, high, low)
    c[:, 0] = 0.0
    return c


def concentration(h, q):
    """c = q / hlay where hlay > 0, else +0.0."""
    wet = h > 0
    with np.errstate(all="ignore"):
        return np.where(wet, q / np.where(wet, h, 1.0), 0.0), wet


def _face(flux, c, wet, back, here):
    """flux * cf over all cells 0..ndeg: the upwind cell's concentration, the other side's where the upwind cell is empty."""
    pos = flux > 0
    a = np.where(pos, back, here)
    b = np.where(pos, here, back)
    return flux * np.where(wet[a], c[a], c[b])


def update(f, hlay, h_u, h_v, q, rq, ctrg, gene, ramp, ctim):
    """Returns (q_new, rq_new); the arguments are left as they are.  ctrg = None: +0.0 everywhere."""
    p = f.p
    E, N, W, S = (f.neig[:, k].astype(np.int64) for k in (0, 2, 4, 6))
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
            c, wet = concentration(h, q[t, l])
            Fu = _face(h_u[l], c, wet, W, here)
            Fv = _face(h_v[l], c, wet, S, here)
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
