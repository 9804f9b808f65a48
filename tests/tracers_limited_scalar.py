"""The flux-limited tracer update (beom_set_tracer_scheme, scheme 2) once more, one cell, layer and tracer at a time: written
from the contract text of include/beom_hip.h ("Passive tracers", beom_set_tracer_scheme) and the header comment of
beom_tracers_lim.h alone, in plain Python loops over Python floats (IEEE FP64), with math.copysign and min, every expression
in the written order.  It shares no line with tracers_limited_ref or tracers_ref and imports neither: where the vectorised
restatement gathers whole arrays through np.where, this follows neig from a cell to its (U, D, UU) and decides every face on
its own.  The whole update of a cell: the four faces, src under hdot, the multistep rhsi, nudging with ctrg.  No tide (the
callers' frames have none; it is refused).  Slow, and meant to be.

Shapes as in tracers_ref: hlay, h_u, h_v [nlay, ndeg+1]; q, ctrg [ntrc, nlay, ndeg+1]; rq [ntrc, nlay, ndeg+1, 2]."""
import math

import numpy as np

T3 = 1.0 / 3.0


def conc(q, h):
    """c(x) = hlay(x,l) > 0 ? q(x,l) / hlay(x,l) : +0.0"""
    return q / h if h > 0.0 else 0.0


def stencil(x, F, back, fwd):
    """(U, D, UU) of the face of cell x towards its back neighbour B = back[x], F = the transport stored at x."""
    B = back[x]
    if F > 0.0:
        return B, x, back[B]
    return x, B, fwd[x]


def face_value(cU, wU, cD, wD, cUU, wUU):
    """cf of a face from the concentrations and wet flags of its (U, D, UU)."""
    first = cU if wU else cD
    if not (wU and wD and wUU):
        return first
    du = cU - cUU
    dd = cD - cU
    if du * dd > 0.0:
        m = min(min(2.0 * abs(du), 2.0 * abs(dd)), abs((du + 2.0 * dd) * T3))
        lim = math.copysign(m, dd)
    else:
        lim = 0.0
    return cU + 0.5 * lim


def flux(x, F, back, fwd, h, q):
    """flux = F * cf of the face of cell x towards back[x]; h, q: one layer of one tracer as lists over 0..ndeg."""
    U, D, UU = stencil(x, F, back, fwd)
    cf = face_value(conc(q[U], h[U]), h[U] > 0.0, conc(q[D], h[D]), h[D] > 0.0, conc(q[UU], h[UU]), h[UU] > 0.0)
    return F * cf


def update(f, hlay, h_u, h_v, q, rq, ctrg, gene):
    """Returns (q_new, rq_new) as arrays; the arguments are left as they are.  ctrg = None: +0.0 everywhere."""
    p = f.p
    nlay, n1 = int(p.nlay), int(p.ndeg) + 1
    assert not (f.has.get("tide", False) and np.any(f.tide != 0.0)), "the scalar reference leaves the tide out"
    E, N, W, S = (f.neig[:, k].tolist() for k in (0, 2, 4, 6))        # neig(1|3|5|7, p)
    assert E[0] == 0 and N[0] == 0 and W[0] == 0 and S[0] == 0
    i_dl = 1.0 / float(p.dl)
    dt, beta = float(p.dt), float(p.beta)
    gene = float(gene)
    hdot_present = bool(f.has.get("hdot", True)) and bool(np.any(f.hdot != 0.0))
    mk_n = np.asarray(f.mk_n, dtype=np.float64).tolist()
    nudg = np.asarray(f.nudg[0], dtype=np.float64).tolist()
    q = np.asarray(q, dtype=np.float64)
    rq = np.asarray(rq, dtype=np.float64)
    qn, rqn = q.copy(), rq.copy()
    for t in range(q.shape[0]):
        for l in range(nlay):
            h = np.asarray(hlay[l], dtype=np.float64).tolist()
            hu = np.asarray(h_u[l], dtype=np.float64).tolist()
            hv = np.asarray(h_v[l], dtype=np.float64).tolist()
            ql = q[t, l].tolist()
            r1l, r2l = rq[t, l, :, 0].tolist(), rq[t, l, :, 1].tolist()
            ctl = ctrg[t, l].tolist() if ctrg is not None else [0.0] * n1
            hd = np.asarray(f.hdot[l], dtype=np.float64).tolist() if hdot_present else None
            hfor = np.asarray(f.fnud[0, l], dtype=np.float64).tolist()
            for x in range(1, n1):
                Fu = flux(x, hu[x], W, E, h, ql)
                FuE = flux(E[x], hu[E[x]], W, E, h, ql)
                Fv = flux(x, hv[x], S, N, h, ql)
                FvN = flux(N[x], hv[N[x]], S, N, h, ql)
                if hdot_present:
                    src = hd[x] * (ctl[x] if hd[x] > 0.0 else conc(ql[x], h[x]))
                else:
                    src = 0.0
                r3 = ((Fu - FuE) * i_dl + (Fv - FvN) * i_dl + src) * mk_n[x]
                qh = ql[x] + (((1.5 + beta) * r3 - (0.5 + 2.0 * beta) * r2l[x] + beta * r1l[x]) * dt * gene + r3 * dt * (1.0 - gene))
                qn[t, l, x] = (ctl[x] * hfor[x]) * nudg[x] + (1.0 - nudg[x]) * qh
                rqn[t, l, x, 0] = r2l[x]
                rqn[t, l, x, 1] = r3
    return qn, rqn
