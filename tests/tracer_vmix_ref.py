"""The tracers' vertical (diapycnal) diffusion of include/beom_hip.h (beom_set_tracer_vmixing) restated in numpy: the
yardstick of the vertical-mixing tests.

One backward-Euler application to every water column from the thicknesses and contents of one time level: the tridiagonal
system of the FLUXES G_k through the interfaces k = 1..nlay-1 (between layers k and k+1, 1 = top), eliminated downwards and
substituted back, every expression in the order the header writes it.  dtype = np.float64 is the contract; np.longdouble
runs the same statements in extended precision on the same FP64 inputs (the measure of the contract's rounding).  Imports
nothing from the code under test (f is the init mirror's Fields, or anything with p.ndeg, p.nlay, p.dt and mk_n [ndeg+1]).

Shapes as in tracers_ref: hlay [nlay, ndeg+1]; q [ntrc, nlay, ndeg+1]; kappa_v broadcast to [ntrc, nlay-1]."""
import numpy as np


def coefficients(x, ntrc, nlay):
    """None, a scalar, [nlay-1] or [ntrc, nlay-1] -> [ntrc, nlay-1]; None = +0.0."""
    if x is None:
        return np.zeros((ntrc, nlay - 1))
    return np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), (ntrc, nlay - 1)))


def rk(p, kappa_v, dtype=np.float64):
    """1 / (dt * kappa_v) as the host forms it (product first, then reciprocal), +0.0 where kappa_v == 0."""
    k = np.asarray(kappa_v, dtype=np.float64).astype(dtype)
    prod = dtype(float(p.dt)) * k
    on = k != 0
    return np.where(on, dtype(1.0) / np.where(on, prod, dtype(1.0)), dtype(0.0))


def vmix(f, hlay, q, kappa_v, dtype=np.float64):
    """Returns (q', G); the arguments are left as they are.  q' [ntrc, nlay, ndeg+1] in dtype; G [ntrc, nlay+1, ndeg+1] with
    G[t, k] the content moved from layer k into layer k+1 (1-based), G[t, 0] = G[t, nlay] = +0.  Cell 0 keeps its q."""
    p = f.p
    nl = int(p.nlay)
    q = np.asarray(q, dtype=np.float64)
    ntrc, n = q.shape[0], q.shape[2]
    h = np.asarray(hlay, dtype=np.float64).astype(dtype)
    r = rk(p, coefficients(kappa_v, ntrc, nl), dtype)
    one, zero, half = dtype(1.0), dtype(0.0), dtype(0.5)
    m = h > 0
    cell = np.asarray(f.mk_n, dtype=np.float64) > 0.5
    out = q.astype(dtype)
    G = np.zeros((ntrc, nl + 1, n), dtype=dtype)
    with np.errstate(all="ignore"):
        b = np.where(m, one / np.where(m, h, one), zero)
        for t in range(ntrc):
            qq = q[t].astype(dtype)
            c = np.where(m, qq / np.where(m, h, one), zero)
            s, y = np.full(n, one, dtype=dtype), np.zeros(n, dtype=dtype)
            g, ys = np.zeros((max(nl - 1, 0), n), dtype=dtype), np.zeros((max(nl - 1, 0), n), dtype=dtype)
            for k in range(nl - 1):                     # interface k+1, between layers k+1 and k+2
                R = (half * (h[k] + h[k + 1])) * r[t, k]
                pp = R + b[k] * s
                den = pp + b[k + 1]
                inv = one / den
                num = (c[k] - c[k + 1]) + b[k] * y
                op = cell & m[k] & m[k + 1] & (r[t, k] > 0)
                g[k] = np.where(op, b[k + 1] * inv, zero)
                y = np.where(op, num * inv, zero)
                s = np.where(op, pp * inv, one)
                ys[k] = y
            if nl > 1:
                G[t, nl - 1] = ys[nl - 2]
            for k in range(nl - 2, 0, -1):
                G[t, k] = ys[k - 1] + g[k - 1] * G[t, k + 1]
            new = np.where(m, (qq + G[t, :nl]) - G[t, 1:], qq)
            out[t, :, 1:] = new[:, 1:]
    return out, G


def scale(q, G):
    """|q_l| + |G_{l-1}| + |G_l|: what the rounding of a layer's new content is measured in."""
    nl = q.shape[1]
    return np.abs(np.asarray(q, dtype=np.float64)) + np.abs(G[:, :nl]).astype(np.float64) + np.abs(G[:, 1:]).astype(np.float64)
