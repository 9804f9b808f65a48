"""The real*4 output records and the scans of write_outputs / write_array (private_mod.f95:2772-2974) restated in numpy
(helper module of test_outputs_cpu and test_gpu_outputs; not a conftest, imports nothing from the code under test: it
reads a Fields object of the init mirror and float64 state arrays [nlay, ndeg + 1]).  test_outputs_cpu pins it to the
real reference's files of every golden fixture.

Number formats: the state is real*8, every record real*4.  A real*4 value that goes on being used is rounded where the
reference rounds it: each partial sum of `eta_` (:2851-2869) and each term of `mont` (:2935-2947) is a real*4.
"""
import numpy as np

F4, F8 = np.float32, np.float64


def _p(f):
    p = f.p
    return p, int(p.nlay), int(p.ndeg)


def _r4(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a, dtype=F8).astype(F4)


def records(f, hlay, u, v, h0r4, pi_s=None):
    """eta, u4, v4 as float32 [nlay, ndeg] (:2848-2883).  eta is accumulated bottom-up, each partial sum rounded to real*4
    before the next layer is added; with rgld = 1 the top record is pi_s in real*4 (:2873).  (With one layer the reference
    reads ior4(:, 2), which does not exist; the one-layer goldens hold hlay - h_0, and so does this.)"""
    p, nl, nd = _p(f)
    h0r4 = np.asarray(h0r4, dtype=F4).reshape(nl, nd)
    eta = np.zeros((nl, nd), dtype=F4)
    for k in range(nl - 1, -1, -1):
        d = np.asarray(hlay[k, 1:], dtype=F8) - h0r4[k].astype(F8)
        eta[k] = _r4(d) if k == nl - 1 else _r4(d + eta[k + 1].astype(F8))
    if float(p.rgld) > 0.5:
        eta[0] = _r4(np.asarray(pi_s, dtype=F8)[1:])
    return eta, _r4(np.asarray(u)[:, 1:]), _r4(np.asarray(v)[:, 1:])


def scan_masks(f):
    """The cells 0..ndeg that the min/max of h, u and v run over (:2772-2793): wet cells; the u (v) points, or every cell,
    index 0 included, when no point of the mask is set."""
    n1 = int(f.p.ndeg) + 1
    wet = np.asarray(f.mk_n) > 0.5
    mu, mv = np.asarray(f.mk_u) > 0.5, np.asarray(f.mk_v) > 0.5
    return wet, (mu if mu.any() else np.ones(n1, bool)), (mv if mv.any() else np.ones(n1, bool))


def scans(f, hlay, u, v):
    """minmax [nlay, 6] = min h, max h, min u, max u, min v, max v per layer, and the thin-layer flag.

    The flag: the reference's loop (:2798-2808) runs ilay = 1, 2, ... and quits at the FIRST layer that has a wet cell
    1..ndeg with hlay < hmin / 2, with errc = -ilay; the Fortran host (beom_host_mod.f95, write_outputs) fails with
    -thin_layer and the same message.  So the flag names the LOWEST-NUMBERED (topmost) thin layer, 0 if there is none."""
    p, nl, nd = _p(f)
    wet, mu, mv = scan_masks(f)
    mm = np.zeros((nl, 6))
    thin = 0
    half = F8(0.5) * F8(p.hmin)
    for k in range(nl):
        h, a, b = np.asarray(hlay[k], dtype=F8), np.asarray(u[k], dtype=F8), np.asarray(v[k], dtype=F8)
        mm[k] = (h[wet].min(), h[wet].max(), a[mu].min(), a[mu].max(), b[mv].min(), b[mv].max())
        if thin == 0 and np.any(wet[1:] & (h[1:] < half)):
            thin = k + 1
    return mm, thin


def _powi(x, n):
    """x**n for a constant integer n: the left-to-right product."""
    r = x
    for _ in range(n - 1):
        r = r * x
    return r


def diag(f, hlay, u, v):
    """pvor, mont, v_cc as float32 [nlay, ndeg] (:2884-2974)."""
    p, nl, nd = _p(f)
    nb = np.asarray(f.neig).astype(np.int64)
    c1, c2, c3, c5, c6, c7 = (nb[:, k] for k in (0, 1, 2, 4, 5, 6))
    dl, uadv, bvis, dvis = F8(p.dl), F8(p.uadv), F8(p.bvis), F8(p.dvis)
    ocrp, hsal, hmin, nsal = F8(p.ocrp), F8(p.hsal), F8(p.hmin), int(p.nsal)
    rhon = np.asarray(p.rhon_v, dtype=F8)
    mkn, mkpe, mkpi = (np.asarray(getattr(f, k), dtype=F8) for k in ("mk_n", "mkpe", "mkpi"))
    fcor, h_th = np.asarray(f.fcor, dtype=F8), np.asarray(f.h_th, dtype=F8)
    H, U, V = (np.asarray(a, dtype=F8) for a in (hlay, u, v))
    pvor, mont, vcc = (np.zeros((nl, nd), dtype=F4) for _ in range(3))
    hsum = H[0].copy()                                             # sum( hlay(ipnt, :) ): left to right
    for m in range(1, nl):
        hsum = hsum + H[m]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k in range(nl):
            h, a, b = H[k], U[k], V[k]
            w1 = ((b - b[c5]) / dl - (a - a[c7]) / dl) * mkpe
            w2 = (a[c1] - a) / dl + (b[c3] - b) / dl
            w1[0] = 0.0; w2[0] = 0.0                               # wrk1(0, :), wrk2(0, :) keep their initial 0 (:2888-2893)
            q = ((w1[c1] - w1) ** 2 + (w1[c2] - w1[c3]) ** 2 + (w1[c3] - w1) ** 2 + (w1[c2] - w1[c1]) ** 2
                 + (w2[c1] - w2) ** 2 + (w2 - w2[c5]) ** 2 + (w2[c3] - w2) ** 2 + (w2 - w2[c7]) ** 2)
            vcc[k] = _r4(bvis + dvis * (dl * dl) * np.sqrt(q))[1:]
            acc = _r4(-(ocrp / F8(nsal - 1) * hsal * mkn * _powi(hsal / (hmin * (F8(1.0) - mkn) + h), nsal - 1)))
            for m in range(k):
                acc = acc - _r4((rhon[k] - rhon[m]) * H[m] / rhon[k])
            mont[k] = (acc + _r4(hsum - h_th))[1:]
            zeta = ((b - b[c5]) / dl - (a - a[c7]) / dl) * mkpe
            pvor[k] = _r4((fcor + zeta * uadv) * mkpi * (mkn + mkn[c5] + mkn[c7] + mkn[c6])
                          / (h + h[c5] + h[c6] + h[c7]))[1:]
    return pvor, mont, vcc


def same_r4(a, b):
    """Two real*4 records hold the same bits."""
    a, b = np.ascontiguousarray(a, dtype=F4), np.ascontiguousarray(b, dtype=F4)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))

