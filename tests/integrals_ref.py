"""The conservation integrals of include/beom_hip.h (beom_integrals) restated in numpy: the yardstick of the integral tests.

Terms by gathering through neig from a Fields object and a state dict (hlay, u, v as [nlay, ndeg+1]), FP64 throughout, every
expression in the order the header writes it; the scatter to the (mm+1) x (lm+1) rectangle by subc; a row by the pairwise
tree over the aligned column index (repeated a[0::2] + a[1::2], the row padded with +0.0 to a power of two), the row sums by
the same tree.  Imports nothing from the code under test (f is the init mirror's Fields)."""
import numpy as np

QUANTITIES = ("vol", "ke", "ens", "circ")


def tree(a):
    """Pairwise tree over the last axis, padded with +0.0 to the next power of two."""
    a = np.asarray(a, dtype=np.float64)
    n = 1
    while n < a.shape[-1]:
        n *= 2
    b = np.zeros(a.shape[:-1] + (n,))
    b[..., :a.shape[-1]] = a
    while b.shape[-1] > 1:
        b = b[..., 0::2] + b[..., 1::2]
    return b[..., 0]


def vorticity(f, st, l):
    """rvor, pvor of layer l (0-based) as update_mont_rvor_pvor_dive_kine stores them (private_mod.f95:2388-2389, 2421-2433),
    and have, nm."""
    p = f.p
    W, SW, S = (f.neig[:, k].astype(np.int64) for k in (4, 5, 6))
    h, u, v = st["hlay"][l], st["u"][l], st["v"][l]
    idl = 1.0 / float(p.dl)                                     # :2321
    rv = (v - v[W] - u + u[S]) * idl * f.mkpe
    have = h + h[W] + h[SW] + h[S]
    nm = f.mk_n + f.mk_n[W] + f.mk_n[SW] + f.mk_n[S]
    with np.errstate(all="ignore"):
        pv = (f.fcor + rv * float(p.uadv)) * f.mkpi * nm / have
    pv[0] = 0.0                                                 # the sentinel is never written (:273)
    rv[0] = 0.0
    return rv, pv, have, nm


def terms(f, st, mask_duplicates=True):
    """[4*nlay + 1, ndeg+1]: the term of every packed cell, +0.0 at the sentinel and (mask_duplicates) at the duplicated
    column lm+1 / row mm+1 of a periodic frame."""
    p = f.p
    W, S = f.neig[:, 4].astype(np.int64), f.neig[:, 6].astype(np.int64)
    out = []
    hcol = np.zeros(p.ndeg + 1)
    for l in range(p.nlay):
        h, u, v = st["hlay"][l], st["u"][l], st["v"][l]
        hcol = hcol + h                                        # :2367-2373
        hcu = (h[W] + h) / (1.0 + f.mk_u)                      # :1438
        hcv = (h + h[S]) / (1.0 + f.mk_v)                      # :1521
        rv, pv, have, nm = vorticity(f, st, l)
        with np.errstate(all="ignore"):
            ens = np.where((f.mkpi > 0.5) & (nm > 0), 0.5 * (pv * pv) * (have / nm), 0.0)
        out += [f.mk_n * h, f.mk_u * ((u * u) * hcu) + f.mk_v * ((v * v) * hcv), ens, rv]
    eta = hcol - f.h_th
    out.append(f.mk_n * (eta * eta))
    t = np.array(out)
    t[:, 0] = 0.0
    if mask_duplicates:
        dup = np.zeros(p.ndeg + 1, dtype=bool)
        if float(p.xper) > 0.5:
            dup |= f.subc[0] == p.lm + 1
        if float(p.yper) > 0.5:
            dup |= f.subc[1] == p.mm + 1
        t[:, dup] = 0.0
    return t


def row_sums(f, t):
    """[mm+1, 4*nlay + 1]: the terms on the rectangle (+0.0 where there is no packed cell), every row through the tree."""
    p = f.p
    R = np.zeros((t.shape[0], p.mm + 1, p.lm + 1))
    R[:, f.subc[1, 1:] - 1, f.subc[0, 1:] - 1] = t[:, 1:]
    return np.ascontiguousarray(tree(R).T)


def combine(rows):
    """[count]: the tree over the row sums rows[nrows, count]."""
    return tree(np.asarray(rows, dtype=np.float64).T)


def integrals(f, st):
    """The 4*nlay + 1 raw sums, layout out[l*4 + q] for q = vol, ke, ens, circ, then eta2."""
    return combine(row_sums(f, terms(f, st)))
