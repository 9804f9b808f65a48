"""The tracer series of include/beom_hip.h (beom_set_tracer_series) restated in numpy: the yardstick of the tracer series tests.

A record holds, per tracer and layer, the row sums of x_q = q, x_v = x_q * c (rounded, then summed), x_fu, x_fv (the upstream
faces) and the bounds of x_b = c + 0.0 over the live wet cells of the row.  x_q, c, x_fu, x_fv are rows 0, 1, 2, 3 of
tracer_moments_ref.quantities; the live rule is the duplicate mask of series_ref.transport_terms; the rows go through
integrals_ref.row_sums (the integrals' pairwise tree); the bounds are np.min / np.max with +inf / -inf as initial values.
Imports nothing from the code under test (f is the init mirror's Fields).

Shapes: hlay, h_u, h_v [nlay, ndeg+1]; q [ntrc, nlay, ndeg+1]; a record [mm+1, ntrc*nlay*nq], entry (t*nlay + l)*nq + m."""
import numpy as np

import integrals_ref as R
import series_ref as S
import tracer_moments_ref as TM

NAMES = ("inv", "var", "fu", "fv", "cmin", "cmax")


def nq(level):
    assert level in (1, 2, 3), level
    return 2 * level


def count(ntrc, nlay, level):
    return ntrc * nlay * nq(level)


def live_mask(f):
    """[ndeg+1] bool: packed cells that are not on the duplicated column / row of a periodic frame (the sentinel is not
    live) — where series_ref.transport_terms lets a value through."""
    one = np.ones((f.p.nlay, f.p.ndeg + 1))
    return S.transport_terms(f, {"h_u": one, "h_v": one})[0] != 0.0


def cell_terms(f, hlay, h_u, h_v, q):
    """x[4, ntrc, nlay, ndeg+1] = x_q, x_v, x_fu, x_fv with +0.0 where the cell is not live; xb[ntrc, nlay, ndeg+1] = c + 0.0;
    wet[nlay, ndeg+1] = live and hlay > 0."""
    x = TM.quantities(f, hlay, h_u, h_v, q)
    live = live_mask(f)
    xv = x[0] * x[1]
    t = np.stack([x[0], xv, x[2], x[3]])
    t = np.where(live, t, 0.0)
    xb = x[1] + 0.0
    wet = live[None, :] & (np.asarray(hlay, dtype=np.float64) > 0.0)
    return t, xb, wet


def row_record(f, hlay, h_u, h_v, q, level):
    """[mm+1, count]: one record of the tracer series for the arrays as they stand."""
    p = f.p
    n = nq(level)
    q = np.asarray(q, dtype=np.float64)
    ntrc, nlay = q.shape[0], p.nlay
    t, xb, wet = cell_terms(f, hlay, h_u, h_v, q)
    M = p.mm + 1
    rec = np.zeros((M, ntrc, nlay, n))
    ns = min(n, 4)
    sums = R.row_sums(f, t[:ns].reshape(ns * ntrc * nlay, p.ndeg + 1))          # [M, ns*ntrc*nlay]
    rec[..., :ns] = np.moveaxis(sums.reshape(M, ns, ntrc, nlay), 1, 3)
    if level >= 3:
        jj, ii = f.subc[1, 1:] - 1, f.subc[0, 1:] - 1
        for m, (pad, red) in enumerate(((np.inf, np.min), (-np.inf, np.max))):
            B = np.full((ntrc, nlay, M, p.lm + 1), pad)                      # the rectangle, the identity where nothing is live and wet
            B[:, :, jj, ii] = np.where(wet[None, :, 1:], xb[:, :, 1:], pad)
            rec[..., 4 + m] = np.moveaxis(red(B, axis=-1, initial=pad), 2, 0)
    return np.ascontiguousarray(rec.reshape(M, ntrc * nlay * n))


def views(rows, ntrc, nlay, level):
    """dict of inv, var (, fu, fv (, cmin, cmax)) [..., mm+1, ntrc, nlay] from rows[..., mm+1, count]."""
    rows = np.asarray(rows)
    n = nq(level)
    r = rows.reshape(rows.shape[:-1] + (ntrc, nlay, n))
    return {NAMES[m]: r[..., m] for m in range(n)}


def total(rows, ntrc, nlay, level):
    """[..., ntrc, nlay]: the integrals' tree over the rows of inv."""
    inv = views(rows, ntrc, nlay, level)["inv"]
    return R.tree(np.moveaxis(inv, -3, -1))
