"""The tracer column series of include/beom_hip.h (beom_set_tracer_column_series) restated in numpy: the yardstick of its tests.

A record holds, per column of the (mm+1) x (lm+1) rectangle, tracer and layer, the column sums of the tracer series' per-cell
terms x_q, x_v, x_fu, x_fv (tracer_series_ref.cell_terms: +0.0 where a cell is not live) and the bounds of x_b = c + 0.0 over
the column's live wet cells.  The terms are scattered onto the rectangle, +0.0 where there is no packed cell and in every row
outside the window, and every column goes through the integrals' pairwise tree over the rows (integrals_ref.tree); the bounds
are np.min / np.max over the window with +inf / -inf as initial values.  Imports tracer_series_ref and integrals_ref and
nothing from the code under test (f is the init mirror's Fields).

Shapes: hlay, h_u, h_v [nlay, ndeg+1]; q [ntrc, nlay, ndeg+1]; a record [lm+1, ntrc*nlay*nq], entry (t*nlay + l)*nq + m."""
import numpy as np

import integrals_ref as R
import tracer_series_ref as TS

NAMES = TS.NAMES
nq = TS.nq
count = TS.count


def column_record(f, hlay, h_u, h_v, q, level, rows=None):
    """[lm+1, count]: one record of the tracer column series for the arrays as they stand; rows = (jlo, jhi), 1-based and
    inclusive, None = 1..mm+1."""
    p = f.p
    n = nq(level)
    q = np.asarray(q, dtype=np.float64)
    ntrc, nlay = q.shape[0], p.nlay
    t, xb, wet = TS.cell_terms(f, hlay, h_u, h_v, q)
    M, L = p.mm + 1, p.lm + 1
    jlo, jhi = (1, M) if rows is None else rows
    jj, ii = f.subc[1, 1:] - 1, f.subc[0, 1:] - 1
    ns = min(n, 4)
    a = np.zeros((ns, ntrc, nlay, M, L))
    a[..., jj, ii] = t[:ns][..., 1:]
    a[..., :jlo - 1, :] = 0.0
    a[..., jhi:, :] = 0.0
    rec = np.zeros((L, ntrc, nlay, n))
    sums = R.tree(np.swapaxes(a, -1, -2).reshape(ns * ntrc * nlay, L, M))          # [ns*ntrc*nlay, L]
    rec[..., :ns] = np.moveaxis(sums.reshape(ns, ntrc, nlay, L), (0, 3), (3, 0))
    if level >= 3:
        for m, (pad, red) in enumerate(((np.inf, np.min), (-np.inf, np.max))):
            B = np.full((ntrc, nlay, M, L), pad)                       # the rectangle, the identity where nothing is live and wet
            B[:, :, jj, ii] = np.where(wet[None, :, 1:], xb[:, :, 1:], pad)
            B[:, :, :jlo - 1, :] = pad
            B[:, :, jhi:, :] = pad
            rec[..., 4 + m] = np.moveaxis(red(B, axis=2, initial=pad), 2, 0)
    return np.ascontiguousarray(rec.reshape(L, ntrc * nlay * n))


def views(cols, ntrc, nlay, level):
    """dict of inv, var (, fu, fv (, cmin, cmax)) [..., lm+1, ntrc, nlay] from cols[..., lm+1, count]."""
    return TS.views(cols, ntrc, nlay, level)


def total(cols, ntrc, nlay, level):
    """[..., ntrc, nlay]: the integrals' tree over the columns of inv."""
    return TS.total(cols, ntrc, nlay, level)


def gamma_bound(f, hlay, h_u, h_v, q):
    """[ntrc, nlay]: 2 * gamma_D * sum |x_q|, the bound on the difference of two pairwise trees over the same terms (rows first
    or columns first), as column_series_ref.gamma_bound derives it: gamma_D = D*u / (1 - D*u), u = 2^-53,
    D = ceil(log2 L) + ceil(log2 M)."""
    p = f.p
    D = int(np.ceil(np.log2(p.lm + 1))) + int(np.ceil(np.log2(p.mm + 1)))
    u = 2.0 ** -53
    t, _, _ = TS.cell_terms(f, hlay, h_u, h_v, q)
    return 2.0 * (D * u / (1.0 - D * u)) * np.abs(t[0]).sum(axis=-1)
