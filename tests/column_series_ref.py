"""The column series of include/beom_hip.h (beom_set_column_series) restated in numpy: the yardstick of its tests.

A record is, per column of the (mm+1) x (lm+1) rectangle, the integrals' terms (integrals_ref.terms) followed, at level 2, by
the stored transports h_u, h_v per layer (series_ref.transport_terms): the value of every packed cell on the rectangle, +0.0
where there is no packed cell, at the duplicated column lm+1 / row mm+1 of a periodic frame and in every row outside the
window, every column through the integrals' pairwise tree over the rows.  Imports integrals_ref and series_ref and nothing
from the code under test (f is the init mirror's Fields)."""
import numpy as np

import integrals_ref as R
import series_ref as S

count = S.count


def rectangle(f, st, level, rows=None):
    """[count, mm+1, lm+1]: the terms on the rectangle, the rows outside the window rows = (jlo, jhi) (1-based, inclusive)
    zeroed."""
    p = f.p
    t = R.terms(f, st)
    if level >= 2:
        t = np.concatenate([t, S.transport_terms(f, st)])
    a = np.zeros((t.shape[0], p.mm + 1, p.lm + 1))
    a[:, f.subc[1, 1:] - 1, f.subc[0, 1:] - 1] = t[:, 1:]
    if rows is not None:
        jlo, jhi = rows
        a[:, :jlo - 1, :] = 0.0
        a[:, jhi:, :] = 0.0
    return a


def column_record(f, st, level, rows=None):
    """[lm+1, count]: one record of the column series for the state st (hlay, u, v and, at level 2, h_u, h_v as
    [nlay, ndeg+1])."""
    a = rectangle(f, st, level, rows)
    return np.ascontiguousarray(R.tree(np.swapaxes(a, 1, 2)).T)


def total(cols, nlay):
    """[4*nlay + 1]: the integrals' tree over the columns of a record."""
    return R.tree(np.asarray(cols, dtype=np.float64)[:, :4 * nlay + 1].T)


def phi(cols, p):
    """[..., lm+1, nlay] = dl * cumsum over layers of tu, from level-2 records cols[..., lm+1, 6*nlay+1]."""
    nl = p.nlay
    return float(p.dl) * np.cumsum(np.asarray(cols)[..., 4 * nl + 1:5 * nl + 1], axis=-1)


def gamma_bound(f, st):
    """[4*nlay + 1]: 2 * gamma_D * sum |T_k|, the bound on the difference of two pairwise trees over the same terms (rows
    first or columns first): gamma_D = D*u / (1 - D*u), u = 2^-53, D = ceil(log2 L) + ceil(log2 M)."""
    p = f.p
    D = int(np.ceil(np.log2(p.lm + 1))) + int(np.ceil(np.log2(p.mm + 1)))
    u = 2.0 ** -53
    return 2.0 * (D * u / (1.0 - D * u)) * np.abs(R.terms(f, st)).sum(axis=1)
