"""The series of row sums of include/beom_hip.h (beom_set_series) restated in numpy: the yardstick of the series tests.

A record is the integrals' row sums (integrals_ref.row_sums of integrals_ref.terms) followed, at level 2, by the row sums of
the stored transports h_u, h_v per layer: the value of every packed cell on the (mm+1) x (lm+1) rectangle, +0.0 where there
is no packed cell and at the duplicated column lm+1 / row mm+1 of a periodic frame, every row through the integrals' pairwise
tree.  Imports integrals_ref and nothing from the code under test (f is the init mirror's Fields)."""
import numpy as np

import integrals_ref as R


def count(nlay, level):
    return (6 if level >= 2 else 4) * nlay + 1


def transport_terms(f, st):
    """[2*nlay, ndeg+1]: h_u per layer, then h_v per layer, +0.0 at the sentinel and at the duplicated column / row."""
    p = f.p
    t = np.concatenate([np.asarray(st["h_u"], dtype=np.float64), np.asarray(st["h_v"], dtype=np.float64)])
    dup = np.zeros(p.ndeg + 1, dtype=bool)
    dup[0] = True
    if float(p.xper) > 0.5:
        dup |= f.subc[0] == p.lm + 1
    if float(p.yper) > 0.5:
        dup |= f.subc[1] == p.mm + 1
    return np.where(dup[None, :], 0.0, t)


def row_record(f, st, level):
    """[mm+1, count]: one record of the series for the state st (hlay, u, v and, at level 2, h_u, h_v as [nlay, ndeg+1])."""
    rows = R.row_sums(f, R.terms(f, st))
    if level < 2:
        return rows
    return np.ascontiguousarray(np.concatenate([rows, R.row_sums(f, transport_terms(f, st))], axis=1))


def psi(rows, p):
    """[..., mm+1, nlay] = dl * cumsum over layers of tv: the transport above the base of layer l through the south faces of
    a row, from level-2 records rows[..., mm+1, 6*nlay+1]."""
    nl = p.nlay
    return float(p.dl) * np.cumsum(np.asarray(rows)[..., 5 * nl + 1:6 * nl + 1], axis=-1)
