"""The maps of include/beom_hip.h (beom_set_maps) restated in numpy: the yardstick of their tests.

A record is, per aligned B x B block of the (mm+1) x (lm+1) rectangle, the sum of 1.0 over the live cells (n) and the sums of
the integrals' vol and ke terms (integrals_ref.terms), of the cells' own u and v, of the stored transports h_u, h_v and of the
tracer contents q: the value of every packed cell on the rectangle, +0.0 where there is no packed cell and at the duplicated
column lm+1 / row mm+1 of a periodic frame, the rectangle padded with +0.0 to whole blocks.  Inside a block each column's B
rows go through the pairwise tree over the row offset, then the B column sums through the pairwise tree over the column
offset.  Imports integrals_ref and nothing from the code under test (f is the init mirror's Fields)."""
import numpy as np

import integrals_ref as R

NAMES = ("h", "u", "v", "ke", "hu", "hv")


def entries(level):
    return 6 if level >= 2 else 3


def count(ntrc, nlay, level):
    return 0 if level < 1 else 1 + entries(level) * nlay + (ntrc * nlay if level >= 3 else 0)


def duplicates(f):
    """[ndeg+1] bool: the sentinel and the cells of the duplicated column lm+1 / row mm+1 of a periodic frame."""
    p = f.p
    dup = np.zeros(p.ndeg + 1, dtype=bool)
    dup[0] = True
    if float(p.xper) > 0.5:
        dup |= f.subc[0] == p.lm + 1
    if float(p.yper) > 0.5:
        dup |= f.subc[1] == p.mm + 1
    return dup


def terms(f, st, level, q=None):
    """[count, ndeg+1]: the term of every packed cell in a record's order of entries, +0.0 where the cell is not live."""
    nl = f.p.nlay
    dup = duplicates(f)
    t4 = R.terms(f, st)                                        # (vol, ke, ens, circ per layer, eta2; masked as the integrals are)
    own = lambda a: np.where(dup, 0.0, np.asarray(a, dtype=np.float64))
    out = [np.where(dup, 0.0, 1.0)]
    for l in range(nl):
        out += [t4[4 * l], own(st["u"][l]), own(st["v"][l])]
        if level >= 2:
            out += [t4[4 * l + 1], own(st["h_u"][l]), own(st["h_v"][l])]
    if level >= 3:
        q = np.asarray(q, dtype=np.float64)
        out += [own(q[t, l]) for t in range(q.shape[0]) for l in range(nl)]
    return np.array(out)


def rectangle(f, t):
    """[count, mm+1, lm+1]: the terms on the rectangle by integrals_ref.row_sums' scatter, +0.0 where there is no packed cell."""
    p = f.p
    a = np.zeros((t.shape[0], p.mm + 1, p.lm + 1))
    a[:, f.subc[1, 1:] - 1, f.subc[0, 1:] - 1] = t[:, 1:]
    return a


def block_sums(a, B):
    """[..., Mc, Lc]: a[..., M, L] padded with +0.0 to whole B x B blocks, rows of a block first, then its columns."""
    assert B >= 2 and B & (B - 1) == 0
    M, L = a.shape[-2:]
    Mc, Lc = -(-M // B), -(-L // B)
    b = np.zeros(a.shape[:-2] + (Mc * B, Lc * B))
    b[..., :M, :L] = a
    b = b.reshape(a.shape[:-2] + (Mc, B, Lc, B))
    while b.shape[-3] > 1:                                     # the row offset
        b = b[..., 0::2, :, :] + b[..., 1::2, :, :]
    while b.shape[-1] > 1:                                     # then the column offset
        b = b[..., 0::2] + b[..., 1::2]
    return b[..., 0, :, 0]


def record(f, st, level, B, q=None):
    """[count, Mc, Lc]: one record of the maps for the state st (hlay, u, v and, at level 2, h_u, h_v as [nlay, ndeg+1]; at
    level 3 q[ntrc, nlay, ndeg+1])."""
    return block_sums(rectangle(f, terms(f, st, level, q)), B)


def views(rec, ntrc, nlay, level):
    """n[Mc, Lc], h, u, v (ke, hu, hv) [nlay, Mc, Lc] and q[ntrc, nlay, Mc, Lc] of a record."""
    E = entries(level)
    Mc, Lc = rec.shape[-2:]
    fld = rec[1:1 + E * nlay].reshape(nlay, E, Mc, Lc)
    out = {"n": rec[0]}
    for m in range(E):
        out[NAMES[m]] = fld[:, m]
    if level >= 3:
        out["q"] = rec[1 + 6 * nlay:].reshape(ntrc, nlay, Mc, Lc)
    return out
