"""The column series (beom_set_column_series), the part that needs no GPU: the numpy restatement (column_series_ref) against a
plain Python loop in tree order and against the integrals' restatement, on states the oracle has stepped from rough inputs
(as test_series_cpu builds them) and on the rough 130 x 18 frames."""
import numpy as np
import pytest

import column_series_ref as CS
import integrals_ref as R
import rough_inputs as RI
import series_ref as S
from helpers import same_bits
from test_series_cpu import _stepped, _tree_py

NAMES = ["island_ragged_3l", "jet_xyper_2l"]
FIELDS = ("hlay", "u", "v", "h_u", "h_v")


def _rough(config):
    g = RI.rough_fields(RI.base_fields(config, "130x18"), 1)
    return g, {k: getattr(g, k) for k in FIELDS}


def _loop_columns(f, t, rows=None):
    """[lm+1, count]: every column of the terms t[count, ndeg+1] placed on its rows (+0.0 elsewhere and outside the window)
    and added in tree order, one Python float at a time."""
    p = f.p
    out = np.zeros((p.lm + 1, t.shape[0]))
    cells = [[] for _ in range(p.lm + 2)]
    for ipnt in range(1, p.ndeg + 1):
        cells[int(f.subc[0, ipnt])].append(ipnt)
    jlo, jhi = rows or (1, p.mm + 1)
    for i in range(1, p.lm + 2):
        for k in range(t.shape[0]):
            col = [0.0] * (p.mm + 1)
            for ipnt in cells[i]:
                j = int(f.subc[1, ipnt])
                if jlo <= j <= jhi:
                    col[j - 1] = t[k, ipnt]
            out[i - 1, k] = _tree_py(col)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_a_plain_loop_in_tree_order(name):
    """island_ragged_3l: land leaves gaps in the columns.  jet_xyper_2l: the duplicated column and row contribute +0.0."""
    g, st = _stepped(name)
    nl = g.p.nlay
    t = np.concatenate([R.terms(g, st), S.transport_terms(g, st)])
    want = _loop_columns(g, t)
    rec = CS.column_record(g, st, 2)
    assert rec.shape == (g.p.lm + 1, CS.count(nl, 2)) and same_bits(rec, want)
    assert same_bits(CS.column_record(g, st, 1), want[:, :4 * nl + 1])
    assert same_bits(CS.phi(rec, g.p)[:, nl - 1], float(g.p.dl) * np.cumsum(rec[:, 4 * nl + 1:5 * nl + 1], axis=1)[:, nl - 1])


def _check_bound(g, st):
    """-> how many entries differ between the two orders, the largest ratio to the bound."""
    nl = g.p.nlay
    a, b = CS.total(CS.column_record(g, st, 1), nl), R.integrals(g, st)
    bound = CS.gamma_bound(g, st)
    diff = np.abs(a - b)
    print("columns first vs rows first: |diff| / bound =", diff / np.where(bound > 0, bound, 1.0))
    assert np.all(diff <= bound), (diff, bound)
    return int((a != b).sum()), float(np.max(diff / np.where(bound > 0, bound, 1.0)))


@pytest.mark.parametrize("name", NAMES)
def test_tree_over_the_columns_is_within_the_bound_of_the_integrals(name):
    """Two pairwise trees over the same terms, columns first and rows first: each entry within 2 * gamma_D * sum |T_k|, on the
    oracle-stepped state and on the rough 130 x 18 frame; on the latter the two differ in most entries, so the comparison is
    not vacuous."""
    _check_bound(*_stepped(name))
    ndiff, _ = _check_bound(*_rough(name))
    assert ndiff >= 1, "the two orders of summation agree bit for bit everywhere: nothing compared"


@pytest.mark.parametrize("name", NAMES)
def test_row_window(name):
    g, st = _stepped(name)
    M = g.p.mm + 1
    whole = CS.column_record(g, st, 2)
    assert same_bits(CS.column_record(g, st, 2, rows=(1, M)), whole)
    t = np.concatenate([R.terms(g, st), S.transport_terms(g, st)])
    for rows in ((20, 41), (M, M), (1, 1)):
        rec = CS.column_record(g, st, 2, rows=rows)
        assert same_bits(rec, _loop_columns(g, t, rows)), rows
        out = (g.subc[1] < rows[0]) | (g.subc[1] > rows[1])
        assert same_bits(rec, _loop_columns(g, np.where(out[None, :], 0.0, t))), rows
    assert not same_bits(CS.column_record(g, st, 2, rows=(20, 41)), whole)


def test_rough_transports_differ_from_column_to_column():
    g, st = _rough("jet_xyper_2l")
    p, nl = g.p, g.p.nlay
    tu = CS.column_record(g, st, 2)[:, 4 * nl + 1:5 * nl + 1]
    assert np.all(tu[1:p.lm] != 0.0)
    assert np.all(tu[2:p.lm] != tu[1:p.lm - 1])


def test_duplicated_column_is_plus_zero():
    for g, st in (_stepped("jet_xyper_2l"), _rough("jet_xyper_2l")):
        p = g.p
        assert float(p.xper) > 0.5
        dup = (g.subc[0] == p.lm + 1) | (g.subc[1] == p.mm + 1)
        dup[0] = False
        st2 = dict(st, h_u=np.where(dup[None, :], 1.5, st["h_u"]), h_v=np.where(dup[None, :], -2.5, st["h_v"]))
        rec = CS.column_record(g, st2, 2)
        assert not rec[p.lm].any() and not np.signbit(rec[p.lm]).any()
        assert same_bits(rec, CS.column_record(g, st, 2))
