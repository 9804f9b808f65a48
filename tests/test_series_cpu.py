"""The series of row sums (beom_set_series), the part that needs no GPU: the numpy restatement (series_ref) against the
integrals' restatement and against a plain Python loop in tree order, on states the oracle has stepped from rough inputs; and
the record sizes the library reports."""
import numpy as np
import pytest

import integrals_ref as R
import oracle_lib
import rough_inputs as RI
import series_ref as S
from beom_amd import capi
from beom_amd.grid import read_input_data
from helpers import same_bits
from test_gpu_biharm_tiled import CASES

_STATES = {}


def _stepped(name):
    """(rough fields, the oracle's state 3 steps on) of a frame of CASES, built once."""
    if name not in _STATES:
        p, files = CASES[name][0]()
        g = RI.rough_fields(read_input_data(p.replace(svis="0."), files=files), 1)
        o = oracle_lib.Oracle(g)
        o.step(1, 3)
        _STATES[name] = (g, {k: np.array(v, copy=True) for k, v in o.state().items()})
    return _STATES[name]


def _tree_py(vals):
    n = 1
    while n < len(vals):
        n *= 2
    w = [float(x) for x in vals] + [0.0] * (n - len(vals))
    while len(w) > 1:
        w = [w[2 * m] + w[2 * m + 1] for m in range(len(w) // 2)]
    return w[0]


def _loop_rows(f, a, xdup, ydup):
    """[mm+1, nlay]: every row of a[nlay, ndeg+1] placed on its columns (+0.0 elsewhere) and added in tree order."""
    p = f.p
    out = np.zeros((p.mm + 1, p.nlay))
    cells = [[] for _ in range(p.mm + 2)]
    for ipnt in range(1, p.ndeg + 1):
        cells[int(f.subc[1, ipnt])].append(ipnt)
    for j in range(1, p.mm + 2):
        for l in range(p.nlay):
            row = [0.0] * (p.lm + 1)
            for ipnt in cells[j]:
                i = int(f.subc[0, ipnt])
                if (xdup and i == p.lm + 1) or (ydup and j == p.mm + 1):
                    continue
                row[i - 1] = a[l, ipnt]
            out[j - 1, l] = _tree_py(row)
    return out


@pytest.mark.parametrize("name", ["island_ragged_3l", "jet_xyper_2l"])
def test_level_1_part_is_the_integrals_row_sums(name):
    g, st = _stepped(name)
    nl = g.p.nlay
    want = R.row_sums(g, R.terms(g, st))
    assert same_bits(S.row_record(g, st, 1), want)
    rec = S.row_record(g, st, 2)
    assert rec.shape == (g.p.mm + 1, S.count(nl, 2)) and same_bits(rec[:, :4 * nl + 1], want)


@pytest.mark.parametrize("name", ["island_ragged_3l", "jet_xyper_2l"])
def test_transport_part_is_a_plain_loop_in_tree_order(name):
    """island_ragged_3l: land leaves gaps in the rows.  jet_xyper_2l: the duplicated column and row contribute +0.0."""
    g, st = _stepped(name)
    p, nl = g.p, g.p.nlay
    xdup, ydup = float(p.xper) > 0.5, float(p.yper) > 0.5
    assert (xdup and ydup) == (name == "jet_xyper_2l")
    if name == "island_ragged_3l":
        assert p.ndeg < (p.lm + 1) * (p.mm + 1)
    rec = S.row_record(g, st, 2)
    tu, tv = rec[:, 4 * nl + 1:5 * nl + 1], rec[:, 5 * nl + 1:]
    assert same_bits(tu, _loop_rows(g, st["h_u"], xdup, ydup))
    assert same_bits(tv, _loop_rows(g, st["h_v"], xdup, ydup))
    assert np.all(tu[1:p.mm] != 0.0) and np.all(tv[1:p.mm] != 0.0), "a transport at rest: nothing tested"
    if ydup:
        assert not rec[p.mm].any() and not np.signbit(rec[p.mm]).any()
        # the oracle leaves +0 in the duplicated cells (their masks are 0): the rule shows on values put there
        dup = (g.subc[0] == p.lm + 1) | (g.subc[1] == p.mm + 1)
        dup[0] = False
        assert dup.sum() == p.lm + p.mm + 1 and not st["h_u"][:, dup].any() and not st["h_v"][:, dup].any()
        st2 = dict(st, h_u=np.where(dup[None, :], 1.5, st["h_u"]), h_v=np.where(dup[None, :], -2.5, st["h_v"]))
        assert same_bits(S.row_record(g, st2, 2), rec)
        assert not same_bits(_loop_rows(g, st2["h_u"], False, False), tu)


def test_closed_frame_has_no_transport_through_its_southern_wall():
    g, st = _stepped("closed_12l")
    nl = g.p.nlay
    rec = S.row_record(g, st, 2)
    assert np.all(rec[0, 5 * nl + 1:] == 0.0)
    assert np.all(rec[1:g.p.mm, 5 * nl + 1:] != 0.0)          # (row mm+1 is the dry margin)


def test_tree_over_the_vol_rows_is_the_integrals_vol():
    g, st = _stepped("island_ragged_3l")
    nl = g.p.nlay
    rec = S.row_record(g, st, 2)
    assert same_bits(R.combine(rec[:, :4 * nl + 1]), R.integrals(g, st))
    assert same_bits(R.tree(rec[:, 0:4 * nl:4].T), R.integrals(g, st)[0:4 * nl:4])


@pytest.mark.parametrize("config", ["island_ragged_3l", "closed_leith_3l"])
def test_rough_inputs_give_a_transport_that_differs_from_row_to_row(config):
    g = RI.rough_fields(RI.base_fields(config, "130x18"), 1)
    p, nl = g.p, g.p.nlay
    rec = S.row_record(g, {k: getattr(g, k) for k in ("hlay", "u", "v", "h_u", "h_v")}, 2)
    tu, tv = rec[:, 4 * nl + 1:5 * nl + 1], rec[:, 5 * nl + 1:]
    for t in (tu, tv):                                          # rows 2..mm: row 1 has a wall to the south, row mm+1 is dry
        assert np.all(t[1:p.mm] != 0.0)
        assert np.all(t[2:p.mm] != t[1:p.mm - 1])
    assert np.all(tu[1:p.mm] != tv[1:p.mm])
    assert same_bits(S.psi(rec, p)[:, 0], float(p.dl) * tv[:, 0])
    assert same_bits(S.psi(rec, p)[:, nl - 1], float(p.dl) * np.cumsum(tv, axis=1)[:, nl - 1])


def test_record_sizes_of_the_library():
    lib = capi.load()
    for nlay in (1, 2, 12, 16):
        assert lib.beom_series_count(nlay, 1) == 4 * nlay + 1 == lib.beom_integral_count(nlay) == S.count(nlay, 1)
        assert lib.beom_series_count(nlay, 2) == 6 * nlay + 1 == S.count(nlay, 2)
