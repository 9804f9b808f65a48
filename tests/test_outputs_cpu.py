"""outputs_ref (the numpy restatement of write_outputs / write_array, private_mod.f95:2772-2974) against the real reference's
own files, and the conditions on the states test_gpu_outputs feeds the device kernels with.  No GPU.

1. Every golden fixture holds the reference's eta_.bin, u___.bin, v___.bin (and pvor.bin, mont.bin, v_cc.bin with diag = 1).
   Record 0 is restated from the fixture's initial state and record 1 from the stored step whose u and v in real*4 are that
   record of u___.bin and v___.bin — the pairing is searched and asserted, not assumed.  The files of a restarted run begin
   with the first run's records and its initial state was read back from real*4: there every record is tried against the
   stored steps only.  Bytes must be equal.
2. The rough states: every record differs from its copy shifted by one cell in x, in y and by one layer at >= 80 % of the
   places; pvor and mont are finite.
3. The placed extremes and thin cells: the restatement's scans of every doctored state return exactly the placed values and
   the intended layer (a placement that got lost fails here, without a GPU).  The states and placements are outputs_cases'."""
import types

import numpy as np
import pytest

import outputs_cases as K
import outputs_ref as O
from helpers import GOLDEN_STEPS, Golden, golden_names

RECORDS = ("eta_", "u___", "v___")
DIAG = ("pvor", "mont", "v_cc")


def _file(g, var):
    key = "file_%s_bin" % var
    if key not in g.z.files:
        return None
    return np.frombuffer(g.z[key].tobytes(), dtype="<f4").reshape(-1, g.p.nlay, g.p.ndeg)


def _module_state(g):
    """The reference's own module state after initialisation, as the fixture stores it (test_oracle_golden holds the init
    mirror, Golden.fields(), to these arrays bit for bit; reading them here spares the outcropping rest state's iteration,
    minutes for 16 layers)."""
    names = ("neig", "mk_n", "mk_u", "mk_v", "mkpe", "mkpi", "fcor", "h_th", "hlay", "u", "v")
    f = types.SimpleNamespace(p=g.p, **{k: g.static(k) for k in names})
    f.pi_s = g.static("pi_s") if float(g.p.rgld) > 0.5 else None
    assert f.neig.shape == (g.p.ndeg + 1, 8)
    return f


def _states(g, f):
    """[(label, hlay, u, v, pi_s)]: the initial state and every stored step."""
    lid = float(g.p.rgld) > 0.5
    out = [("init", f.hlay, f.u, f.v, f.pi_s if lid else None)]
    for t in GOLDEN_STEPS:
        if "step%d_u" % t in g.z.files:
            out.append(("step%d" % t, g.step(t, "hlay"), g.step(t, "u"), g.step(t, "v"), g.step(t, "pi_s") if lid else None))
    return out


_PAIRED = {}          # golden -> (records compared, records no stored state matches)


def _compare(name):
    """Compares every record of the golden that can be paired with a state; returns (compared, skipped record numbers)."""
    if name in _PAIRED:
        return _PAIRED[name]
    g = Golden(name)
    f = _module_state(g)
    files = {v: _file(g, v) for v in RECORDS + DIAG}
    assert all(files[v] is not None for v in RECORDS)
    has_diag = float(g.p.diag) > 0.5
    if not has_diag:
        assert all(files[v] is None for v in DIAG), name
    has_diag = has_diag and all(files[v] is not None for v in DIAG)    # (one fixture with diag = 1 holds the three records only)
    h0r4 = np.frombuffer(g.z["file_h_0_bin"].tobytes(), dtype="<f4").reshape(g.p.nlay, g.p.ndeg)
    states = _states(g, f)
    restart = float(g.p.rsta) > 0.5
    nrec = files["u___"].shape[0]
    compared, skipped = [], []
    for rec in (range(nrec) if restart else range(min(nrec, 2))):
        u_rec = files["u___"][rec]
        if rec == 0 and not restart:
            match = states[:1]                                       # record 0 is the initial state: asserted below, not searched
        else:
            match = [s for s in states[1:] if O.same_r4(O._r4(np.asarray(s[2])[:, 1:]), u_rec)
                     and O.same_r4(O._r4(np.asarray(s[3])[:, 1:]), files["v___"][rec])]
        if not match:
            skipped.append(rec)
            continue
        label, hlay, u, v, pi_s = match[0]
        eta, u4, v4 = O.records(f, hlay, u, v, h0r4, pi_s)
        assert O.same_r4(u4, u_rec) and O.same_r4(v4, files["v___"][rec]), (name, rec, label)
        assert O.same_r4(eta, files["eta_"][rec]), (name, rec, label, "eta_")
        if float(g.p.rgld) > 0.5:
            assert O.same_r4(files["eta_"][rec][0], O._r4(np.asarray(pi_s)[1:])), (name, rec, label, "the lid pressure")
        if has_diag and rec < files["pvor"].shape[0]:
            for nm, a in zip(DIAG, O.diag(f, hlay, u, v)):
                assert O.same_r4(a, files[nm][rec]), (name, rec, label, nm)
        compared.append(rec)
    _PAIRED[name] = (compared, skipped, nrec)
    return _PAIRED[name]


@pytest.mark.parametrize("name", golden_names())
def test_restatement_reproduces_the_reference_files(name):
    compared, skipped, nrec = _compare(name)
    assert compared, (name, "no record could be paired with a stored state")
    if not name.startswith("restart_"):
        assert 0 in compared and set(skipped) <= {1}


# record 1 was written at a step the fixture does not store (its dt_o is not 4 steps)
NO_STORED_STEP = {"rigid_lid_sill_2l", "sill_16l_ocrp", "sill_2l_ocrp", "sill_4l_ocrp", "soliton_31x15_xper", "topdrag_sill_ocrp_2l"}


def test_pairing_left_only_the_known_records_out():
    """Lists the records no stored state matched.  Of the runs from rest these are the second records of NO_STORED_STEP; a
    restarted run's first records belong to the run it continues."""
    skipped = {n: _compare(n)[1] for n in golden_names()}
    print("records without a stored state:", {n: r for n, r in skipped.items() if r})
    assert {n for n, r in skipped.items() if r and not n.startswith("restart_")} == NO_STORED_STEP
    diag_pinned = [n for n in golden_names() if float(Golden(n).p.diag) > 0.5 and _file(Golden(n), "pvor") is not None
                   and len(_compare(n)[0]) >= 2]
    assert len(diag_pinned) >= 10, diag_pinned                         # the diag records, at two records each


# ---- the rough states of test_gpu_outputs ------------------------------------------------------------------------------------
def _state(g):
    return {k: getattr(g, k) for k in ("hlay", "u", "v")}


def _shift_fractions(f, rec):
    """rec [nlay, ndeg] -> {shift: fraction of places that differ from the copy shifted by one cell in x, in y, one layer}
    over the places where the cell and its neighbour are both wet."""
    wet = np.asarray(f.mk_n) > 0.5
    a = np.concatenate([np.zeros((rec.shape[0], 1), rec.dtype), rec], axis=1)
    out = {}
    for shift, col in (("x", 4), ("y", 6)):
        nb = f.neig[:, col].astype(np.int64)
        ok = wet & wet[nb] & (nb > 0)
        out[shift] = float(np.mean(a[:, ok] != a[:, nb[ok]]))
    if rec.shape[0] > 1:
        out["layer"] = float(np.mean(a[:-1][:, wet] != a[1:][:, wet]))
    return out


@pytest.mark.parametrize("config,frame", K.ROUGH_CASES)
def test_records_of_the_rough_states_are_rough(config, frame):
    g = K.rough_state(config, frame)
    st = _state(g)
    eta, u4, v4 = O.records(g, st["hlay"], st["u"], st["v"], K.h0_rough(g))
    pvor, mont, vcc = O.diag(g, st["hlay"], st["u"], st["v"])
    assert np.isfinite(pvor).all() and np.isfinite(mont).all(), (config, frame)
    for nm, rec in (("eta", eta), ("u", u4), ("v", v4), ("pvor", pvor), ("mont", mont), ("v_cc", vcc)):
        if nm == "v_cc" and float(g.p.dvis) == 0.0:
            assert config in K.CONSTANT_V_CC                            # dvis = 0: v_cc is bvis everywhere
            continue
        for shift, frac in _shift_fractions(g, rec).items():
            assert frac >= 0.80, (config, frame, nm, shift, frac)
    mm, thin = O.scans(g, st["hlay"], st["u"], st["v"])
    assert thin == 0 and np.isfinite(mm).all()


# ---- placed extremes and thin cells -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,config,frame", K.SCAN_HANDLES)
def test_placed_extremes_reach_the_restatement(kind, config, frame):
    g = K.rough_state(config, frame)
    st = _state(g)
    base, _ = O.scans(g, st["hlay"], st["u"], st["v"])
    cells = K.scan_cells(g, kind)
    s, last = K.slots(g, kind)
    assert s[cells["lane255"]] % K.BLOCK == K.BLOCK - 1 and s[cells["lane0"]] == s[cells["lane255"]] + 1
    assert s[cells["lastblock"]] // K.BLOCK == last // K.BLOCK and (last + 1) % K.BLOCK != 0
    if kind != "table":
        assert (int(g.p.lm) + 1) % 16 != 0                             # the pitch is padded
    masks = O.scan_masks(g)
    counted = np.zeros(6, int)
    for rank, (cls, cell) in enumerate(cells.items()):
        for lay_min, lay_max in K.layer_pairs(g.p.nlay):
            doc, want = K.place_extremes(g, st, cell, rank, lay_min, lay_max)
            got, thin = O.scans(g, doc["hlay"], doc["u"], doc["v"])
            assert thin == 0 and np.array_equal(got, want), (kind, cls, lay_min, lay_max)
            for q in range(6):
                k = lay_min if q % 2 == 0 else lay_max
                if masks[q // 2][cell]:
                    assert got[k, q] == K.placed_value(base, q, k, rank) != base[k, q], (kind, cls, q)
                    assert (got[k, q] < base[k, q]) if q % 2 == 0 else (got[k, q] > base[k, q]), (kind, cls, q)
                    counted[q] += 1
                else:
                    assert got[k, q] == base[k, q]
    # every extreme counts in the workgroup-boundary pair, in the first and last cell of its mask and in one more at least
    assert (counted >= 2 * 4).all(), counted
    doc, want = K.place_ignored(g, st)
    for k in ("hlay", "u", "v"):
        assert not np.array_equal(doc[k], st[k])
    got, thin = O.scans(g, doc["hlay"], doc["u"], doc["v"])
    assert thin == 0 and np.array_equal(got, base) and np.array_equal(want, base)


@pytest.mark.parametrize("kind,config,frame", K.SCAN_HANDLES)
def test_placed_thin_cells_reach_the_restatement(kind, config, frame):
    g = K.rough_state(config, frame)
    st = _state(g)
    cases = K.thin_cases(g, kind)
    assert {"layer2_only", "layers_3_and_2_in_different_blocks", "last_wet_cell_last_layer", "dry_cells_only"} <= set(cases)
    for nm, (where, flag) in cases.items():
        doc = K.place_thin(g, st, where)
        assert O.scans(g, doc["hlay"], doc["u"], doc["v"])[1] == flag, (kind, nm)
    assert sorted(flag for _, flag in cases.values()) == [0, 2, 2, 2, 3]


@pytest.mark.parametrize("config", K.BAND_CONFIGS)
def test_placements_by_rows_reach_the_restatement(config):
    """The band tests place by rows of the frame, known only once the handle has dealt its bands: here every row a seam could
    fall on is tried, with the checks the GPU test repeats for its own rows."""
    g = K.rough_state(config, K.BAND_FRAME)
    st = _state(g)
    mm = int(g.p.mm)
    rows = sorted({1, 2, mm - 1, mm, mm + 1} | set(range(20, mm - 10, 7)))
    counted = K.check_row_placements(g, st, rows)
    assert counted >= 6 * 2 * (len(rows) - 2), counted                 # all but row mm + 1 (dry) and at most one more
    ring = float(g.p.yper) > 0.5
    if ring:
        cell = K.row_cells(g, [mm + 1])["row%d" % (mm + 1)]
        assert not any(m[cell] for m in O.scan_masks(g))                # the orphan row counts for nothing
    # thin cells by rows: the cases of the GPU test, over bands dealt by rows (the handle's own deal may cut elsewhere)
    nl = int(g.p.nlay)
    for nband in (2, 3):
        bands = K.guessed_bands(g, nband)
        assert bands[0][0] == 1 and bands[-1][1] == (mm if ring else mm + 1)
        cases = K.band_thin_cases(g, bands)
        assert len(cases) == 6 * nband + int(ring)
        edge_won = 0
        for nm, (where, flag) in cases.items():
            doc = K.place_thin(g, st, where)
            assert O.scans(g, doc["hlay"], doc["u"], doc["v"])[1] == flag, (config, nband, nm)
            edge_won += "upper layer" in nm and "middle" not in nm and flag == nl - 1
        # the edge row's own band decides the flag in every edge row but the dry margin row of a frame that is not a ring
        assert edge_won >= 2 * nband - (0 if ring else 1), (config, nband, edge_won)
        assert sorted({flag for _, flag in cases.values()}) == ([0] if ring else []) + [nl - 1, nl]
