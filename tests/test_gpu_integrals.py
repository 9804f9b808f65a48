"""Conservation integrals on the device (beom_integrals, include/beom_hip.h) against the numpy restatement
(integrals_ref) applied to the state downloaded from the same handle.  Every comparison is helpers.same_bits: the order of
summation is part of the contract, so a dense handle, an embedded one, the table path, a frame cut into bands (chain, ring)
and bands in separate processes must all give the same bits.  No tolerance anywhere."""
import os
import queue
import sys
import uuid

import numpy as np
import pytest

import integrals_ref as R
from beom_amd import capi, inputs as I
from beom_amd.grid import read_input_data
from helpers import Golden, same_bits
from test_gpu_biharm_tiled import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
HUV = ("hlay", "u", "v")


def _fields(g):
    f = g.fields()
    f.invf = float(g.static("invf"))
    return f


def _case(name):
    if name == "wide_67_chunks":                       # 4201 columns: 66 chunks, the chunk tree is padded to 128
        p, files = I.case_headline(4200, 9, 2)
    else:
        p, files = CASES[name][0]()
    return read_input_data(p.replace(svis="0."), files=files)


def _check(e, f, what):
    """The handle's integrals against the restatement on the handle's own state; returns the raw sums."""
    got = e.integrals()
    want = R.integrals(f, e.download(HUV))
    assert np.isfinite(want).all(), (what, want)
    assert same_bits(got["raw"], want), (what, got["raw"], want)
    nl = f.p.nlay
    assert same_bits(got["vol"], want[0:4 * nl:4]) and same_bits(got["circ"], want[3:4 * nl:4]) and got["eta2"] == want[4 * nl]
    assert np.allclose(got["volume_m3"], float(f.p.dl) ** 2 * want[0:4 * nl:4], rtol=1e-15)
    return got["raw"]


@pytest.mark.parametrize("dense_hint", [1, 0])
@pytest.mark.parametrize("name", ["stommel_24x16", "soliton_31x15_xper", "jet_2l_xyper", "island_3l_forced",
                                  "random_coast_2l_xper", "sill_16l_ocrp", "carrier_beach", "rigid_lid_sill_2l"])
def test_golden_state_of_step_10(name, dense_hint):
    """The reference's own state of step 10 uploaded into a fresh handle (hlay, u, v: all the integrals read)."""
    g = Golden(name)
    f = _fields(g)
    e = capi.Engine(f, variant=g.variant, dense_hint=dense_hint)
    e.upload(**{k: np.ascontiguousarray(g.step(10, k), dtype=np.float64) for k in HUV})
    raw = _check(e, f, (name, dense_hint))
    assert (raw[1:4 * g.p.nlay:4] >= 0).all() and (raw[2:4 * g.p.nlay:4] >= 0).all()
    e.close()


@pytest.mark.parametrize("name", ["jet_xyper_2l", "closed_12l", "island_ragged_3l", "island_ragged_no_leith_4l", "wide_67_chunks"])
def test_frames_of_many_chunks_after_12_steps(name):
    """Odd widths spanning several 64-column chunks, after 12 steps of the engine; the dense (or embedded) handle and the
    table path give the same bits."""
    f = _case(name)
    e, tab = capi.Engine(f), capi.Engine(f, dense_hint=0)
    assert e.is_dense and not tab.is_dense
    if name in CASES:
        assert e.is_embedded == CASES[name][1]
    e.step(1, 12); tab.step(1, 12)
    a, b = _check(e, f, (name, "dense")), _check(tab, f, (name, "table"))
    assert same_bits(a, b), (name, a, b)
    assert a[1] > 0 and a[2] > 0, (name, "the top layer is at rest: nothing tested")
    e.close(); tab.close()


@pytest.mark.parametrize("name", ["jet_xyper_2l", "island_ragged_3l"])
def test_row_ranges_combine_to_the_whole(name):
    f = _case(name)
    e = capi.Engine(f)
    e.step(1, 5)
    whole = e.integrals()["raw"]
    M = f.p.mm + 1
    cut = 37
    rows = np.concatenate([e.integral_rows(1, cut), e.integral_rows(cut + 1, M - cut)])
    assert same_bits(rows, R.row_sums(f, R.terms(f, e.download(HUV)))), name
    assert same_bits(capi.combine_integral_rows(rows), whole), name
    with pytest.raises(capi.BeomError):
        e.integral_rows(M, 2)
    e.close()


def _band_case(case):
    if case == "closed_12l":
        return I.case_headline(150, 37, 12)
    if case == "sill_sponges":
        return I.case_sill_exchange3d(lm=133, mm=199, nlay=4, dt_s=0.01, npts=5, sill_halfwidth=20.0)
    if case == "jet_ring":
        return I.case_unstable_jet(lm=131, mm=151, nlay=2, dt_s=1.5)
    raise ValueError(case)


@pytest.mark.parametrize("nband", [2, 3])
@pytest.mark.parametrize("case", ["closed_12l", "sill_sponges", "jet_ring"])
def test_bands_in_one_process_give_the_single_handles_bits(case, nband):
    p, files = _band_case(case)
    f = read_input_data(p, files=files)
    one, many = capi.Engine(f), capi.MultiEngine(f, devices=[0] * nband)
    assert many.count == nband and many.describe()["ring"] == int(float(p.yper) > 0.5)
    for x in (one, many):
        x.step(1, 7); x.step(8, 6)
    a = _check(one, f, (case, "single"))
    b = many.integrals()["raw"]
    assert same_bits(a, b), (case, nband, a, b)
    one.close(); many.close()


# ---- two processes over the shared-memory transport (the pattern of test_gpu_bands_multiproc) -------------------------------
def _recipe(case):
    if case == "closed":
        return I.recipe_headline(150, 131, 3)
    if case == "jet_ring":
        return I.recipe_unstable_jet(lm=131, mm=151, nlay=2, dt_s=1.5)
    raise ValueError(case)


def _worker(rank, world, case, shm_name, q, calls):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.setdefault("BEOM_SHM_TIMEOUT_S", "90")
    from beom_amd import slab
    recipe = _recipe(case)
    p = recipe.p
    f, g, orphan = slab.build_band(recipe, world, rank)
    band = capi.BandEngine(f, p, world, rank, device=0, shm_name=shm_name, orphan=orphan)
    t = 1
    for n in calls:
        band.step(t, n)
        t += n
    own0, own1, rows = band.integral_rows()
    assert (own0, own1) == (g.own0, g.own1) and rows.shape[0] == own1 - own0 + 1
    with pytest.raises(capi.BeomError):
        band.integrals()
    if rank != 0:
        q.put((own0, own1, rows))
        band.close()
        return
    count = rows.shape[1]
    allrows = np.zeros((p.mm + 1, count))               # (row mm+1 of the ring: the duplicated row, all +0)
    allrows[own0 - 1:own1] = rows
    seen = own1 - own0 + 1
    for _ in range(world - 1):
        try:
            a, b, r = q.get(timeout=240)                # a missing rank is an error, not a hang
        except queue.Empty:
            raise AssertionError("a rank did not deliver its row sums")
        allrows[a - 1:b] = r
        seen += b - a + 1
    yper = float(p.yper) > 0.5
    assert seen == (p.mm if yper else p.mm + 1)
    got = capi.combine_integral_rows(allrows)
    ff = read_input_data(p, files=recipe.rows(0, p.mm + 1))
    whole = capi.Engine(ff)
    whole.step(1, t - 1)
    want = whole.integrals()["raw"]
    assert np.isfinite(want).all(), (case, want)
    assert same_bits(want, R.integrals(ff, whole.download(HUV))), case
    assert same_bits(got, want), (case, got, want)
    band.close(); whole.close()


def _run(world, case, calls=(7, 6)):
    """Spawned before anything in this process touches the GPU; raises if a rank's comparison fails."""
    import torch.multiprocessing as mp
    name = "/beom_test_%d_%s" % (os.getpid(), uuid.uuid4().hex[:12])
    q = mp.get_context("spawn").Queue()
    try:
        mp.spawn(_worker, args=(world, case, name, q, tuple(calls)), nprocs=world, join=True)
    finally:
        try:
            os.unlink("/dev/shm" + name)
        except OSError:
            pass


@pytest.mark.parametrize("case", ["closed", "jet_ring"])
def test_two_processes_gather_their_row_sums(case):
    _run(2, case)


# ---- the Fortran host with BEOM_INTEGRALS=1 ---------------------------------------------------------------------------------
def _run_fortran_host(g, work, env_extra):
    import subprocess
    from beom_amd.host import build_host
    exe = build_host.build(g.p, os.path.join(work, "beom_gpu"), variant=g.variant)
    I.write_inputs(work, g.files)
    env = dict(os.environ)
    env.pop("BEOM_INTEGRALS", None)
    env.update(env_extra)
    r = subprocess.run([exe], cwd=work, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "ERROR CODE" not in r.stderr, (r.stdout[-1500:], r.stderr[-1500:])
    os.remove(exe)
    return {fn: open(os.path.join(work, fn), "rb").read() for fn in sorted(os.listdir(work)) if os.path.isfile(os.path.join(work, fn))}


def _parse_es(tok):
    import re
    return float(re.sub(r"(?<=\d)([+-]\d{3})$", r"E\1", tok))       # es24.16 drops the E in front of a three-digit exponent


@pytest.mark.parametrize("ngpu", [1, 3])
def test_fortran_host_writes_integrals_txt(ngpu, tmp_path):
    """tc_conservation_xyper_stdfb: one line of integrals.txt per record of time.txt, its figures (es24.16 round-trips FP64)
    are Engine.integrals()'s of the Python host at those steps, and every other output file is byte-identical to the run
    without the variable.  ngpu = 3: the same through BEOM_NGPU (a ring of bands on the one GPU of the box)."""
    g = Golden("tc_conservation_xyper_stdfb")
    multi = {"BEOM_NGPU": str(ngpu), "BEOM_MULTI_WRAP_DEVICES": "1"} if ngpu > 1 else {}
    a_dir, b_dir = tmp_path / "plain", tmp_path / "with"
    a_dir.mkdir(); b_dir.mkdir()
    plain = _run_fortran_host(g, str(a_dir), multi)
    withi = _run_fortran_host(g, str(b_dir), dict(multi, BEOM_INTEGRALS="1"))
    assert "integrals.txt" not in plain and "integrals.txt" in withi
    assert sorted(plain) == sorted(k for k in withi if k != "integrals.txt")
    for fn in plain:
        assert plain[fn] == withi[fn], fn
    times = [float(x) for x in withi["time.txt"].decode().split()]
    lines = [ln.split() for ln in withi["integrals.txt"].decode().splitlines() if ln.strip()]
    assert len(lines) == len(times) >= 2
    f = _fields(g)
    nl = g.p.nlay
    e = capi.Engine(f, variant=g.variant)
    t = 0
    for ctim, ln in zip(times, lines):
        vals = np.array([_parse_es(x) for x in ln])
        assert len(vals) == 4 * nl + 2 and vals[0] == ctim
        step = int(round(ctim / float(g.p.dtd8)))
        if step > t:
            e.step(t + 1, step - t)
            t = step
        s = e.integrals()
        want = np.concatenate([np.stack([s["volume_m3"], s["kinetic_J"], s["enstrophy"], s["circulation"]], axis=1).ravel(),
                               [s["potential_J"]]])
        assert same_bits(vals[1:], want), (ngpu, ctim, step, vals[1:], want)
    assert t > 0
    e.close()
