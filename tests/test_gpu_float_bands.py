"""Lagrangian floats on a frame cut into bands (beom_multi_set_floats ..., include/beom_hip.h "Floats on bands"): chains of 2
and 3 bands with and without land, a ring of 2 bands and a ring of one, all on device 0.  The yardsticks are exact: the numpy
restatement of the scheme (floats_ref) on rough velocities, and the single handle's floats on real steps.  Every comparison is
helpers.same_bits on x, y and equality of `rejected`.  The inputs and the conditions on the restatement's own trajectories
(owner changes per seam and direction, floats that come back, rejected steps) are float_bands_ref's, which
test_float_bands_cpu holds to the same thresholds without a GPU."""
import os
import uuid

import numpy as np
import pytest

import float_bands_ref as B
import floats_ref as R
from beom_amd import capi, inputs as I
from helpers import STATE, same_bits

pytestmark = pytest.mark.gpu
NSTEPS = B.NSTEPS
CALLS = ((5, 7), (1,) * NSTEPS)


def _many(name, nb, overlap=1, real=False):
    f = B.real_frame(name) if real else B.frame(name)
    many = capi.MultiEngine(f, devices=[0] * nb, ring1=(name == "ring" and nb == 1))
    assert many.count == nb and many.describe()["ring"] == (1 if name == "ring" else 0)
    cuts = tuple((b["own0"], b["own1"]) for b in (many.band(k) for k in range(nb)))
    assert cuts == B.CUTS[(name, nb)], (name, nb, cuts)
    many.set_option("overlap", overlap)
    return many


def _same_floats(got, x, y, rejected, what):
    assert same_bits(got["x"], x), (what, "x", float(np.max(np.abs(got["x"] - x))))
    assert same_bits(got["y"], y), (what, "y", float(np.max(np.abs(got["y"] - y))))
    assert np.array_equal(got["rejected"], rejected), (what, "rejected")


def _calls(e, calls):
    t = 1
    for k in calls:
        e.step(t, k)
        t += k
    assert t - 1 == NSTEPS


# ---- 1. rough velocities against the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,nb", B.CASES)
def test_rough_velocities_equal_the_restatement(name, nb):
    many = _many(name, nb)
    big = B.COUNTS[-1]
    # the restatement's trajectory alone, before the device is looked at (3 floats cannot change owner 100 times: the
    # thresholds are held on the largest count)
    ch = B.rough_changes(name, nb, big)
    print("%s, %d bands: owner changes %d (per step %s), north %s, south %s, came back %d, seam wraps %d / %d"
          % (name, nb, ch.total, ch.per_step, ch.north, ch.south, ch.came_back, ch.seam_wraps_north, ch.seam_wraps_south))
    if nb > 1:
        assert ch.total >= 100, (name, nb, ch.total)
        for s in ch.north:
            assert ch.north[s] >= 20 and ch.south[s] >= 20, (name, nb, s, ch.north, ch.south)
        assert ch.came_back >= 1
    else:                     # one band owns every row of the ring: its floats cross the seam y = 0 = mm and stay its own
        assert ch.total == 0 and ch.seam_wraps_north >= 20 and ch.seam_wraps_south >= 20, (ch.seam_wraps_north, ch.seam_wraps_south)
    if name == "island":
        rej = B.rough_reference(name, nb, big)[3][-1][4]
        assert rej.sum() >= 20, (name, nb, int(rej.sum()))
    for n in B.COUNTS:
        x0, y0, layer, steps = B.rough_reference(name, nb, n)
        want = B.rough_changes(name, nb, n).total
        many.set_floats(x0, y0, layer)
        assert many.info("floats") == n
        got = many.download_floats()
        assert same_bits(got["x"], x0) and same_bits(got["y"], y0) and np.array_equal(got["layer"], layer)
        assert not got["rejected"].any() and many.info("float_handovers") == 0
        for t, (before, after, x, y, rej) in enumerate(steps, 1):
            many.upload(u=before[0], v=before[1])
            many.update_floats(1)
            many.upload(u=after[0], v=after[1])
            many.update_floats(2)
            _same_floats(many.download_floats(), x, y, rej, (name, nb, n, t))
        assert many.info("float_handovers") == want, (name, nb, n, many.info("float_handovers"), want)
    many.close()


# ---- 2. real steps against the single handle -----------------------------------------------------------------------------------
_REAL = {}


def _seam_seeds(f, name, cuts, x, y, layer, v0, v1, reach, vmax):
    """Moves the second half of the floats next to the seams, where the single handle's own v carries them across: float t
    goes to a column of its seam drawn with weight |v| of the seam's face in the float's layer (v0, v1: before and after the
    steps), on either side of the seam, at a distance of NSTEPS * cdt * |v| there times 10^(-6 uniform) — never more than
    `reach` = NSTEPS * cdt * max|v|.  (The flow at a face may reverse within the steps — gravity waves — so the net drift is
    a fraction of that bound, unknown beforehand: distances spread over six decades, on both sides, put floats within it.)"""
    fr = R.Frame(f)
    n = x.size
    r = np.random.default_rng([B.SEED, 78, n])
    ss = B.seams(name, cuts)
    x, y = x.copy(), y.copy()
    for s, t in zip(ss, np.array_split(np.arange(n - n // 2, n), len(ss))):
        cells = fr.cmap[1:fr.lm + 1, int(s) + 1]                      # v(p) sits on the south face of row s + 1: the seam
        for l in range(1, fr.nlay + 1):
            tl = t[layer[t] == l]
            a0, a1 = v0[l - 1, cells], v1[l - 1, cells]
            north = fr.N[fr.cmap[1:fr.lm + 1, int(s) if s > 0.0 else fr.mm]] == cells     # (both sides of the face wet and linked)
            w = np.where(fr.wetc[cells] & north, np.maximum(np.abs(a0), np.abs(a1)), 0.0)
            if not tl.size or not w.sum() > 0.0:
                continue
            i = r.choice(fr.lm, size=tl.size, p=w / w.sum())
            d = 10.0 ** (-6.0 * r.uniform(0.0, 1.0, tl.size)) * reach * (w[i] / vmax)
            up = r.integers(0, 2, tl.size) == 1                       # start south of the seam
            yy = np.where(up, s - d, s + d)
            yy = np.where(up & (yy >= s), np.nextafter(s, -np.inf), yy)
            if fr.yper:
                yy = np.where(yy < 0.0, yy + fr.mm, yy)
                yy = np.where(yy >= fr.mm, yy - fr.mm, yy)
            x[tl] = np.minimum(i + r.uniform(0.05, 0.95, tl.size), np.nextafter(i + 1.0, 0.0))
            y[tl] = yy
    assert fr.wet(x, y).all()
    return x, y


def _real_reference(name, nb):
    """Once per case: the seeds (half anywhere, half within NSTEPS * cdt * max|v| of the seams; v the single handle's before
    and after the steps), the single handle's floats after calls of (5, 7) steps and the owner changes along its recorded
    track."""
    key = (name, nb)
    if key not in _REAL:
        f = B.real_frame(name)
        cuts = B.CUTS[key]
        e = capi.Engine(f)
        v0 = e.download(("v",))["v"]
        _calls(e, CALLS[0])
        v1 = e.download(("v",))["v"]
        e.close()
        vmax = max(float(np.max(np.abs(v0))), float(np.max(np.abs(v1))))
        reach = NSTEPS * B.cdt_of(f) * vmax
        assert reach > 0.0
        x, y, layer = R.seed_floats(f, 1000, B.SEED)
        x, y = _seam_seeds(f, name, cuts, x, y, layer, v0, v1, reach, vmax)
        far = np.min([np.minimum(np.abs(y[500:] - s), np.abs(y[500:] - s - (f.p.mm if name == "ring" else 0))) for s in B.seams(name, cuts)], axis=0)
        assert far.max() <= reach * (1.0 + 1e-12), (far.max(), reach)
        e = capi.Engine(f)
        e.set_floats(x, y, layer, records=NSTEPS, stride=1)
        _calls(e, CALLS[0])
        fl, tr, st = e.download_floats(), e.download_float_track(), e.download()
        e.close()
        assert tr["tstp"].tolist() == list(range(1, NSTEPS + 1))
        ch = B.Changes(name, cuts, [y] + [tr["y"][k] for k in range(NSTEPS)], int(f.p.mm))
        print("%s, %d bands: reach %.3g rows, owner changes on the single handle's track %d, seam wraps %d / %d"
              % (name, nb, reach, ch.total, ch.seam_wraps_north, ch.seam_wraps_south))
        _REAL[key] = (x, y, layer, fl, st, ch)
    return _REAL[key]


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("name,nb", B.CASES)
def test_real_steps_equal_the_single_handle(name, nb, overlap):
    x, y, layer, want, _, ch = _real_reference(name, nb)
    if nb > 1:
        assert ch.total >= 10, (name, nb, ch.total)
    else:
        assert ch.seam_wraps_north + ch.seam_wraps_south >= 10, (name, ch.seam_wraps_north, ch.seam_wraps_south)
    assert not same_bits(want["x"], x) and not same_bits(want["y"], y), "the floats did not move: nothing tested"
    for calls in CALLS + (CALLS[0],):                 # (the last: a second identical run gives the same bits)
        plain = _many(name, nb, overlap, real=True)
        _calls(plain, calls)
        split, state = plain.stats()["split"], plain.download()
        assert plain.info("float_launches") == 0
        plain.close()
        many = _many(name, nb, overlap, real=True)
        many.set_floats(x, y, layer)
        _calls(many, calls)
        _same_floats(many.download_floats(), want["x"], want["y"], want["rejected"], (name, nb, overlap, calls))
        assert many.stats()["split"] == split, (name, nb, overlap, many.stats(), split)
        assert many.info("float_launches") == sum(k + 1 for k in calls), (calls, many.info("float_launches"))
        assert many.info("float_handovers") == ch.total, (name, nb, many.info("float_handovers"), ch.total)
        got = many.download()
        for key in STATE:
            assert same_bits(got[key], state[key]), (name, nb, overlap, calls, key, "a handle with floats steps as one without")
        many.close()


# ---- 3. a handle with floats steps as one without -------------------------------------------------------------------------------
def test_floats_leave_the_step_as_it_was_and_run_beside_moments_and_tracers():
    name, nb = "closed", 3
    f = B.frame(name)
    x, y, layer, want, _, _ = _real_reference(name, nb)
    q = np.ascontiguousarray(np.stack([np.asarray(f.hlay, dtype=np.float64), 0.5 * np.asarray(f.hlay, dtype=np.float64)]))

    def run(floats, others):
        many = _many(name, nb)
        if others:
            many.set_tracers(2)
            many.upload_tracers(q=q)
            many.set_moments(3, 2)
        if floats:
            many.set_floats(x, y, layer)
        _calls(many, CALLS[0])
        out = (many.download(), many.download_floats() if floats else None, many.download_tracers() if others else None,
               many.download_moments() if others else None, many.stats())
        many.close()
        return out

    st0, _, _, _, stats0 = run(False, False)
    st1, fl1, _, _, stats1 = run(True, False)
    st2, fl2, tr2, mo2, _ = run(True, True)
    _, _, tr3, mo3, _ = run(False, True)
    for key in STATE:
        assert same_bits(st0[key], st1[key]) and same_bits(st0[key], st2[key]), key
    assert stats0 == stats1
    for fl in (fl1, fl2):
        _same_floats(fl, want["x"], want["y"], want["rejected"], "3 bands")
    assert same_bits(tr2["q"], tr3["q"]) and same_bits(tr2["rq"], tr3["rq"])
    assert mo2["count"] == mo3["count"] == 6
    for key in ("ref", "sum", "sq"):
        assert same_bits(mo2[key], mo3[key]), key


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def _refused(call, code):
    with pytest.raises(capi.BeomError) as ei:
        call()
    msg = str(ei.value)
    tag = "error %d:" % code
    assert tag in msg and len(msg.split(tag)[1].strip()) > 20, msg
    return msg


def test_refusals():
    name, nb = "island", 3
    f = B.frame(name)
    fr = R.Frame(f)
    x0, y0, layer, steps = B.rough_reference(name, nb, B.COUNTS[-1])
    many = _many(name, nb)
    # no track recorder on bands
    _refused(lambda: many.set_floats(x0, y0, layer, records=4), -6)
    assert many.info("floats") == 0
    # a dry start: nothing uploaded, the smallest dry index named (two offenders, owned by different bands)
    dry = np.flatnonzero(~fr.wetc & (np.arange(fr.n1) > 0))
    lo, hi = dry[np.argmin(fr.j[dry])], dry[np.argmax(fr.j[dry])]
    assert B.owner(B.CUTS[(name, nb)], np.array([fr.j[lo] - 0.5]))[0] != B.owner(B.CUTS[(name, nb)], np.array([fr.j[hi] - 0.5]))[0]
    xb, yb = x0.copy(), y0.copy()
    xb[37], yb[37] = fr.i[hi] - 0.5, fr.j[hi] - 0.5
    xb[1500], yb[1500] = fr.i[lo] - 0.5, fr.j[lo] - 0.5
    msg = _refused(lambda: many.set_floats(xb, yb, layer), -3)
    assert "float 37 " in msg, msg
    assert many.info("floats") == 0
    many.set_floats(x0, y0, layer)
    rc = many.lib.beom_multi_upload_floats(many.h, capi._dp(xb), capi._dp(yb), capi._ip(layer), many._err, capi.ERRLEN)
    assert rc == -3
    got = many.download_floats()
    _same_floats(got, x0, y0, np.zeros(x0.size, dtype=np.int32), "after a refused upload")
    yb = y0.copy(); yb[5] = float("nan")
    assert "float 5 " in _refused(lambda: many.set_floats(x0, yb, layer), -3)
    # capacity 1: records are dropped, the download says so
    many.set_floats(x0, y0, layer, capacity=1)
    before, after = steps[0][0], steps[0][1]
    many.upload(u=before[0], v=before[1]); many.update_floats(1)
    many.upload(u=after[0], v=after[1]); many.update_floats(2)
    msg = _refused(many.download_floats, capi.ERR_FLOAT_OVERFLOW)
    assert int(msg.split("download_floats:")[1].split()[0]) > 0, msg
    # cdt max|v| = 3: lookups leave the windows — counted, nothing read outside them; the single handle follows the restatement
    cdt = B.cdt_of(f)
    amp = 3.0 / cdt
    before, after = R.rough_velocities(f, B.SEED, 101, amp), R.rough_velocities(f, B.SEED, 102, amp)
    xw, yw, branch = R.step(fr, before, after, x0, y0, layer, cdt)
    one = capi.Engine(f)
    one.set_floats(x0, y0, layer)
    one.upload(u=before[0], v=before[1]); one.update_floats(1)
    one.upload(u=after[0], v=after[1]); one.update_floats(2)
    _same_floats(one.download_floats(), xw, yw, (branch != 0).astype(np.int32), "the single handle at cdt max|v| = 3")
    one.close()
    many.set_floats(x0, y0, layer)
    many.upload(u=before[0], v=before[1]); many.update_floats(1)
    many.upload(u=after[0], v=after[1]); many.update_floats(2)
    msg = _refused(many.download_floats, capi.ERR_FLOAT_REACH)
    assert int(msg.split("download_floats:")[1].split()[0]) > 0, msg
    many.close()
    # a handle that holds one band's window
    from beom_amd import slab
    recipe = I.recipe_headline(150, 131, 3)
    fw, _, orphan = slab.build_band(recipe, 2, 0)
    band = capi.BandEngine(fw, recipe.p, 2, 0, device=0, orphan=orphan, loopback=True,
                           shm_name="/beom_fltb_%d_%s" % (os.getpid(), uuid.uuid4().hex[:8]))
    _refused(lambda: band.set_floats(x0[:10], y0[:10], layer[:10]), -6)
    band.close()
