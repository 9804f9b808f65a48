"""The trajectory conditions of test_gpu_float_bands on the restatement alone (floats_ref through float_bands_ref), with the
bands' rows fixed by hand: the rough inputs hand floats over in both directions across every seam, some come back, and the
island's coast rejects steps.  No GPU."""
import numpy as np
import pytest

import float_bands_ref as B
import floats_ref as R


@pytest.mark.parametrize("name,nb", B.CASES)
def test_rough_inputs_hand_floats_over(name, nb):
    f = B.frame(name)
    fr = R.Frame(f)
    cuts = B.CUTS[(name, nb)]
    rows = int(f.p.mm) if name == "ring" else int(f.p.mm) + 1
    assert cuts[0][0] == 1 and cuts[-1][1] == rows and all(cuts[k + 1][0] == cuts[k][1] + 1 for k in range(nb - 1))
    assert fr.yper == (name == "ring")
    n = B.COUNTS[-1]
    x0, y0, layer, steps = B.rough_reference(name, nb, n)
    assert fr.wet(x0, y0).all() and layer.min() == 1 and layer.max() == f.p.nlay
    for _, _, x, y, _ in steps:
        assert fr.wet(x, y).all()
    ch = B.rough_changes(name, nb, n)
    print(name, nb, ch.total, ch.north, ch.south, ch.came_back, ch.seam_wraps_north, ch.seam_wraps_south)
    if nb > 1:
        assert ch.total >= 100
        for s in ch.north:
            assert ch.north[s] >= 20 and ch.south[s] >= 20, (s, ch.north, ch.south)
        assert ch.came_back >= 1
        assert max(ch.per_step) > 1                  # (an outbox of one record overflows)
        assert max(ch.per_step) <= 4096              # (the default capacity holds every step's records)
    else:
        assert ch.total == 0 and ch.seam_wraps_north >= 20 and ch.seam_wraps_south >= 20
    if name == "island":
        assert steps[-1][4].sum() >= 20, int(steps[-1][4].sum())
    # the seam floats start within the strip of their seam
    half = n - n // 2
    d = np.min([np.abs(y0[half:] - s) for s in B.seams(name, cuts)] + ([np.abs(y0[half:] - rows)] if name == "ring" else []), axis=0)
    assert d.max() <= B.STRIPS.get((name, nb), B.STRIP)


def test_owner_changes_are_counted_per_seam_and_direction():
    cuts = ((1, 4), (5, 8))
    ys = [np.array([3.5, 4.5, 0.5, 7.5]), np.array([4.5, 3.5, 7.5, 0.5]), np.array([3.9, 3.6, 7.6, 0.6])]
    ch = B.Changes("ring", cuts, ys, 8)
    assert ch.total == 5 and ch.per_step == [4, 1]
    assert ch.north == {4.0: 1, 0.0: 1} and ch.south == {4.0: 2, 0.0: 1}
    assert ch.came_back == 1


@pytest.mark.parametrize("name,nb", B.CASES)
def test_real_steps_carry_floats_across_the_seams(name, nb):
    """The seeds of test_gpu_float_bands' real steps, on the C oracle's steps of the same frames: at least 10 owner changes
    along the restatement's track (on the ring of one band: seam crossings), every seam float within NSTEPS cdt max|v|."""
    import oracle_lib
    from test_gpu_float_bands import _seam_seeds
    f = B.real_frame(name)
    fr, cdt, cuts = R.Frame(f), B.cdt_of(f), B.CUTS[(name, nb)]
    o = oracle_lib.Oracle(f)
    st = [(np.array(o.state()["u"]), np.array(o.state()["v"]))]
    for t in range(1, B.NSTEPS + 1):
        o.step(t, 1)
        st.append((np.array(o.state()["u"]), np.array(o.state()["v"])))
    vmax = max(float(np.abs(st[0][1]).max()), float(np.abs(st[-1][1]).max()))
    reach = B.NSTEPS * cdt * vmax
    x, y, layer = R.seed_floats(f, 1000, B.SEED)
    x, y = _seam_seeds(f, name, cuts, x, y, layer, st[0][1], st[-1][1], reach, vmax)
    ys = [y]
    for t in range(B.NSTEPS):
        x, y, _ = R.step(fr, st[t], st[t + 1], x, y, layer, cdt)
        ys.append(y)
    ch = B.Changes(name, cuts, ys, int(f.p.mm))
    print(name, nb, ch.total, ch.north, ch.south, ch.seam_wraps_north, ch.seam_wraps_south)
    if nb > 1:
        assert ch.total >= 10, ch.total
    else:
        assert ch.seam_wraps_north + ch.seam_wraps_south >= 10
