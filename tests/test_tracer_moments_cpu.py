"""The tracer moments' contract on the CPU (include/beom_hip.h, "Tracer moments").  The numpy restatement
(tracer_moments_ref) is driven by tracers_ref and the oracle on goldens, step by step as test_tracers_cpu drives the scheme:
the tracer update in front of every oracle step, one sample behind it.

  identity   a tracer with q = hlay and ctrg = 1 IS the layer thickness (test_tracers_cpu pins that), so its moments of q, fu, fv
             must be moments_ref's moments of hlay, h_u, h_v bit for bit, and its concentration is 1 with S = Q = +0: the
             feature is tied to two things already pinned, not to itself.
  accuracy   mean and var_c against a long-double two-pass over the same rounded FP64 samples, within the bounds that
             test_moments_cpu writes out.
  liveness   what the chosen goldens and the patchy concentration have to show, asserted before any comparison.

No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import moments_ref as MR
import oracle_lib
import rough_inputs as R
import tracer_moments_ref as TM
import tracers_ref as T
from beom_amd import capi
from helpers import Golden, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
NSTEPS = 20
# a doubly periodic jet, a forced frame with an island, and an open boundary whose transports enter from outside the frame
# (the upwind cell of those faces is the sentinel, which is dry: the no-gradient branch)
GOLDENS = ("jet_2l_xyper", "island_3l_forced", "obc_mcbc0_2l")


def _fields(g):
    f = g.fields()
    f.invf = float(g.static("invf"))
    return f


_RUNS = {}


def _driven(name):
    """NSTEPS of the oracle with two tracers, q = hlay (ctrg = 1) and a patchy concentration; behind every step one sample of
    the tracer moments and one of moments_ref's field moments.  Built once per golden."""
    if name in _RUNS:
        return _RUNS[name]
    g = Golden(name)
    assert not g.uses_cos(), name
    f = _fields(g)
    o = oracle_lib.Oracle(f, variant=g.variant)
    h0 = np.array(f.hlay, dtype=np.float64)
    q = np.stack([h0, T.patchy(f) * h0])
    rq = np.zeros(q.shape + (2,))
    rq[0] = f.rs_h
    ctrg = np.ones_like(q)
    W, S = f.neig[:, 4].astype(np.int64), f.neig[:, 6].astype(np.int64)
    tm, fm = TM.TracerMoments(f, 3), MR.Moments(2)
    n1 = f.p.ndeg + 1
    run = {"f": f, "tm": tm, "fm": fm, "wet": np.ones((f.p.nlay, n1), bool), "face_u": np.ones((f.p.nlay, n1), bool),
           "face_v": np.ones((f.p.nlay, n1), bool), "signs": set(), "dry_upwind": 0}
    for t in range(1, NSTEPS + 1):
        if t <= 3:
            o.rebuild_fluxes()                      # what the step is about to do itself: the same values
        gene, ramp, ctim = T.step_scalars(f.p, t, float(getattr(f, "tres", 0.0)))
        st = o.state()
        q, rq = T.update(f, st["hlay"], st["h_u"], st["h_v"], q, rq, ctrg, gene, ramp, ctim)
        o.step(t, 1)
        st = o.state()
        tm.sample(st["hlay"], st["h_u"], st["h_v"], q)
        fm.sample(st)
        wet = st["hlay"] > 0
        run["wet"] &= wet
        run["face_u"] &= wet | wet[:, W]
        run["face_v"] &= wet | wet[:, S]
        for key, fl, B in (("u", st["h_u"], W), ("v", st["h_v"], S)):
            if np.any(fl[:, 1:] > 0):
                run["signs"].add(key + "+")
            if np.any(fl[:, 1:] < 0):
                run["signs"].add(key + "-")
            # the upwind cell is dry and the other side is not: cf is the other side's concentration
            dry_up = ((fl > 0) & ~wet[:, B] & wet) | ((fl < 0) & ~wet & wet[:, B])
            run["dry_upwind"] += int(dry_up[:, 1:].sum())
    _RUNS[name] = run
    return run


def _assert_live():
    """The liveness the issue asks for, from the restatement alone; every comparison below calls this first."""
    signs, dry = set(), 0
    for name in GOLDENS:
        run = _driven(name)
        tm = run["tm"]
        for k in range(4):
            assert np.any(tm.sum[k, 1][:, 1:] != 0.0), (name, TM.QUANTITIES[k], "S of the patchy tracer never moved")
        assert np.any(tm.sq[1][:, 1:] != 0.0), (name, "Q of the patchy tracer never moved")
        signs |= run["signs"]
        dry += run["dry_upwind"]
        assert {"u+", "u-", "v+", "v-"} <= run["signs"], (name, run["signs"])
    assert dry > 0 and _driven("obc_mcbc0_2l")["dry_upwind"] > 0, "no sampled face has a dry upwind cell: the no-gradient branch is not reached"


def test_liveness_of_the_driven_runs():
    _assert_live()
    for name in GOLDENS:
        print(name, "faces with a dry upwind cell:", _driven(name)["dry_upwind"], "signs:", sorted(_driven(name)["signs"]))


@pytest.mark.parametrize("name", GOLDENS)
def test_a_tracer_equal_to_hlay_has_the_field_moments(name):
    _assert_live()
    run = _driven(name)
    tm, fm = run["tm"], run["fm"]
    assert tm.count == fm.count == NSTEPS
    # q: ref and S are those of hlay
    assert same_bits(tm.ref[0, 0][:, 1:], fm.ref[0][:, 1:]), (name, "ref_q vs ref of hlay")
    assert same_bits(tm.sum[0, 0][:, 1:], fm.sum[0][:, 1:]), (name, "S_q vs S of hlay")
    assert np.any(fm.sum[0][:, 1:] != 0.0), (name, "hlay never moved: nothing tested")
    # c: exactly 1 where the cell is wet in every sample, and its sums +0
    wet = run["wet"].copy()
    wet[:, 0] = False
    assert wet.any()
    assert np.all(tm.ref[1, 0][wet] == 1.0), (name, "ref_c")
    for a, what in ((tm.sum[1, 0], "S_c"), (tm.sq[0], "Q")):
        assert np.all(a[wet] == 0.0) and not np.any(np.signbit(a[wet])), (name, what)
    # fu, fv: those of h_u, h_v at every face with a wet cell on either side
    for k, fidx, key in ((2, 3, "face_u"), (3, 4, "face_v")):
        m = run[key].copy()
        m[:, 0] = False
        assert m.any() and np.any(fm.sum[fidx][m] != 0.0), (name, key)
        assert same_bits(tm.ref[k, 0][m], fm.ref[fidx][m]), (name, TM.QUANTITIES[k], "ref")
        assert same_bits(tm.sum[k, 0][m], fm.sum[fidx][m]), (name, TM.QUANTITIES[k], "S")
    # index 0 is no real cell: +0
    for a in (tm.ref, tm.sum, tm.sq):
        assert not np.any(a[..., 0]) and not np.any(np.signbit(a[..., 0]))


# ---- accuracy ---------------------------------------------------------------------------------------------------------------
NSAMPLES = 40
_SAMPLES = {}


def _rough_samples():
    """The bounds of test_moments_cpu count the roundings of the sequential sums; the single rounding of ref + S/N, half an ulp
    of the MEAN, is covered by their factor 2 only where the samples move by more than about |mean| / (4 (N-1)).  The driven
    runs above do not: away from the patch edges a concentration changes by rounding noise in 20 steps, and err - bound then is
    that half ulp (measured 5.6e-17 on c, 1.4e-14 on q).  So, as test_moments_cpu does, the samples are rough: 40 states of
    rough_inputs.rough_fields on the island golden's own Fields (thicknesses moved by up to 10 % of a layer, transports of both
    signs with exact zeros) and a patchy concentration scaled per cell and sample by a factor in [0.6, 1.4], negative in one
    cell in sixteen.  x[NSAMPLES, 4, 1, nlay, ndeg+1], the rounded FP64 quantities of the restatement."""
    if "x" not in _SAMPLES:
        f = _fields(Golden("island_3l_forced"))
        patch = T.patchy(f)
        xs = []
        for seed in range(1, NSAMPLES + 1):
            g = R.rough_fields(f, seed)
            r = np.random.default_rng([seed, 20261019])
            c = patch * r.uniform(0.6, 1.4, patch.shape) * np.where(r.uniform(0.0, 1.0, patch.shape) < 1.0 / 16.0, -1.0, 1.0)
            h = np.array(g.hlay, dtype=np.float64)
            xs.append(TM.quantities(f, h, g.h_u, g.h_v, (c * h)[None]))
        _SAMPLES["f"], _SAMPLES["x"] = f, np.stack(xs)
    return _SAMPLES["f"], _SAMPLES["x"]


def _fed(level, f, x):
    m = TM.TracerMoments(f, level)
    for s in x:
        m.sample_x(s)
    return m


def test_means_against_two_pass():
    """|mean - two-pass mean| <= 2 (N-1) 2^-53 sum|d| / N per element, the bound of test_moments_cpu.test_means_against_two_pass."""
    _assert_live()
    f, x = _rough_samples()
    N = x.shape[0]
    m = _fed(3, f, x)
    assert m.count == N
    for k in range(4):
        assert np.mean(x[:, k][..., 1:].std(axis=0) > 0.0) > 0.3, (TM.QUANTITIES[k], "hardly any element varies")
        two_pass = np.mean(x[:, k].astype(np.longdouble), axis=0)
        d = x[:, k] - m.ref[k][None]
        bound = 2.0 * (N - 1) * EPS * np.abs(d).sum(axis=0) / N
        err = np.abs(m.mean[k].astype(np.longdouble) - two_pass).astype(np.float64)
        worst = float(np.max(err - bound))
        print("%s: max |err| %.3g, max bound %.3g, worst err - bound %.3g" % (TM.QUANTITIES[k], err.max(), bound.max(), worst))
        assert np.all(err <= bound), (TM.QUANTITIES[k], worst)
    assert np.any(x[:, 1] < 0.0), "no negative concentration among the samples"


def test_variance_against_two_pass():
    """var_c = Q/N - (S_c/N)^2 within 2 (N-1) 2^-53 (P + 2 A A) + E E, A = sum|d_c| / N, P = sum|d_c d_c| / N,
    E = 2 (N-1) 2^-53 A: the bound of test_moments_cpu.test_variances_against_two_pass with a = b = c."""
    _assert_live()
    f, x = _rough_samples()
    N = x.shape[0]
    m = _fed(3, f, x)
    xc = x[:, 1].astype(np.longdouble)
    two_pass = np.mean((xc - xc.mean(axis=0)[None]) ** 2, axis=0)          # the second pass
    d = x[:, 1] - m.ref[1][None]
    A, P = np.abs(d).sum(axis=0) / N, np.abs(d * d).sum(axis=0) / N
    c = 2.0 * (N - 1) * EPS
    bound = c * (P + 2.0 * A * A) + (c * A) * (c * A)
    err = np.abs(m.var_c.astype(np.longdouble) - two_pass).astype(np.float64)
    print("var_c: max |err| %.3g, max bound %.3g, worst err - bound %.3g" % (err.max(), bound.max(), float(np.max(err - bound))))
    assert np.all(err <= bound), float(np.max(err - bound))
    assert float(np.max(two_pass)) > 0.0


def test_levels_reset_and_signed_zeros():
    _assert_live()
    f, x = _rough_samples()
    m3 = _fed(3, f, x[:8])
    for level, nq in ((1, 2), (2, 4)):
        m = _fed(level, f, x[:8])
        assert m.sq is None and m.ref.shape[0] == nq
        assert same_bits(m.ref, m3.ref[:nq]) and same_bits(m.sum, m3.sum[:nq]) and same_bits(m.mean, m3.mean[:nq]), level
    other = _fed(3, f, x[20:27])                   # something else first, then reset and the same samples: the same bits
    other.reset()
    assert other.count == 0
    for s in x[:8]:
        other.sample_x(s)
    for k in ("ref", "sum", "sq"):
        assert same_bits(getattr(other, k), getattr(m3, k)), k
    same3 = _fed(3, f, [x[0], x[0], x[0]])         # a sample equal to the reference leaves +0
    for a in (same3.sum, same3.sq):
        assert np.all(a == 0.0) and not np.any(np.signbit(a))


# ---- the header and the binding ---------------------------------------------------------------------------------------------------
NEW = capi.TRACER_MOMENT_EXPORTS
_CTYPE = {"beom_handle": C.c_void_p, "beom_multi_handle": C.c_void_p, "int": C.c_int, "double *": C.POINTER(C.c_double),
          "long long *": C.POINTER(C.c_longlong), "int *": C.POINTER(C.c_int), "char *": C.c_char_p}


def test_header_states_the_contract_and_the_binding_matches_it():
    want = {"beom_set_tracer_moments", "beom_reset_tracer_moments", "beom_sample_tracer_moments", "beom_download_tracer_moments",
            "beom_multi_set_tracer_moments", "beom_multi_reset_tracer_moments", "beom_multi_download_tracer_moments"}
    assert set(NEW) == want and want <= set(capi.EXPORTS)
    txt = open(os.path.join(ROOT, "include", "beom_hip.h")).read()
    assert re.search(r"^#define\s+BEOM_ABI_VERSION\s+2\s*$", txt, flags=re.M)
    assert "trc_conc" in txt and "trc_face" in txt and "STILL the upstream" in txt       # the contract names the sweep's own helpers
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = {}
    for name, args in re.findall(r"\bint\s+(beom_\w+)\s*\(([^)]*)\)\s*;", code):
        protos[name] = [" ".join(re.match(r"^\s*(.*?)(\w+)\s*$", " ".join(a.split())).group(1).split()) for a in args.split(",")]
    lib = capi.load()
    for name in want:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int, name
        assert list(fn.argtypes) == [_CTYPE[t] for t in protos[name]], (name, protos[name], fn.argtypes)
    for cls in (capi.Engine, capi.MultiEngine):
        for meth in ("set_tracer_moments", "reset_tracer_moments", "download_tracer_moments"):
            assert callable(getattr(cls, meth)), (cls.__name__, meth)
    assert callable(capi.Engine.sample_tracer_moments)


def test_null_handle_is_refused():
    lib = capi.load()
    err = C.create_string_buffer(200)
    assert lib.beom_set_tracer_moments(None, 1, 1, err, 199) == -1
    assert lib.beom_reset_tracer_moments(None) == -1
    assert lib.beom_sample_tracer_moments(None) == -1
    assert lib.beom_download_tracer_moments(None, None, None, None, None, None, None, err, 199) == -1
    assert lib.beom_multi_set_tracer_moments(None, 1, 1, err, 199) == -1
    assert lib.beom_multi_reset_tracer_moments(None, err, 199) == -1
    assert lib.beom_multi_download_tracer_moments(None, None, None, None, None, None, None, err, 199) == -1
