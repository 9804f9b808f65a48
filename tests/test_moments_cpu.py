"""The moments' contract on the CPU (include/beom_hip.h, "Moments"): the numpy restatement (moments_ref) against two-pass
means and variances in long double on rough samples, with the error bounds written out; the reason for the shift, on the
deep-layer signal the header quotes; reset, levels, signed zeros; the header and the binding.  No GPU."""
import os
import re

import numpy as np

import moments_ref as MR
import rough_inputs as R
from beom_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
NSAMPLES = 40


def _rough_samples(n=NSAMPLES):
    """n rough states of one small three-layer frame (rough_inputs amplitudes: thicknesses moved by up to 10 % of a layer,
    velocities in +-5 cm/s with exact +0 and -0 sprinkled in), each a list of the five fields [nlay, ndeg+1]."""
    f = R.base_fields("closed_leith_3l", "130x18")
    out = []
    for seed in range(1, n + 1):
        g = R.rough_fields(f, seed)
        out.append([np.array(getattr(g, k), dtype=np.float64) for k in MR.FIELDS])
    return out


_SAMPLES = {}


def samples():
    if "s" not in _SAMPLES:
        _SAMPLES["s"] = _rough_samples()
    return _SAMPLES["s"]


def _fed(level, smp):
    m = MR.Moments(level)
    for s in smp:
        m.sample(s)
    return m


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_rough_samples_are_rough():
    smp = samples()
    u = np.stack([s[1] for s in smp])
    assert np.any((u == 0.0) & ~np.signbit(u) & (np.abs(u).max(axis=0) > 0.0)[None]), "no exact +0 among moving velocities"
    assert np.any((u == 0.0) & np.signbit(u)), "no exact -0 in the velocities"
    for f in range(5):
        x = np.stack([s[f] for s in smp])
        assert np.mean(x.std(axis=0) > 0.0) > 0.3, (MR.FIELDS[f], "hardly any element varies")


def test_means_against_two_pass():
    """|mean - two-pass mean| <= 2 (N-1) 2^-53 sum|d| / N per element: the bound of a sequential sum of the N - 1 terms d
    ((N-1) 2^-53 sum|d| for S, over N), with a factor 2 for the roundings of d = x - ref, of S / N and of ref + S / N."""
    smp = samples()
    N = len(smp)
    m = _fed(3, smp)
    assert m.count == N
    for f in range(5):
        x = np.stack([s[f] for s in smp])
        two_pass = np.mean(x.astype(np.longdouble), axis=0)
        d = x - m.ref[f][None]
        bound = 2.0 * (N - 1) * EPS * np.abs(d).sum(axis=0) / N
        err = np.abs(m.mean[f].astype(np.longdouble) - two_pass).astype(np.float64)
        worst = float(np.max(err - bound))
        print("%s: max |err| %.3g, max bound %.3g, worst err - bound %.3g" % (MR.FIELDS[f], err.max(), bound.max(), worst))
        assert np.all(err <= bound), (MR.FIELDS[f], worst)


def test_variances_against_two_pass():
    """var = Q/N - (S_a/N)(S_b/N).  With A_a = sum|d_a| / N and P = sum|d_a d_b| / N the same sequential-sum bound gives
    2 (N-1) 2^-53 P for Q / N and E_a = 2 (N-1) 2^-53 A_a for S_a / N, whose product with S_b / N (|S_b / N| <= A_b) is then
    off by at most E_a A_b + E_b A_a + E_a E_b.  Bound: 2 (N-1) 2^-53 (P + 2 A_a A_b) + E_a E_b."""
    smp = samples()
    N = len(smp)
    m = _fed(3, smp)
    var = m.var
    for k, (a, b) in enumerate(MR.PAIRS):
        xa = np.stack([s[a] for s in smp]).astype(np.longdouble)
        xb = np.stack([s[b] for s in smp]).astype(np.longdouble)
        two_pass = np.mean((xa - xa.mean(axis=0)[None]) * (xb - xb.mean(axis=0)[None]), axis=0)      # the second pass
        da = np.stack([s[a] for s in smp]) - m.ref[a][None]
        db = np.stack([s[b] for s in smp]) - m.ref[b][None]
        A, B, P = np.abs(da).sum(axis=0) / N, np.abs(db).sum(axis=0) / N, np.abs(da * db).sum(axis=0) / N
        c = 2.0 * (N - 1) * EPS
        bound = c * (P + 2.0 * A * B) + (c * A) * (c * B)
        err = np.abs(var[k].astype(np.longdouble) - two_pass).astype(np.float64)
        print("moment %d %s: max |err| %.3g, max bound %.3g, worst err - bound %.3g"
              % (k, (MR.FIELDS[a], MR.FIELDS[b]), err.max(), bound.max(), float(np.max(err - bound))))
        assert np.all(err <= bound), (k, float(np.max(err - bound)))
        assert float(np.max(two_pass)) > 0.0


def test_the_shift_keeps_a_deep_layers_variance():
    """h = 4000 + 0.01 sin(0.0137 t + phi) + 0.003 noise, 16 cells, 100 000 samples: the shifted variance is within 1e-10
    relative of the long-double two-pass value (measured 5.8e-14); the plain sums of x and x*x, accumulated the same way, are
    off by more than 1e-4 (measured 7.2e-3)."""
    rng = np.random.default_rng(20261017)
    n, cells = 100000, 16
    t = np.arange(n, dtype=np.float64)[:, None]
    phi = rng.uniform(0.0, 2.0 * np.pi, cells)[None, :]
    h = 4000.0 + 0.01 * np.sin(0.0137 * t + phi) + 0.003 * rng.standard_normal((n, cells))
    zero = np.zeros(cells)
    m = MR.Moments(3)
    for k in range(n):
        m.sample((h[k], zero, zero, zero, zero))
    hl = h.astype(np.longdouble)
    two_pass = np.mean((hl - hl.mean(axis=0)[None]) ** 2, axis=0)
    shifted = float(np.max(np.abs(m.var[0].astype(np.longdouble) - two_pass) / two_pass))
    sx, sxx = np.cumsum(h, axis=0)[-1], np.cumsum(h * h, axis=0)[-1]          # (cumsum adds in sequence, in FP64)
    plain_var = sxx / n - (sx / n) * (sx / n)
    plain = float(np.max(np.abs(plain_var.astype(np.longdouble) - two_pass) / two_pass))
    print("relative error of the variance: shifted %.3g, plain %.3g" % (shifted, plain))
    assert shifted <= 1.0e-10, shifted
    assert plain > 1.0e-4, plain


def test_reset_then_the_same_samples_gives_the_same_bits():
    smp = samples()[:8]
    m = _fed(3, samples()[20:27])          # something else first
    first = _fed(3, smp)
    m.reset()
    assert m.count == 0
    for s in smp:
        m.sample(s)
    for k in ("ref", "sum", "sq"):
        assert np.array_equal(_bits(getattr(m, k)), _bits(getattr(first, k))), k
    assert m.count == first.count == 8


def test_levels_1_and_2_are_level_3s_subset():
    smp = samples()[:8]
    m3 = _fed(3, smp)
    for level, nf in ((1, 3), (2, 5)):
        m = _fed(level, smp)
        assert m.sq is None and m.ref.shape[0] == nf
        assert np.array_equal(_bits(m.ref), _bits(m3.ref[:nf])) and np.array_equal(_bits(m.sum), _bits(m3.sum[:nf])), level
        assert np.array_equal(_bits(m.mean), _bits(m3.mean[:nf])), level


def test_a_sample_equal_to_the_reference_leaves_plus_zero():
    s = samples()[0]
    assert np.any(np.signbit(s[1]) & (s[1] == 0.0))      # -0.0 among the references too
    m = _fed(3, [s, s, s])
    assert m.count == 3
    for a in (m.sum, m.sq):
        assert np.all(a == 0.0) and not np.any(np.signbit(a))
    assert np.array_equal(_bits(m.ref), _bits(np.stack(s)))


def _header():
    return open(os.path.join(ROOT, "include", "beom_hip.h")).read()


def test_header_declares_the_moments_and_keeps_the_abi_version():
    txt = _header()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\bint\s+(beom_\w+)\s*\(", code))
    want = {"beom_set_moments", "beom_reset_moments", "beom_sample_moments", "beom_download_moments",
            "beom_multi_set_moments", "beom_multi_reset_moments", "beom_multi_download_moments"}
    assert want <= declared, want - declared
    assert re.search(r"^#define\s+BEOM_ABI_VERSION\s+2\s*$", txt, flags=re.M)
    assert capi.BEOM_ABI_VERSION == 2
    assert "7.2e-3" in txt and "5.8e-14" in txt          # the reason for the shift is stated where the contract is


def test_binding_has_every_moments_call():
    want = {"beom_set_moments", "beom_reset_moments", "beom_sample_moments", "beom_download_moments",
            "beom_multi_set_moments", "beom_multi_reset_moments", "beom_multi_download_moments"}
    assert want <= set(capi.EXPORTS)
    lib = capi.load()
    for name in want:
        assert getattr(lib, name).argtypes is not None, name
    for cls in (capi.Engine, capi.MultiEngine):
        for meth in ("set_moments", "reset_moments", "download_moments"):
            assert callable(getattr(cls, meth)), (cls.__name__, meth)
    assert callable(capi.Engine.sample_moments)
