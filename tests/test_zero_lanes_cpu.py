"""The two facts the zero-lane shortcut of uv_core rests on, without a GPU.

1. With a zero rate and a +0 target the nudging expression of a lane whose velocity is an exact zero is +0 whatever the
   sign of that zero: numpy float64 (IEEE, round to nearest), compared by bit pattern.
2. beom_dense::vel_targets_zero (beom_amd/csrc/beom_dense_host.h), the host scan behind DevView::vel_targets_zero:
   tests/vel_targets_check.cpp, a stand-alone program built here with AddressSanitizer and UBSan and run as a child process."""
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "vel_targets_check.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def test_the_replaced_expression_is_plus_zero_for_either_zero():
    vold = np.array([0.0, -0.0])
    assert list(_bits(vold)) == [0, 1 << 63]
    f_ng = np.float64(0.0)
    for xdir in (True, False):
        vfor = np.full(2, 0.0)                             # the target, +0
        vfor = vfor + 0.0 if xdir else vfor - 0.0          # the Ekman term of the plain form
        vfor = vfor + 0.0                                  # the tide of the plain form
        new = vfor * f_ng + vold * (1.0 - f_ng)
        assert list(_bits(new)) == [0, 0], (xdir, new)
    # and why a -0.0 target must clear the flag: (-0)*0 + (-0)*(1-0) keeps the sign
    assert _bits(np.float64(-0.0) * f_ng + np.float64(-0.0) * (1.0 - f_ng)) == 1 << 63


def _compiler():
    for cxx in ("g++", "/opt/rocm/llvm/bin/clang++"):
        found = shutil.which(cxx)
        if found:
            return found
    raise AssertionError("no host C++ compiler (g++ or ROCm's clang++): the scan cannot be checked")


def test_the_scan_of_the_velocity_targets(tmp_path):
    exe = str(tmp_path / "vel_targets_check")
    cxx = _compiler()
    # (g++ would leave ASan's runtime in a shared library: test_band_rows_cpu.py)
    static = ["-static-libasan"] if os.path.basename(cxx) == "g++" else []
    cc = subprocess.run([cxx] + FLAGS + static + ["-o", exe, SRC], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert "checks held" in run.stdout, run.stdout
