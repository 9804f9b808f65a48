"""beom_plan::plan_step (beom_amd/csrc/beom_plan.h), the one function that decides which form a time step takes, without a
GPU: tests/step_plan_check.cpp, a stand-alone program built here with AddressSanitizer and UBSan and run as a child process.
It checks the invariants the engine's dispatcher relies on over combinations of the facts, options and step arguments, and
the rows DESIGN.md and the GPU tests state (the headline flow, the wind-driven fold, keep_diag, fold_stress = 0, a lid).
The header includes no HIP header: it compiles with a plain host compiler."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "step_plan_check.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _compiler():
    for cxx in ("g++", "/opt/rocm/llvm/bin/clang++"):
        found = shutil.which(cxx)
        if found:
            return found
    raise AssertionError("no host C++ compiler (g++ or ROCm's clang++): the plan cannot be checked")


def test_the_plan_of_every_step(tmp_path):
    exe = str(tmp_path / "step_plan_check")
    cxx = _compiler()
    # (g++ would leave ASan's runtime in a shared library: test_band_rows_cpu.py)
    static = ["-static-libasan"] if os.path.basename(cxx) == "g++" else []
    cc = subprocess.run([cxx] + FLAGS + static + ["-o", exe, SRC], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert "checks held" in run.stdout, run.stdout
    if os.environ.get("BEOM_STEP_PLAN_FULL"):       # the whole product, 1.9e10 plans: optimised and unsanitised, some 20 minutes
        cc = subprocess.run([cxx, "-std=c++17", "-O2", "-o", exe + "_full", SRC], capture_output=True, text=True)
        assert cc.returncode == 0, cc.stderr[-4000:]
        run = subprocess.run([exe + "_full", "full"], capture_output=True, text=True)
        assert run.returncode == 0 and "checks held" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
