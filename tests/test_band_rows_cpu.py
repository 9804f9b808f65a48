"""The band geometry and the one row copy of beom_amd/csrc/beom_bands_host.h (every scatter and gather of global arrays in
beom_multi.hip) against their definition index by index: tests/band_rows_check.cpp, a stand-alone program built here with
AddressSanitizer and UBSan and run as a child process.  No GPU: the header is host index arithmetic only."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "band_rows_check.cpp")
HEADER = os.path.join(HERE, "..", "beom_amd", "csrc", "beom_bands_host.h")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _compiler():
    for cxx in ("g++", "/opt/rocm/llvm/bin/clang++"):
        found = shutil.which(cxx)
        if found:
            return found
    raise AssertionError("no host C++ compiler (g++ or ROCm's clang++): the band geometry cannot be checked")


def test_band_rows_against_their_definition(tmp_path):
    with open(SRC) as f:
        text = f.read()
    includes = [ln for ln in text.splitlines() if ln.startswith('#include "')]
    assert includes == ['#include "../beom_amd/csrc/beom_bands_host.h"'], includes      # the header stands alone
    with open(HEADER) as f:
        assert not [ln for ln in f.read().splitlines() if ln.startswith("#include") and "hip" in ln.lower()]      # no HIP, no C ABI
    exe = str(tmp_path / "band_rows_check")
    cxx = _compiler()
    # g++ would leave ASan's runtime in a shared library, which insists on being the first one loaded; inside the program
    # (clang++'s default) it runs whatever else the loader brings along
    static = ["-static-libasan"] if os.path.basename(cxx) == "g++" else []
    cc = subprocess.run([cxx] + FLAGS + static + ["-o", exe, SRC], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert "checks held" in run.stdout, run.stdout
