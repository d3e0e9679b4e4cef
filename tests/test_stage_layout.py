"""CPU: the layout of the host forms' staging arena (cityflow_amd/csrc/hip/cfx_stage_layout.h, plain C++).

tests/tools/stage_layout_main.cpp includes the header, is built here with the host compiler and run: offsets are multiples of
256 and the fields do not overlap, a null host pointer gives a null device address and takes no space, a host pointer with
zero bytes gives a distinct address inside the arena, the size is at least the sum of the fields', and the same fields declared
in another order give a valid layout again."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_stage_layout_rules(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    assert shutil.which(cxx), "no host compiler (%s)" % cxx
    exe = str(tmp_path / "stage_layout")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "cityflow_amd", "csrc", "hip"),
                           os.path.join(ROOT, "tests", "tools", "stage_layout_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
