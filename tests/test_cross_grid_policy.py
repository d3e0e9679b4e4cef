"""CPU: the sizing of kr_cross's grid (cityflow_amd/csrc/hip/cfx_launch_policy.h, plain C++) on synthetic job-count traces.

tests/tools/cross_grid_policy_main.cpp includes the header, is built here with the host compiler and run: a 35-step signal
cycle with trough to peak 1 : 3 reported 18 steps late (no launch after the first cycle may have fewer groups than the step
has jobs: a condition, not a tolerance), a count that falls to a quarter for good (within 2x of the last report's grid after
at most 512 steps), the behaviour before the first report, a constant trace, a single spike, and reports that repeat and skip
steps; with floor, cap, margin and the forced grid of the developer knob."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_cross_grid_policy_on_synthetic_traces(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    assert shutil.which(cxx), "no host compiler (%s)" % cxx
    exe = str(tmp_path / "cross_grid_policy")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "cityflow_amd", "csrc", "hip"),
                           os.path.join(ROOT, "tests", "tools", "cross_grid_policy_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
