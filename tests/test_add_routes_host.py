"""CPU: Spawner::addRoutes (cityflow_amd/csrc/host/flow.cpp), the host side of Engine.add_routes, outside Python.

tests/tools/add_routes_main.cpp is built here with flow.cpp and roadnet.cpp by the host compiler and run on example_1x1's files:
handles, dedupe against the flows' routes, every road pair either a route or refused as a whole, the index named for an unknown
road, an empty list and a single road with nothing added, the CSR tables whole, nothing dropped by a reset.  (The same program
is what a -fsanitize=address,undefined build runs.)"""
import json
import os
import shutil
import subprocess

from conftest import ROOT


def test_add_routes_program(scen, workdir, tmp_path):
    cxx = os.environ.get("CXX", "g++")
    assert shutil.which(cxx), "no host compiler (%s)" % cxx
    host = os.path.join(ROOT, "cityflow_amd", "csrc", "host")
    exe = str(tmp_path / "add_routes")
    subprocess.check_call([cxx, "-std=c++17", "-O0", "-Wall", "-Wno-sign-compare", "-ffp-contract=off", "-I" + host,
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "add_routes_main.cpp"),
                           os.path.join(host, "flow.cpp"), os.path.join(host, "roadnet.cpp"), "-o", exe])
    with open(scen.materialize("example_1x1", workdir)) as f:
        cfg = json.load(f)
    r = subprocess.run([exe, os.path.join(cfg["dir"], cfg["roadnetFile"]), os.path.join(cfg["dir"], cfg["flowFile"])],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
