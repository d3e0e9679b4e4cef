"""CPU: no step kernel of the built device library reads through a generic pointer.

A kernel that picks the vehicle-template table's copy in LDS or the table in global memory at run time holds a pointer of
unknown address space; every field read through it is a flat_load, and the wait for a flat_load (vmcnt(0) and lgkmcnt(0)) drains
every global load the kernel has in flight — the load rounds the step kernels are written in fall apart.  The
kernels take the table's place as a template flag instead (`templatesOf`, csrc/hip/cfx_kernels.h).  This reads the library's
gfx950 code with tools/isa_rounds.py; skipped where the library or LLVM's objdump / readelf are not there."""
import importlib.util
import os

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "cityflow_amd", "lib", "libcfx_hip.so")
# the kernels that stage the template table, by source file: cfx_ring_kernels.h, cfx_kernels.h, cfx_dense_kernels.h
KERNELS = ("kr_admit", "kr_cross", "kr_action", "kl_action", "k_action", "k_cross", "k_cross2", "kd_admit", "kd_action")


def _tool():
    spec = importlib.util.spec_from_file_location("isa_rounds", os.path.join(ROOT, "tools", "isa_rounds.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    tool = _tool()
    if not os.path.exists(LIB):
        pytest.skip("the device library is not built")
    if not tool.find_tool("llvm-objdump") or not tool.find_tool("llvm-readelf"):
        pytest.skip("no llvm-objdump / llvm-readelf")
    co = tool.code_object(LIB, str(tmp_path_factory.mktemp("code_object")))
    code = tool.disassemble(co)
    return tool, {sym: (tool.demangle(sym), ins) for sym, ins in code.items()}


def test_step_kernels_have_no_flat_load(listing):
    tool, code = listing
    seen = set()
    for sym, (pretty, ins) in sorted(code.items()):
        base = tool.base_name(pretty)
        if base not in KERNELS:
            continue
        seen.add(base)
        flat = [i for i in ins if i.split()[0].startswith("flat_load")]
        assert not flat, "%s: %d flat_load, the first `%s`" % (pretty, len(flat), flat[0])
    assert seen == set(KERNELS), "kernels not found in the library: %s" % sorted(set(KERNELS) - seen)


def test_both_places_of_the_table_are_built(listing):
    """every one of those kernels exists reading LDS (ds_read) and reading global memory only (no LDS copy of the table)"""
    tool, code = listing
    by_base = {}
    for sym, (pretty, ins) in code.items():
        base = tool.base_name(pretty)
        if base in KERNELS:
            by_base.setdefault(base, []).append((pretty, sum(i.split()[0].startswith("ds_read") for i in ins)))
    for base in KERNELS:
        inst = by_base[base]
        assert len(inst) % 2 == 0, (base, sorted(inst))
        lds = sorted(p for p, _n in inst if p.rstrip(" >").endswith("false"))
        glb = sorted(p for p, _n in inst if p.rstrip(" >").endswith("true"))
        assert len(lds) == len(glb) == len(inst) // 2, (base, sorted(inst))
        n = dict(inst)
        for a, b in zip(lds, glb):
            assert n[a] > n[b], "%s reads LDS %d times, %s %d times" % (a, n[a], b, n[b])
