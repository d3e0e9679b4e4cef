"""Developer tool: the load rounds of the step kernels as the compiler emitted them (profiles/load_rounds.txt).
usage: python tools/isa_rounds.py <libcfx_hip.so> [--kernels kr_action,kr_cross,...] [--all-instances]

The step kernels are chains of dependent load rounds; what a round costs is a wait, whatever it carries.  Per kernel this
prints the registers and scratch of its code object's metadata, how many of its loads go through a generic pointer
(flat_load: waited for with vmcnt(0) lgkmcnt(0), which drains every global load in flight), and — in the order of the
listing, which is the order of the source for straight-line code, not of any one path through the branches — every
s_waitcnt that names vmcnt, with the memory loads issued since the previous one:

    g3 f1 | vmcnt(0) lgkmcnt(0)       three global loads and one flat load, then a full drain

g = global_load, f = flat_load, b = buffer_load, s = scratch_load (a spill's reload).  Loads from LDS (ds_read) and scalar
loads are counted per kernel only: they do not wait on vmcnt.  Needs llvm-objdump and llvm-readelf (ROCm's llvm/bin, or PATH).
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

STEP_KERNELS = ("kr_admit", "kr_action", "kl_action", "kr_cross", "k_cross2", "kd_admit", "kd_action", "k_action", "k_cross")
LOAD_KINDS = (("global_load", "g"), ("flat_load", "f"), ("buffer_load", "b"), ("scratch_load", "s"))


def find_tool(name):
    """Path of an LLVM tool: next to hipcc ($HIPCC or /opt/rocm), or on PATH; None where there is none."""
    roots = [os.path.join(os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "llvm", "bin"),
             "/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin"]
    for r in roots:
        p = os.path.join(r, name)
        if os.access(p, os.X_OK):
            return p
    return shutil.which(name)


def code_object(lib, workdir):
    """The gfx950 code object of the library's fat binary, extracted into `workdir` (llvm-objdump --offloading writes
    next to its input: the input is a copy)."""
    objdump = find_tool("llvm-objdump")
    if not objdump:
        raise RuntimeError("no llvm-objdump")
    copy = os.path.join(workdir, "lib.so")
    shutil.copyfile(lib, copy)
    subprocess.check_call([objdump, "--offloading", copy], stdout=subprocess.DEVNULL)
    cos = sorted(f for f in os.listdir(workdir) if "amdgcn" in f and "gfx950" in f)
    if not cos:
        raise RuntimeError("no gfx950 code object in " + lib)
    return os.path.join(workdir, cos[0])


def demangle(sym):
    """Readable name of an Itanium-mangled kernel symbol, good enough for this library: `name<template arguments>`."""
    filt = shutil.which("c++filt") or find_tool("llvm-cxxfilt")
    if filt:
        out = subprocess.run([filt, sym], capture_output=True, text=True).stdout.strip()
        if out:
            out = re.sub(r"^void ", "", out)
            depth, cut = 0, len(out)
            for i, ch in enumerate(out):  # the parameter list starts at the first '(' outside the template arguments
                depth += ch == "<"
                depth -= ch == ">"
                if ch == "(" and depth == 0:
                    cut = i
                    break
            return out[:cut].replace("cfxd::", "")
    return sym


def base_name(pretty):
    return pretty.split("<")[0].split("::")[-1]


def metadata(co):
    """{symbol: {vgpr, scratch, vgpr_spill, sgpr_spill, lds}} from the code object's notes."""
    readelf = find_tool("llvm-readelf")
    if not readelf:
        raise RuntimeError("no llvm-readelf")
    txt = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    out, cur = {}, {}
    for line in txt.splitlines():
        m = re.match(r"\s*(?:- )?\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "agpr_count":  # (first key of a kernel's map)
            cur = {}
        cur[k] = v
        if k == "wavefront_size" and "name" in cur:
            out[cur["name"]] = {"vgpr": int(cur.get("vgpr_count", -1)), "scratch": int(cur.get("private_segment_fixed_size", -1)),
                                "vgpr_spill": int(cur.get("vgpr_spill_count", -1)), "sgpr_spill": int(cur.get("sgpr_spill_count", -1)),
                                "lds": int(cur.get("group_segment_fixed_size", -1))}
    return out


def disassemble(co):
    """{symbol: [mnemonic + operands, ...]} of the code object's functions."""
    objdump = find_tool("llvm-objdump")
    txt = subprocess.run([objdump, "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith(("\t", " ")):
            continue
        ins = line.split("//")[0].strip()
        if ins:
            cur.append(ins)
    return out


def rounds(instrs):
    """(counts, [(loads since the previous wait as {kind: n}, the wait's text)]) of one kernel's listing."""
    counts = {"flat_load": 0, "global_load": 0, "buffer_load": 0, "scratch_load": 0, "ds_read": 0, "s_load": 0, "vm_waits": 0, "drains": 0}
    seq, pend = [], {}
    for ins in instrs:
        op = ins.split()[0]
        if op.startswith(("ds_read", "ds_load")):
            counts["ds_read"] += 1
        elif op.startswith(("s_load", "s_buffer_load")):
            counts["s_load"] += 1
        for prefix, tag in LOAD_KINDS:
            if op.startswith(prefix):
                counts[prefix] += 1
                pend[tag] = pend.get(tag, 0) + 1
        if op == "s_waitcnt" and "vmcnt" in ins:
            counts["vm_waits"] += 1
            if "vmcnt(0)" in ins and "lgkmcnt(0)" in ins:
                counts["drains"] += 1
            seq.append((pend, ins[len("s_waitcnt"):].strip()))
            pend = {}
    if pend:
        seq.append((pend, "(end)"))
    return counts, seq


def report(lib, kernels=STEP_KERNELS, all_instances=False, out=sys.stdout):
    with tempfile.TemporaryDirectory() as wd:
        co = code_object(lib, wd)
        meta, code = metadata(co), disassemble(co)
    rows = []
    for sym in code:
        pretty = demangle(sym)
        if base_name(pretty) in kernels and sym in meta:
            rows.append((pretty, sym))
    for pretty, sym in sorted(rows):
        c, seq = rounds(code[sym])
        m = meta[sym]
        out.write("%s\n  vgpr %d, scratch %d B, spilled vgpr %d / sgpr %d, lds %d B; flat_load %d, global_load %d, buffer_load %d, "
                  "scratch_load %d, ds_read %d, s_load %d; vmcnt waits %d, of them vmcnt(0) lgkmcnt(0) %d\n" % (
                      pretty, m["vgpr"], m["scratch"], m["vgpr_spill"], m["sgpr_spill"], m["lds"], c["flat_load"], c["global_load"],
                      c["buffer_load"], c["scratch_load"], c["ds_read"], c["s_load"], c["vm_waits"], c["drains"]))
        if all_instances or is_headline(pretty):
            line = "  "
            for loads, wait in seq:
                item = "%s | %s" % (" ".join("%s%d" % (t, loads[t]) for _p, t in LOAD_KINDS if t in loads) or "-", wait)
                if len(line) + len(item) > 118:
                    out.write(line.rstrip() + "\n")
                    line = "  "
                line += item + ";  "
            out.write(line.rstrip() + "\n")
    return rows


def is_headline(pretty):
    """The instantiations the single engine runs with up to kLdsTempl templates: the wait sequences of the others (tiles'
    ghost lanes, the big batches, tables in global memory) differ little and are printed with --all-instances only."""
    return pretty in ("kr_action<256, false, false>", "kl_action<false, false>", "kr_cross<false>", "kr_cross",
                      "kr_action<256, false>", "kl_action<false>", "kr_admit<true, 128, SpawnBatchT<128>, false>",
                      "kr_admit<true, 128, SpawnBatchT<128> >", "kr_admit<true, 128, SpawnBatchT<128>>", "kd_action<false>", "kd_action")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 1:
        sys.exit(__doc__)
    kernels = STEP_KERNELS
    for a in sys.argv[1:]:
        if a.startswith("--kernels"):
            kernels = tuple(a.split("=", 1)[1].split(","))
    report(args[0], kernels, "--all-instances" in sys.argv)


if __name__ == "__main__":
    main()
