#!/usr/bin/env python3
"""Static instruction table of named kernels from `hipcc -S` output (no GPU needed).

usage: tools/isa_table.py FILE.s [-k SUBSTRING ...] [--regions]
       tools/isa_table.py --compile crowdmod-ddpm-4d_amd/csrc/cm_conv_wino.hip [-k ...]

Per kernel whose (demangled or mangled) name contains every -k substring: static instructions, scalar (s_*), vector ALU (v_* without
the matrix and lane-spill instructions), matrix (v_mfma*), lane-spill instructions (v_readlane / v_writelane: the scalar registers
the allocator parks in vector lanes), v_mov, branches, and the .sgpr_spill_count / .vgpr_count / .sgpr_count metadata.  --regions
splits a kernel at its matrix instructions: before the first, from the first to the last (the chunk loop), after the last.
Static counts are not time: they say what a launch carries, the counters (tools/pmc_insts.sh) say what it executes."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-DCM_PD27=3", "-DCM_PD8=2", "--cuda-device-only", "-S"]


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(name):
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(.*$", "", name)
    return name.replace("cm::", "").replace("(bool)", "").replace("false", "0").replace("true", "1")


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith("v_readlane") or op.startswith("v_writelane"):
        return "lane"
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branch"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    return "other"


def parse(path):
    kernels, meta = {}, {}
    cur, name = None, None
    with open(path) as f:
        for line in f:
            m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", line)
            if m and not m.group(1).startswith(".L"):
                cur = kernels.setdefault(m.group(1), [])
                continue
            if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
                cur = None
                continue
            s = line.strip()
            if cur is not None and s and not s.startswith((";", ".", "//")) and not s.endswith(":"):
                cur.append(s.split()[0])
            m = re.match(r"^\s+\.name:\s+(\S+)", line)
            if m:
                name = m.group(1)
                meta.setdefault(name, {})
            m = re.match(r"^\s+\.(sgpr_spill_count|vgpr_count|sgpr_count|vgpr_spill_count):\s+(\d+)", line)
            if m and name:
                meta[name][m.group(1)] = int(m.group(2))
    return {k: v for k, v in kernels.items() if k in meta}, meta


def counts(ops):
    c = {"all": len(ops), "salu": 0, "valu": 0, "mfma": 0, "lane": 0, "branch": 0, "lds": 0, "vmem": 0, "other": 0, "v_mov": 0}
    for op in ops:
        c[classify(op)] += 1
        if op.startswith("v_mov") or op.startswith("v_accvgpr"):
            c["v_mov"] += 1
    return c


def row(label, c, md=None):
    tail = "" if md is None else " | %5d %5d %5d" % (md.get("sgpr_spill_count", 0), md.get("vgpr_count", 0), md.get("sgpr_count", 0))
    return "%-58s %6d %6d %6d %5d %5d %6d %6d %5d %5d%s" % (label[:58], c["all"], c["salu"], c["valu"], c["mfma"], c["lane"], c["v_mov"],
                                                            c["branch"], c["lds"], c["vmem"], tail)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("file", help="assembly (.s) of hipcc -S, or with --compile a .hip source")
    ap.add_argument("-k", "--kernel", action="append", default=[], help="substring of the kernel name (all must match); repeatable")
    ap.add_argument("--regions", action="store_true", help="split at the first / last matrix instruction")
    ap.add_argument("--compile", action="store_true", help="FILE is a .hip source: compile it for gfx950 first")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    a = ap.parse_args()
    path = a.file
    if a.compile:
        tmp = tempfile.NamedTemporaryFile(suffix=".s", delete=False)
        tmp.close()
        subprocess.run([a.hipcc] + FLAGS + [os.path.basename(a.file), "-o", tmp.name], check=True, cwd=os.path.dirname(os.path.abspath(a.file)),
                       stderr=subprocess.DEVNULL)
        path = tmp.name
    kernels, meta = parse(path)
    if a.compile:
        os.unlink(path)
    dm = demangle(sorted(kernels))
    print("%-58s %6s %6s %6s %5s %5s %6s %6s %5s %5s | %5s %5s %5s" % ("kernel", "instr", "scalar", "vector", "mfma", "lane", "v_mov", "branch", "lds",
                                                                       "vmem", "sgprS", "vgpr", "sgpr"))
    n = 0
    for k in sorted(kernels, key=lambda k: short(dm[k])):
        label = short(dm[k])
        if not all(sub in label or sub in k for sub in a.kernel):
            continue
        n += 1
        ops = kernels[k]
        print(row(label, counts(ops), meta[k]))
        if a.regions:
            mf = [i for i, op in enumerate(ops) if classify(op) == "mfma"]
            if mf:
                print(row("    before the first matrix instruction", counts(ops[:mf[0]])))
                print(row("    first to last matrix instruction", counts(ops[mf[0]:mf[-1] + 1])))
                print(row("    after the last matrix instruction", counts(ops[mf[-1] + 1:])))
    if not n:
        sys.exit("no kernel matches")


if __name__ == "__main__":
    main()
