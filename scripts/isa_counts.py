"""Instruction counts of the step kernels' compiled code, without a GPU: cross-compiles
csrc/fjsp_hip.hip to gfx950 assembly with the library's own flags (_native.HIPCC_FLAGS) and prints,
per kernel instance, the counts of flat_*, global_load_* / global_store_* (and how many of those
use an SGPR base, the saddr form), ds_read_* / ds_write_*, v_lshl_add_u64, the v_* and s_* totals,
v_readlane / v_writelane, VGPRs, SGPRs and the scratch size.  flat_in_loop counts the flat_*
instructions that lie between a label and a later branch back to it (a step loop or a loop inside
one); the others sit in a launch's prologue or epilogue.

usage: python scripts/isa_counts.py [--filter SUBSTR] [--json] [-D...]   (extra -D flags go to hipcc)
"""
import importlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
nat = importlib.import_module("multi-agent-rl-for-fjsp_amd._native")

COLS = ["flat", "flat_in_loop", "global_load", "global_store", "global_saddr", "ds_read", "ds_write",
        "v_lshl_add_u64", "v_total", "s_total", "v_readlane", "v_writelane", "vgpr", "sgpr", "scratch"]
BRANCH = re.compile(r"^s_c?branch\w*\s+(\S+)")


def assemble(defs):
    flags = [f for f in nat.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory(prefix="fjsp_isa_") as tmp:
        out = os.path.join(tmp, "fjsp_hip.s")
        subprocess.run(["hipcc"] + flags + defs + ["--cuda-device-only", "-S", "-o", out, nat.SRC], check=True)
        with open(out) as f:
            return f.read().splitlines()


def demangle(names):
    hipcc = os.path.realpath(shutil.which("hipcc") or "hipcc")   # ROCm's own llvm-cxxfilt lies beside its clang
    rocm_llvm = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "llvm", "bin", "llvm-cxxfilt")
    for tool in ("llvm-cxxfilt", rocm_llvm, "c++filt"):
        try:
            r = subprocess.run([tool] + names, capture_output=True, text=True, check=True)
            return r.stdout.splitlines()
        except (OSError, subprocess.CalledProcessError):
            continue
    return names


def count(body):
    """body: the lines of one function between its label and its end."""
    c = dict.fromkeys(COLS, 0)
    labels, ins = {}, []
    for ln in body:
        s = ln.split(";")[0].strip()
        if not s or s.startswith("."):
            if s.endswith(":"):
                labels[s[:-1]] = len(ins)
            continue
        if s.endswith(":"):
            labels[s[:-1]] = len(ins)
            continue
        ins.append(s)
    loops = []   # [first, last] instruction index of every backward branch's span
    for i, s in enumerate(ins):
        m = BRANCH.match(s)
        if m and m.group(1) in labels and labels[m.group(1)] <= i:
            loops.append((labels[m.group(1)], i))
    for i, s in enumerate(ins):
        op = s.split()[0]
        if op.startswith("flat_"):
            c["flat"] += 1
            c["flat_in_loop"] += any(a <= i <= b for a, b in loops)
        elif op.startswith("global_load_") or op.startswith("global_store_"):
            c["global_load" if op.startswith("global_load_") else "global_store"] += 1
            args = [a.strip() for a in s[len(op):].split(",")]
            c["global_saddr"] += any(a.startswith("s[") for a in args)
        elif op.startswith("ds_read") or op.startswith("ds_write"):
            c["ds_read" if op.startswith("ds_read") else "ds_write"] += 1
        if op.startswith("v_"):
            c["v_total"] += 1
            for k in ("v_lshl_add_u64", "v_readlane", "v_writelane"):
                c[k] += op.startswith(k)
        elif op.startswith("s_"):
            c["s_total"] += 1
    return c


def kernels(lines):
    kern = {m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m}
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(\w+):", lines[i])
        if m and m.group(1) in kern:
            name, j = m.group(1), i + 1
            while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
                j += 1
            c = count(lines[i + 1:j])
            for k in range(j, min(j + 80, len(lines))):   # the function's resource comments
                for key, pat in (("vgpr", r";\s*NumVgprs:\s*(\d+)"), ("sgpr", r";\s*TotalNumSgprs:\s*(\d+)"),
                                 ("scratch", r";\s*ScratchSize:\s*(\d+)")):
                    mm = re.match(pat, lines[k].strip())
                    if mm:
                        c[key] = int(mm.group(1))
            out[name] = c
            i = j
        i += 1
    return out


def main():
    args = sys.argv[1:]
    defs = [a for a in args if a.startswith("-D")]
    filt = args[args.index("--filter") + 1] if "--filter" in args else ""
    ks = kernels(assemble(defs))
    names = sorted(ks)
    nice = dict(zip(names, demangle(names)))
    short = lambda s: re.sub(r"^void ", "", s.replace("(anonymous namespace)::", "")).split("(")[0]
    rows = {short(nice[k]): ks[k] for k in names if filt in nice[k]}
    if "--json" in args:
        print(json.dumps(rows, indent=1))
        return
    w = max(len(k) for k in rows)
    print("| " + "kernel".ljust(w) + " | " + " | ".join(COLS) + " |")
    print("|" + "---|" * (len(COLS) + 1))
    for k in sorted(rows):
        print("| " + k.ljust(w) + " | " + " | ".join(str(rows[k][c]) for c in COLS) + " |")


if __name__ == "__main__":
    main()
