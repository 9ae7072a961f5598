"""Compare the gfx950 code of every kernel two builds share, instruction for instruction.

Usage:  python scripts/isa_diff.py parent.s result.s [--json out.json]

Both files are device assembly of one source file (hipcc --offload-arch=gfx950 -O3 -std=c++17
-ffp-contract=off --cuda-device-only -S).  A kernel's body is the text between its label and its
.Lfunc_end; basic-block labels are renumbered per function (their numbers count the functions in
front) and an empty trailing parameter pack (`J E` in the mangled template arguments, `DpT1_` at
the end of the name) is dropped, so that
k_step<true, 64> of a build with the pack pairs with k_step<true, 64> of one without.  Prints one
line per kernel: same / DIFFERENT / only in one build; exit status 1 if a shared kernel differs."""
import json
import re
import sys


def kernels(path):
    text = open(path).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out = {}
    for name in names:
        m = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S)
        body = m.group(0)
        lines = []
        for ln in body.splitlines()[1:-1]:
            ln = ln.split(";")[0].rstrip()
            if not ln.strip() or ln.lstrip().startswith((".p2align", ".loc", ".file", ".cfi")):
                continue
            lines.append(re.sub(r"\.L(BB|Ltmp|tmp)\d+_", r".L\1_", ln))
        key = re.sub(r"DpT\d+_$", "", name.replace("EJEEEv", "EEEv")) if "EJEEEv" in name else name
        out[key] = [l.replace(name, key) for l in lines]
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    res = {"same": [], "different": [], "only_parent": sorted(set(a) - set(b)), "only_result": sorted(set(b) - set(a))}
    for k in sorted(set(a) & set(b)):
        res["same" if a[k] == b[k] else "different"].append({"kernel": k, "instructions": len(a[k])})
    for k in res["same"]:
        print("same      %6d  %s" % (k["instructions"], k["kernel"]))
    for k in res["different"]:
        print("DIFFERENT %6d  %s" % (k["instructions"], k["kernel"]))
    for k in res["only_parent"]:
        print("only in the first build   ", k)
    for k in res["only_result"]:
        print("only in the second build  ", k)
    if "--json" in sys.argv:
        json.dump(res, open(sys.argv[sys.argv.index("--json") + 1], "w"), indent=1)
    return 1 if res["different"] else 0


if __name__ == "__main__":
    sys.exit(main())
