"""Instruction counts of the step loops of one k_step_ag instance, without a GPU: cross-compiles
csrc/fjsp_hip.hip as scripts/isa_counts.py does and prints, for every innermost loop that holds the
per-step workgroup barrier, its instructions in all and by class: v_*, s_*, ds_*, ds_bpermute /
ds_permute, global_*, ds_or_rtn.  K's step loop is the one with ds_or_rtn (the order words' atomic
OR); the loops come in the order of the roles' branches in the kernel.  A role whose step loop
holds inner loops shows as the innermost one around its barrier, so the table tells which loops a
change touched, not every role's full step.

usage: python scripts/isa_loops.py [EPW]      (16, 32 or 64; default 16)
"""
import importlib
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
isa = importlib.import_module("scripts.isa_counts")

LABEL = re.compile(r"^(\.L\S+):")
BRANCH = re.compile(r"^s_c?branch\w*\s+(\S+)")


def loops(lines, epw):
    body, on = [], False
    for l in lines:
        if re.match(r"^_Z\S*k_step_agILi%dELb0E\S*:" % epw, l):
            on = True
            continue
        if on and l.startswith(".Lfunc_end"):
            break
        if on:
            body.append(l.strip())
    labels = {m.group(1): i for i, l in enumerate(body) for m in [LABEL.match(l)] if m}
    ins = [(i, l) for i, l in enumerate(body) if l and not l.startswith((".", ";", "//"))]
    back = []
    for i, l in ins:
        m = BRANCH.match(l)
        if m and labels.get(m.group(1), i) < i:
            back.append((labels[m.group(1)], i))
    rows, seen = [], set()
    for b in (i for i, l in ins if l.startswith("s_barrier")):
        holding = [lp for lp in back if lp[0] < b < lp[1]]
        if not holding:
            continue
        lp = min(holding, key=lambda x: x[1] - x[0])
        if lp in seen:
            continue
        seen.add(lp)
        code = [l for i, l in ins if lp[0] <= i <= lp[1]]
        n = lambda p: sum(1 for l in code if l.startswith(p))   # noqa: E731
        rows.append((len(code), n("v_"), n("s_"), n("ds_"), n("ds_bpermute") + n("ds_permute"), n("global_"), n("ds_or_rtn")))
    return rows


if __name__ == "__main__":
    epw = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    print("| loop | instructions | v_ | s_ | ds_ | ds_(b)permute | global_ | ds_or_rtn |")
    print("|---|---|---|---|---|---|---|---|")
    for k, r in enumerate(loops(isa.assemble([]), epw)):
        print("| %d | %s |" % (k, " | ".join(str(x) for x in r)))
