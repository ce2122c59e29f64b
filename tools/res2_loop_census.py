#!/usr/bin/env python3
"""Instruction census of the solve loop of one k_admm_res2 instantiation, from the ISA (no GPU needed):

    tools/res2_loop_census.py                                  # the headline tile, product build
    tools/res2_loop_census.py --kernel "Res2Cfg<10, 10, 4, 10>, false, false, false"
    tools/res2_loop_census.py --src old/rqp_resident2.hip      # another version of the file
    tools/res2_loop_census.py --asm saved.s                    # an assembly listing made earlier

The file is compiled to assembly with the flags of reluqp-py_amd/csrc/Makefile (plus --cuda-device-only -S).  The solve loop is
the depth-1 loop of the kernel with the most packed FMAs.  The ORDINARY iteration is cut into the segments its barriers delimit:

    head      loop header .. B3            (loop control)
    A'nu+Hx   B3 .. B1
    Kd+x+Adx  B1 .. B2
    rows      B2 .. the first jump to the loop latch (the row pass of an iteration without a check; the check lies behind it)
    latch     the latch block (counter, exit test, backward branch)

and every instruction is counted once, in the class its mnemonic prefix puts it in.  The counts are per wave and static: lane
predication (s_cbranch_execz skips) is not followed, every instruction between the two ends of a segment counts.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("packed FMA", "other float VALU", "integer VALU", "DPP + lane swap", "LDS read", "LDS write", "wait", "s_nop",
           "scalar", "memory")
VALU = CLASSES[:4]


def classify(mn, ops):
    if mn.startswith("v_"):
        if mn.startswith("v_permlane") or mn.endswith("_dpp") or "quad_perm" in ops or "row_" in ops:
            return "DPP + lane swap"
        if mn.startswith("v_pk_fma_f32"):
            return "packed FMA"
        if re.search(r"_f(16|32|64)", mn) or mn.startswith("v_fma_mix"):
            return "other float VALU"
        return "integer VALU"
    if mn.startswith("ds_read") or mn.startswith("ds_load"):
        return "LDS read"
    if mn.startswith("ds_"):
        return "LDS write"
    if mn.startswith("s_waitcnt"):
        return "wait"
    if mn.startswith("s_nop"):
        return "s_nop"
    if mn.startswith("s_"):
        return "scalar"
    return "memory"                                  # global_ / scratch_ / flat_ / buffer_


def compile_asm(src):
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "reluqp-py_amd", "csrc"),
           "--cuda-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, check=True)
    with open(out) as f:
        text = f.read().splitlines()
    os.unlink(out)
    return text


def kernel_body(lines, want):
    """Lines of the function whose demangled name contains `want`."""
    heads = [(i, l.split(":")[0]) for i, l in enumerate(lines) if l.startswith("_Z") and ":" in l and "k_admm_res2" in l]
    names = subprocess.run(["c++filt"] + [h for _, h in heads], check=True, capture_output=True, text=True).stdout.splitlines()
    for (i, _), d in zip(heads, names):
        if want in d:
            j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
            return d.split("(SolveArgs")[0], lines[i + 1:j]
    sys.exit("no k_admm_res2 instantiation matches %r; there are:\n  %s" % (want, "\n  ".join(n.split("(SolveArgs")[0] for n in names)))


def parse(body):
    """[(label or None, mnemonic, operands)] -- labels as entries of their own, directives and comments dropped."""
    out = []
    for l in body:
        l = l.split(";")[0].rstrip()
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            out.append((m.group(1), None, None))
            continue
        l = l.strip()
        if not l or l.startswith(".") or l.endswith(":"):
            continue
        p = l.split(None, 1)
        out.append((None, p[0], p[1] if len(p) > 1 else ""))
    return out


def solve_loop(body, ins):
    """(index of the header label, index of the backward branch) of the depth-1 loop with the most packed FMAs."""
    headers = []
    for l in body:
        m = re.match(r"^(\.LBB\d+_\d+):.*Loop Header: Depth=1", l)
        if m:
            headers.append(m.group(1))
    pos = {e[0]: i for i, e in enumerate(ins) if e[0]}
    best = None
    for h in headers:
        back = [i for i, e in enumerate(ins) if e[1] and e[1].startswith("s_cbranch") or e[1] == "s_branch"]
        back = [i for i in back if ins[i][2].strip() == h and i > pos[h]]
        if not back:
            continue
        end = max(back)
        n = sum(1 for e in ins[pos[h]:end] if e[1] and e[1].startswith("v_pk_fma_f32"))
        if best is None or n > best[0]:
            best = (n, pos[h], end)
    if best is None:
        sys.exit("no loop found")
    return best[1], best[2]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--src", default=os.path.join(ROOT, "reluqp-py_amd", "csrc", "rqp_resident2.hip"))
    ap.add_argument("--asm", help="use this assembly listing instead of compiling --src")
    ap.add_argument("--kernel", default="Res2Cfg<10, 13, 4, 13>, false, false, false",
                    help="substring of the demangled instantiation name")
    a = ap.parse_args()
    if a.asm:
        with open(a.asm) as f:
            lines = f.read().splitlines()
    else:
        lines = compile_asm(a.src)
    name, body = kernel_body(lines, a.kernel)
    ins = parse(body)
    h, back = solve_loop(body, ins)
    # the latch block: from the last label in front of the backward branch
    latch = max(i for i in range(h, back) if ins[i][0])
    latch_label = ins[latch][0]
    bars = [i for i in range(h, back) if ins[i][1] == "s_barrier"]
    if len(bars) < 3:
        sys.exit("fewer than three barriers in the loop")
    rows_end = next((i for i in range(bars[2], back) if ins[i][1] and ins[i][1].startswith(("s_cbranch", "s_branch"))
                     and ins[i][2].strip() == latch_label), bars[3] if len(bars) > 3 else latch)
    segs = (("head", h, bars[0] + 1), ("A'nu+Hx", bars[0] + 1, bars[1] + 1), ("Kd+x+Adx", bars[1] + 1, bars[2] + 1),
            ("rows", bars[2] + 1, rows_end + 1), ("latch", latch, back + 1))
    counts = {s[0]: dict.fromkeys(CLASSES, 0) for s in segs}
    for sname, lo, hi in segs:
        for lab, mn, ops in ins[lo:hi]:
            if mn:
                counts[sname][classify(mn, ops)] += 1
    print("%s" % name)
    print("solve loop: %d barriers, %d instructions in all (the check included); ordinary iteration below" %
          (len(bars), sum(1 for e in ins[h:back + 1] if e[1])))
    w = max(len(c) for c in CLASSES)
    print("%-*s" % (w, "class") + "".join("%10s" % s[0] for s in segs) + "%10s" % "total")
    for c in CLASSES:
        row = [counts[s[0]][c] for s in segs]
        print("%-*s" % (w, c) + "".join("%10d" % v for v in row) + "%10d" % sum(row))
    vrow = [sum(counts[s[0]][c] for c in VALU) for s in segs]
    print("%-*s" % (w, "all VALU") + "".join("%10d" % v for v in vrow) + "%10d" % sum(vrow))
    arow = [sum(counts[s[0]].values()) for s in segs]
    print("%-*s" % (w, "all") + "".join("%10d" % v for v in arow) + "%10d" % sum(arow))


if __name__ == "__main__":
    main()
