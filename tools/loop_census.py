#!/usr/bin/env python3
"""Loop census of a kernel: what the compiler emits per loop, counted by broad instruction class.

Compiles graphaligner_amd/csrc/ga_device.hip to gfx950 assembly with the product's flags (device side only, in a temporary
directory, no GPU needed) -- or reads an assembly file made that way (--asm) -- and prints, for every kernel whose demangled name
contains --kernel, one row per loop and the kernel's totals.  A loop is what a backward branch closes: the instructions from the
branch's target label to the branch.  Loops nest, so an outer loop's row includes its inner loops.  Instructions are classed by the
prefix of their mnemonic and nothing else:

  valu    vector ALU (v_*, without the two classes below)      lane    lane moves (v_readlane / v_writelane / v_readfirstlane)
  acc     accumulator-register moves (v_accvgpr_*)              salu    scalar ALU (s_*, without the classes below)
  sbr     scalar branches (s_branch, s_cbranch_*)               wait    s_waitcnt*, s_nop, s_sleep, s_barrier
  sld     scalar loads (s_load_*)                               lds     ds_*
  vld/vst vector memory loads / stores and atomics (global_*, flat_*, buffer_*, scratch_*)

The count of a loop is static: a loop without branches inside executes its count per iteration; for a loop with forward branches
inside, --blocks LABEL lists the loop's basic blocks with their counts and where each one branches to, so that an executed path can be
added up by hand.

  python tools/loop_census.py --kernel "ga_lanes_kernel<10, 64>"
  python tools/loop_census.py --asm build/ga_device.s --kernel "ga_lanes_moves_kernel<10, 64>" --blocks .LBB5_210
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "graphaligner_amd", "csrc", "ga_device.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PRODUCT_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-DGA_WAVES_EU=%s" % os.environ.get("GA_WAVES_EU", "6")]
CLASSES = ["valu", "salu", "sbr", "lds", "vld", "vst", "sld", "wait", "lane", "acc", "other"]


def classify(mn):
    if mn.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane"
    if mn.startswith("v_accvgpr"):
        return "acc"
    if mn.startswith("v_"):
        return "valu"
    if mn.startswith(("s_branch", "s_cbranch")):
        return "sbr"
    if mn.startswith(("s_waitcnt", "s_nop", "s_sleep", "s_barrier")):
        return "wait"
    if mn.startswith("s_load"):
        return "sld"
    if mn.startswith("s_"):
        return "salu"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vld" if "_load" in mn else "vst"
    return "other"


def compile_asm(extra, out):
    cmd = [HIPCC] + PRODUCT_FLAGS + extra + ["--cuda-device-only", "-S", SOURCE, "-o", out]
    print("+ " + " ".join(cmd), file=sys.stderr, flush=True)
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def demangle(names):
    if not names:
        return {}
    p = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True)
    out = p.stdout.splitlines()
    return {n: re.sub(r"^void |\(anonymous namespace\)::|\(.*$", "", d) for n, d in zip(names, out)}


def kernels_of(path):
    """{symbol: [(kind, text)]} with kind 'label' or 'ins', for every function of the assembly file"""
    funcs, cur, name = {}, None, None
    sym = re.compile(r"^([A-Za-z_][\w$.]*):")
    for line in open(path, errors="replace"):
        line = line.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        m = sym.match(line)
        if m and not m.group(1).startswith(".L"):
            name, cur = m.group(1), []
            funcs[name] = cur
            continue
        if cur is None:
            continue
        s = line.strip()
        if s.startswith(".Lfunc_end"):
            cur, name = None, None
            continue
        m = re.match(r"^(\.L\w+):", s)
        if m:
            cur.append(("label", m.group(1)))
            continue
        if s.startswith(".") or not line.startswith(("\t", " ")):
            continue
        cur.append(("ins", s))
    return {k: v for k, v in funcs.items() if any(kind == "ins" for kind, _ in v)}


def count(items):
    c = dict.fromkeys(CLASSES, 0)
    for kind, text in items:
        if kind == "ins":
            c[classify(text.split()[0])] += 1
    return c


def loops_of(items):
    """[(label, first, last)]: the spans closed by backward branches, the widest span per target label"""
    at = {text: i for i, (kind, text) in enumerate(items) if kind == "label"}
    spans = {}
    for i, (kind, text) in enumerate(items):
        if kind != "ins":
            continue
        parts = text.split()
        if classify(parts[0]) == "sbr" and len(parts) > 1 and parts[-1] in at and at[parts[-1]] < i:
            spans[parts[-1]] = max(spans.get(parts[-1], 0), i)
    return sorted(((lab, at[lab], last) for lab, last in spans.items()), key=lambda t: t[1])


def row(name, c):
    return "%-28s %6d " % (name, sum(c.values())) + " ".join("%5d" % c[k] for k in CLASSES)


def report(name, items, blocks, out):
    print("kernel %s" % name, file=out)
    print("%-28s %6s " % ("loop (depth, lines of the listing)", "total") + " ".join("%5s" % k for k in CLASSES), file=out)
    loops = loops_of(items)
    for lab, a, b in loops:
        depth = sum(1 for _, x, y in loops if x <= a and b <= y) - 1
        inner = not any(x > a and y <= b for _, x, y in loops)
        print(row("%s%s d%d%s" % ("  " * min(depth, 4), lab, depth, " innermost" if inner else ""), count(items[a:b + 1])), file=out)
    print(row("whole kernel", count(items)), file=out)
    for lab, a, b in loops:
        if lab != blocks:
            continue
        print("blocks of %s: label, instructions, branches" % lab, file=out)
        cur, n, br = lab, 0, []
        for kind, text in items[a:b + 1] + [("label", "(end)")]:
            if kind == "label":
                if n or br:
                    print("  %-14s %4d  %s" % (cur, n, " ".join(br)), file=out)
                cur, n, br = text, 0, []
            else:
                n += 1
                if classify(text.split()[0]) == "sbr":
                    br.append(text.replace("\t", " "))
    return len(loops)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", default="ga_lanes_kernel<10, 64>", help="substring of the demangled kernel name")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--blocks", help="also list the basic blocks of the loop that starts at this label")
    ap.add_argument("-D", dest="defs", action="append", default=[], help="extra -D for the compile")
    a = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as tmp:
        path = a.asm
        if not path:
            path = os.path.join(tmp, "ga_device.s")
            compile_asm(["-D" + d for d in a.defs], path)
        funcs = kernels_of(path)
    names = demangle(list(funcs))
    found = 0
    for sym_, items in funcs.items():
        if a.kernel in names.get(sym_, sym_):
            found += 1
            report(names.get(sym_, sym_), items, a.blocks, sys.stdout)
            print()
    if not found:
        print("no kernel whose name contains %r" % a.kernel, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
