#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel.  Needs hipcc, no GPU.

  tools/compare_kernel_asm.py emit <csrc dir> <out dir> [-j N]   every translation unit of <csrc dir>/Makefile (SRCS and the part
                                                                 rules) -> <out dir>/<unit>.s (its flags + --cuda-device-only -S)
  tools/compare_kernel_asm.py diff <out dir A> <out dir B>       kernels compared / removed / added / differing

Two kernels are equal when their instruction streams and their .amdhsa_ descriptor (registers, scratch, LDS, ...) are
identical after dropping comments and renumbering the compiler-local labels (.LBB<function>_<block>).  `diff` exits 1 when a
kernel present in both builds differs or when B has a kernel that A has not.
"""
import argparse
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys

MAKEFILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "fsw_gnn_amd", "csrc", "Makefile")


def units_of(makefile_text):
    """[(source without .hip, define or "", unit name)] from the Makefile's text: one unit per file of SRCS, and for every part rule
    `$(OBJDIR)/name_%.o: src.hip ...` with `-DMACRO=$*` in its recipe one unit per `$(OBJDIR)/name_<n>.o` listed in OBJS"""
    text = makefile_text.replace("\\\n", " ")
    var = lambda name: re.search(r"^%s\s*:?=\s*(.*)$" % name, text, re.M).group(1).split()
    units = [(f[:-4], "", f[:-4]) for f in var("SRCS") if f.endswith(".hip")]
    objs = var("OBJS")
    for m in re.finditer(r"^\$\(OBJDIR\)/(\w+)_%\.o:\s*(\w+)\.hip\b.*\n(?:\t.*\n)*?\t.*-D(\w+)=\$\*", text, re.M):
        stem, src, macro = m.groups()
        for o in objs:
            n = re.fullmatch(r"\$\(OBJDIR\)/%s_(\d+)\.o" % re.escape(stem), o)
            if n:
                units.append((src, "-D%s=%s" % (macro, n.group(1)), "%s_%s" % (stem, n.group(1))))
    return units


UNITS = units_of(open(MAKEFILE).read()) if os.path.exists(MAKEFILE) else []
FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function --cuda-device-only -S".split()


def emit(csrc, out, jobs):
    os.makedirs(out, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

    def one(u):
        src, define, name = u
        cmd = [hipcc] + FLAGS + ([define] if define else []) + [src + ".hip", "-o", os.path.join(os.path.abspath(out), name + ".s")]
        return name, subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)

    failed = 0
    units = units_of(open(os.path.join(csrc, "Makefile")).read())
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        for name, r in pool.map(one, units):
            print("%-18s %s" % (name, "ok" if r.returncode == 0 else "FAILED\n" + r.stderr))
            failed += r.returncode != 0
    return 1 if failed else 0


LABEL = re.compile(r"\.L(BB|JTI|tmp|func_begin|func_end)(\d+)(_\d+)?")


def kernels(path):
    """{kernel symbol: (normalised instruction lines, descriptor lines)} of one assembly file"""
    lines = open(path).read().split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m]
    body, desc = {}, {}
    cur = None
    for ln in lines:
        s = ln.split(";", 1)[0].rstrip()
        if not s.strip():
            continue
        m = re.match(r"(\S+):$", s)
        if m and m.group(1) in names and m.group(1) not in body:
            cur = ("body", m.group(1))
            body[cur[1]] = []
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", s)
        if m:
            cur = ("desc", m.group(1))
            desc[cur[1]] = []
            continue
        if cur is None:
            continue
        if re.match(r"\.Lfunc_end\d+:", s) or s.strip() == ".end_amdhsa_kernel":
            cur = None
            continue
        s = LABEL.sub(lambda m: ".L%s%s" % (m.group(1), m.group(3) or ""), " ".join(s.split()))
        (body if cur[0] == "body" else desc)[cur[1]].append(s)
    return {k: (body.get(k, []), desc.get(k, [])) for k in names}


def diff(a, b):
    def load(d):
        out = {}
        for f in sorted(os.listdir(d)):
            if f.endswith(".s"):
                for k, v in kernels(os.path.join(d, f)).items():
                    out[(f, k)] = v
        return out

    ka, kb = load(a), load(b)
    # a kernel may move between translation units: match by symbol when the unit differs
    sym_a = {k[1]: v for k, v in ka.items()}
    sym_b = {k[1]: v for k, v in kb.items()}
    common = sorted(set(sym_a) & set(sym_b))
    removed = sorted(set(sym_a) - set(sym_b))
    added = sorted(set(sym_b) - set(sym_a))
    differing = [k for k in common if sym_a[k] != sym_b[k]]

    def demangle(names):
        if not names or not shutil.which("c++filt"):
            return names
        r = subprocess.run(["c++filt"] + names, capture_output=True, text=True)
        return r.stdout.split("\n")[:len(names)] if r.returncode == 0 else names

    for title, names in (("removed", removed), ("added", added), ("differing", differing)):
        for n in demangle(names):
            print("%-9s %s" % (title, n))
    for k in differing:
        (ia, da), (ib, db) = sym_a[k], sym_b[k]
        print("  %s: %d / %d instructions; descriptor lines differing: %s" % (k, len(ia), len(ib), [x for x in da if x not in db][:6]))
    print("kernels compared %d, removed %d, added %d, differing %d" % (len(common), len(removed), len(added), len(differing)))
    return 1 if differing or added else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    e = sub.add_parser("emit")
    e.add_argument("csrc")
    e.add_argument("out")
    e.add_argument("-j", type=int, default=4)
    d = sub.add_parser("diff")
    d.add_argument("a")
    d.add_argument("b")
    args = ap.parse_args()
    sys.exit(emit(args.csrc, args.out, args.j) if args.cmd == "emit" else diff(args.a, args.b))
