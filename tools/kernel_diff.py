"""Per-kernel comparison of the gfx950 machine code of two builds (a refactor and its parent).  Needs no GPU.

  python tools/kernel_diff.py TREE_A TREE_B fh_sparse.hip [fh_bcocg.hip ...] [--map REGEX=REPL] [--all] [--keep DIR]
  python tools/kernel_diff.py A.s B.s [--map REGEX=REPL] [--all]

A tree is a checkout of this repository (or its csrc directory).  Each named .hip of each tree is compiled with the CXXFLAGS of
that tree's Makefile plus `--cuda-device-only -S`, and the assembly is split at the kernel symbols.  Per kernel: the resource
lines (SGPR, VGPR, AGPR, scratch bytes per lane, occupancy in waves per SIMD, LDS bytes per workgroup), the instruction count,
and whether the body is the same text once comments, the kernel's own name and the function number inside local labels are
taken out.  Kernels are matched by demangled name (--map rewrites the names of side A first, for a kernel whose template
parameters changed); kernels of one side only are listed.  Without --all only the kernels that differ are printed.  Exit
status 1 when a kernel differs in resources or body or exists on one side only."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

RES = (("TotalNumSgprs", "S"), ("NumVgprs", "V"), ("NumAgprs", "A"), ("ScratchSize", "scr"), ("Occupancy", "occ"), ("LDSByteSize", "LDS"))


def csrc_of(tree):
    sub = os.path.join(tree, "feastkit.jl_amd", "csrc")
    return sub if os.path.isdir(sub) else tree


def compile_s(tree, hip, out):
    """the Makefile's compiler and flags, device side only, to assembly"""
    d = csrc_of(tree)
    text = open(os.path.join(d, "Makefile")).read()
    var = {k: v.strip() for k, v in re.findall(r"^(\w+)\s*\??=\s*(.*)$", text, re.M)}
    flags = re.sub(r"\$\((\w+)\)", lambda m: os.environ.get(m.group(1), var.get(m.group(1), "")), var["CXXFLAGS"])
    cmd = [os.environ.get("HIPCC", var["HIPCC"])] + flags.split() + ["--cuda-device-only", "-S", hip, "-o", out]
    return subprocess.Popen(cmd, cwd=d)


def short_names(mangled):
    out = subprocess.run([shutil.which("llvm-cxxfilt") or shutil.which("c++filt")], input="\n".join(mangled), capture_output=True, text=True, check=True)
    names = []
    for line in out.stdout.splitlines():
        line = re.sub(r"^void ", "", line)
        depth, cut = 0, len(line)
        for i, ch in enumerate(line):               # the argument list: the first '(' outside the template brackets
            depth += (ch == "<") - (ch == ">")
            if ch == "(" and depth == 0:
                cut = i
                break
        line = line[:cut].replace("HIP_vector_type<double, 2u>", "cplx").replace("HIP_vector_type<float, 2u>", "cplxf")
        names.append(line)
    return names


def kernels(path, renames):
    """demangled name -> (resources, instruction count, normalised body)"""
    text = open(path).read()
    syms = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    found = {}
    for sym, name in zip(syms, short_names(syms)):
        for pat, repl in renames:
            name = re.sub(pat, repl, name)
        body = text[text.index("\n%s:" % sym) + len(sym) + 2:]
        body = body[:re.search(r"^\.Lfunc_end\d+:", body, re.M).start()]
        lines = []
        for ln in body.splitlines():
            ln = ln.split(";", 1)[0].strip().replace(sym, "<self>")
            if ln:
                lines.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
        instr = sum(1 for ln in lines if not ln.endswith(":") and not ln.startswith("."))
        info = text[text.index(".amdhsa_kernel %s\n" % sym):]
        info = info[:info.index("; Occupancy") + 40]
        res = tuple(int(re.search(r"; %s: (\d+)" % key, info).group(1)) for key, _ in RES)
        found[name] = (res, instr, "\n".join(lines))
    return found


def compare(path_a, path_b, renames, show_all):
    a, b = kernels(path_a, renames), kernels(path_b, [])
    both = sorted(set(a) & set(b))
    width = max([len(k) for k in both] + [6])
    print("kernels: A %d, B %d, in both %d        (%s)" % (len(a), len(b), len(both), " ".join(s for _, s in RES)))
    print("%-*s  %-24s %-24s %-5s %-11s %s" % (width, "kernel", "A", "B", "equal", "instr", "body"))
    nres = nbody = 0
    for k in both:
        (ra, ia, ta), (rb, ib, tb) = a[k], b[k]
        nres += ra != rb
        nbody += ta != tb
        if show_all or ra != rb or ta != tb:
            print("%-*s  %-24s %-24s %-5s %-11s %s" % (width, k, " ".join(map(str, ra)), " ".join(map(str, rb)), "yes" if ra == rb else "NO",
                                                      str(ia) if ia == ib else "%d -> %d" % (ia, ib), "identical" if ta == tb else "DIFFERS"))
    for side, only in (("A", sorted(set(a) - set(b))), ("B", sorted(set(b) - set(a)))):
        for k in only:
            print("only in %s: %s" % (side, k))
    print("resources differ: %d, bodies differ: %d, on one side only: %d" % (nres, nbody, len(set(a) ^ set(b))))
    return nres or nbody or set(a) != set(b)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("hip", nargs="*", help="the .hip units to compare when A and B are trees")
    ap.add_argument("--map", action="append", default=[], metavar="REGEX=REPL", help="rename kernels of side A before matching")
    ap.add_argument("--all", action="store_true", help="print every kernel, not only those that differ")
    ap.add_argument("--keep", default=None, help="directory that keeps the .s files (default: a temporary one)")
    args = ap.parse_args()
    renames = [tuple(m.split("=", 1)) for m in args.map]
    bad = False
    if os.path.isfile(args.a):
        bad = compare(args.a, args.b, renames, args.all)
    else:
        with tempfile.TemporaryDirectory() as tmp:
            keep = args.keep or tmp
            os.makedirs(keep, exist_ok=True)
            for hip in args.hip:
                sa, sb = (os.path.join(os.path.abspath(keep), "%s_%s.s" % (side, hip[:-4])) for side in "AB")
                procs = [compile_s(args.a, hip, sa), compile_s(args.b, hip, sb)]          # both sides at once
                if any([p.wait() for p in procs]):
                    sys.exit("compiling %s failed" % hip)
                print("== %s" % hip)
                bad = compare(sa, sb, renames, args.all) or bad
    sys.exit(1 if bad else 0)
