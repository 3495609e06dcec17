#!/usr/bin/env python3
"""Is every kernel of the device library the parent's, instruction for instruction?  For changes that move code between files.

    python tools/kernel_asm_diff.py PARENT_TREE [--out FILE] [--jobs N] [--only NAME.hip ...]

PARENT_TREE is a checkout of the commit to compare with (git worktree add, or git archive REV | tar -x -C DIR).  Every source in
build.DEVICE_SRCS of both trees is compiled to gfx950 assembly with build.DEVICE_FLAGS (minus -shared), in both builtin modes
(plain and -DRT355_REF_BUILTINS); needs hipcc, no GPU.  A kernel is compared by its instructions and its .amdhsa_ descriptor, from
its entry label to .end_amdhsa_kernel, after normalising only what a kernel's position in a file changes: the __hip_cuid_<hash>
symbol and the function index in local labels (.LBB<n>_<m>, .Lfunc_end<n>); comments are dropped.  A kernel must exist exactly once on
each side, or - a library template that several files instantiate, each its own copy - in the same files on both sides, file by file the same.
Prints which file holds each kernel on either side and its -Rpass-analysis=kernel-resource-usage figures; exit status 1 on any
difference.  With --only, both sides compile just the named files (those the parent lacks are skipped there).
"""
import argparse
import concurrent.futures
import os
import re
import runpy
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (("ieee", []), ("refb", ["-DRT355_REF_BUILTINS"]))
FIGURES = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
LABEL = re.compile(r"(\.L[A-Za-z_]+?)\d+(_\d+)\b|(\.Lfunc_(?:begin|end))\d+\b")
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")


def tree_build(root):
    """DEVICE_SRCS and DEVICE_FLAGS of a tree, from its own build.py."""
    g = runpy.run_path(os.path.join(root, "magr_ray_tracer_amd", "build.py"), run_name="build_of_tree")
    return g["HIPCC"], g["DEVICE_SRCS"], [f for f in g["DEVICE_FLAGS"] if f != "-shared"]


def compile_one(hipcc, flags, extra, src, out):
    cmd = [hipcc] + flags + extra + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", out]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    if p.returncode != 0:
        raise RuntimeError("%s\n%s" % (" ".join(cmd), p.stderr[-4000:]))
    with open(out) as f:
        return f.read(), p.stderr


def kernels_of(asm):
    """name -> normalised text from the entry label to .end_amdhsa_kernel (a list: a kernel defined twice shows as two)."""
    lines = asm.split("\n")
    start = {}
    for i, ln in enumerate(lines):
        m = re.match(r"(\w+):\s", ln)
        if m:
            start[m.group(1)] = i
    out = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel (\w+)", ln)
        if not m:
            continue
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        # (without the assembler's comments: their column moves with the width of a label)
        body = "\n".join(c for c in (l.split(";")[0].rstrip() for l in lines[start[m.group(1)]:end + 1]) if c)
        body = CUID.sub("__hip_cuid_#", LABEL.sub(lambda l: (l.group(1) + "#" + l.group(2)) if l.group(1) else l.group(3) + "#", body))
        out.setdefault(m.group(1), []).append(body)
    return out


def figures_of(remarks):
    out, name = {}, None
    for ln in remarks.split("\n"):
        m = re.search(r"remark: Function Name: (\w+)", ln)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass-analysis", ln)
        if m and name:
            out[name][m.group(1)] = m.group(2)
    return out


def side(root, only, tmp, tag, pool):
    hipcc, srcs, flags = tree_build(root)
    if only:
        srcs = [s for s in srcs if os.path.basename(s) in only]
    jobs = {}
    for mode, extra in MODES:
        for s in srcs:
            out = os.path.join(tmp, "%s_%s_%s.s" % (tag, mode, os.path.basename(s)))
            jobs[(mode, os.path.basename(s))] = pool.submit(compile_one, hipcc, flags, extra, s, out)
    return jobs


def collect(jobs):
    res = {m: {} for m, _ in MODES}   # mode -> kernel -> [(file, text, figures)]
    for (mode, f), fut in jobs.items():
        asm, remarks = fut.result()
        figs = figures_of(remarks)
        for k, bodies in kernels_of(asm).items():
            for b in bodies:
                res[mode].setdefault(k, []).append((f, b, figs.get(k, {})))
    return res


def demangle(names):
    try:
        p = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, universal_newlines=True)
        return dict(zip(names, p.stdout.split("\n")))
    except OSError:
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("--out")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--only", nargs="*", default=[])
    a = ap.parse_args()
    rows, bad = [], 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        pj, bj = side(a.parent, a.only, tmp, "parent", pool), side(HERE, a.only, tmp, "branch", pool)
        parent, branch = collect(pj), collect(bj)
    for mode, _ in MODES:
        P, B = parent[mode], branch[mode]
        names = sorted(set(P) | set(B))
        pretty = demangle(names)
        same = 0
        rows.append("== %s: %d kernels in the parent, %d in the branch" % (mode, sum(len(v) for v in P.values()), sum(len(v) for v in B.values())))
        rows.append("%-9s %-16s %-16s %s   | kernel" % ("verdict", "parent file", "branch file", " / ".join(FIGURES)))
        for k in names:
            p, b = P.get(k, []), B.get(k, [])
            if len(p) == 1 and len(b) == 1:   # (wherever it is now)
                verdict = "same" if p[0][1] == b[0][1] else "DIFFERS"
            elif p and sorted(e[0] for e in p) == sorted(e[0] for e in b):   # a library template that several files instantiate, each its own copy
                verdict = "same" if sorted(e[:2] for e in p) == sorted(e[:2] for e in b) else "DIFFERS"
            else:
                verdict = "COUNT %d:%d" % (len(p), len(b))
            same += verdict == "same"
            bad += verdict != "same"
            fig = lambda e: " ".join(e[0][2].get(f, "?") for f in FIGURES) if e else "-"
            rows.append("%-9s %-16s %-16s %s -> %s   | %s" % (verdict, ",".join(e[0] for e in p) or "-", ",".join(e[0] for e in b) or "-", fig(p), fig(b), pretty[k]))
        rows.append("== %s: %d of %d kernels identical" % (mode, same, len(names)))
    text = "\n".join(rows) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
