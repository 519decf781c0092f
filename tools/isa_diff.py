"""Is the DEVICE code of two source trees the same?  No GPU needed.

    python tools/isa_diff.py PARENT_TREE THIS_TREE [--jobs 8] [--out profiles/NAME.md]

(e.g. PARENT_TREE = a `git worktree add` of the parent commit.)  Every csrc/*.hip of both trees is compiled with its tree's Makefile
CXXFLAGS plus `--cuda-device-only -S`; each .s is split by symbol and compared per symbol: the instruction text of every function, the
kernel descriptor block of every kernel (registers, LDS, scratch, kernarg size), the set of symbols, and what is left of the file
(constants, metadata) as an unordered set of lines.  Ignored: comments, the per-compile `__hip_cuid_*` lines (the only thing that differs
between two compiles of one source), the order of the functions in the file and the numbering of local labels, which follows it.
Exit status 0: identical."""
import argparse
import concurrent.futures as cf
import glob
import os
import re
import subprocess
import sys
import tempfile

PKG = "geometric_aware_dense_matching_amd"


def cxxflags(csrc):
    mk = open(os.path.join(csrc, "Makefile")).read()
    var = {k: v.strip() for k, v in re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", mk, re.M)}
    flags = re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], var["CXXFLAGS"])
    return os.environ.get("HIPCC", var["HIPCC"]), flags.split()


def compile_s(job):
    hipcc, flags, src, dst = job
    subprocess.check_call([hipcc] + flags + ["--cuda-device-only", "-S", os.path.basename(src), "-o", dst], cwd=os.path.dirname(src))
    return dst


LABEL = re.compile(r"\.L(BB|func_end|func_begin)\d+")            # these carry the function's index in the file
COUNTED = re.compile(r"\.L([A-Za-z_]+?)(\d+)\b")                   # other local labels are counted through the file (.Lpost_getpc12)


def renumber(lines):
    """file-wide label counters -> order of first appearance inside the function"""
    seen = {}
    return [COUNTED.sub(lambda m: ".L%s#%d" % (m.group(1), seen.setdefault(m.group(0), len(seen))), l) for l in lines]


def split(path):
    """-> {symbol: [instruction lines]}, {kernel: [descriptor lines]}, sorted rest"""
    funcs, descs, rest = {}, {}, []
    cur = None                                                     # the list lines go to
    pending = None                                                 # symbol named by the last `.type X,@function`
    for raw in open(path):
        line = LABEL.sub(lambda m: ".L" + m.group(1), raw.split(";")[0].rstrip()).strip()
        if not line or "__hip_cuid_" in line:
            continue
        m = re.match(r"\.type\s+(\S+),@function", line)
        if m:
            pending = m.group(1)
            continue
        if pending and line == pending + ":":
            cur = funcs.setdefault(pending, [])
            pending = None
            continue
        if cur is not None and line == ".Lfunc_end:":
            cur = None
            continue
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = descs.setdefault(m.group(1), [])
            continue
        if line == ".end_amdhsa_kernel":
            cur = None
            continue
        (rest if cur is None else cur).append(line)
    return {k: renumber(v) for k, v in funcs.items()}, descs, sorted(rest)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out")
    ap.add_argument("--only", help="comma-separated translation units (gdm_conv,gdm_image) instead of all")
    a = ap.parse_args()
    jobs, names = [], None
    tmp = tempfile.mkdtemp(prefix="isa_diff_")
    for side, tree in (("a", a.parent), ("b", a.this)):
        csrc = os.path.join(tree, PKG, "csrc")
        hipcc, flags = cxxflags(csrc)
        srcs = sorted(s for s in glob.glob(os.path.join(csrc, "*.hip")) if not a.only or os.path.basename(s)[:-4] in a.only.split(","))
        tu = [os.path.basename(s)[:-4] for s in srcs]
        if names is not None and tu != names:
            sys.exit("the trees hold different translation units: %s" % sorted(set(tu) ^ set(names)))
        names = tu
        jobs += [(hipcc, flags, s, os.path.join(tmp, "%s_%s.s" % (side, t))) for s, t in zip(srcs, tu)]
    jobs.sort(key=lambda j: -os.path.getsize(j[2]))                # the long compiles first
    with cf.ThreadPoolExecutor(max(1, min(a.jobs, 16))) as ex:
        list(ex.map(compile_s, jobs))
    lines = ["| translation unit | functions | kernels | instruction lines | differing symbols |", "|---|---|---|---|---|"]
    bad = 0
    for t in names:
        fa, da, ra = split(os.path.join(tmp, "a_%s.s" % t))
        fb, db, rb = split(os.path.join(tmp, "b_%s.s" % t))
        diff = ["only in parent: " + s for s in sorted(set(fa) - set(fb))] + ["only here: " + s for s in sorted(set(fb) - set(fa))]
        diff += ["code: " + s for s in sorted(set(fa) & set(fb)) if fa[s] != fb[s]]
        diff += ["descriptor: " + s for s in sorted(set(da) | set(db)) if da.get(s) != db.get(s)]
        if ra != rb:
            diff.append("data / metadata outside the functions")
        bad += len(diff)
        lines.append("| %s | %d | %d | %d | %s |" % (t, len(fb), len(db), sum(len(v) for v in fb.values()), "<br>".join(diff) if diff else "none"))
    lines.append("")
    lines.append("%d translation units; %s" % (len(names), "device code identical" if not bad else "%d DIFFERENCES" % bad))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        open(a.out, "w").write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
