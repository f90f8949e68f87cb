#!/usr/bin/env python3
"""Do two source trees compile to the same kernels?  CPU only (hipcc cross-compiles).

    python tools/codeobj_diff.py PARENT_TREE NEW_TREE [-j JOBS] [--keep DIR]

Every *.hip of sperr_amd/csrc in both trees is compiled to ISA text with that tree's Makefile FLAGS plus
--cuda-device-only -S.  Printed: a file-by-file table, then, kernel by kernel, every kernel of the parent's files that
are not the same file in the new tree -- where it went, instructions, VGPRs, SGPRs, LDS, scratch, spills, and
"identical" or the first line that differs.  A kernel's text runs from its .globl line to the end of its "Kernel info"
comments and is compared together with its entry of amdhsa.kernels, after the __hip_cuid_* symbol, the block labels,
.Lfunc_end and the other local labels (numbered per file) and the trailing comments have been normalised.

Exit status: 0 when every kernel of the parent is in the new tree exactly once and identical, 1 otherwise."""
import argparse
import concurrent.futures
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

CSRC = os.path.join("sperr_amd", "csrc")
PRINT_VAR = "print-%: ; @echo $($*)"


def make_var(tree, var):
    out = subprocess.run(["make", "-s", "--no-print-directory", "-C", os.path.join(tree, CSRC), "--eval", PRINT_VAR, "print-" + var],
                         capture_output=True, text=True, check=True).stdout
    return out.split()


def compile_tree(tree, outdir, jobs):
    """{unit.hip: path of its ISA text}"""
    hipcc = (make_var(tree, "HIPCC") or ["hipcc"])[0]
    flags = make_var(tree, "FLAGS")
    srcs = sorted(glob.glob(os.path.join(tree, CSRC, "*.hip")))
    os.makedirs(outdir, exist_ok=True)

    def one(src):
        dst = os.path.join(outdir, os.path.basename(src)[:-4] + ".s")
        r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", src, "-o", dst], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("%s does not compile:\n%s" % (src, r.stderr[-3000:]))
        return os.path.basename(src), dst

    with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as pool:
        return dict(pool.map(one, srcs)), flags


LOCAL = re.compile(r"\.L([A-Za-z_]+?)(\d+)\b")


def normalise(lines):
    """the lines of one kernel (or one file) with everything that only numbers things within the file taken out"""
    seen = {}
    out = []

    def local(m):
        kind = m.group(1)
        if kind == "func_end":
            return ".Lfunc_end"
        key = m.group(0)
        if key not in seen:
            seen[key] = ".L%s#%d" % (kind, sum(1 for k in seen.values() if k.startswith(".L%s#" % kind)))
        return seen[key]

    for ln in lines:
        ln = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", ln)
        if not ln.lstrip().startswith(";"):
            ln = re.sub(r"\s*;.*$", "", ln)                 # trailing comment
        ln = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", ln)      # block labels: .LBB<function>_<block>
        ln = re.sub(r"\bBB\d+_(\d+)", r"BB_\1", ln)         # ... and the comments that name them
        ln = LOCAL.sub(local, ln)
        out.append(ln.rstrip())
    return out


def parse(path):
    """file text for the whole-file comparison, and {symbol: kernel record}"""
    lines = open(path).read().split("\n")
    whole = normalise([ln for ln in lines if not re.match(r"\s*\.(file|ident)\b", ln)])
    # amdhsa.kernels entries
    entries = {}
    try:
        i = next(k for k, ln in enumerate(lines) if ln.strip() == "amdhsa.kernels:") + 1
    except StopIteration:
        i = len(lines)
    if i < len(lines) and re.match(r"^(\s*)- ", lines[i]):
        lead = re.match(r"^(\s*)- ", lines[i]).group(1)
        cur = None
        while i < len(lines) and (lines[i].startswith(lead + "- ") or lines[i].startswith(lead + "  ")):
            if lines[i].startswith(lead + "- "):
                cur = []
                entries[len(entries)] = cur
            cur.append(lines[i])
            i += 1
    kernels = {}
    for blk in entries.values():
        text = "\n".join(blk)
        sym = re.search(r"\.name:\s+(\S+)", text).group(1)
        nums = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", text, flags=re.M)}
        kernels[sym] = {"meta": normalise(blk), "nums": nums}
    # the functions
    index = {ln.split()[1]: k for k, ln in enumerate(lines) if ln.lstrip().startswith(".globl") and len(ln.split()) > 1}
    for sym, rec in kernels.items():
        a = index[sym]
        b = a
        while not lines[b].startswith("; Kernel info:"):
            b += 1
        while b < len(lines) and lines[b].startswith(";"):
            b += 1
        body = lines[a:b]
        start = next(k for k, ln in enumerate(body) if ln.startswith(sym + ":"))
        end = next(k for k, ln in enumerate(body) if ln.startswith(".Lfunc_end"))
        rec["ninstr"] = sum(1 for ln in body[start + 1:end]
                            if ln.startswith("\t") and not ln.lstrip().startswith((".", ";")))
        rec["text"] = normalise(body)
    return whole, kernels


def demangle(symbols):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        out = subprocess.run([tool], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        return {s: s for s in symbols}
    names = {}
    for s, d in zip(symbols, out):
        d = re.sub(r"^void ", "", d).replace("sperrhip::", "")
        depth = 0
        for k, ch in enumerate(d):   # cut the parameter list: the first '(' outside <...>
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0 and not d.startswith("(anonymous", k):
                d = d[:k]
                break
        names[s] = d
    return names


def first_difference(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return "line %d: %r | %r" % (k + 1, x.strip()[:60], y.strip()[:60])
    return "length: %d | %d lines" % (len(a), len(b))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("-j", "--jobs", type=int, default=8)
    ap.add_argument("--keep", help="keep the ISA text under this directory")
    args = ap.parse_args()
    jobs = max(1, min(16, args.jobs))
    work = args.keep or tempfile.mkdtemp(prefix="codeobj_diff_")
    try:
        sides = []
        for tag, tree in (("parent", args.parent), ("new", args.new)):
            files, flags = compile_tree(os.path.abspath(tree), os.path.join(work, tag), jobs)
            sides.append(({unit: parse(p) for unit, p in files.items()}, flags))
    finally:
        if not args.keep:
            shutil.rmtree(work, ignore_errors=True)
    (old, old_flags), (new, new_flags) = sides
    print("flags: " + " ".join(new_flags) + " --cuda-device-only -S"
          + ("" if old_flags == new_flags else "   (parent: " + " ".join(old_flags) + ")"))

    print("\nfile by file (identical: but for the __hip_cuid_* symbol and the .file line)")
    width = max(len(u) for u in list(old) + list(new)) + 2
    changed = []
    for unit in list(old) + [u for u in new if u not in old]:
        if unit in old and unit in new:
            same = old[unit][0] == new[unit][0]
            if same:
                print("  %-*s identical  %3d kernels  %7d lines" % (width, unit, len(new[unit][1]), len(new[unit][0])))
            else:
                changed.append(unit)
                print("  %-*s differs    %3d kernels -> %d" % (width, unit, len(old[unit][1]), len(new[unit][1])))
        elif unit in old:
            changed.append(unit)
            print("  %-*s gone       %3d kernels" % (width, unit, len(old[unit][1])))
        else:
            print("  %-*s new        %3d kernels" % (width, unit, len(new[unit][1])))

    where = {}
    for unit, (_, ks) in new.items():
        for sym in ks:
            where.setdefault(sym, []).append(unit)
    wanted = {sym: unit for unit in changed for sym in old[unit][1]}
    targets = [u for u in new if u not in old or u in changed]
    got = {sym for u in targets for sym in new[u][1]}
    missing = sorted(s for s in wanted if s not in where)
    doubled = sorted(s for s in wanted if len(where.get(s, [])) > 1)
    extra = sorted(got - set(wanted))
    names = demangle(sorted(set(wanted) | got))
    print("\nparent %s: %d kernels; new %s: %d kernels, %d of them in more than one unit"
          % (", ".join(changed) or "-", len(wanted), ", ".join(targets) or "-", len(got), len(doubled)))
    print("missing from the new units: " + (", ".join(names[s] for s in missing) or "none"))
    print("not in the parent: " + (", ".join(names[s] for s in extra) or "none"))
    print("\n  %-46s %-22s %-14s %5s %5s %8s %8s %10s" % ("kernel", "unit", "instructions", "VGPRs", "SGPRs", "LDS (B)", "scratch", "spills v/s"))
    differ = 0
    for sym in sorted(wanted, key=lambda s: names[s]):
        if sym not in where:
            continue
        a = old[wanted[sym]][1][sym]
        for unit in where[sym]:
            b = new[unit][1][sym]
            if a["text"] == b["text"] and a["meta"] == b["meta"]:
                verdict = "identical"
            else:
                differ += 1
                verdict = "DIFFERS, " + (first_difference(a["text"], b["text"]) if a["text"] != b["text"]
                                         else "amdhsa.kernels " + first_difference(a["meta"], b["meta"]))
            n = b["nums"]
            print("  %-46s %-22s %6d = %-6d %5d %5d %8d %8d %6d/%-3d  %s"
                  % (names[sym], unit, a["ninstr"], b["ninstr"], n.get("vgpr_count", 0), n.get("sgpr_count", 0),
                     n.get("group_segment_fixed_size", 0), n.get("private_segment_fixed_size", 0),
                     n.get("vgpr_spill_count", 0), n.get("sgpr_spill_count", 0), verdict))
    print("\n%d kernels differ" % differ)
    return 1 if (missing or doubled or differ) else 0


if __name__ == "__main__":
    sys.exit(main())
