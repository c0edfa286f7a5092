#!/usr/bin/env python
"""Device code of csrc/*.hip at a git revision against the working tree, kernel by kernel.

    python tools/isa_compare.py <git-rev> file.hip [...] [--defines D ...] [--tree DIR] [--diff] [--jobs N]

The revision's univs_amd/csrc and include are written to a temporary directory (git archive); both trees are compiled with the flags
of univs_amd/build.py plus `-S --cuda-device-only -Rpass-analysis=kernel-resource-usage`.  One line per kernel: instructions and
labels of the body, the first 12 hex digits of the SHA-1 of the normalised body at the revision and here (comments, directives and the
__hip_cuid symbol dropped, mangled names replaced by one token), identical / N lines differing, and the resource remarks (VGPR, AGPR,
SGPR, scratch bytes per lane, waves per SIMD, static LDS bytes), same / changed.  Exit status 1 if any kernel differs in either.
--tree: a directory with univs_amd/csrc and include to take for "this" instead of the working tree; --diff: the differing lines.
It compares listings; it searches them for nothing.  No GPU is needed.
"""
import argparse
import difflib
import hashlib
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from univs_amd import build as ubuild  # noqa: E402

RES_KEYS = (("VGPRs", "VGPR"), ("AGPRs", "AGPR"), ("TotalSGPRs", "SGPR"), ("ScratchSize [bytes/lane]", "scratch"),
            ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "LDS"))


def flags_for(tree, defines):
    """build._flags() with the include directory of `tree` (a checkout root) in place of this tree's."""
    out, skip = [], False
    for f in ubuild._flags(defines):
        if skip:
            skip = False
            continue
        if f == "-I":
            skip = True
            continue
        out.append(f)
    return out + ["-I", os.path.join(tree, "include")]


def compile_listing(tree, name, defines, outdir):
    """-> (assembly text, remark text) of univs_amd/csrc/<name> in `tree`."""
    src = os.path.join(tree, "univs_amd", "csrc", name)
    asm = os.path.join(outdir, name + ".s")
    cmd = [ubuild._hipcc(), *flags_for(tree, defines), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", src, "-o", asm]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}\n{p.stderr[-4000:]}")
    with open(asm) as f:
        return f.read(), p.stderr


def kernel_bodies(asm):
    """{mangled kernel name: normalised body lines}, in file order."""
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    lines = asm.split("\n")
    start = {}
    for i, ln in enumerate(lines):
        m = re.match(r"([A-Za-z_$][\w$.]*):", ln)                 # `name:   ; @name`
        if m:
            start[m.group(1)] = i
    out = {}
    for k in kernels:
        body = []
        for ln in lines[start[k] + 1:]:
            if ln.startswith(".Lfunc_end"):
                break
            ln = ln.split(";", 1)[0].strip()
            if not ln or (ln.startswith(".") and not ln.endswith(":")):
                continue                                          # comment or directive (labels stay)
            ln = re.sub(r"__hip_cuid_\w+", "", ln)
            ln = re.sub(r"\b_Z\w+", "SYM", ln)
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
            body.append(re.sub(r"\s+", " ", ln))
        out[k] = body
    return out


def kernel_resources(remarks):
    """{mangled kernel name: {column: value}} from the kernel-resource-usage remarks."""
    out, cur = {}, None
    for ln in remarks.split("\n"):
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for key, col in RES_KEYS:
            m = re.search(r"remark:\s+" + re.escape(key) + r": (\S+)", ln)
            if m:
                cur[col] = m.group(1)
    return out


def demangle(names):
    try:                                                          # (without c++filt the table shows the mangled names)
        p = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True)
        full = p.stdout.split("\n")[:len(names)]
    except (OSError, subprocess.CalledProcessError):
        return list(names)
    short = []
    for s in full:
        s = re.sub(r"^void ", "", s).replace("univs::", "")
        depth, cut = 0, len(s)
        for i, ch in enumerate(s):                                # drop the parameter list: the first '(' outside template brackets
            if ch == "<":
                depth += 1
            elif ch == ">":
                depth -= 1
            elif ch == "(" and depth == 0:
                cut = i
                break
        short.append(s[:cut].replace(", ", ",").replace("true", "1").replace("false", "0"))
    return short


def lines_differing(a, b):
    sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
    return sum(max(i2 - i1, j2 - j1) for op, i1, i2, j1, j2 in sm.get_opcodes() if op != "equal")


def sha(body):
    return hashlib.sha1("\n".join(body).encode()).hexdigest()[:12]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev")
    ap.add_argument("files", nargs="+", help="names under univs_amd/csrc")
    ap.add_argument("--defines", nargs="*", default=[], help="as build.py's instrumented builds, e.g. UNIVS_TRACE_MLP ML_PS_ABL=1")
    ap.add_argument("--tree", default=ROOT, help="root of the tree compared with the revision (default: the working tree)")
    ap.add_argument("--diff", action="store_true", help="print the unified diff of every differing kernel's normalised body")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 2))
    args = ap.parse_args(argv)
    files = [os.path.basename(f) for f in args.files]

    with tempfile.TemporaryDirectory(prefix="isa_compare_") as tmp:
        parent = os.path.join(tmp, "parent")
        os.makedirs(parent)
        tar = os.path.join(tmp, "parent.tar")
        subprocess.run(["git", "-C", ROOT, "archive", "-o", tar, args.rev, "univs_amd/csrc", "include"], check=True)
        with tarfile.open(tar) as t:
            t.extractall(parent)
        jobs = [(tree, tag, f) for f in files for tree, tag in ((parent, "parent"), (os.path.abspath(args.tree), "this"))]
        for _, tag, _ in jobs:
            os.makedirs(os.path.join(tmp, "s_" + tag), exist_ok=True)
        with ThreadPoolExecutor(max_workers=max(1, args.jobs)) as ex:
            done = list(ex.map(lambda j: compile_listing(j[0], j[2], args.defines, os.path.join(tmp, "s_" + j[1])), jobs))
    listing = {(tag, f): r for (_, tag, f), r in zip(jobs, done)}

    ver = subprocess.run([ubuild._hipcc(), "--version"], stdout=subprocess.PIPE, text=True).stdout.split("\n")
    print("# " + " ".join(["python", "tools/isa_compare.py", *(argv if argv is not None else sys.argv[1:])]))
    print("# " + "; ".join(v.strip() for v in ver[:2] if v.strip()))
    print("# " + " ".join(["hipcc", *[f for f in flags_for("<tree>", args.defines)], "-S", "--cuda-device-only",
                            "-Rpass-analysis=kernel-resource-usage"]))
    cols = [c for _, c in RES_KEYS]
    fw = max(len(f) for f in files)
    rows, bad, diffs = [], 0, []
    for f in files:
        pb, tb = kernel_bodies(listing[("parent", f)][0]), kernel_bodies(listing[("this", f)][0])
        pr, tr = kernel_resources(listing[("parent", f)][1]), kernel_resources(listing[("this", f)][1])
        names = list(tb) + [k for k in pb if k not in tb]
        for k, short in zip(names, demangle(names)):
            if k not in pb or k not in tb:
                rows.append((f, short, len(tb.get(k, pb.get(k))), sha(pb[k]) if k in pb else "-" * 12, sha(tb[k]) if k in tb else "-" * 12,
                             "only here" if k in tb else "only parent", tr.get(k, pr.get(k, {})), "changed"))
                bad += 1
                continue
            same = pb[k] == tb[k]
            stream = "identical" if same else f"{lines_differing(pb[k], tb[k])} lines differing"
            res_same = pr.get(k) == tr.get(k)
            res = dict(tr.get(k, {}))
            if not res_same:
                res = {c: (res.get(c, "?") if pr.get(k, {}).get(c) == res.get(c) else f"{pr.get(k, {}).get(c, '?')}>{res.get(c, '?')}") for c in cols}
            rows.append((f, short, len(tb[k]), sha(pb[k]), sha(tb[k]), stream, res, "same" if res_same else "changed"))
            bad += 0 if (same and res_same) else 1
            if args.diff and not same:
                diffs.append("\n".join(difflib.unified_diff(pb[k], tb[k], f"{args.rev}: {short}", f"this: {short}", n=2, lineterm="")))
    kw = max([len(r[1]) for r in rows] + [6])
    print(f"  {'file':<{fw}}  {'kernel':<{kw}} {'instr':>6} {'sha1 parent':<12} {'sha1 this':<12}  {'stream':<20} " +
          " ".join(f"{c:>7}" for c in cols) + "  resources")
    for f, short, n, sp, st, stream, res, rs in rows:
        print(f"  {f:<{fw}}  {short:<{kw}} {n:>6} {sp:<12} {st:<12}  {stream:<20} " + " ".join(f"{res.get(c, '?'):>7}" for c in cols) + f"  {rs}")
    print(f"# {len(rows)} kernels, {bad} differing")
    for d in diffs:
        print(d)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
