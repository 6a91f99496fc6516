#!/usr/bin/env python3
"""Device code of every kernel translation unit, one source tree against another: normalised gfx950 assembly, line count and SHA-256.

usage: python scripts/isa_identity.py PARENT [CHANGE] [--jobs N] [--keep DIR] [--kernels REGEX]

PARENT and CHANGE are checkouts of this repository (CHANGE defaults to the tree this script is in); a PARENT that is no directory
is taken as a git revision of this repository and exported to a temporary directory.  Every source of build.py::SOURCES except
cmps_capi.hip (host code only) is compiled device-only with build.py's flags, its EXTRA_FLAGS included, and the two sources with
diagnostic blocks once more under their diagnostic flag sets.  The only normalisation is the __hip_cuid_<hash> symbol, which is
a hash of the source path.  Whole files are hashed and compared; a refactor that moves force-inlined device code, or rewrites host
code only, expects every row "identical".  Needs hipcc, no GPU.  --keep DIR leaves the .s files in DIR/parent and DIR/change.
--kernels REGEX adds one row per kernel whose (mangled) symbol matches, in the translation units that differ: the kernel's body
(its label to its end label) and its .amdhsa_kernel descriptor block, compared as text with the kernel's own symbol and the
function index of its labels normalised -- for a change that adds kernels or instances to a file and must leave the existing ones
alone.  Kernels are paired by demangled name, trailing template arguments `false` dropped.  "same instructions": only directives
differ (the kernel-argument segment grew, the kernel moved to a template instance's section) and, where the segment grew by g bytes,
scalar loads of hidden kernel arguments that moved g bytes with it; each such line is printed."""
import argparse
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("cmps_build", os.path.join(ROOT, "audio_mps_amd", "build.py"))
B = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(B)

# diagnostic flag sets (compile only): the timing blocks of the two sources that have them
DIAG = {"cmps_pair.hip": ["-DCMPS_DIAG", "-DPABL_TIMING", "-DC16_TIMING"], "cmps_wave16.hip": ["-DCMPS_DIAG", "-DW16_TIMING"]}


def jobs_of():
    out = []
    for s in sorted(B.SOURCES):
        if s == "cmps_capi.hip":
            continue
        extra = B.EXTRA_FLAGS.get(s, [])
        if s in DIAG:
            out.append((s + " [diag]", s, extra + DIAG[s]))
        out.append((s, s, extra))
    return out


def assemble(tree, src, extra, keep, label):
    """(lines, sha256) of the normalised device assembly of tree's `src`, or an error string"""
    path = os.path.join(tree, "audio_mps_amd", "csrc", src)
    if not os.path.exists(path):
        return "missing"
    cmd = [B._hipcc()] + B._flags() + ["--cuda-device-only", "-S"] + extra + [path, "-o", "-"]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if proc.returncode != 0:
        return "hipcc failed: " + proc.stderr.strip().splitlines()[-1]
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", proc.stdout)
    if keep:
        os.makedirs(keep, exist_ok=True)
        with open(os.path.join(keep, label.replace(" [diag]", ".diag") + ".s"), "w") as f:
            f.write(text)
    return text.count("\n"), hashlib.sha256(text.encode()).hexdigest(), text


def kernel_key(sym):
    """What identifies a kernel across the two trees: its demangled name without return type and arguments, and without TRAILING template
    arguments `false` (a kernel that gained a bool template parameter at the end keeps its key in the instance that passes false)."""
    import shutil
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt:
        raise RuntimeError("--kernels needs c++filt (or llvm-cxxfilt) to pair the kernels of the two trees")
    name = subprocess.run([filt, sym], stdout=subprocess.PIPE, text=True, check=True).stdout.strip()
    name = name.replace("(anonymous namespace)", "{anonymous}")          # (its parenthesis is not the argument list's)
    name = re.sub(r"^void ", "", name.split("(")[0]).replace(" ", "")
    args = [x for x in re.sub(r"^[^<]*<?|>$", "", name).split(",") if x] if "<" in name else []
    while args and args[-1] == "false":
        args.pop()
    return name.split("<")[0] + ("<" + ",".join(args) + ">" if args else "")


def kernels_of(text, pattern):
    """{key: (symbol, body + descriptor block)} of the kernels of an assembly file whose symbol matches `pattern`, the kernel's own
    symbol replaced by a placeholder"""
    out = {}
    for sym in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M):
        if not re.search(pattern, sym):
            continue
        body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(sym), text, flags=re.M | re.S)
        desc = re.search(r"^\s*\.amdhsa_kernel\s+%s\n.*?\.end_amdhsa_kernel" % re.escape(sym), text, flags=re.M | re.S)
        both = (body.group(0) if body else "") + "\n" + (desc.group(0) if desc else "")
        both = re.sub(r"(BB|func_end)\d+", r"\1N", both.replace(sym, "KERNEL"))      # (labels carry the function's index in its file)
        both = re.sub(r"[ \t]+;", " ;", both)                                          # (... and their comments are aligned behind them)
        out[kernel_key(sym)] = (sym, both)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("change", nargs="?", default=ROOT)
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 2))
    ap.add_argument("--keep")
    ap.add_argument("--kernels", help="regular expression on kernel symbols: compare these kernels one by one in the files that differ")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        parent = a.parent
        if not os.path.isdir(parent):
            ar = subprocess.run(["git", "-C", ROOT, "archive", parent, "audio_mps_amd/csrc", "include"], stdout=subprocess.PIPE, check=True)
            subprocess.run(["tar", "-x", "-C", tmp], input=ar.stdout, check=True)
            parent = tmp
        todo = jobs_of()
        with ThreadPoolExecutor(max_workers=a.jobs) as pool:
            fp = [pool.submit(assemble, parent, s, x, a.keep and os.path.join(a.keep, "parent"), lab) for lab, s, x in todo]
            fc = [pool.submit(assemble, a.change, s, x, a.keep and os.path.join(a.keep, "change"), lab) for lab, s, x in todo]
            rp, rc = [f.result() for f in fp], [f.result() for f in fc]
    print(f"{'translation unit':28s} {'lines(P)':>8s} {'lines(C)':>8s}  {'sha256 parent':64s}  {'sha256 change':64s}  verdict")
    same = 0
    for (lab, _, _), p, c in zip(todo, rp, rc):
        if isinstance(p, str) or isinstance(c, str):
            print(f"{lab:28s} parent: {p if isinstance(p, str) else 'ok'}; change: {c if isinstance(c, str) else 'ok'}")
            continue
        same += p[:2] == c[:2]
        print(f"{lab:28s} {p[0]:8d} {c[0]:8d}  {p[1]}  {c[1]}  {'identical' if p[:2] == c[:2] else 'DIFFERENT'}")
    print(f"\n{same} of {len(todo)} identical ({len(todo) - len(DIAG)} translation units, {len(DIAG)} diagnostic flag sets)")
    if a.kernels:
        ksame = ktotal = 0
        print(f"\nkernels matching /{a.kernels}/ in the translation units that differ")
        print(f"{'translation unit':20s} {'lines(P)':>8s} {'lines(C)':>8s}  {'verdict':22s} kernel")
        for (lab, _, _), p, c in zip(todo, rp, rc):
            if isinstance(p, str) or isinstance(c, str) or p[:2] == c[:2]:
                continue
            kp, kc = kernels_of(p[2], a.kernels), kernels_of(c[2], a.kernels)
            for key in sorted(set(kp) | set(kc)):
                tp, tc = kp.get(key, (None, None))[1], kc.get(key, (None, None))[1]
                verdict = "only in change" if tp is None else "only in parent" if tc is None else "identical" if tp == tc else "DIFFERENT"
                extra = []
                if verdict == "DIFFERENT":
                    # every instruction the same and only directives apart (the kernel-argument segment grew, or the kernel became a
                    # template instance and moved to its own section): say so, and which
                    lp, lc = tp.split("\n"), tc.split("\n")
                    if len(lp) == len(lc):
                        extra = [(x.strip(), y.strip()) for x, y in zip(lp, lc) if x != y]
                        directive = r"\.(amdhsa_kernarg_size|text|section)\b"
                        # a kernel-argument segment that grew by g bytes moves the 256 bytes of hidden arguments behind it by g: a scalar
                        # load from the kernarg pointer s[0:1] at an offset inside the parent's hidden block, the same load g bytes further
                        # on in the change, is the same instruction reading the same hidden argument
                        size = [int(m.group(1)) if m else 0 for m in (re.search(r"\.amdhsa_kernarg_size (\d+)", t) for t in (tp, tc))]
                        load = r"(s_load_dword\w* s\S+ s\[0:1\], )(0x[0-9a-f]+)$"

                        def moved(x, y):
                            mx, my = re.match(load, x), re.match(load, y)
                            return bool(mx and my and mx.group(1) == my.group(1) and int(mx.group(2), 16) >= size[0] - 256
                                        and int(my.group(2), 16) - int(mx.group(2), 16) == size[1] - size[0] != 0)
                        if all((re.match(directive, x) and re.match(directive, y)) or moved(x, y) for x, y in extra):
                            verdict = "same instructions"
                ktotal += tp is not None
                ksame += verdict in ("identical", "same instructions")
                print(f"{lab:20s} {tp.count(chr(10)) if tp else 0:8d} {tc.count(chr(10)) if tc else 0:8d}  {verdict:22s} {key}")
                for x, y in sorted(set(extra)) if verdict == "same instructions" else []:
                    print(f"{'':40s}    {'directive' if x.startswith('.') else 'hidden argument'}: {x}  ->  {y}")
        print(f"\n{ksame} of {ktotal} kernels of the parent with identical instructions")
        return 0 if ksame == ktotal else 1
    return 0 if same == len(todo) else 1


if __name__ == "__main__":
    sys.exit(main())
