#!/usr/bin/env python3
"""Device code of every kernel translation unit, one source tree against another: normalised gfx950 assembly, line count and SHA-256.

usage: python scripts/isa_identity.py PARENT [CHANGE] [--jobs N] [--keep DIR]

PARENT and CHANGE are checkouts of this repository (CHANGE defaults to the tree this script is in); a PARENT that is no directory
is taken as a git revision of this repository and exported to a temporary directory.  Every source of build.py::SOURCES except
cmps_capi.hip (host code only) is compiled device-only with build.py's flags, its EXTRA_FLAGS included, and the two sources with
diagnostic blocks once more under their diagnostic flag sets.  The only normalisation is the __hip_cuid_<hash> symbol, which is
a hash of the source path.  Whole files are hashed and compared; a refactor that moves force-inlined device code, or rewrites host
code only, expects every row "identical".  Needs hipcc, no GPU.  --keep DIR leaves the .s files in DIR/parent and DIR/change."""
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
    return text.count("\n"), hashlib.sha256(text.encode()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("change", nargs="?", default=ROOT)
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 2))
    ap.add_argument("--keep")
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
        same += p == c
        print(f"{lab:28s} {p[0]:8d} {c[0]:8d}  {p[1]}  {c[1]}  {'identical' if p == c else 'DIFFERENT'}")
    print(f"\n{same} of {len(todo)} identical ({len(todo) - len(DIAG)} translation units, {len(DIAG)} diagnostic flag sets)")
    return 0 if same == len(todo) else 1


if __name__ == "__main__":
    sys.exit(main())
