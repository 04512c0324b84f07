#!/usr/bin/env python3
"""Per-kernel comparison of the device assembly of one translation unit between a git revision and the work tree.

  python scripts/kernel_isa_diff.py resample2d.hip --base HEAD [--debug]

Both copies are compiled with build.py's HIP_FLAGS plus `--cuda-device-only -S` (`--debug`: plus -DFN2_DEBUG_BUILD, the
translation unit of libflownet2_hip_debug.so).  The base copy is `git archive`d into a temporary directory; nothing is checked out.
One line per kernel:
  identical    equal text once the lines naming __hip_cuid_ are dropped
  renamed      same sequence of instruction mnemonics, same resource entries in .amdgpu_metadata (registers renamed)
  rescheduled  same multiset of mnemonics, same resource entries, another order
  changed      anything else (also: a kernel only one side has)
Exit status 1 if any kernel is `changed`.  The script compares the two outputs; it knows no instruction by name.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "flownet2-pytorch_amd"
sys.path.insert(0, os.path.join(ROOT, PKG))
from build import HIP_FLAGS, HIPCC  # noqa: E402

RESOURCES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
             ".sgpr_spill_count", ".vgpr_spill_count")


def compile_asm(tree, src, debug, out):
    cmd = [HIPCC] + HIP_FLAGS + (["-DFN2_DEBUG_BUILD"] if debug else []) + \
          ["--cuda-device-only", "-S", os.path.join(tree, PKG, "csrc", src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(" ".join(cmd) + "\n" + r.stdout + r.stderr)
    return open(out).read().splitlines()


def split_kernels(lines):
    """{kernel symbol: (text lines, mnemonics, resource entries)}, in the order of the file."""
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
    start = {ln[:-1].split(":")[0]: i for i, ln in enumerate(lines) if ln and not ln[0].isspace() and ln.split(":")[0] in set(names)}
    meta, cur, inside = {}, None, False
    for ln in lines:
        if ln.strip() == "amdhsa.kernels:":
            inside = True
        elif inside and re.match(r"^\S", ln):
            inside = False
        elif inside:
            m = re.match(r"^( {2}- | {4})(\.\w+):\s*(.*)$", ln)
            if not m:
                continue
            if m.group(1).startswith("  -"):
                cur = {}
            cur[m.group(2)] = m.group(3).strip()
            if m.group(2) == ".name":
                meta[cur[".name"]] = cur
    out = collections.OrderedDict()
    for n in names:
        i = start[n]
        j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))   # the code, then the kernel descriptor
        text = [ln for ln in lines[i:j + 1] if "__hip_cuid_" not in ln]
        mnem = [ln.split()[0] for ln in text[1:] if ln[:1].isspace() and ln.strip() and ln.strip()[0] not in ".;"]
        out[n] = (text, mnem, tuple(meta.get(n, {}).get(k) for k in RESOURCES))
    return out


def classify(a, b):
    if a is None or b is None:
        return "changed"
    if a[0] == b[0]:
        return "identical"
    if a[2] != b[2]:
        return "changed"
    if a[1] == b[1]:
        return "renamed"
    if collections.Counter(a[1]) == collections.Counter(b[1]):
        return "rescheduled"
    return "changed"


def demangle(names):
    rocm = os.path.join(os.path.dirname(HIPCC), "..")
    for filt in (os.path.join(rocm, "lib", "llvm", "bin", "llvm-cxxfilt"), os.path.join(rocm, "llvm", "bin", "llvm-cxxfilt"), "c++filt"):
        try:
            out = subprocess.run([filt] + names, capture_output=True, text=True, check=True).stdout.splitlines()
            return dict(zip(names, (re.sub(r"^void |\(.*$", "", o) for o in out)))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("src", help="a file of %s/csrc, e.g. resample2d.hip" % PKG)
    ap.add_argument("--base", required=True, help="git revision to compare the work tree with")
    ap.add_argument("--debug", action="store_true", help="compile with -DFN2_DEBUG_BUILD")
    a = ap.parse_args()
    src = os.path.basename(a.src)
    with tempfile.TemporaryDirectory() as tmp:
        ar = subprocess.run(["git", "-C", ROOT, "archive", a.base, PKG + "/csrc", "include"], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=ar, check=True)
        with ThreadPoolExecutor(max_workers=2) as pool:
            fb = pool.submit(compile_asm, tmp, src, a.debug, os.path.join(tmp, "base.s"))
            fw = pool.submit(compile_asm, ROOT, src, a.debug, os.path.join(tmp, "work.s"))
            base, work = split_kernels(fb.result()), split_kernels(fw.result())
    names = list(base) + [n for n in work if n not in base]
    pretty = demangle(names)
    counts = collections.Counter()
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", a.base], capture_output=True, text=True, check=True).stdout.strip()
    print("# %s, %s build: %s against the work tree (%d / %d kernels)" % (src, "debug" if a.debug else "release", rev, len(base), len(work)))
    for n in names:
        cls = classify(base.get(n), work.get(n))
        counts[cls] += 1
        print("%-12s %s" % (cls, pretty[n]))
    print("# " + ", ".join("%d %s" % (counts[c], c) for c in ("identical", "renamed", "rescheduled", "changed")))
    return 1 if counts["changed"] else 0


if __name__ == "__main__":
    sys.exit(main())
