#!/usr/bin/env python3
"""isa_equal.py -- are two builds of the kernels the same device code?  No GPU needed; the first check of a kernel refactor.

  python tools/isa_equal.py [--diff] A B        A, B: two .s files, or two directories holding .s files of the same names; --diff: also a unified diff of what differs

The .s files are device assembly (hipcc <the product's flags of that file> --cuda-device-only -S, thallo_amd/csrc/Makefile).  Each file is split per kernel
symbol: the kernel's text from its section to its end label, its kernel descriptor (.amdhsa_kernel) and its entry of the code object's metadata.  Dropped before
the comparison: .file, .ident, comment lines and the per-compilation __hip_cuid_* symbol; the function number in local labels (.LBB<n>_, .Lfunc_end<n>) is taken
out, so a kernel does not differ because another one was added in front of it.  What lies outside every kernel is compared as one more entry.
Prints one line per kernel -- `equal` or `differs`, and VGPRs, SGPRs, scratch and LDS bytes from the metadata as A / B -- and exits non-zero if anything differs
or a kernel exists on one side only.  The comparison is of text; nothing is looked for in it.
"""
import difflib
import os
import re
import shutil
import subprocess
import sys

REST = "(outside the kernels)"
META = ((".vgpr_count", "VGPRs"), (".sgpr_count", "SGPRs"), (".private_segment_fixed_size", "scratch"), (".group_segment_fixed_size", "LDS"))


def split(path):
    """{kernel symbol or REST: [lines]}, {kernel symbol: {metadata key: value}}"""
    lines = open(path).read().split("\n")
    kernels = set(m.group(1) for ln in lines for m in [re.match(r"\t\.amdhsa_kernel\s+(\S+)", ln)] if m)
    parts, meta, owner, entry, in_meta = {REST: []}, {}, REST, None, False

    def close(entry):
        text = "\n".join(entry)
        name = re.search(r"\.name:\s+(\S+)", text).group(1)
        parts.setdefault(name, []).extend(entry)
        meta[name] = {k: re.search(re.escape(k) + r":\s+(\d+)", text).group(1) for k, _ in META}

    for ln in lines:
        t = ln.strip()
        if not t or t.startswith(";") or t.startswith((".file", ".ident")) or "__hip_cuid_" in t:
            continue
        if t == "amdhsa.kernels:":
            in_meta = True
        elif in_meta and not ln.startswith(" "):        # amdhsa.target: the list of kernels is over
            if entry: close(entry)
            in_meta, entry, owner = False, None, REST
        elif in_meta:
            if ln.startswith("  - "):
                if entry: close(entry)
                entry = []
            entry.append(ln)
            continue
        m = re.match(r"\t\.(?:section\t\.text\.|globl\t|protected\t)([^,\s]+)", ln)
        if m and m.group(1) in kernels:
            owner = m.group(1)
        elif re.match(r"\t\.section\t\.AMDGPU\.", ln):
            owner = REST
        ln = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", ln))
        parts.setdefault(owner, []).append(ln)
    return parts, meta


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or (os.path.exists("/opt/rocm/llvm/bin/llvm-cxxfilt") and "/opt/rocm/llvm/bin/llvm-cxxfilt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool] + list(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(anonymous namespace\)::|\(.*", "", d) for n, d in zip(names, out)}


def compare(a, b, label, diff=False):
    (pa, ma), (pb, mb) = split(a), split(b)
    names = [n for n in pa if n != REST] + [n for n in pb if n not in pa] + [REST]
    pretty = demangle([n for n in names if n != REST])
    bad = 0
    for n in names:
        same = pa.get(n) == pb.get(n)
        bad += not same
        what = "equal  " if same else "differs" if n in pa and n in pb else "only in " + ("A" if n in pa else "B")
        res = "  ".join("%s %s / %s" % (t, ma.get(n, {}).get(k, "-"), mb.get(n, {}).get(k, "-")) for k, t in META) if n != REST else ""
        print("%s  %s: %s%s" % (what, label, pretty.get(n, n), "   " + res if res else ""))
        if diff and not same:
            print("\n".join(difflib.unified_diff(pa.get(n, []), pb.get(n, []), "A", "B", lineterm="", n=2)))
    return bad


def main():
    diff = "--diff" in sys.argv[1:]
    args = [x for x in sys.argv[1:] if x != "--diff"]
    if len(args) != 2:
        sys.exit(__doc__)
    a, b = args
    if os.path.isdir(a) != os.path.isdir(b):
        sys.exit("two .s files or two directories")
    bad = 0
    if os.path.isdir(a):
        fa, fb = (sorted(f for f in os.listdir(d) if f.endswith(".s")) for d in (a, b))
        for f in sorted(set(fa) | set(fb)):
            if f in fa and f in fb:
                bad += compare(os.path.join(a, f), os.path.join(b, f), f, diff)
            else:
                print("only in %s  %s" % ("A" if f in fa else "B", f)); bad += 1
    else:
        bad = compare(a, b, os.path.basename(a), diff)
    print("%d differ" % bad if bad else "all equal")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
