#!/usr/bin/env python3
"""march_rc_isa.py -- the marching PCG iteration without the A p plane (thallo_amd/csrc/energy_image_warping_march_rc.hip) in gfx950 ISA, no GPU needed.

  python tools/march_rc_isa.py [--src FILE] [--keep DIR] [--rows R] [--all]

Compiles the kernel file with the product's flags (thallo_amd/csrc/Makefile: -O3 -ffp-contract=on -fno-slp-vectorize, --cuda-device-only -S) and prints, for each
product instantiation k_iter_march_rc<DMODE, DEPTH, NTM 5, OCC 2, SLAB>:
  * the register use the compiler reports (VGPRs, scratch, SGPR spills);
  * the steady row loop -- the smallest loop whose body holds four row steps' worth of `take` moves (inline-asm v_mov, four rows per trip) -- per row step, by class:
    VALU (all v_*), of which packed (v_pk_*), f64 (any v_*_f64, converts included) and DPP; SALU (s_* but s_waitcnt / s_nop), s_waitcnt and the vmcnt values
    the loop waits for, s_nop, memory (buffer / global / LDS).  Blocks of a loop nested inside it and blocks that load through global / scalar loads (the
    iteration's scalars, once per launch) are left out of the per-step figure and counted separately;
  * row steps per segment at 2048^2 (R rows per segment: the product grid at 256 CUs, 35 rows), by what each step does.
--src: another version of the kernel file (e.g. `git show <rev>:<path> > old.hip`), compiled against this tree's headers.  --all: every instantiation.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "thallo_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-private-field",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-ffp-contract=on", "-fno-slp-vectorize", "--cuda-device-only", "-S",
         "-Rpass-analysis=kernel-resource-usage"]
PRODUCT = [(1, 4, 0), (1, 2, 0), (0, 4, 0), (2, 4, 0), (1, 4, 1), (1, 4, 2), (1, 2, 2)]          # (DMODE, DEPTH, SLAB)
TAKES = {0: 12, 1: 9, 2: 15}        # take moves per row step: po 2 pa 1 cs 2 f 1 ro 2 ra 1 (+ delta 3, + p_{k-2} 3)


def compile_isa(src, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    s_path = os.path.join(out, "rc.s")
    r = subprocess.run([hipcc] + FLAGS + [src, "-o", s_path], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    return open(s_path).read(), r.stderr


def resources(remarks):
    res = {}
    for b in remarks.split("Function Name: ")[1:]:
        name = b.split()[0]
        g = lambda k: int(re.search(k + r": (\d+)", b).group(1))
        res[name] = dict(vgpr=g("VGPRs"), scratch=g(r"ScratchSize \[bytes/lane\]"), sspill=g("SGPRs Spill"), vspill=g("VGPRs Spill"))
    return res


def blocks_of(lines, name):
    start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    order, blocks, cur, in_asm = ["entry"], {"entry": []}, "entry", False
    for ln in lines[start + 1:end]:
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            cur = m.group(1); blocks[cur] = []; order.append(cur); continue
        t = ln.strip()
        if t.startswith(";;#ASMSTART"): in_asm = True; continue
        if t.startswith(";;#ASMEND"): in_asm = False; continue
        if ln.startswith("\t") and t and not t.startswith((".", ";")):
            blocks[cur].append((t, in_asm))
    return order, blocks


def loops(order, blocks):
    idx = {b: i for i, b in enumerate(order)}
    out = []
    for b in order:
        for ins, _ in blocks[b]:
            m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", ins)
            if m and m.group(1) in idx and idx[m.group(1)] <= idx[b]:
                out.append((idx[m.group(1)], idx[b]))
    return out


def classify(ins):
    op = ins.split()[0]
    c = {"all": 1}
    if op.startswith("v_"):
        c["valu"] = 1
        if op.startswith("v_pk_"): c["packed"] = 1
        if "f64" in op: c["f64"] = 1
        if "dpp" in ins or "wave_sh" in ins or "row_" in ins: c["dpp"] = 1
        if op.startswith("v_mov_b32") or op.startswith("v_mov_b64"): c["vmov"] = 1
    elif op.startswith(("buffer_", "global_", "flat_", "scratch_", "ds_")):
        c["mem"] = 1
    elif op == "s_waitcnt":
        c["waitcnt"] = 1
    elif op == "s_nop":
        c["nop"] = 1
    elif op.startswith("s_"):
        c["salu"] = 1
    return c


def steady_loop(order, blocks, dmode):
    want = 4 * TAKES[dmode]
    lps = loops(order, blocks)
    best = None
    for a, b in lps:
        body = [x for bb in order[a:b + 1] for x in blocks[bb]]
        takes = sum(1 for ins, asm in body if asm and ins.startswith("v_mov"))
        if takes == want and (best is None or (b - a) < (best[1] - best[0])):
            best = (a, b)
    if best is None:
        return None
    a, b = best
    nested = set()
    for x, y in lps:
        if a <= x and y <= b and (x, y) != (a, b):
            nested.update(range(x, y + 1))
    idx = {bb: i for i, bb in enumerate(order)}
    cold_i = {i for i in range(a, b + 1) if i in nested or any(re.match(r"(global_load|flat_load|s_load|s_buffer_load)", ins) for ins, _ in blocks[order[i]])}
    # a uniform forward branch that jumps over a once-per-launch region: everything it skips is that region
    for i in range(a, b + 1):
        for ins, _ in blocks[order[i]]:
            m = re.match(r"s_cbranch_(scc[01]|vccn?z)\s+(\.LBB\d+_\d+)", ins)
            if m and m.group(2) in idx and i < idx[m.group(2)] <= b + 1:
                skipped = set(range(i + 1, idx[m.group(2)]))
                if skipped & cold_i:
                    cold_i |= skipped
    hot, cold = [], []
    for i in range(a, b + 1):
        (cold if i in cold_i else hot).extend(ins for ins, _ in blocks[order[i]])
    return hot, cold


def row_steps(src_text, R, depth):
    """row steps of one R-row segment: (what they are, total)"""
    if "PH_FULL" in src_text:        # phase-specialised march: rows ya-2 .. yb+1, no lead-in, no rounding
        return "2 enter + 2 stencil-1 + %d full" % R, R + 4
    n = R + 4 + depth                # one loop from ya-2-DEPTH to yb+1 in whole trips of four, every step full
    n4 = (n + 3) // 4 * 4
    return "%d full (%d lead-in, %d rounding)" % (n4, depth, n4 - n), n4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(CSRC, "energy_image_warping_march_rc.hip"))
    ap.add_argument("--keep", default=None)
    ap.add_argument("--rows", type=int, default=35)
    ap.add_argument("--all", action="store_true")
    a = ap.parse_args()
    out = a.keep or tempfile.mkdtemp(prefix="march_rc_isa_")
    os.makedirs(out, exist_ok=True)
    isa, remarks = compile_isa(os.path.abspath(a.src), out)
    res = resources(remarks)
    lines = isa.split("\n")
    src_text = open(a.src).read()
    names = [ln[:-1].split(":")[0] for ln in lines if re.match(r"^_Z\S*k_iter_march_rc\S*:", ln)]
    print("source: %s" % os.path.relpath(os.path.abspath(a.src), ROOT) if os.path.abspath(a.src).startswith(ROOT) else "source: %s" % a.src)
    for name in names:
        m = re.search(r"ILi(\d)ELi(\d)ELi(\d+)ELi(\d)ELi(\d)E", name)
        dmode, depth, ntm, occ, slab = map(int, m.groups())
        if not a.all and (dmode, depth, slab) not in PRODUCT:
            continue
        r = res.get(name, {})
        order, blocks = blocks_of(lines, name)
        st = steady_loop(order, blocks, dmode)
        print("k_iter_march_rc<DMODE %d, DEPTH %d, NTM %d, OCC %d, SLAB %d>: VGPRs %s, scratch %s B, SGPR spills %s, VGPR spills %s"
              % (dmode, depth, ntm, occ, slab, r.get("vgpr"), r.get("scratch"), r.get("sspill"), r.get("vspill")))
        if st is None:
            print("  steady loop: not found"); continue
        hot, cold = st
        tot = {}
        for ins in hot:
            for k, v in classify(ins).items():
                tot[k] = tot.get(k, 0) + v
        g = lambda k: tot.get(k, 0) / 4.0
        vm = sorted(set(re.search(r"vmcnt\((\d+)\)", x).group(1) for x in hot if x.startswith("s_waitcnt") and "vmcnt" in x), key=int)
        print("  steady row step: %.1f instructions | VALU %.1f (packed %.1f, f64 %.1f, DPP %.1f, v_mov %.1f) | SALU %.1f | s_waitcnt %.1f | s_nop %.1f | memory %.1f"
              % (g("all"), g("valu"), g("packed"), g("f64"), g("dpp"), g("vmov"), g("salu"), g("waitcnt"), g("nop"), g("mem")))
        print("    (loop body %d instructions for 4 rows%s; waits vmcnt %s)" % (len(hot) + len(cold), ", of them %d once-per-launch scalars" % len(cold) if cold else "", ",".join(vm) or "-"))
        what, n = row_steps(src_text, a.rows, depth)
        print("  row steps per %d-row segment: %d = %s" % (a.rows, n, what))


if __name__ == "__main__":
    main()
