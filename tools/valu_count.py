#!/usr/bin/env python3
"""Static instruction count of one kernel of mcmc_amd/csrc/hmc_launch.hip, per basic block.

    python tools/valu_count.py ["hmc_gauss_mfma_kernel<8, 8, false, false, false, false, true>"] [--inner-trips 15] [--tu hmc_launch.hip]

Compiles the translation unit to gfx950 assembly with the Makefile's flags (device side only), finds the one kernel whose
demangled name contains the argument, and prints for every basic block the number of
    mfma   v_mfma*                       valu   every other v_*          ds     ds_*
    vmem   global_* / flat_* / scratch_*                                 wait   s_waitcnt*
Classes are told apart by the opcode's prefix, nothing else.  The draw loop is the largest natural loop of the kernel's control-flow
graph; the loops nested in it (the leapfrog loop) show as depth 2.  The last lines sum the classes over the draw loop, a block at
depth 1 + k counted (inner trips)^k times -- with 15 trips this is one draw of an L = 16 trajectory in which every block of the draw
loop runs once: the accept AND the reject path, and the kept-draw row.  Registers and spills come from the kernel's metadata.
"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function",
         "-I" + os.path.join(ROOT, "include", "mi_mcmc_engine")]
CLASSES = ("mfma", "valu", "ds", "vmem", "wait")


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "ds"
    if op.startswith(("global_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_waitcnt"):
        return "wait"
    return None


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def assembly(tu, extra):
    cmd = [HIPCC] + FLAGS + extra + ["--cuda-device-only", "-S", "-o", "-", tu]
    return subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, check=True).stdout


def kernel_body(asm, want):
    """lines between the kernel's label and its .end_amdhsa_kernel / s_endpgm tail; the mangled name"""
    lines = asm.split("\n")
    starts = [(i, m.group(1)) for i, ln in enumerate(lines) if (m := re.match(r"^(_Z\w+):", ln))]
    names = demangle([n for _, n in starts])
    hits = [(i, n) for i, n in starts if want in names[n].replace("mi::", "")]
    hits = [(i, n) for i, n in hits if not n.endswith(".kd")]
    if len(hits) != 1:
        sys.exit("kernel %r matches %d symbols: %s" % (want, len(hits), [names[n] for _, n in hits][:8]))
    i0, sym = hits[0]
    i1 = next(i for i in range(i0, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    return lines[i0 + 1:i1], sym, names[sym]


def blocks_of(body):
    """[(label, [opcodes], [branch targets])] in layout order"""
    out = [("entry", [], [])]
    for ln in body:
        ln = ln.split(";")[0].strip()
        if not ln:
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            out.append((m.group(1), [], []))
            continue
        if ln.startswith(".") or ln.endswith(":"):
            continue
        op = ln.split()[0]
        out[-1][1].append(op)
        if op.startswith(("s_cbranch", "s_branch")):
            out[-1][2].append(ln.split()[-1])
    return out


def loops_of(blocks):
    """natural loops of the control-flow graph: {header index: set of block indices}.  The layout order says nothing (the compiler
    places the leapfrog loop behind the block it returns to), so: successors, dominators, back edges, bodies."""
    index = {lab: k for k, (lab, _, _) in enumerate(blocks)}
    n = len(blocks)
    succ = [set() for _ in range(n)]
    for k, (_, ops, targets) in enumerate(blocks):
        succ[k].update(index[t] for t in targets if t in index)
        last = ops[-1] if ops else ""
        if k + 1 < n and not last.startswith(("s_branch", "s_endpgm", "s_setpc")):
            succ[k].add(k + 1)
    pred = [set() for _ in range(n)]
    for k in range(n):
        for s in succ[k]:
            pred[s].add(k)
    dom = [set(range(n)) for _ in range(n)]
    dom[0] = {0}
    changed = True
    while changed:
        changed = False
        for k in range(1, n):
            new = set.intersection(*(dom[p] for p in pred[k])) | {k} if pred[k] else {k}
            if new != dom[k]:
                dom[k], changed = new, True
    loops = {}
    for u in range(n):
        for h in succ[u]:
            if h in dom[u]:                                  # back edge u -> h
                body, work = loops.setdefault(h, {h}), [u]
                while work:
                    x = work.pop()
                    if x not in body:
                        body.add(x)
                        work.extend(pred[x])
    return loops


def metadata(asm, sym):
    meta = asm[asm.find("amdhsa.kernels:"):]
    items = re.split(r"\n  - (?=\.)", meta)                  # one list item per kernel
    blk = next((it for it in items if re.search(r"\.name:\s+" + re.escape(sym) + r"\s", it)), "")
    get = lambda key: (re.search(r"\." + key + r":\s+(\d+)", blk) or [None, "?"])[1]
    return {k: get(k) for k in ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kernel", nargs="?", default="hmc_gauss_mfma_kernel<8, 8, false, false, false, false, true>",
                    help="part of the demangled name; default: the full-tile instantiation bench config 2 launches (hmc_dense.hpp)")
    ap.add_argument("--inner-trips", type=int, default=15, help="trips of a loop nested in the draw loop (L - 1)")
    ap.add_argument("--tu", default="hmc_launch.hip")
    ap.add_argument("-D", action="append", default=[], help="extra -D flags")
    ap.add_argument("--keep-asm", default=None, help="also write the translation unit's assembly to this file")
    a = ap.parse_args()
    asm = assembly(a.tu, ["-D" + x for x in a.D])
    if a.keep_asm:
        with open(a.keep_asm, "w") as f:
            f.write(asm)
    body, sym, name = kernel_body(asm, a.kernel)
    blocks = blocks_of(body)
    loops = loops_of(blocks)
    if not loops:
        sys.exit("no loop in " + name)
    head = max(loops, key=lambda h: len(loops[h]))
    draw = loops[head]
    inner = {h: b for h, b in loops.items() if h != head and b <= draw}
    print("kernel  %s" % name)
    print("regs    " + "  ".join("%s=%s" % kv for kv in metadata(asm, sym).items()))
    print("loop    draw loop: header %s, %d blocks; loops nested in it: %s" % (blocks[head][0], len(draw),
          ", ".join("%s (%d blocks)" % (blocks[h][0], len(b)) for h, b in sorted(inner.items())) or "none"))
    print("%-12s %5s %6s %6s %6s %6s %6s" % (("block", "depth") + CLASSES))
    total = dict.fromkeys(CLASSES, 0)
    static = dict.fromkeys(CLASSES, 0)
    for k, (lab, ops, _) in enumerate(blocks):
        n = dict.fromkeys(CLASSES, 0)
        for op in ops:
            c = classify(op)
            if c:
                n[c] += 1
        in_draw = k in draw
        depth = sum(1 for b in inner.values() if k in b) if in_draw else 0
        if sum(n.values()):
            print("%-12s %5s %6d %6d %6d %6d %6d" % ((lab, ("%d" % (depth + 1)) if in_draw else "-") + tuple(n[c] for c in CLASSES)))
        if in_draw:
            for c in CLASSES:
                static[c] += n[c]
                total[c] += n[c] * a.inner_trips ** depth
    print("draw loop, every block once:           " + "  ".join("%s=%d" % (c, static[c]) for c in CLASSES))
    print("draw loop, nested loops x %-3d:          " % a.inner_trips + "  ".join("%s=%d" % (c, total[c]) for c in CLASSES)
          + "  mfma+valu=%d" % (total["mfma"] + total["valu"]))


if __name__ == "__main__":
    main()
