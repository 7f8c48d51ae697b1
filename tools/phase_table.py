#!/usr/bin/env python3
"""Per-phase instruction table of the persistent step kernel (diagnostic; hipcc only, no GPU):
    python tools/phase_table.py [stamps.txt]
Compiles the STAMPS build (-DEVG_DIAG -DEVG_STAMPS: a sched-barrier + s_memtime at every phase boundary, so nothing moves across a boundary) to ISA and counts the
instructions between consecutive stamps of evg_step_kernel<float, 64, MULTI = true> (two-lane persistent form, float32 observations): the STATIC stream a
wavefront walks through once per turn.  Straight-line phases (orders, movement, aggregates, observation build / write-out) execute every one of them; the
combat phases hold loops and wave-uniform skips, so their dynamic count differs -- compare the static sum with the SQ counter total of the build
(profiles/*_sq_counters.json).  With the output of tools/stamps.py (run on the GPU: wave cycles per phase) as argument, the two are merged into one table."""
import os
import re
import subprocess
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "everglades-ai-wargame_amd", "csrc")
NAMES = ["tables+state load", "orders", "combat0 snapshot", "combat1 worklist", "combatA draws", "combatB apply", "movement",
         "aggregates+capture", "rewards+stats+reset", "obs build", "state store", "obs write-out", "reset fill"]
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _prof  # noqa: E402
KERNEL = _prof.step_kernel_symbol("persistent", "float32")
KINDS = ("valu", "salu", "lds", "vmem", "branch", "waitcnt")


def main():
    asm = "/tmp/evg_phase_table.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-DEVG_DIAG",
                           "-DEVG_STAMPS", "-Wno-unused-command-line-argument", "-S", "--cuda-device-only", "-o", asm, "evg_kernels.hip"], cwd=CSRC)
    lines = open(asm).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(KERNEL + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".end_amdhsa_kernel") or lines[i].strip().startswith(".section"))
    seg, cur = [], dict.fromkeys(KINDS, 0)
    for l in lines[start:end]:
        t = l.strip()
        if t.startswith("s_memtime"):
            seg.append(cur)
            cur = dict.fromkeys(KINDS, 0)
        elif t.startswith("v_"):
            cur["valu"] += 1
        elif t.startswith("s_waitcnt"):
            cur["waitcnt"] += 1
        elif t.startswith("s_cbranch") or t.startswith("s_branch"):
            cur["branch"] += 1
        elif t.startswith("s_"):
            cur["salu"] += 1
        elif t.startswith("ds_"):
            cur["lds"] += 1
        elif t.startswith("global_") or t.startswith("buffer_") or t.startswith("flat_"):
            cur["vmem"] += 1
    seg.append(cur)
    assert len(seg) == 16, "expected STAMP(0) + PHASE(0..13): 15 stamps, got %d" % (len(seg) - 1)
    cycles, heads = {}, []
    if len(sys.argv) > 1:
        for b in open(sys.argv[1]).read().split("turn ")[1:]:
            heads.append(b.split(":")[0])
            for m in re.finditer(r"^\s+(.+?)\s+mean\s+([\d.]+)\s+max\s+([\d.]+)", b, re.M):
                cycles.setdefault(m.group(1).strip(), []).append(float(m.group(2)))
    print("evg_step_kernel<float, 64, MULTI = true> (persistent two-lane form), stamps build: static ISA between consecutive phase stamps%s"
          % ("; wave cycles per phase = s_memtime (shader clock; stamps build) of tools/stamps.py at game turns %s, mean over the 2 048 wavefronts" % " / ".join(heads) if cycles else ""))
    print("%-22s %5s %5s %4s %5s %6s %7s   %s" % ("phase", "VALU", "SALU", "LDS", "VMEM", "branch", "waitcnt", "wave cycles" if cycles else ""))
    tot = dict.fromkeys(KINDS, 0)
    c = seg[1]
    print("%-22s %5d %5d %4d %5d %6d %7d   (STAMP(0) .. PHASE(0): once per launch)" % ("launch prologue", c["valu"], c["salu"], c["lds"], c["vmem"], c["branch"],
                                                                                      c["waitcnt"]))
    for i, nm in enumerate(NAMES):              # NAMES[i] = PHASE(i) .. PHASE(i + 1) = segment i + 2 (tools/stamps.py's names; in the persistent form with orders
        c = seg[i + 2]                          # drawn in the kernel its first phase is the drawing of both players' 7 rows, not a load)
        for k in KINDS:
            tot[k] += c[k]
        label = "order rows drawn" if i == 0 else nm
        print("%-22s %5d %5d %4d %5d %6d %7d   %s" % (label, c["valu"], c["salu"], c["lds"], c["vmem"], c["branch"], c["waitcnt"],
                                                      "  ".join("%6.0f" % x for x in cycles.get(nm, []))))
    c = seg[15]
    print("%-22s %5d %5d %4d %5d %6d %7d   (basic blocks the compiler placed behind the loop: the sparse last combat round, cold paths, the chunk epilogue)"
          % ("after the last stamp", c["valu"], c["salu"], c["lds"], c["vmem"], c["branch"], c["waitcnt"]))
    print("%-22s %5d %5d %4d %5d %6d %7d   static sum of the 13 per-turn phases (the dynamic count per wave-turn is in profiles/*_sq_counters.json: loops and "
          "wave-uniform skips in the combat phases make the two differ)" % ("sum per turn", tot["valu"], tot["salu"], tot["lds"], tot["vmem"], tot["branch"],
                                                                            tot["waitcnt"]))


if __name__ == "__main__":
    main()
