#!/usr/bin/env python3
"""Static instruction count of k_small by phase, from the gfx950 assembly (profiles/valu_budget.md).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -g -Iinclude -S --cuda-device-only \
        -o k.s bsseqconsensusreads_amd/csrc/bsdc_kernels.hip
    python profiles/valu_budget.py k.s [--tags]

Every instruction of the kernel is attributed to a phase by the source line of its `.loc`: a line
inside small_family names its phase; a line of an inlined helper above it (lookup4v, resolve4,
bytes_past, ...) inherits the phase of the last small_family line seen, which holds as far as the
scheduler keeps a helper's instructions next to their call.  Prints VALU / SALU / LDS / VMEM / SMEM
per phase, and the kernel's register metadata.  The phases' line ranges are found from the section
comments of small_family, so the script follows the source as it moves.
"""
import os
import re
import sys
from collections import OrderedDict

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bsseqconsensusreads_amd", "csrc", "bsdc_kernels.hip")
# (phase, the text that opens it in small_family), in source order
MARKS = [("entry+staging", "__device__ __forceinline__ void small_family("),
         ("convert", "// ---- tool 1: every converted record"),
         ("extend", "// ---- tool 2: gap extension"),
         ("dump (off)", "// ---- stage dump ----"),
         ("overlap", "// ---- overlapping-bases consensus ----"),
         ("source reads", "// ---- source reads: read-through trim"),
         ("cigar filter (rare)", "// ---- most-common-alignment filter"),
         ("descriptors", "// ---- read descriptors by set"),
         ("vote setup", "// ---- single-strand vote + duplex combine"),
         ("vote read loop", "if (c < lv) {"),
         ("vote epilogue", "uint32_t bm[2]"),
         ("vote tags", "if (TAGS && c < lv) {"),
         ("queue", "// queued columns: the general path"),
         ("pack/store", "// pack and store: lanes 0-31 end 0"),
         ("status", "// single-strand lengths of the consensus tags"),
         ("(end)", "// One wavefront per family, the grid covering")]


def phase_lines(path):
    src = open(path).read().split("\n")
    out, at = [], 0
    for name, text in MARKS:
        at = next(i for i in range(at, len(src)) if text in src[i])
        out.append((at + 1, name))
    return out


def kind(op):
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "SMEM"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "VMEM"
    return "other"


def main():
    asm = sys.argv[1]
    sym = "7k_smallILb1EEEv" if "--tags" in sys.argv else "7k_smallILb0EEEv"
    marks = phase_lines(SRC)
    lo, hi = marks[0][0], marks[-1][0]
    files, cur_file, phase = {}, None, marks[0][1]
    counts = OrderedDict((n, {}) for _, n in marks[:-1])
    inside, meta = False, {}
    for ln in open(asm):
        s = ln.strip()
        m = re.match(r'\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', s)
        if m:
            files[int(m.group(1))] = (m.group(2) + "/" + m.group(3)) if m.group(3) else m.group(2)
            continue
        if not inside:
            if re.match(r"_Z\w*%s\w*:" % sym, s):
                inside = True
            m = re.match(r"\.(sgpr_count|vgpr_count|agpr_count|private_segment_fixed_size|vgpr_spill_count):\s+(\d+)", s)
            if m and meta.get("armed"):
                meta[m.group(1)] = int(m.group(2))
            if s.startswith(".name:") and sym in s:
                meta["armed"] = True
            elif s.startswith(".name:"):
                meta["armed"] = False
            continue
        if s.startswith(".Lfunc_end"):
            inside = False
            continue
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            f, line = files.get(int(m.group(1)), ""), int(m.group(2))
            if f.endswith("bsdc_kernels.hip") and lo <= line < hi:
                phase = [n for at, n in marks if at <= line][-1]
            continue
        if not s or s[0] in ".;" or s.endswith(":"):
            continue
        k = kind(s.split()[0])
        counts[phase][k] = counts[phase].get(k, 0) + 1
    cols = ["VALU", "SALU", "LDS", "VMEM", "SMEM", "other"]
    print("| phase | " + " | ".join(cols) + " |")
    print("|---|" + "---:|" * len(cols))
    tot = dict.fromkeys(cols, 0)
    for n, c in counts.items():
        if not c:  # (a phase the instance has no code for: the tag stores of the plain one)
            continue
        print("| %s | " % n + " | ".join(str(c.get(k, 0)) for k in cols) + " |")
        for k in cols:
            tot[k] += c.get(k, 0)
    print("| **static total** | " + " | ".join(str(tot[k]) for k in cols) + " |")
    meta.pop("armed", None)
    print("\nregisters:", ", ".join("%s %d" % kv for kv in sorted(meta.items())))


if __name__ == "__main__":
    main()
