#!/usr/bin/env python3
"""Issue-slot model of an MFMA stream, from the compiled code (CPU only: hipcc cross-compiles):

    python tools/ef_gap_model.py                                   # edgeconv_f16b.hip, <5,true>, runs 120,240,960
    python tools/ef_gap_model.py --unit conv_f16.hip --kernel <mangled name or a part of it> --runs 64,64
    python tools/ef_gap_model.py --asm some.s ...                   # an assembly file made earlier

The unit is compiled with the flags of learning3d_amd/build.py plus `--cuda-device-only -S`.  Inside the named kernel the
tool takes the body of the (outermost) loop -- the whole kernel if there is none -- and walks it in program order, closed
into a ring when it is a loop.  A GAP is what stands between one `v_mfma_*_16x16x32_*` and the next; its FILLERS are the
instructions that take a vector issue slot: VALU (v_*, other MFMAs included), LDS (ds_*), VMEM (global_/buffer_/flat_/
scratch_) and s_nop.  With one wave per SIMD the MFMA holds the issue for 8 of its 16 cycles and a filler costs >= 4, so a
gap runs about max(16, 8 + 4 c) cycles: two fillers are nearly free, every further one costs its issue.

The compiler may rotate the loop: in edgeconv_f16b<5,true> the body's text begins with layer 4's LAST pair (120 MFMAs, then
the tile's tail and layer 1), so the layers are runs 120,240,960 only with --rotate 120; without it the first "run" is that
pair plus the wrap and the second is layer 2 plus half of layer 3.

--runs a,b,c splits the MFMAs of the body into consecutive runs (the layers of edgeconv_f16b: 120, 240, 960); a gap
belongs to the run of the MFMA in front of it, so the last run carries the wrap to the next trip.  Per run: the filler
histogram, the s_nop count (all, and those in gaps that hold more than two fillers), the model's cycles and the floor.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from learning3d_amd.build import CSRC, FLAGS, HIPCC  # noqa: E402

MAIN = re.compile(r"v_mfma_\w*16x16x32_")
VMEM = ("global_", "buffer_", "flat_", "scratch_")


def compile_asm(unit, defines):
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    cmd = [HIPCC, *[f for f in FLAGS if f != "-fPIC"], *defines, "--cuda-device-only", "-S", os.path.join(CSRC, unit), "-o", out]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
    with open(out) as f:
        text = f.read()
    os.remove(out)
    return text


def kernel_lines(text, name):
    """[(label | None, mnemonic, rest)] of the one kernel whose symbol contains `name`, and its metadata comments."""
    lines = text.splitlines()
    starts = [i for i, l in enumerate(lines) if re.match(r"^[A-Za-z_][\w$.]*:", l) and name in l.split(":")[0] and not l.startswith(".")]
    if len(starts) != 1:
        raise SystemExit(f"{len(starts)} kernels match {name!r}")
    end = next(i for i in range(starts[0], len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = []
    for l in lines[starts[0] + 1:end]:
        code = l.split(";")[0].strip()
        if not code:
            continue
        if code.endswith(":"):
            body.append((code[:-1], None, ""))
        elif not code.startswith("."):
            mn, _, rest = code.partition(" ")
            body.append((None, mn, rest.strip()))
    meta = {}
    for l in lines[end:end + 80]:
        m = re.match(r";\s*(NumVgprs|NumAgprs|ScratchSize|codeLenInByte|TotalNumVgprs|LDSByteSize):\s*(\d+)", l.strip())
        if m:
            meta[m.group(1)] = int(m.group(2))
    return body, meta


def loop_body(body):
    """The outermost loop: from the earliest label that a LATER branch jumps back to, up to the last such branch."""
    pos = {lab: i for i, (lab, _, _) in enumerate(body) if lab}
    best = None
    for i, (_, mn, rest) in enumerate(body):
        if mn and mn.startswith(("s_cbranch", "s_branch")) and rest in pos and pos[rest] < i:
            if best is None or pos[rest] < best[0] or (pos[rest] == best[0] and i > best[1]):
                best = (pos[rest], i)
    return (body[best[0]:best[1] + 1], True) if best else (body, False)


def is_filler(mn):
    return mn.startswith(("v_", "ds_")) or mn.startswith(VMEM) or mn == "s_nop"


def gaps_of(body, ring):
    """Per main MFMA, the list of fillers between it and the next one (ring: the last gap wraps to the first MFMA)."""
    ins = [mn for _, mn, _ in body if mn]
    at = [i for i, mn in enumerate(ins) if MAIN.match(mn)]
    if not at:
        raise SystemExit("no 16x16x32 MFMA in the body")
    gaps = []
    for n, i in enumerate(at):
        if n + 1 < len(at):
            seg = ins[i + 1:at[n + 1]]
        else:
            seg = ins[i + 1:] + (ins[:at[0]] if ring else [])
        gaps.append([mn for mn in seg if is_filler(mn)])
    return gaps


def report(gaps, runs):
    if sum(runs) != len(gaps):
        print(f"note: --runs sums to {sum(runs)}, the body holds {len(gaps)} MFMAs; the last run takes the rest")
        runs = runs[:-1] + [len(gaps) - sum(runs[:-1])]
    lo = 0
    tot_model = tot_floor = 0
    for n, cnt in enumerate(runs):
        seg = gaps[lo:lo + cnt]
        lo += cnt
        hist = collections.Counter(len(g) for g in seg)
        fill = sum(len(g) for g in seg)
        nops = sum(mn == "s_nop" for g in seg for mn in g)
        nops_over = sum(mn == "s_nop" for g in seg if len(g) > 2 for mn in g)
        model = sum(max(16, 8 + 4 * len(g)) for g in seg)
        unused = sum(max(0, 2 - len(g)) for g in seg)
        over = sum(max(0, len(g) - 2) for g in seg)
        tot_model += model
        tot_floor += 16 * cnt
        print(f"run {n}: {cnt} MFMAs  fillers {fill}  s_nop {nops} ({nops_over} in gaps of more than two fillers)  "
              f"model {model} cycles  floor {16 * cnt}  free slots unused {unused}  fillers past two {over}")
        print("   fillers/gap: " + "  ".join(f"{c}:{hist[c]}" for c in sorted(hist)))
    print(f"all: model {tot_model} cycles, floor {tot_floor}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--unit", default="edgeconv_f16b.hip")
    ap.add_argument("--kernel", default="_Z20edgeconv_f16b_kernelILi5ELb1EE")
    ap.add_argument("--runs", default="120,240,960")
    ap.add_argument("--rotate", type=int, default=0, help="start the runs at this MFMA of the body's text order (a rotated loop)")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("-D", action="append", default=[], dest="defs")
    ap.add_argument("--mix", action="store_true", help="also print the instruction mix of the body")
    a = ap.parse_args()
    text = open(a.asm).read() if a.asm else compile_asm(a.unit, ["-D" + d for d in a.defs])
    body, meta = kernel_lines(text, a.kernel)
    print(a.kernel, " ".join(f"{k} {v}" for k, v in meta.items()))
    loop, ring = loop_body(body)
    print(f"body: {sum(1 for _, mn, _ in loop if mn)} instructions, {'loop' if ring else 'whole kernel'}")
    gaps = gaps_of(loop, ring)
    if a.rotate:
        gaps = gaps[a.rotate:] + gaps[:a.rotate]
    report(gaps, [int(x) for x in a.runs.split(",")])
    if a.mix:
        mix = collections.Counter(mn for _, mn, _ in loop if mn and is_filler(mn))
        print("mix: " + "  ".join(f"{k} {v}" for k, v in mix.most_common(30)))


if __name__ == "__main__":
    main()
