"""Instruction mix of the K loops of the pipelined convolutions (csrc/conv.hip: conv_pipe_kernel; csrc/conv_wgrad.hip:
wgrad_pipe_kernel), from the compiler's assembly of the unit that holds the kernel:
    hipcc <Makefile FLAGS> -S --cuda-device-only conv.hip -o conv.s             (or conv_wgrad.hip -o conv_wgrad.s)
    python tools/loop_mix.py conv.s [kernel substring ...]     (default: conv_pipe_kernel wgrad_pipe_kernel)
Per kernel, every depth-1 loop that holds an MFMA: static counts per wave and trip of v_mfma*, other v_* (and, of
those, the 32/64-bit integer multiplies), *load_lds*, ds_read* and *saveexec* lines.  Loop membership is LLVM's own
"in Loop: Header=... Depth=1" / "This Loop Header: Depth=1" block annotation.  A kernel with both a fast and a generic
staging path shows one loop for each; rarely taken blocks inside a loop (a segment switch) are counted like the rest."""
import re
import subprocess
import sys
from collections import OrderedDict

MUL = re.compile(r"v_(mul_lo_u32|mul_hi_u32|mul_hi_i32|mul_lo_i32|mad_u64_u32|mad_i64_i32|mul_u32_u24|mad_u32_u24)")


def loops(path, pats):
    func, hdr = None, None
    out = OrderedDict()
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            func, hdr = m.group(1), None
            continue
        if line.startswith(".Lfunc_end"):
            func = None
            continue
        if func is None or not any(p in func for p in pats):
            continue
        m = re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)(.*)$", line)
        if m:
            note = m.group(2)
            lbl = m.group(1).rstrip(":").lstrip(".L")
            h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=1", note)
            if h:
                hdr = h.group(1)
            elif re.search(r"This (Inner )?Loop Header: Depth=1", note):
                hdr = lbl
            else:
                hdr = None
            continue
        if hdr is None:
            continue
        t = line.strip()
        if not t or t.startswith((";", ".")):
            continue
        op = t.split()[0]
        c = out.setdefault((func, hdr), dict(mfma=0, valu=0, mul=0, lds_dma=0, ds_read=0, saveexec=0))
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            if MUL.match(op):
                c["mul"] += 1
        if "load_lds" in op or (op.startswith(("global_load", "buffer_load")) and " lds" in t):
            c["lds_dma"] += 1
        if op.startswith("ds_read"):
            c["ds_read"] += 1
        if "saveexec" in op:
            c["saveexec"] += 1
    return out


def main():
    path = sys.argv[1]
    pats = sys.argv[2:] or ["conv_pipe_kernel", "wgrad_pipe_kernel"]
    names = {}
    print(f"{'mfma':>5s} {'valu':>5s} {'mul':>4s} {'dma':>4s} {'dsrd':>5s} {'sexec':>5s}  kernel (loop)")
    for (func, hdr), c in loops(path, pats).items():
        if not c["mfma"]:
            continue
        if func not in names:
            dem = subprocess.run(["c++filt", func], capture_output=True, text=True).stdout.strip()
            names[func] = re.sub(r"\(anonymous namespace\)::|void |\(.*$", "", dem)
        print(f"{c['mfma']:5d} {c['valu']:5d} {c['mul']:4d} {c['lds_dma']:4d} {c['ds_read']:5d} {c['saveexec']:5d}  "
              f"{names[func]} ({hdr})")


if __name__ == "__main__":
    main()
