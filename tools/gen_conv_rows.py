"""Record what mer_conv_fwd_rows / mer_conv_dgrad_rows return into tests/golden/conv_rows.json.

Run:  python tools/gen_conv_rows.py   -- on the PARENT of a change to the conv tile plan, with its library built; the
change must then reproduce every record (tests/test_conv_plan_cpu.py).  Both entry points are host-only: no GPU is
needed (the CU count then falls back to 256, the MI355X's), and the fake pointers are never dereferenced.
Records: ["fwd", N, H, W, C, K, R, S, stride, pad, x, w, variant, rows] and
["dgrad", N, H, W, C, K, R, S, stride, pad, dy, wt, ds_dy, variant, rows] (N, H, W, C: the input gradient's shape).
"""
import itertools
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from multimodalemotionrecognition_amd._lib import LIB  # noqa: E402

A, U = 1 << 20, (1 << 20) + 8  # a 16-byte-aligned and an 8-byte-misaligned pointer
# (H, C, K at stride 1 / stride 2, R, pad): the ResNet18 trunk's 3x3 convs, an odd map, the stem's space-to-depth form
shapes = [(h, c, (c, min(2 * c, 512)), 3, 1) for h, c in ((28, 64), (14, 128), (7, 256), (4, 512), (15, 128))]
shapes += [(59, 16, (64, 64), 4, 0)]
recs = []
for n, (h, c, ks, r, pad), st, v in itertools.product((256, 40, 3), shapes, (1, 2), range(-1, 9)):
    k = ks[st - 1]
    halo = v in (-1, 6)  # the variants that test for the halo kernel: the only readers of alignment and of ds_dy
    if not halo and n != 40:  # (pruned) any other explicit variant reports a bound of the pixel count alone
        continue
    for p, ds in ((A, 0), (U, 0), (A, A)) if halo else ((A, 0),):  # dx is [n, h, h, c], dy has k channels
        if not ds:
            recs.append(["fwd", n, h, h, c, k, r, r, st, pad, p, A, v,
                         LIB.call_int("mer_conv_fwd_rows", n, h, h, c, k, r, r, st, pad, p, A, v)])
        recs.append(["dgrad", n, h, h, c, k, r, r, st, pad, p, A, ds, v,
                     LIB.call_int("mer_conv_dgrad_rows", n, h, h, c, k, r, r, st, pad, p, A, ds, v)])
out = ROOT / "tests" / "golden" / "conv_rows.json"
out.write_text("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in recs) + "\n]\n")
print(len(recs), "records ->", out)
