"""Record what kernels.conv_wgrad asks of a weight-gradient launch into tests/golden/wgrad_plan.json.

Run:  python tools/gen_wgrad_plan.py   -- on the PARENT of a change to the weight-gradient plan; the change must then
reproduce every record (tests/test_wgrad_plan_cpu.py).  No GPU and no library are needed: K.conv_wgrad(...,
defer=WgradFolds()) runs with the launch stubbed and torch.empty recording the workspace size, on tensors that are
shapes only.  Read back: the variant and the splits passed to the launch, the slab count in the fold row, the workspace
floats.  Records: [N, H, W, C, Creal, K, R, S, stride, pad, variant asked, splits asked (0: choose), variant, splits,
slabs, workspace floats].
"""
import itertools
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from multimodalemotionrecognition_amd import kernels as K  # noqa: E402


class Shape:
    """What conv_wgrad reads of a tensor."""

    def __init__(self, *shape, dtype=torch.bfloat16):
        self.shape, self.dtype, self.device = tuple(shape), dtype, "cpu"

    def data_ptr(self):
        return 1 << 20

    def numel(self):
        n = 1
        for d in self.shape:
            n *= d
        return n

    def is_contiguous(self):
        return True


def record(N, H, W, C, Kc, R, stride, pad, variant, splits):
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    seen, folds = {}, K.WgradFolds()

    def launch(name, key, fn, *a):
        assert fn == "mer_conv_wgrad_partials"
        seen["splits"], seen["variant"] = a[11], a[13]

    def empty(n, **kw):
        seen["ws"] = n
        return Shape(n, dtype=torch.float32)

    saved = K._launch, K.stream_ptr, torch.empty
    K._launch, K.stream_ptr, torch.empty = launch, lambda: 0, empty
    try:
        K.conv_wgrad(Shape(N, H, W, C), Shape(N, Ho, Wo, Kc), Shape(Kc, C, R, R, dtype=torch.float32), R, R, stride,
                     pad, variant=variant, splits=splits, defer=folds)
    finally:
        K._launch, K.stream_ptr, torch.empty = saved
    return [N, H, W, C, C, Kc, R, R, stride, pad, variant, splits or 0, seen["variant"], seen["splits"],
            folds.rows[0][7], seen["ws"]]


def trunk_shapes(frames, side):
    """(N, H, W, C, K, R, stride, pad) of every ResNet18 conv; the stem in its 4x4 space-to-depth form."""
    yield frames, side // 2 + 3, side // 2 + 3, 16, 64, 4, 1, 0
    h, c = side // 4, 64
    yield frames, h, h, c, c, 3, 1, 1
    for _ in range(3):
        yield frames, h, h, c, 2 * c, 3, 2, 1
        yield frames, h, h, c, 2 * c, 1, 2, 0
        h, c = (h + 1) // 2, 2 * c
        yield frames, h, h, c, c, 3, 1, 1


def main():
    recs = []
    for frames, side in ((8, 112), (64, 112), (256, 112), (320, 112), (64, 96)):
        for s in trunk_shapes(frames, side):
            for v, sp in itertools.product((-1, 4, 8), (None, 1, 3, 64, 1000)):
                recs.append(record(*s, v, sp))
            N, H, W, C, Kc, R, stride, pad = s
            if R == 3 and stride == 1 and C % 64 == 0:  # what the strip kernel takes (K % 64 == 0 on all of these)
                for v, sp in itertools.product((9, 10), (None, 1, 5, 300)):
                    recs.append(record(*s, v, sp))
    out = ROOT / "tests" / "golden" / "wgrad_plan.json"
    out.write_text("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in recs) + "\n]\n")
    print(len(recs), "records ->", out)


if __name__ == "__main__":
    main()
