"""The weight-gradient plan (csrc/conv_wgrad.hip wgrad_plan): mer_conv_wgrad_plan reproduces every record of
tests/golden/wgrad_plan.json, which tools/gen_wgrad_plan.py took from kernels.conv_wgrad while the variant, split and
slab-count rules still lived in Python.  Host-only entry point: no GPU needed.  This pins the plan; that a launch writes
exactly the planned slabs is tests/test_resnet_gpu.py's (rings) and tests/test_wgrad_strip_gpu.py's (strip) to check."""
import ctypes
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
INVALID = 1  # hipErrorInvalidValue


@pytest.fixture(scope="module")
def plan():
    from multimodalemotionrecognition_amd._lib import LIB, lib_path
    if not lib_path().exists():
        subprocess.run(["make", "-C", str(ROOT / "multimodalemotionrecognition_amd" / "csrc"), "-j8"], check=True)

    def call(*args):
        out = (ctypes.c_longlong * 4)(-7, -7, -7, -7)
        return LIB.call_int("mer_conv_wgrad_plan", *args, out), list(out)
    return call


@pytest.fixture(scope="module")
def records():
    recs = json.loads((ROOT / "tests" / "golden" / "wgrad_plan.json").read_text())
    assert len(recs) > 300
    return recs


def test_plan_reproduces_the_recorded_table(plan, records):
    bad = [(r, got) for r in records if (got := plan(*r[:12])) != (0, r[12:])]
    assert not bad, (len(bad), bad[:10])
    # the records cover the automatic choice of both rings, every explicit form, a launch that writes fewer slabs than
    # it was asked for (rings and strip) and the trunk's own launches at the benchmark's 256 frames
    auto = {tuple(r[:10]): r[12:15] for r in records if r[10] == -1 and r[11] == 0}
    assert {v[0] for v in auto.values()} == {4, 8}
    assert {r[12] for r in records} == {4, 8, 9, 10}
    assert any(r[14] < r[13] for r in records if r[12] in (4, 8)) and any(r[14] < r[13] for r in records if r[12] > 8)
    assert auto[(256, 59, 59, 16, 16, 64, 4, 4, 1, 0)] == [4, 384, 381]  # the stem, space-to-depth form
    assert auto[(256, 28, 28, 64, 64, 64, 3, 3, 1, 1)] == [4, 154, 150]  # layer1 3x3
    assert auto[(256, 14, 14, 128, 128, 128, 3, 3, 1, 1)] == [8, 24, 24]  # layer2 3x3 stride 1
    assert auto[(256, 4, 4, 512, 512, 512, 3, 3, 1, 1)] == [8, 3, 3]  # layer4 3x3 stride 1


def test_plan_is_idempotent(plan, records):
    """Planning again from a record's resolved (variant, splits) returns the same record -- what lets the caller plan
    first and the launch plan again from what it is passed; and a launch asked for the slab count writes the same
    slabs (the per-split rounding does not move)."""
    for r in records:
        geom, want = r[:10], r[12:]
        assert plan(*geom, want[0], want[1]) == (0, want), r
        rc, again = plan(*geom, want[0], want[2])
        assert rc == 0 and again[0] == want[0] and again[1] == again[2] == want[2], (r, again)


def test_plan_refusals_leave_out_untouched(plan):
    ok = (4, 14, 14, 64, 64, 128, 3, 3, 1, 1)  # N, H, W, C, Creal, K, R, S, stride, pad: a shape the strip takes
    assert plan(*ok, 9, 0)[0] == 0 and plan(*ok, 10, 0)[0] == 0

    def geom(**kw):
        g = dict(zip("N H W C Creal K R S stride pad".split(), ok))
        g.update(kw)
        return tuple(g.values())

    refused = {
        "strip on stride 2": (geom(stride=2), 9),
        "strip on 1x1": (geom(R=1, S=1, pad=0), 9),
        "C = 8": (geom(C=8, Creal=8), 9),
        "W = 127": (geom(W=127), 9),
        "K % KB != 0 (9)": (geom(K=96), 9),
        "K % KB != 0 (10)": (geom(K=48), 10),
        "variant 11": (ok, 11),
        "R*S = 64": (geom(R=8, S=8, pad=4), 4),
        "C % 8": (geom(C=60, Creal=60), 4),
        "K % 8": (geom(K=100), 4),
        "strip with Creal < C": (geom(Creal=3), 9),
    }
    for name, (g, v) in refused.items():
        for splits in (0, 4):
            assert plan(*g, v, splits) == (INVALID, [-7] * 4), name
    assert plan(*geom(W=126), 9, 0)[0] == 0  # the widest map the X ring holds
    assert plan(*geom(K=96), 10, 0)[0] == 0 and plan(*geom(R=7, S=7, pad=3), 4, 0)[0] == 0
