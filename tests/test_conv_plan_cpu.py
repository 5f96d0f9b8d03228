"""The conv tile plan's row counts (csrc/conv.hip conv_plan): mer_conv_fwd_rows / mer_conv_dgrad_rows reproduce every
record of tests/golden/conv_rows.json, which tools/gen_conv_rows.py took from the library before the launchers and the
row counts were made to share one plan.  Host-only entry points: no GPU needed (the CU count then reads as 256, the
MI355X's).  The table is pruned: variants -1 and 6 (the halo test; the exact counts) are recorded for every shape,
batch, stride, pointer alignment and with / without ds_dy; the other explicit variants, whose result today is a bound
that depends on the pixel count alone, only at N = 40 with aligned pointers and no ds_dy -- a change that makes one of
them read alignment or ds_dy has to extend tools/gen_conv_rows.py with it.  This pins the counts; that a launch writes
exactly that many rows is tests/test_resnet_gpu.py's to check."""
import json
import subprocess
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def test_conv_rows_reproduce_the_recorded_table():
    from multimodalemotionrecognition_amd._lib import LIB, lib_path
    if not lib_path().exists():
        subprocess.run(["make", "-C", str(ROOT / "multimodalemotionrecognition_amd" / "csrc"), "-j8"], check=True)
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the table was recorded for 256 CUs, this device has "
                    f"{torch.cuda.get_device_properties(0).multi_processor_count}")
    recs = json.loads((ROOT / "tests" / "golden" / "conv_rows.json").read_text())
    assert len(recs) > 200
    fns = {"fwd": "mer_conv_fwd_rows", "dgrad": "mer_conv_dgrad_rows"}
    bad = [(r, got) for r in recs if (got := LIB.call_int(fns[r[0]], *r[1:-1])) != r[-1]]
    assert not bad, (len(bad), bad[:10])
    # the records cover the halo kernel, both default pipelined tile heights, the parity-class sums and the error
    rows = {(r[0], r[-2]): set() for r in recs}
    for r in recs:
        rows[(r[0], r[-2])].add(r[-1])
    assert -1 in rows[("fwd", 8)] and -1 in rows[("dgrad", 8)]
    assert {256, 392, 196, 64, 19} <= rows[("fwd", -1)] and {1568, 124} <= rows[("dgrad", -1)]
