"""Standalone timing of the batched weight-gradient fold (mer_wgrad_fold_batch) on the ResNet18 trunk's slabs at B = 32.

Launches the split-K partial pass of every trunk conv's weight gradient once (K.conv_wgrad(..., defer=folds), the
train step's shapes and split counts; the 19 block convs and the stem's map record: the 20 records of a step), then
times the ONE fold launch of all records with HIP events, replaying the same record table N times.  The table's
~350 MB of slabs exceed the 256 MB Infinity Cache, so a replay reads them cold, as the step does.
--per-record also times each record in a launch of its own: per iteration the records are launched one after the
other, an event pair around each, so between two launches of a record the other records' slabs have passed through
the cache; it prints the median us and the TB/s of each record's bytes (slabs read once, dw read and written).  A
record alone can leave CUs idle (a layer1 record is 128 blocks), which the launches of a step do not: --per-flush
times the record groups the step folds together (video.FOLD_EVERY: one flush per ResNet layer, the stem's record with
layer1) the same way.  Compare libraries with MER_HIP_LIB=<alt build>.
    python tools/bench_fold.py [--iters 20] [--per-record] [--per-flush]
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from multimodalemotionrecognition_amd import kernels as K  # noqa: E402


def trunk_wgrad_shapes(N=256):
    """(x shape, dy shape, R, stride, pad) of every block conv's weight gradient (the stem's record is separate)."""
    out = []
    h, c = 28, 64
    for cout, s in ((64, 1), (128, 2), (256, 2), (512, 2)):
        ho = (h + 2 - 3) // s + 1
        out.append(((N, h, h, c), (N, ho, ho, cout), 3, s, 1))  # block 0 conv1
        out.append(((N, ho, ho, cout), (N, ho, ho, cout), 3, 1, 1))  # block 0 conv2
        if s == 2:
            out.append(((N, h, h, c), (N, ho, ho, cout), 1, s, 0))  # downsample
        out.append(((N, ho, ho, cout), (N, ho, ho, cout), 3, 1, 1))  # block 1 conv1
        out.append(((N, ho, ho, cout), (N, ho, ho, cout), 3, 1, 1))  # block 1 conv2
        h, c = ho, cout
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--per-record", action="store_true", help="also time each record in a launch of its own")
    ap.add_argument("--per-flush", action="store_true", help="also time the record groups the step folds together (one per ResNet layer)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    folds = K.WgradFolds()
    keep = []
    for xs, ds, R, s, p in trunk_wgrad_shapes():
        x = torch.randn(*xs, device=dev).bfloat16()
        dy = torch.randn(*ds, device=dev).bfloat16()
        dw = torch.zeros(ds[-1], xs[-1], R, R, device=dev)
        K.conv_wgrad(x, dy, dw, R, R, s, p, defer=folds)
        keep += [x, dy, dw]
    # the stem: 4x4 / stride-1 wgrad on the space-to-depth input, slab columns gathered into the 7x7x3 weight
    from multimodalemotionrecognition_amd.video import S2D_CH, _stem_wgrad_map
    x = torch.randn(256, 115, 115, S2D_CH, device=dev).bfloat16()
    dy = torch.randn(256, 112, 112, 64, device=dev).bfloat16()
    dw = torch.zeros(64, 3, 7, 7, device=dev)
    K.conv_wgrad(x, dy, dw, 4, 4, 1, 0, defer=folds, dw_map=_stem_wgrad_map(7, 7, 3, dev))
    keep += [x, dy, dw]
    del x, dy
    rows, kept = list(folds.rows), list(folds.keep)
    # slabs the fold reads: splits (the count the launch really used) * K * RS * C floats per record
    rec_slab = [r[7] * r[3] * r[6] * r[4] * 4 for r in rows]
    rec_dw = [int(t.numel()) * 4 for t in kept[1::3]]
    slab_bytes = sum(rec_slab)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for it in range(a.iters + 3):
        folds.rows, folds.keep = list(rows), list(kept)
        if it == 3:
            torch.cuda.synchronize()
            ev[0].record()
        folds.flush()
    ev[1].record()
    torch.cuda.synchronize()
    us = ev[0].elapsed_time(ev[1]) * 1e3 / a.iters
    print(f"records {len(rows)}  slab bytes {slab_bytes / 1e6:.1f} MB  fold {us:.1f} us  "
          f"{slab_bytes / us / 1e6:.2f} TB/s")
    n = len(rows)

    def time_groups(groups):
        """Median us of each group of records in a launch of its own, the groups launched in turn per iteration."""
        evs = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in groups]
               for _ in range(a.iters)]
        for it in range(a.iters + 3):
            for gi, g in enumerate(groups):
                folds.rows, folds.keep = [rows[i] for i in g], [t for i in g for t in kept[3 * i:3 * i + 3]]
                if it >= 3:
                    evs[it - 3][gi][0].record()
                folds.flush()
                if it >= 3:
                    evs[it - 3][gi][1].record()
        torch.cuda.synchronize()
        t = np.array([[e0.elapsed_time(e1) * 1e3 for e0, e1 in row] for row in evs])  # [iters, groups] us
        return np.median(t, axis=0)

    if a.per_flush:
        # the step's flushes, in backward order (video.FOLD_EVERY = 2: one per ResNet layer, the stem with layer1)
        groups = [list(range(14, 19)), list(range(9, 14)), list(range(4, 9)), list(range(0, 4)) + [19]]
        med = time_groups(groups)
        for name, g, us_ in zip(("layer4", "layer3", "layer2", "layer1 + stem"), groups, med):
            byt = sum(rec_slab[i] + 2 * rec_dw[i] for i in g)
            print(f"flush {name:<14} {len(g)} records {byt / 1e6:>6.1f} MB {us_:>7.1f} us {byt / us_ / 1e6:>5.2f} TB/s")
        print(f"sum of the per-flush medians {med.sum():.1f} us")
    if a.per_record:
        med = time_groups([[i] for i in range(n)])
        print(f"{'rec':>3} {'K':>4} {'C':>4} {'RS':>3} {'slabs':>5} {'slab MB':>8} {'us':>7} {'TB/s':>6}")
        for i, r in enumerate(rows):
            byt = rec_slab[i] + 2 * rec_dw[i]
            print(f"{i:>3} {r[3]:>4} {r[4]:>4} {r[6]:>3} {r[7]:>5} {rec_slab[i] / 1e6:>8.1f} {med[i]:>7.1f} "
                  f"{byt / med[i] / 1e6:>6.2f}")
        print(f"sum of the per-record medians {med.sum():.1f} us")


if __name__ == "__main__":
    main()
