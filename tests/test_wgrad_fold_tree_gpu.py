"""The batched weight-gradient fold (csrc/conv_wgrad.hip wgrad_fold_batch_kernel) reproduces its summation tree bit for
bit.  The tree is a contract: with `splits` partial slabs, SG = 8 / 4 / 1 split groups for
splits > 48 / > 12 / fewer; group sg takes slabs sg + SG*i in increasing i, slab i into chain a[i % 4] (each from +0),
group partial (a0 + a1) + (a2 + a3); s = 0, s += partial[sg] in order; dw = dw_old + s.  The emulation below does exactly
these fp32 adds with torch on the slabs the split-K pass left, so the comparison is torch.equal.  Only the public
entries are used (K.conv_wgrad(..., defer=), WgradFolds.flush), so the file also passes against an older build of the
library given through MER_HIP_LIB.

Split counts sit on both sides of the two SG thresholds (12 | 13, 48 | 49) with tails that are no multiple of 4 or 8.
N images whose output map is 8x8 and splits = N make the planned slabs of 64 * N pixels in N splits N, so N is the
slab count.
Shapes: a 3x3 conv whose dw runs are 16-byte aligned (also through a dw view one float off, so the run starts and ends
inside a 16-byte vector), a 1x1 / stride-2 conv, a 7x7 / stride-2 conv with Creal = 3 of 8 channels (147 floats per
output channel: every alignment, c >= Creal dropped), and the stem's map record (4x4 space-to-depth slabs gathered into
the 7x7x3 weight).  All records of a case fold in ONE launch, so the block lookup is exercised."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SPLITS = (1, 5, 12, 13, 21, 48, 49, 53)
# (H, C, Creal, K, R, stride, pad, dw view offset in floats): the output map is 8x8 in each
SHAPES = [(8, 64, 64, 64, 3, 1, 1, 0), (8, 64, 64, 64, 3, 1, 1, 1), (16, 128, 128, 8, 1, 2, 0, 0),
          (16, 8, 3, 8, 7, 2, 3, 0)]


def tree_sum(slabs):
    """The fold's sum over slabs [splits, ...] in its own order, one fp32 tensor add per addition of the tree."""
    splits = slabs.shape[0]
    sg_count = 8 if splits > 48 else (4 if splits > 12 else 1)
    s = torch.zeros_like(slabs[0])
    for sg in range(sg_count):
        a = [torch.zeros_like(slabs[0]) for _ in range(4)]
        for i, z in enumerate(range(sg, splits, sg_count)):
            a[i % 4] = a[i % 4] + slabs[z]
        s = s + ((a[0] + a[1]) + (a[2] + a[3]))
    return s


def fold_once(dw, s, Kc, C, creal, R, map_=None):
    """dw_old + s laid out as the fold writes it: [K][c][tap] for c < Creal, or dw[k].flat[map[j]] for a map record."""
    if map_ is None:
        return dw + s.view(Kc, R * R, C)[:, :, :creal].permute(0, 2, 1).reshape(Kc, creal, R, R)
    out = dw.clone().view(Kc, -1)
    valid = (map_ >= 0).nonzero().flatten()
    dest = map_[valid].long()
    assert dest.unique().numel() == dest.numel()
    out[:, dest] = out[:, dest] + s.view(Kc, -1)[:, valid]
    return out.view_as(dw)


@functools.lru_cache(maxsize=None)
def _records(N):
    """Every record of case N: the split-K pass run once (deferred), its slabs kept.  Returns (rows, keep, recs) with
    recs = (init, out, slabs [N, ...], Kc, C, creal, R, map) and `out` the tensor the rows fold into."""
    from multimodalemotionrecognition_amd import kernels as K
    from multimodalemotionrecognition_amd.video import S2D_CH, _stem_wgrad_map

    g = torch.Generator().manual_seed(7000 + N)
    folds = K.WgradFolds()
    recs = []
    for H, C, creal, Kc, R, stride, pad, off in SHAPES:
        x = torch.randn(N, H, H, C, generator=g).bfloat16().cuda()
        dy = torch.randn(N, 8, 8, Kc, generator=g).bfloat16().cuda()
        init = torch.randn(Kc, creal, R, R, generator=g).cuda()
        buf = torch.zeros(init.numel() + off, device="cuda")
        out = buf[off:].view_as(init)
        out.copy_(init)
        K.conv_wgrad(x, dy, out, R, R, stride, pad, creal=creal, splits=N, defer=folds)
        recs.append((init, out, Kc, C, creal, R, None))
    # the stem: 4x4 / stride-1 wgrad on the space-to-depth channels, gathered to [64][3][7][7]
    xs = torch.randn(N, 11, 11, S2D_CH, generator=g).bfloat16().cuda()
    dys = torch.randn(N, 8, 8, 64, generator=g).bfloat16().cuda()
    init = torch.randn(64, 3, 7, 7, generator=g).cuda()
    out = init.clone()
    map_ = _stem_wgrad_map(7, 7, 3, out.device)
    K.conv_wgrad(xs, dys, out, 4, 4, 1, 0, splits=N, defer=folds, dw_map=map_)
    recs.append((init, out, 64, S2D_CH, None, 4, map_))
    rows, keep = list(folds.rows), list(folds.keep)
    folds.rows, folds.keep = [], []
    full = []
    for row, ws, (init, out, Kc, C, creal, R, m) in zip(rows, keep[0::3], recs):
        assert row[7] == N == K.wgrad_plan(N, 8, 8, 64, 64, 64, 1, 1, 1, 0, 4, N).slabs  # the slab count the fold is told
        full.append((init, out, ws.view(N, Kc, R * R * C), Kc, C, creal, R, m))
    torch.cuda.synchronize()
    return rows, keep, full


def _flush(rows, keep):
    from multimodalemotionrecognition_amd import kernels as K

    folds = K.WgradFolds()
    folds.rows, folds.keep = list(rows), list(keep)
    folds.flush()  # one launch: len(rows) <= WgradFolds.MAX


@pytest.mark.parametrize("N", SPLITS)
def test_fold_batch_follows_the_tree(N):
    rows, keep, recs = _records(N)
    for init, out, *_ in recs:
        out.copy_(init)
    _flush(rows, keep)
    for i, (init, out, slabs, Kc, C, creal, R, m) in enumerate(recs):
        assert torch.equal(out, fold_once(init, tree_sum(slabs), Kc, C, creal, R, m)), (N, i)


@pytest.mark.parametrize("N", (5, 21, 53))
def test_fold_batch_accumulates(N):
    """Two flushes of the same records into one dw == the tree's sum added twice (a dw load hoisted across the
    wrong store, or a run's end written twice, would show)."""
    rows, keep, recs = _records(N)
    for init, out, *_ in recs:
        out.copy_(init)
    _flush(rows, keep)
    _flush(rows, keep)
    for i, (init, out, slabs, Kc, C, creal, R, m) in enumerate(recs):
        s = tree_sum(slabs)
        assert torch.equal(out, fold_once(fold_once(init, s, Kc, C, creal, R, m), s, Kc, C, creal, R, m)), (N, i)


def test_fold_batch_leaves_neighbours_alone():
    """The floats in front of a dw run that starts inside a 16-byte vector are not written."""
    rows, keep, recs = _records(13)
    init, out = recs[1][0], recs[1][1]
    base = out._base if out._base is not None else out
    flat = base.view(-1)
    flat[0] = 12345.0
    out.copy_(init)
    _flush(rows, keep)
    assert float(flat[0]) == 12345.0
