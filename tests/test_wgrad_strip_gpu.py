"""The strip weight gradient of the 3x3 / stride-1 / pad-1 convs (csrc/conv_wgrad.hip wgrad_strip_kernel, variants 9 and 10):
the reduction over a padded pixel index, all nine taps served from one LDS strip.  Shapes are the smallest at which
its index walk can go wrong: a full layer1 map, maps smaller than a 64-slot K-step (several images and pad rows in
one step), H != W, two channel chunks on both axes, and a 1x1 map where every tap but the centre is padding."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

STRIP = (9, 10)  # 64 / 32 output channels per tile
SHAPES = [(2, 28, 28, 64, 64), (3, 5, 5, 64, 64), (2, 6, 9, 64, 128), (5, 14, 14, 128, 128), (1, 1, 1, 64, 64)]
# 1, 3, the default (None) and 4: rows = N * (H + 1) split 4 ways leaves the last split ragged at every shape but the
# 1x1 map (58 -> 15,15,15,13; 18 -> 5,5,5,3; 14 -> 4,4,4,2; 75 -> 19,19,19,18); 3 is ragged at 58 and 14 rows
SPLITS = (1, 3, 4, None)


@functools.lru_cache(maxsize=None)
def _case(N, H, W, C, Kc):
    """bf16-rounded random operands (device) and the fp32 / fp64 torch weight gradients of them, computed once."""
    g = torch.Generator().manual_seed(1000 * N + 10 * H + W)
    x = torch.randn(N, H, W, C, generator=g).bfloat16()
    dy = torch.randn(N, H, W, Kc, generator=g).bfloat16()
    xr, dyr = x.double().permute(0, 3, 1, 2), dy.double().permute(0, 3, 1, 2)
    ref64 = torch.nn.grad.conv2d_weight(xr, (Kc, C, 3, 3), dyr, stride=1, padding=1)
    ref32 = torch.nn.grad.conv2d_weight(xr.float(), (Kc, C, 3, 3), dyr.float(), stride=1, padding=1)
    return x.cuda(), dy.cuda(), ref32.cuda(), ref64.cuda()


def _wgrad(x, dy, variant, splits, dw=None):
    from multimodalemotionrecognition_amd import kernels as K

    if dw is None:
        dw = torch.zeros(dy.shape[-1], x.shape[-1], 3, 3, device="cuda")
    K.conv_wgrad(x, dy, dw, 3, 3, 1, 1, variant=variant, splits=splits)
    return dw


def _partials(x, dy, variant, splits, slabs):
    """The split-K pass alone through the raw entry; returns the workspace of `slabs` slabs, NaN where unwritten."""
    from multimodalemotionrecognition_amd import kernels as K
    from multimodalemotionrecognition_amd._lib import LIB

    N, H, W, C = x.shape
    Kc = dy.shape[-1]
    ws = torch.full((slabs, Kc, 9 * C), float("nan"), device="cuda")
    LIB("mer_conv_wgrad_partials", N, H, W, C, Kc, 3, 3, 1, 1, x.data_ptr(), dy.data_ptr(), int(splits), ws.data_ptr(),
        int(variant), K.stream_ptr())
    return ws


@pytest.mark.parametrize("N,H,W,C,Kc", SHAPES)
def test_strip_wgrad_vs_torch(N, H, W, C, Kc):
    """Against torch.nn.grad.conv2d_weight with the bar of test_wgrad_split_k_groups, at every split count."""
    x, dy, ref, _ = _case(N, H, W, C, Kc)
    scale = float(ref.abs().max())
    for v in STRIP:
        for splits in SPLITS:
            err = float((_wgrad(x, dy, v, splits) - ref).abs().max())
            print(f"strip wgrad {(N, H, W, C, Kc)} variant {v} splits {splits}: max err {err:.3e} (max|ref| {scale:.3e})")
            assert err <= 5e-3 * scale + 1e-3, (v, splits)


@pytest.mark.parametrize("N,H,W,C,Kc", SHAPES)
def test_strip_wgrad_border_counts_exact(N, H, W, C, Kc):
    """x = dy = 1: dw[k, c, r, s] is N times the number of output pixels whose tap (r, s) lies inside the map --
    small integers, exact in bf16 and fp32, so a wrong pad slot or a window leaking into the next image is an
    off-by-count."""
    x = torch.ones(N, H, W, C, device="cuda").bfloat16()
    dy = torch.ones(N, H, W, Kc, device="cuda").bfloat16()
    cnt = torch.tensor([[N * (H - abs(r - 1)) * (W - abs(s - 1)) for s in range(3)] for r in range(3)],
                       dtype=torch.float32, device="cuda")
    want = cnt.expand(Kc, C, 3, 3).contiguous()
    for v in STRIP:
        for splits in SPLITS:
            assert torch.equal(_wgrad(x, dy, v, splits), want), (v, splits)


@pytest.mark.parametrize("N,H,W,C,Kc", [(2, 28, 28, 64, 64), (5, 14, 14, 128, 128)])
def test_strip_wgrad_error_vs_ring(N, H, W, C, Kc):
    """The same products in another fp32 grouping: against an fp64 reference the strip kernel's max error is at most
    1.5x the one-group ring's (variant 4) on the same data.  Both run at the SAME split count: the fp32 error grows
    with the length of a split's accumulation chain (one MFMA per 32 pixels), so only equal counts compare like with
    like -- the defaults differ at these small shapes (variant 4 cuts 1,568 pixels into 6 splits, the strip kernel
    takes one), and one chain of 53 MFMAs against six of 9 measured 9.7e-5 against 2.9e-5."""
    x, dy, _, ref64 = _case(N, H, W, C, Kc)
    for splits in (1, 4):
        e4 = float((_wgrad(x, dy, 4, splits).double() - ref64).abs().max())
        for v in STRIP:
            e9 = float((_wgrad(x, dy, v, splits).double() - ref64).abs().max())
            print(f"strip wgrad {(N, H, W, C, Kc)} splits {splits}: max err vs fp64 variant 4 {e4:.3e}, "
                  f"variant {v} {e9:.3e}")
            # measured on MI355X, max |error| against fp64, variant 4 / variants 9 and 10 (equal to each other):
            # (2, 28, 28, 64, 64): 1 split 8.00e-5 / 9.73e-5, 4 splits 4.68e-5 / 3.40e-5;
            # (5, 14, 14, 128, 128): 1 split 5.37e-5 / 8.03e-5, 4 splits 2.09e-5 / 2.03e-5
            assert e9 <= 1.5 * e4, (v, splits, e9, e4)


@pytest.mark.parametrize("N,H,W,C,Kc", [(3, 5, 5, 64, 64), (5, 14, 14, 128, 128)])
def test_strip_wgrad_repeatable_and_split_count(N, H, W, C, Kc):
    """Two launches give equal slabs and an equal dw; the launch writes exactly the planned slabs (every split
    non-empty, never more than asked)."""
    from multimodalemotionrecognition_amd import kernels as K

    x, dy, _, _ = _case(N, H, W, C, Kc)
    for v in STRIP:
        for splits in (4, 7, 1000):
            eff = K.wgrad_plan(N, H, W, C, C, Kc, 3, 3, 1, 1, v, splits).slabs
            assert 1 <= eff <= splits
            a, b = _partials(x, dy, v, splits, min(splits, eff + 1)), _partials(x, dy, v, splits, min(splits, eff + 1))
            assert torch.isfinite(a[:eff]).all() and torch.isnan(a[eff:]).all(), (v, splits)
            assert torch.equal(a[:eff], b[:eff]), (v, splits)
        assert torch.equal(_wgrad(x, dy, v, None), _wgrad(x, dy, v, None))


def test_strip_wgrad_deferred_fold():
    """Slabs left by the strip kernel and folded by ONE mer_wgrad_fold_batch launch against the immediate fold of the
    same launch; dw accumulates (+=).  Bitwise up to three slabs, where the fold kernels add in the same order (the
    batched fold sums four interleaved chains, the immediate one a single chain: from four slabs on they agree to fp32
    rounding, the bar of test_wgrad_fold_batch_matches_immediate_fold)."""
    from multimodalemotionrecognition_amd import kernels as K

    folds = K.WgradFolds()
    pairs = []
    for (N, H, W, C, Kc), v, splits in (((3, 5, 5, 64, 64), 9, 1), ((5, 14, 14, 128, 128), 9, 3),
                                        ((2, 6, 9, 64, 128), 10, 3), ((5, 14, 14, 128, 128), 10, 20)):
        x, dy, _, _ = _case(N, H, W, C, Kc)
        init = torch.randn(Kc, C, 3, 3, device="cuda")
        ref = _wgrad(x, dy, v, splits, init.clone())
        out = init.clone()
        K.conv_wgrad(x, dy, out, 3, 3, 1, 1, variant=v, splits=splits, defer=folds)
        assert folds.rows[-1][7] == K.wgrad_plan(N, H, W, C, C, Kc, 3, 3, 1, 1, v, splits).slabs
        pairs.append((ref, out, init, splits))
    torch.cuda.synchronize()
    assert all(torch.equal(o, i) for _, o, i, _ in pairs)  # nothing folded before the flush
    folds.flush()
    for ref, out, _, splits in pairs:
        if splits <= 3:
            assert torch.equal(out, ref), splits
        else:
            assert (out - ref).abs().max() <= 1e-5 * ref.abs().max(), splits


@pytest.mark.parametrize("N,H,C,Kc,R,stride,pad", [(2, 14, 64, 128, 3, 2, 1), (2, 14, 64, 128, 1, 1, 0),
                                                   (2, 14, 8, 64, 3, 1, 1)])
def test_strip_wgrad_refuses_unsupported(N, H, C, Kc, R, stride, pad):
    """Stride 2, 1x1 and C = 8 are refused by variants 9 / 10 (dw untouched); the automatic choice runs them on the
    kernels it always did, bit for bit."""
    from multimodalemotionrecognition_amd import kernels as K
    from multimodalemotionrecognition_amd._lib import MerKernelError

    torch.manual_seed(5)
    Ho = (H + 2 * pad - R) // stride + 1
    x = torch.randn(N, H, H, C, device="cuda").bfloat16()
    dy = torch.randn(N, Ho, Ho, Kc, device="cuda").bfloat16()
    for v in STRIP:
        dw = torch.zeros(Kc, C, R, R, device="cuda")
        with pytest.raises(MerKernelError):
            K.conv_wgrad(x, dy, dw, R, R, stride, pad, variant=v)
        assert not dw.any()
    auto, ring = torch.zeros(Kc, C, R, R, device="cuda"), torch.zeros(Kc, C, R, R, device="cuda")
    K.conv_wgrad(x, dy, auto, R, R, stride, pad)
    K.conv_wgrad(x, dy, ring, R, R, stride, pad, variant=4)
    assert torch.equal(auto, ring)
    ref = torch.nn.grad.conv2d_weight(x.float().permute(0, 3, 1, 2), (Kc, C, R, R), dy.float().permute(0, 3, 1, 2),
                                      stride=stride, padding=pad)
    assert (auto - ref).abs().max() <= 5e-3 * ref.abs().max() + 1e-3
